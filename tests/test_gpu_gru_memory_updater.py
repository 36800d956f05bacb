"""nn.GRUMemoryUpdater with fused_gru on against off, from one state dict, on a small synthetic
block (N = 40 source rows, R = 12 destination rows): the three dim_node cases, with and without
time encoding, a GRU cell with and without bias.

The rule is that of tests/gru_cell_ref.py, per tensor T of b.srcdata['h'], last_updated_memory
and every parameter gradient: with T_64 the same module in float64 on the CPU and T_torch the
flag-off module on the device,  e_fused <= 2 e_torch + 2^-23 max |T_64|.  Under bfloat16 autocast
the same with e_torch the flag-off module's error under autocast.  Then one models.DGNN step
with memory, flag on against flag off: Memory's tables within that rule.  Each test prints its
largest e_fused / bound (run with -s)."""
import copy

import numpy as np
import pytest

from tests import gru_cell_ref as GR

pytestmark = pytest.mark.gpu

N_ROWS, R_ROWS = 40, 12
DIM_EDGE, DIM_MEM = 6, 16
# (dim_node, dim_time): dim_node == dim_embed (h + updated), another dim_node (node_feat_proj)
# and none, each with and without the time encoding; dim_embed = dim_memory = 16
CONFIGS = [(dn, dt) for dn in (16, 10, 0) for dt in (8, 0)]


class _Block:
    """What GRUMemoryUpdater reads of a block: srcdata and the number of destination rows."""

    def __init__(self, srcdata, num_dst):
        self.srcdata, self._num_dst = srcdata, num_dst

    def num_dst_nodes(self):
        return self._num_dst


def _srcdata(dim_node, seed):
    """float32 / int64 CPU tensors as Memory.prepare_input leaves them; ts and mem_ts on a grid
    of 1/8 so that their float32 difference is exact."""
    import torch
    rng = np.random.RandomState(seed)
    f = lambda *s: torch.from_numpy(rng.standard_normal(s).astype(np.float32))      # noqa: E731
    d = {"ID": torch.from_numpy(rng.permutation(200)[:N_ROWS].astype(np.int64)),
         "ts": torch.from_numpy((rng.randint(80, 160, N_ROWS) / 8.0).astype(np.float32)),
         "mem_ts": torch.from_numpy((rng.randint(0, 80, N_ROWS) / 8.0).astype(np.float32)),
         "mem_input": f(N_ROWS, 2 * DIM_MEM + DIM_EDGE), "mem": f(N_ROWS, DIM_MEM)}
    if dim_node:
        d["h"] = f(N_ROWS, dim_node)
    return d


def _module(dim_node, dim_time, bias, seed=3):
    import torch
    from gnnflow_amd import nn as gnn
    torch.manual_seed(seed)
    m = gnn.GRUMemoryUpdater(dim_node, DIM_EDGE, dim_time, DIM_MEM, DIM_MEM)
    if not bias:
        m.updater = torch.nn.GRUCell(m.dim_message + dim_time, DIM_MEM, bias=False)
    if dim_time:
        with torch.no_grad():      # a bias away from its zero initialisation
            m.time_enc.w.bias.normal_()
    return m


def _run(module, src, G, device, dtype, autocast=False):
    """One forward + backward -> ({name: numpy}, last)."""
    import torch
    b = _Block({k: (v.to(device, dtype) if v.is_floating_point() else v.to(device))
                for k, v in src.items()}, R_ROWS)
    mem = b.srcdata['mem']
    module.zero_grad()
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
        last = module(b)
    h = b.srcdata['h']
    assert tuple(h.shape) == (N_ROWS, DIM_MEM) and h.dtype == dtype
    (h * G.to(device, dtype)).sum().backward()
    out = {"h": h, "last_updated_memory": last["last_updated_memory"]}
    out.update({"grad " + k: p.grad for k, p in module.named_parameters()})
    assert all(v is not None for v in out.values())
    assert b.srcdata['mem'] is mem
    return {k: v.detach().cpu().double().numpy() for k, v in out.items()}, last


def _compare(what, fused, unfused, want):
    worst = 0.0
    assert set(fused) == set(unfused) == set(want)
    for k in want:
        r = GR.ratio(fused[k], unfused[k], want[k])
        worst = max(worst, r)
        assert r <= 1.0, "{} {}: e_fused / bound = {:.3g} (e_fused {:.3g}, e_torch {:.3g})".format(
            what, k, r, GR.max_error(fused[k], want[k]), GR.max_error(unfused[k], want[k]))
    print("\n[e_fused/bound] {}: {:.3g}".format(what, worst))


@pytest.mark.parametrize("autocast", [False, True], ids=["float32", "autocast"])
@pytest.mark.parametrize("bias", [True, False], ids=["bias", "no_bias"])
@pytest.mark.parametrize("cfg", CONFIGS, ids=lambda c: "node{}_time{}".format(*c))
def test_fused_against_unfused(cfg, bias, autocast, monkeypatch):
    import torch
    from gnnflow_amd import ops
    dim_node, dim_time = cfg
    src = _srcdata(dim_node, 500 + dim_node + dim_time)
    G = torch.from_numpy(np.random.RandomState(9).standard_normal((N_ROWS, DIM_MEM))
                         .astype(np.float32))
    cpu = _module(dim_node, dim_time, bias)
    gpu = copy.deepcopy(cpu).cuda()
    want, last64 = _run(cpu.double(), src, G, "cpu", torch.float64)
    calls = []
    real = ops.gru_cell

    def counted(gi, gh, hx, residual=None, num_last=0):
        calls.append((gi.dtype, hx.dtype, None if residual is None else residual.dtype, num_last))
        return real(gi, gh, hx, residual=residual, num_last=num_last)
    monkeypatch.setattr(ops, "gru_cell", counted)

    assert gpu.fused_gru is False
    unfused, last_off = _run(gpu, src, G, "cuda", torch.float32, autocast)
    assert not calls
    state = {k: v.clone() for k, v in gpu.state_dict().items()}
    gpu.fused_gru = True
    fused, last_on = _run(gpu, src, G, "cuda", torch.float32, autocast)
    assert all(torch.equal(v, state[k]) for k, v in gpu.state_dict().items())
    gates = torch.bfloat16 if autocast else torch.float32
    res = None if not dim_node else (gates if dim_node != DIM_MEM else torch.float32)
    assert calls == [(gates, torch.float32, res, R_ROWS)]

    assert set(last_on) == {"last_updated_nid", "last_updated_memory", "last_updated_ts"}
    for k in ("last_updated_nid", "last_updated_ts"):
        assert torch.equal(last_on[k], last_off[k])
        assert torch.equal(last_on[k].cpu().to(last64[k].dtype), last64[k])
    mem = last_on["last_updated_memory"]
    assert mem.dtype == torch.float32 and tuple(mem.shape) == (R_ROWS, DIM_MEM)
    for v in last_on.values():
        assert not v.requires_grad and v.grad_fn is None and v.is_cuda
    _compare("updater node{} time{}".format(*cfg), fused, unfused, want)


def test_other_rows_take_the_torch_line(monkeypatch):
    """With the flag on, rows that are not float32 on the GPU go through nn.GRUCell."""
    import torch
    from gnnflow_amd import ops

    def never(*a, **k):
        raise AssertionError("ops.gru_cell called")
    monkeypatch.setattr(ops, "gru_cell", never)
    src = _srcdata(16, 1)
    G = torch.ones(N_ROWS, DIM_MEM)
    m = _module(16, 8, True)
    m.fused_gru = True
    _run(m, src, G, "cpu", torch.float32)
    _run(m.double(), src, G, "cpu", torch.float64)


# ---- one DGNN step -----------------------------------------------------------------------------
def _dgnn_step(world, fused, codes=False):
    """prepare_input -> updater -> forward -> loss -> backward -> update_mem_mail on a model
    whose memory is not all zeros -> (node_memory, mailbox, last_updated, the block's srcdata)."""
    import torch
    import torch.nn.functional as F
    from gnnflow_amd.models import DGNN
    from tests.test_gpu_models import N
    kw = dict(dim_node=32, dim_edge=16, dim_time=20, dim_embed=16, num_layers=2, num_snapshots=1,
              att_head=2, dropout=0.0, att_dropout=0.0, use_memory=True, dim_memory=16,
              num_nodes=N)
    torch.manual_seed(11)
    model = DGNN(**kw).cuda().train()
    model.memory_updater.fused_gru = fused
    mem = model.memory
    g = torch.Generator().manual_seed(12)
    mem.node_memory.copy_(torch.randn(mem.node_memory.shape, generator=g))
    mem.mailbox.copy_(torch.randn(mem.mailbox.shape, generator=g))
    mfgs = world.mfgs(kw, 0)
    b = mfgs[0][0]
    mem.prepare_input(b)
    src = {k: b.srcdata[k].detach().cpu().clone()
           for k in ("ID", "ts", "mem_ts", "mem_input", "mem", "h")}
    model.last_updated = last = model.memory_updater(b)
    pos, neg = model(mfgs)
    loss = F.binary_cross_entropy_with_logits(pos, torch.ones_like(pos)) + \
        F.binary_cross_entropy_with_logits(neg, torch.zeros_like(neg))
    loss.backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in model.parameters())
    if codes:      # every row of last_updated_memory carries the indices of its own entries
        R, H = last["last_updated_memory"].shape
        last = dict(last, last_updated_memory=torch.arange(
            1, R * H + 1, dtype=torch.float32, device="cuda").reshape(R, H))
        mem.node_memory.fill_(0)
        mem.mailbox.fill_(0)
    # the outer block of a 2-layer model has any number of destination rows; update_mem_mail
    # takes whole (src, dst, neg) thirds and refuses a remainder, so the rows behind the last
    # whole third go (it read none of them when it still let them through)
    whole = last["last_updated_nid"].shape[0] // 3 * 3
    with torch.no_grad():
        mem.update_mem_mail(**{k: v[:whole] for k, v in last.items()}, edge_feats=None,
                            neg_sample_ratio=1)
    return mem.node_memory.clone(), mem.mailbox.clone(), model.last_updated, src, model


def test_one_dgnn_step_leaves_the_same_memory():
    import torch
    from tests.test_gpu_models import _World
    world = _World()
    mem_off, mail_off, last_off, src, model = _dgnn_step(world, False)
    mem_on, mail_on, last_on, src_on, _ = _dgnn_step(world, True)
    assert all(torch.equal(src[k], src_on[k]) for k in src)
    assert torch.equal(last_on["last_updated_nid"], last_off["last_updated_nid"])
    assert torch.equal(last_on["last_updated_ts"], last_off["last_updated_ts"])
    assert not last_on["last_updated_memory"].requires_grad
    # T_64: the updater in float64 on the CPU on the same rows, and update_mem_mail's copies of
    # them, located by a run whose last_updated_memory holds 1 + the flat index of each entry
    # (tables zeroed first: 0 = not written from last_updated_memory)
    code_mem, code_mail, _, _, _ = _dgnn_step(world, False, codes=True)
    up64 = copy.deepcopy(model.memory_updater).cpu().double()
    up64.fused_gru = False
    R = last_on["last_updated_nid"].shape[0]
    b64 = _Block({k: (v.double() if v.is_floating_point() else v) for k, v in src.items()}, R)
    with torch.no_grad():
        last64 = up64(b64)["last_updated_memory"].numpy()
    flat = np.concatenate([[0.0], last64.reshape(-1)])
    worst = 0.0
    assert (code_mem > 0).any() and (code_mail > 0).any()
    for what, on, off, code in (("node_memory", mem_on, mem_off, code_mem),
                                ("mailbox", mail_on, mail_off, code_mail)):
        on, off = on.cpu().double().numpy(), off.cpu().double().numpy()
        code = code.cpu().numpy().astype(np.int64)
        # entries that are no copy of last_updated_memory are the same bits on both sides
        assert np.array_equal(on[code == 0], off[code == 0]), what
        want = np.where(code > 0, flat[code], off)
        r = GR.ratio(on, off, want)
        worst = max(worst, r)
        assert r <= 1.0, "{}: e_fused / bound = {:.3g}".format(what, r)
    r = GR.ratio(last_on["last_updated_memory"].cpu().numpy(),
                 last_off["last_updated_memory"].cpu().numpy(), last64)
    assert r <= 1.0
    print("\n[e_fused/bound] one DGNN step: {:.3g}".format(max(worst, r)))
