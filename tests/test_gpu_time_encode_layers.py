"""nn.TemporalAttentionLayer and nn.GRUMemoryUpdater with fused_time_encode on and off, on a
sampler block, against float64 restatements on the CPU.  The rule is that of
tests/test_gpu_temporal_attention_layer.py: per tensor, the error of the path with
ops.time_encode_cat is at most 4 x the error of the path without it on the same inputs,
measured in the same test and printed (run with -s)."""
import numpy as np
import pytest

from tests.test_gpu_temporal_attention_layer import (DIM_OUT, HEADS, _reference64,
                                                      _sampled_block)

pytestmark = pytest.mark.gpu

LAYER_CONFIGS = [(32, 16, 20), (0, 16, 20)]
UPDATER_CONFIGS = [(0, 0, 100, 100, 100), (32, 16, 20, 24, 24), (24, 16, 20, 24, 24),
                   (32, 0, 0, 24, 24)]


def _count_calls(monkeypatch):
    """ops.time_encode_cat wrapped: records the shape of every result."""
    from gnnflow_amd import ops
    calls = []
    real = ops.time_encode_cat

    def counted(*a, **k):
        out = real(*a, **k)
        calls.append(tuple(out.shape))
        return out
    monkeypatch.setattr(ops, "time_encode_cat", counted)
    return calls


def _four_times_rule(what, unfused, fused):
    print("\n[fp32 - float64] {}: unfused max {:.3g}, fused max {:.3g}".format(
        what, max(unfused.values()), max(fused.values())))
    for k in fused:
        assert unfused[k] > 0 or fused[k] == 0, k
        assert fused[k] <= 4 * unfused[k], "{}: fused {:.3g} > 4 x unfused {:.3g}".format(
            k, fused[k], unfused[k])


@pytest.mark.parametrize("cfg", LAYER_CONFIGS, ids=lambda c: "_".join(map(str, c)))
def test_attention_layer_with_fused_time_encode(cfg, monkeypatch):
    import torch
    from gnnflow_amd import nn as gnn
    dn, de, dtm = cfg
    b = _sampled_block()
    R, E, ns = b.num_dst_nodes(), b.num_edges(), b.num_src_nodes()
    rng = np.random.RandomState(160 + dn + de + dtm)
    h = torch.from_numpy(rng.randn(ns, max(dn, 1)).astype(np.float32))
    f = torch.from_numpy(rng.randn(E, max(de, 1)).astype(np.float32))
    G = torch.from_numpy(rng.randn(R, DIM_OUT).astype(np.float32))
    if dn:
        b.srcdata['h'] = h.cuda()
    if de:
        b.edata['f'] = f.cuda()
    torch.manual_seed(161)
    layer = gnn.TemporalAttentionLayer(dn, de, dtm, DIM_OUT, HEADS, 0.0, 0.0).cuda().eval()
    with torch.no_grad():       # a bias away from its zero initialisation
        layer.time_enc.w.bias.copy_(torch.from_numpy(rng.randn(dtm).astype(np.float32)))
    params = dict(layer.named_parameters())
    row = b.edges()[1].cpu()
    want, want_g = _reference64(cfg, params, h.double(), f.double(), b.edata['dt'].double().cpu(),
                                row, R, G.double())
    calls = _count_calls(monkeypatch)

    def run(fused):
        layer.fused_time_encode = fused
        layer.zero_grad()
        out = layer(b)
        (out * G.cuda()).sum().backward()
        err = {"out": np.abs(out.detach().cpu().numpy() - want).max()}
        for k, v in params.items():
            err[k] = np.abs(v.grad.cpu().numpy() - want_g[k]).max() if v.grad is not None else 0.0
        return err

    unfused = run(False)
    assert not calls
    fused = run(True)
    # one call for the query rows and one for the K / V rows
    assert sorted(calls) == sorted([(R, dn + dtm), (E, dn + de + dtm)])
    assert set(want_g) == {k for k, v in params.items() if v.grad is not None}
    _four_times_rule("layer " + "_".join(map(str, cfg)), unfused, fused)


def _updater64(cfg, state, src, R, G):
    """GRUMemoryUpdater's forward in float64 plain torch on the CPU, torch.nn.GRUCell in double
    loaded from the same state dict; returns (h, updated[:R], {param: grad})."""
    import torch
    dn, de, dtm, demb, dm = cfg
    cell = torch.nn.GRUCell(2 * dm + de + dtm, dm).double()
    cell.load_state_dict({k[len("updater."):]: v.detach().double().cpu()
                          for k, v in state.items() if k.startswith("updater.")})
    p = {k: v.detach().double().cpu().requires_grad_(True) for k, v in state.items()
         if not k.startswith("updater.")}
    x = src['mem_input']
    if dtm:
        dt = (src['ts'] - src['mem_ts']).reshape(-1, 1)     # the fp32 difference, as the layer's
        x = torch.cat([x, torch.cos(dt.double() @ p["time_enc.w.weight"].T + p["time_enc.w.bias"])], 1)
    updated = cell(x.double(), src['mem'].double())
    if dn and dn == demb:
        h = src['h'].double() + updated
    elif dn:
        h = updated + src['h'].double() @ p["node_feat_proj.weight"].T + p["node_feat_proj.bias"]
    else:
        h = updated
    (h * G).sum().backward()
    grads = {"updater." + k: v.grad.numpy() for k, v in cell.named_parameters()}
    grads.update({k: v.grad.numpy() for k, v in p.items()})
    return h.detach().numpy(), updated[:R].detach().numpy(), grads


@pytest.mark.parametrize("cfg", UPDATER_CONFIGS, ids=lambda c: "_".join(map(str, c)))
def test_gru_memory_updater(cfg, monkeypatch):
    import torch
    from gnnflow_amd import nn as gnn
    from gnnflow_amd.memory import Memory
    dn, de, dtm, demb, dm = cfg
    b = _sampled_block()
    R, ns = b.num_dst_nodes(), b.num_src_nodes()
    rng = np.random.RandomState(170 + sum(cfg))

    def rand(*shape):
        return torch.from_numpy(rng.randn(*shape).astype(np.float32))

    memory = Memory(300, de, dm, 'cuda')
    memory.node_memory.copy_(rand(300, dm))
    memory.mailbox.copy_(rand(300, 2 * dm + de))
    memory.node_memory_ts.copy_(torch.from_numpy(rng.uniform(0, 0.5, 300).astype(np.float32)))
    memory.mailbox_ts.copy_(memory.node_memory_ts)
    memory.prepare_input(b)
    h0 = rand(ns, dn).cuda() if dn else None
    G = rand(ns, dm)
    torch.manual_seed(171)
    updater = gnn.GRUMemoryUpdater(*cfg).cuda()
    assert gnn.GRUMemeoryUpdater is gnn.GRUMemoryUpdater
    if dtm:
        with torch.no_grad():
            updater.time_enc.w.bias.copy_(rand(dtm))
    params = dict(updater.named_parameters())
    keys = ('ts', 'mem_ts', 'mem_input', 'mem', 'ID')
    src = {k: b.srcdata[k].detach().cpu() for k in keys}
    if dn:
        src['h'] = h0.cpu()
    mem_input = b.srcdata['mem_input']
    want_h, want_mem, want_g = _updater64(cfg, updater.state_dict(), src, R, G.double())
    calls = _count_calls(monkeypatch)

    def run(fused):
        updater.fused_time_encode = fused
        updater.zero_grad()
        if dn:
            b.srcdata['h'] = h0.clone()
        else:
            b.srcdata.pop('h', None)
        last = updater(b)
        h = b.srcdata['h']
        assert tuple(h.shape) == (ns, dm)
        (h * G.cuda()).sum().backward()
        # the three returned tensors: the first R rows, detached, and copies of their own
        assert set(last) == {"last_updated_nid", "last_updated_memory", "last_updated_ts"}
        assert torch.equal(last["last_updated_nid"], b.srcdata['ID'][:R])
        assert torch.equal(last["last_updated_ts"], b.srcdata['ts'][:R])
        assert tuple(last["last_updated_memory"].shape) == (R, dm)
        for v in last.values():
            assert not v.requires_grad and v.grad_fn is None and v.is_cuda
        assert last["last_updated_nid"].data_ptr() != b.srcdata['ID'].data_ptr()
        assert last["last_updated_ts"].data_ptr() != b.srcdata['ts'].data_ptr()
        assert b.srcdata['mem_input'] is mem_input        # not written back
        err = {"h": np.abs(h.detach().cpu().numpy() - want_h).max(),
               "last_updated_memory":
                   np.abs(last["last_updated_memory"].cpu().numpy() - want_mem).max()}
        for k, v in params.items():
            err[k] = np.abs(v.grad.cpu().numpy() - want_g[k]).max()
        # last_updated_memory does not alias the updated memory behind h
        before = h.detach().clone()
        last["last_updated_memory"].add_(1.0)
        assert torch.equal(h.detach(), before)
        return err

    unfused = run(False)
    assert not calls
    fused = run(True)
    assert calls == ([(ns, 2 * dm + de + dtm)] if dtm else [])
    assert set(want_g) == set(params)
    _four_times_rule("updater " + "_".join(map(str, cfg)), unfused, fused)
