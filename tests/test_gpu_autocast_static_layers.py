"""nn.SAGEConv and nn.GATConv under torch.autocast('cuda', dtype=torch.bfloat16): forward and
backward run with no cast by the caller, give finite results, and agree with the same layer
outside autocast.

The tolerance.  tests/test_gpu_autocast_layers.py holds no numeric tolerance for
TemporalAttentionLayer (it asserts bit equality with a restatement under the same autocast
region), so the one used here is derived from the number format and fixed before any run.
bfloat16 keeps 8 significant bits: one rounding moves a value by at most half a step, 2^-8 of
its size.  Between the input and the output of one of these layers a value is rounded at most 8
times (the input and the weight of the first GEMM, its output, the aggregate, the input and the
weight of a second GEMM, its output, the sum with the self / residual term and the bias); the
backward pass doubles that.  Each rounding is granted its worst case, 2^-8, where a typical one
costs a third of that: the difference is the room for a GEMM or a segment sum with cancellation,
which passes on a perturbation relative to sum |w x|, not |sum w x|.  Hence, in the Frobenius
norm over a tensor,

    |out_amp - out|  <= 8 * 2^-8 |out|          |grad_amp - grad| <= 16 * 2^-8 |grad|.

SAGEConv('pool') takes a maximum, whose gradient jumps where two candidates tie; its inputs are
small integers with an integer fc_pool, so relu(fc_pool(x)) is exact in bfloat16 and in float32
and both runs route the gradient through the same edges."""
import numpy as np
import pytest

from tests import block_ops_ref as R
from tests.test_gpu_block_ops_fp64 import _col_less, _explicit

pytestmark = pytest.mark.gpu

FWD_TOL = 8 * 2.0 ** -8
BWD_TOL = 16 * 2.0 ** -8
NUM_DST = 24


def autocast():
    import torch
    return torch.autocast("cuda", dtype=torch.bfloat16)


@pytest.fixture(scope="module")
def layout():
    degs = np.random.RandomState(80).randint(0, 9, NUM_DST)
    degs[[0, 5]] = 0
    return R.block_layout(degs, True, 0)


def _close(got, want, tol, what):
    import torch
    assert torch.isfinite(got).all(), what
    err = float((got.float() - want).norm())
    size = float(want.norm())
    print("\n[{}] error / (tol * norm) = {:.3g}".format(what, err / max(tol * size, 1e-30)))
    assert err <= tol * size, (what, err, size)


def _both(layer, call):
    """call(layer) -> out, inside and outside autocast; outputs and parameter gradients."""
    import torch
    res = []
    for amp in (False, True):
        layer.zero_grad()
        torch.manual_seed(9)                     # the same dropout seed / mask on both sides
        if amp:
            with autocast():
                out = call(layer)
        else:
            out = call(layer)
        att = None
        if isinstance(out, tuple):
            out, att = out
            att = att.detach()
        torch.manual_seed(10)
        g = torch.randn(out.shape, device="cuda")
        (out.float() * g).sum().backward()       # outside the region, as loss.backward() is
        res.append((out.detach(), att, {k: p.grad.clone() for k, p in layer.named_parameters()}))
    (out, att, grads), (out_amp, att_amp, grads_amp) = res
    assert out.dtype == torch.float32 and out_amp.dtype == torch.bfloat16
    assert out.abs().sum() > 0
    _close(out_amp, out, FWD_TOL, "out")
    assert set(grads) == set(grads_amp) and grads
    for k in grads:
        assert grads_amp[k].dtype == torch.float32
        _close(grads_amp[k], grads[k], BWD_TOL, k)
    return att, att_amp


# SAGEConv('pool') takes no edge weights, inside or outside autocast
SAGE_CASES = [(agg, dims, weighted) for agg in ("mean", "gcn", "pool")
              for dims in ((40, 24), (24, 40)) for weighted in (False, True)
              if not (agg == "pool" and weighted)]


@pytest.mark.parametrize("agg,dims,weighted", SAGE_CASES,
                         ids=["{}-{}to{}{}".format(a, d[0], d[1], "-edge_weight" if w else "")
                              for a, d, w in SAGE_CASES])
def test_sageconv(layout, agg, dims, weighted):
    import torch
    from gnnflow_amd import nn as gnn
    b = _col_less(*layout)
    fin, fout = dims
    torch.manual_seed(81)
    layer = gnn.SAGEConv(fin, fout, agg).cuda()
    rng = np.random.RandomState(82)
    with torch.no_grad():
        layer.bias.uniform_(-1, 1)
    if agg == "pool":
        with torch.no_grad():
            layer.fc_pool.weight.copy_(torch.from_numpy(
                rng.randint(-1, 2, (fin, fin)).astype(np.float32)))
            layer.fc_pool.bias.copy_(torch.from_numpy(rng.randint(-1, 2, fin).astype(np.float32)))
        x = torch.from_numpy(rng.randint(0, 2, (b.num_src_nodes(), fin)).astype(np.float32)).cuda()
    else:
        x = torch.from_numpy(rng.randn(b.num_src_nodes(), fin).astype(np.float32)).cuda()
    w = torch.from_numpy(rng.uniform(0.5, 1.5, b.num_edges()).astype(np.float32)).cuda() \
        if weighted else None
    assert (fin > fout) == (dims == (40, 24))      # either side of lin_before_mp
    _both(layer, lambda m: m(b, x, edge_weight=w))


GAT_CONFIGS = {
    "composed": dict(),
    "composed_residual": dict(residual=True),
    "fused": dict(fused=True),
    "fused_residual": dict(fused=True, residual=True),
    "fused_dropout": dict(fused=True, fused_dropout=True, attn_drop=0.3),
    "fused_dropout_residual": dict(fused=True, fused_dropout=True, attn_drop=0.3, residual=True),
    "get_attention": dict(get_attention=True),
}


def _gat(cfg):
    import torch
    from gnnflow_amd import nn as gnn
    torch.manual_seed(83)
    layer = gnn.GATConv(24, 8, 3, attn_drop=cfg.get("attn_drop", 0.0),
                        residual=cfg.get("residual", False), allow_zero_in_degree=True).cuda()
    layer.train()
    layer.fused_attention = cfg.get("fused", False)
    layer.fused_attention_dropout = cfg.get("fused_dropout", False)
    with torch.no_grad():
        layer.bias.uniform_(-1, 1)
    return layer


@pytest.mark.parametrize("explicit", [False, True], ids=["sampler_layout", "explicit_col"])
@pytest.mark.parametrize("name", list(GAT_CONFIGS))
def test_gatconv(layout, name, explicit):
    import torch
    cfg = GAT_CONFIGS[name]
    b = (_explicit if explicit else _col_less)(*layout)
    layer = _gat(cfg)
    x = torch.from_numpy(np.random.RandomState(84).randn(b.num_src_nodes(), 24)
                         .astype(np.float32)).cuda()
    get_att = cfg.get("get_attention", False)
    att, att_amp = _both(layer, lambda m: m(b, x, get_attention=get_att))
    if get_att:
        assert att_amp.dtype == torch.float32 and att_amp.shape == (b.num_edges(), 3, 1)
        _close(att_amp, att, FWD_TOL, "attention")
    assert not layer.fused_attention or not get_att


def test_fused_dropout_gatconv_is_reproducible_on_a_sampler_block(layout):
    """The sampler's layout has no atomics: the same seed gives the same bits, run after run."""
    import torch
    b = _col_less(*layout)
    assert b.segments()[1] is None
    layer = _gat(GAT_CONFIGS["fused_dropout"])
    x = torch.from_numpy(np.random.RandomState(85).randn(b.num_src_nodes(), 24)
                         .astype(np.float32)).cuda()
    runs = []
    for seed in (21, 21, 22):
        layer.zero_grad()
        torch.manual_seed(seed)
        with autocast():
            out = layer(b, x)
        out.float().square().sum().backward()
        runs.append([out.detach().view(torch.int16)] +
                    [p.grad.clone() for p in layer.parameters()])
    assert all(torch.equal(a, c) for a, c in zip(runs[0], runs[1]))
    assert not torch.equal(runs[0][0], runs[2][0])      # another seed, another mask
