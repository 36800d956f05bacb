"""nn.GATConv with `fused_attention` (one ops.block_gat call) against the same layer on the
composed chain, same parameters, same block, same upstream gradient.

Tolerances.  Both layers run the same torch ops on the same bits up to the attention (fc, el, er,
the residual, the bias), so they differ only in what the attention returns: out, and the
gradients gfeat, gel, ger it hands back.  tests/block_gat_ref.py bounds the fused side of each
(b_x) on the layer's own fp32 feat_src / el / er; the composed side stays within k b_x, k =
(D + 2) / (D + 1) (tests/test_gpu_block_gat.py::test_composed_chain_cross_check), so
|difference| <= (1 + k) b_x =: d_x.  These differences reach the parameters linearly:
    G = gfeat + gel attn_l + [ger attn_r ; 0]      grad of feat_src, dG = d_gfeat + d_gel |attn_l|
                                                    + [d_ger |attn_r| ; 0] + 4 u (sum of |terms|)
    fc.weight.grad = G^T h       bound  dG^T |h|        + 2 gamma_{n+2} |G|^T |h|
    attn_l.grad    = sum gel f   bound  sum d_gel |f|   + 2 gamma_{n+2} sum |gel f|
    attn_r.grad    = sum ger f   bound  sum d_ger |f|   + 2 gamma_{n+2} sum |ger f|
(n rows summed in fp32 by each side in an order of its own), and bias.grad and
res_fc.weight.grad do not depend on the attention at all: 2 gamma_{n+2} sum |terms|."""
import numpy as np
import pytest

from tests import block_gat_ref as Gr
from tests.block_ops_ref import U, error_ratio, gamma

pytestmark = pytest.mark.gpu
IN, H, D = 12, 3, 5


def _np(t):
    return t.detach().cpu().numpy().astype(np.float64)


def _block(zero_degree):
    """A hand-built block with repeated sources; destination 2 without in-edges on request."""
    import torch
    from gnnflow_amd import MFGBlock
    rng = np.random.RandomState(70)
    degs = np.array([3, 5, 0 if zero_degree else 2, 9, 1, 4])
    row = Gr.rows_of(degs)
    nd, ns = len(degs), len(degs) + 10
    col = rng.randint(0, ns, len(row)).astype(np.int64)
    p = rng.permutation(len(row))
    return MFGBlock(ns, nd, torch.from_numpy(col[p]).cuda(), torch.from_numpy(row[p]).cuda()), \
        col[p], row[p], nd, ns


def _layers(**kw):
    import torch
    from gnnflow_amd import nn as gnn
    torch.manual_seed(3)
    a = gnn.GATConv(IN, D, H, **kw).cuda()
    b = gnn.GATConv(IN, D, H, **kw).cuda()
    b.load_state_dict(a.state_dict())
    if a.bias is not None:
        with torch.no_grad():
            a.bias.normal_()
            b.bias.copy_(a.bias)
    b.fused_attention = True
    return a, b


def _calls(monkeypatch):
    from gnnflow_amd import ops
    seen = []
    real = ops.block_gat
    monkeypatch.setattr(ops, "block_gat", lambda *a, **k: (seen.append(k), real(*a, **k))[1])
    return seen


@pytest.mark.parametrize("training", [False, True], ids=["eval", "train"])
@pytest.mark.parametrize("residual,bias,zero", [(False, True, False), (True, True, True),
                                                (True, False, False), (False, False, True)])
def test_fused_layer_matches_composed(monkeypatch, residual, bias, zero, training):
    import torch
    seen = _calls(monkeypatch)
    blk, col, row, nd, ns = _block(zero)
    composed, fused = _layers(residual=residual, bias=bias, allow_zero_in_degree=zero,
                              attn_drop=0.0, feat_drop=0.0)
    for m in (composed, fused):
        m.train(training)
    rng = np.random.RandomState(71)
    h = torch.from_numpy(rng.randn(ns, IN).astype(np.float32)).cuda()
    g0 = torch.from_numpy(rng.randn(nd, H, D).astype(np.float32)).cuda()
    outs = []
    for m in (composed, fused):
        out = m(blk, h)
        (out * g0).sum().backward()
        outs.append(out)
    assert len(seen) == 1                          # the fused layer, once; the composed never
    # the attention's own inputs, as both layers computed them (same bits)
    with torch.no_grad():
        feat_src = composed.fc(h).view(-1, H, D)
        el = (feat_src * composed.attn_l).sum(-1)
        er = (feat_src[:nd] * composed.attn_r).sum(-1)
    ref = Gr.Reference(col, row, nd, ns, _np(feat_src), _np(el), _np(er), _np(g0), 0.2)
    ref.assert_clear_of_kink()
    k = 1.0 + (D + 2.0) / (D + 1.0)
    d_out, d_gfeat, d_gel, d_ger = (k * b for b in (ref.b_out, ref.b_gfeat, ref.b_gel, ref.b_ger))
    al, ar = np.abs(_np(composed.attn_l)), np.abs(_np(composed.attn_r))
    f, ha = np.abs(_np(feat_src)), np.abs(_np(h))
    pad = lambda x: np.concatenate([x, np.zeros((ns - nd,) + x.shape[1:])])   # noqa: E731
    terms = np.abs(ref.gfeat) + np.abs(ref.gel)[:, :, None] * al + \
        pad(np.abs(ref.ger)[:, :, None] * ar)
    dG = d_gfeat + d_gel[:, :, None] * al + pad(d_ger[:, :, None] * ar) + 4 * U * terms
    gn = 2 * gamma(ns + 2)
    bounds = {
        "fc.weight": (dG + gn * terms).reshape(ns, H * D).T @ ha,
        "attn_l": ((d_gel + gn * np.abs(ref.gel))[:, :, None] * f).sum(0)[None],
        "attn_r": ((d_ger + gn * np.abs(ref.ger))[:, :, None] * f[:nd]).sum(0)[None],
        "bias": gn * np.abs(_np(g0)).sum(0).reshape(-1),
        "res_fc.weight": gn * np.abs(_np(g0)).reshape(nd, H * D).T @ ha[:nd],
    }
    r = error_ratio(_np(outs[1]), _np(outs[0]), d_out)
    assert r <= 1.0, ("out", r)
    if zero:        # the zero-degree destination: residual and bias alone, the same bits
        assert torch.equal(outs[0][2], outs[1][2])
    worst = {"out": r}
    names = [n for n, _ in composed.named_parameters()]
    assert names == [n for n, _ in fused.named_parameters()] and set(names) <= set(bounds)
    for (name, pc), (_, pf) in zip(composed.named_parameters(), fused.named_parameters()):
        assert pc.grad is not None and pf.grad is not None
        worst[name] = error_ratio(_np(pf.grad), _np(pc.grad), bounds[name])
        assert worst[name] <= 1.0, (name, worst[name])
    print("\n[error/bound] {}".format(" ".join("{}={:.3g}".format(*x) for x in worst.items())))


def test_fused_dropout_is_reproducible_under_manual_seed(monkeypatch):
    import torch
    seen = _calls(monkeypatch)
    blk, col, row, nd, ns = _block(False)
    _, layer = _layers(attn_drop=0.5)
    h = torch.from_numpy(np.random.RandomState(72).randn(ns, IN).astype(np.float32)).cuda()
    layer.train()
    before = layer(blk, h)                  # fused_attention alone: dropout takes the chain
    assert not seen
    layer.fused_attention_dropout = True
    torch.manual_seed(11)
    first = layer(blk, h)
    torch.manual_seed(11)
    second = layer(blk, h)
    third = layer(blk, h)                   # the next seed of the generator: another mask
    assert len(seen) == 3 and all(k["dropout_p"] == 0.5 for k in seen)
    assert seen[0]["dropout_seed"] == seen[1]["dropout_seed"] != seen[2]["dropout_seed"]
    assert torch.equal(first, second) and not torch.equal(first, third)
    assert before.shape == first.shape
    layer.eval()                            # eval: no dropout, still the fused op
    layer(blk, h)
    assert len(seen) == 4 and "dropout_p" not in seen[3]


def test_get_attention_takes_the_composed_chain(monkeypatch):
    import torch
    seen = _calls(monkeypatch)
    blk, col, row, nd, ns = _block(False)
    composed, fused = _layers()
    h = torch.from_numpy(np.random.RandomState(73).randn(ns, IN).astype(np.float32)).cuda()
    out_c, att_c = composed(blk, h, get_attention=True)
    out_f, att_f = fused(blk, h, get_attention=True)
    assert not seen and torch.equal(out_c, out_f) and torch.equal(att_c, att_f)
    assert att_f.shape == (len(row), H, 1) and att_f.requires_grad


def test_defaults_and_state_dict():
    from gnnflow_amd import nn as gnn
    assert gnn.FUSED_GAT_DEFAULT is False and gnn.FUSED_GAT_DROPOUT_DEFAULT is False
    layer = gnn.GATConv(IN, D, H, residual=True)
    assert layer.fused_attention is False and layer.fused_attention_dropout is False
    assert sorted(layer.state_dict()) == ["attn_l", "attn_r", "bias", "fc.weight",
                                          "res_fc.weight"]
    layer.fused_attention = layer.fused_attention_dropout = True
    assert sorted(layer.state_dict()) == ["attn_l", "attn_r", "bias", "fc.weight",
                                          "res_fc.weight"]
