"""nn.TemporalAttentionLayer.fused_attention_dropout: the default routing is unchanged, the
switch sends training with attention dropout through ops.block_attention(dropout_p=, dropout_seed=)
with a seed from torch's CPU generator, and output and parameter gradients match a float64
plain-torch restatement that applies the same (numpy) mask."""
import numpy as np
import pytest

from tests import attention_dropout_ref as R

pytestmark = pytest.mark.gpu

DIM_OUT, HEADS = 24, 2
CONFIGS = [(32, 16, 20), (0, 16, 0)]
P = 0.5


def _sampled_block():
    """The small sampler block of tests/test_gpu_temporal_attention_layer.py."""
    from gnnflow_amd import DynamicGraph, TemporalSampler
    rng = np.random.RandomState(20)
    N, E = 300, 5000
    src, dst = rng.randint(0, N, E), rng.randint(0, N, E)
    ts = np.sort(rng.rand(E)).astype(np.float32)
    g = DynamicGraph(1 << 20, 64 << 20, "cuda", 16, 64, "insert")
    g.add_edges(src.astype(np.int64), dst.astype(np.int64), ts, add_reverse=True)
    rng = np.random.RandomState(24)
    b = TemporalSampler(g, [10], "recent").sample(
        rng.randint(0, N, 120).astype(np.int64), rng.uniform(0.6, 1.0, 120).astype(np.float32))[0][0]
    assert b.num_edges() > 0 and b.segments()[1] is None and b.segments()[2] is None
    return b


def _layer_and_block(cfg=(32, 16, 20), att_dropout=P):
    import torch
    from gnnflow_amd import nn as gnn
    b = _sampled_block()
    rng = np.random.RandomState(70 + sum(cfg))
    h = torch.from_numpy(rng.randn(b.num_src_nodes(), max(cfg[0], 1)).astype(np.float32))
    f = torch.from_numpy(rng.randn(b.num_edges(), max(cfg[1], 1)).astype(np.float32))
    if cfg[0]:
        b.srcdata['h'] = h.cuda()
    if cfg[1]:
        b.edata['f'] = f.cuda()
    torch.manual_seed(71)
    layer = gnn.TemporalAttentionLayer(*cfg, DIM_OUT, HEADS, 0.0, att_dropout).cuda()
    return layer, b, h, f


def _spy(monkeypatch):
    from gnnflow_amd import ops
    fused, softmax = [], []
    real_f, real_s = ops.block_attention, ops.edge_softmax
    monkeypatch.setattr(ops, "block_attention",
                        lambda *a, **k: fused.append(k) or real_f(*a, **k))
    monkeypatch.setattr(ops, "edge_softmax", lambda *a, **k: softmax.append(1) or real_s(*a, **k))
    return fused, softmax


def test_routing_default_and_switch(monkeypatch):
    import torch
    from gnnflow_amd import nn as gnn
    assert gnn.FUSED_ATTENTION_DROPOUT_DEFAULT is False
    layer, b, _, _ = _layer_and_block()
    assert layer.fused_attention_dropout is gnn.FUSED_ATTENTION_DROPOUT_DEFAULT
    assert "fused_attention_dropout" not in layer.state_dict()
    fused, softmax = _spy(monkeypatch)
    layer.train()
    layer(b)                                   # the default: the composed chain, as before
    assert not fused and len(softmax) == 1
    layer.fused_attention_dropout = True
    out = layer(b)
    assert out.shape == (b.num_dst_nodes(), DIM_OUT) and bool(torch.isfinite(out).all())
    assert len(fused) == 1 and len(softmax) == 1
    assert fused[0]["dropout_p"] == P and isinstance(fused[0]["dropout_seed"], int)
    assert 0 <= fused[0]["dropout_seed"] < 2 ** 63
    layer.fused_attention = False              # the switch alone does not take the fused op
    layer(b)
    assert len(fused) == 1 and len(softmax) == 2


def test_eval_mode_passes_no_dropout(monkeypatch):
    import torch
    layer, b, _, _ = _layer_and_block()
    layer.eval()
    want = layer(b)
    fused, softmax = _spy(monkeypatch)
    layer.fused_attention_dropout = True
    got = layer(b)
    assert len(fused) == 1 and not softmax
    assert "dropout_p" not in fused[0] and "dropout_seed" not in fused[0]
    assert torch.equal(got, want)
    layer.train()
    layer.att_dropout.p = 0.0                  # training without attention dropout: likewise
    layer(b)
    assert len(fused) == 2 and "dropout_p" not in fused[1]


def test_reproducible_under_manual_seed(monkeypatch):
    import torch
    layer, b, _, _ = _layer_and_block()
    layer.fused_attention_dropout = True
    layer.train()
    fused, _ = _spy(monkeypatch)
    torch.manual_seed(5)
    first, again = layer(b), layer(b)
    torch.manual_seed(5)
    second = layer(b)
    seeds = [k["dropout_seed"] for k in fused]
    assert seeds[0] == seeds[2] and seeds[0] != seeds[1]       # consecutive forwards: new seeds
    assert torch.equal(first, second) and not torch.equal(first, again)


def _reference64(cfg, params, h, f, dt, row, R_, G, w):
    """The reference's forward in float64 plain torch on the CPU with the attention weights
    multiplied by w [E, HEADS]; returns (out, {param: grad})."""
    import torch
    import torch.nn.functional as F
    dn, de, dtm = cfg
    p = {k: v.detach().double().cpu().requires_grad_(True) for k, v in params.items()}
    E = len(row)

    def time_enc(x):
        return torch.cos(x.reshape(-1, 1) @ p["time_enc.w.weight"].T + p["time_enc.w.bias"])

    def lin(name, x):
        return x @ p[name + ".weight"].T + p[name + ".bias"]

    empty_e = torch.zeros((E, 0), dtype=torch.float64)
    empty_r = torch.zeros((R_, 0), dtype=torch.float64)
    tgt = h[:R_] if dn else (empty_r if dtm else torch.ones((R_, DIM_OUT), dtype=torch.float64))
    srcs = h[R_:] if dn else empty_e
    ef = f if de else empty_e
    tf = time_enc(dt) if dtm else empty_e
    zf = time_enc(torch.zeros(R_, dtype=torch.float64)) if dtm else empty_r
    Q = torch.cat([tgt, zf], 1)
    Q = lin("w_q", Q) if (dn or dtm) else Q
    KV = torch.cat([srcs, ef, tf], 1)
    Q = Q[row].reshape(E, HEADS, -1)
    K = lin("w_k", KV).reshape(E, HEADS, -1)
    V = lin("w_v", KV).reshape(E, HEADS, -1)
    s = F.leaky_relu((Q * K).sum(2), 0.2)
    idx = row[:, None].expand(E, HEADS)
    m = torch.full((R_, HEADS), -float("inf"), dtype=torch.float64).scatter_reduce(
        0, idx, s.detach(), "amax")
    ex = torch.exp(s - m[row])
    att = ex / torch.zeros((R_, HEADS), dtype=torch.float64).index_add_(0, row, ex)[row]
    att = att * w
    agg = torch.zeros((R_, DIM_OUT), dtype=torch.float64).index_add_(
        0, row, (V * att[:, :, None]).reshape(E, -1))
    rst = lin("w_out", torch.cat([agg, tgt], 1) if dn else agg)
    out = F.layer_norm(F.relu(rst), (DIM_OUT,), p["layer_norm.weight"], p["layer_norm.bias"])
    (out * G).sum().backward()
    return out.detach().numpy(), {k: v.grad.numpy() for k, v in p.items() if v.grad is not None}


@pytest.mark.parametrize("cfg", CONFIGS, ids=["{}_{}_{}".format(*c) for c in CONFIGS])
def test_parameter_gradients_match_float64_reference(cfg, monkeypatch):
    """Tolerance per tensor: 4 x the largest fp32-vs-float64 difference of the COMPOSED path fed
    the SAME mask on the same inputs (the rule of test_layer_matches_float64_reference).  Prints
    both differences."""
    import torch
    import torch.nn as tnn
    layer, b, h, f = _layer_and_block(cfg)
    layer.dropout.p = 0.0
    layer.train()
    Rn, E = b.num_dst_nodes(), b.num_edges()
    G = torch.from_numpy(np.random.RandomState(72).randn(Rn, DIM_OUT).astype(np.float32))
    params = dict(layer.named_parameters())
    fused_calls, softmax = _spy(monkeypatch)

    def run():
        layer.zero_grad()
        out = layer(b)
        (out * G.cuda()).sum().backward()
        return out.detach().cpu().numpy(), {k: v.grad.cpu().numpy() for k, v in params.items()
                                            if v.grad is not None}

    layer.fused_attention_dropout = True
    torch.manual_seed(73)
    got, got_g = run()
    assert len(fused_calls) == 1 and not softmax
    seed = fused_calls[0]["dropout_seed"]
    keep = R.keep_mask(E, HEADS, P, seed)          # a sampler block: grouped order = edge order
    assert 0.3 < keep.mean() < 0.7
    want, want_g = _reference64(
        cfg, params, h.double(), f.double(), b.edata['dt'].double().cpu(), b.edges()[1].cpu(), Rn,
        G.double(), torch.from_numpy(keep.astype(np.float64) / (1.0 - P)))

    class FixedMask(tnn.Module):                   # the composed chain with the same mask
        p = P

        def forward(self, att):
            return att * torch.from_numpy(np.where(keep, R.scale(P), np.float32(0))).cuda()

    layer.att_dropout = FixedMask()
    layer.fused_attention = False
    comp, comp_g = run()
    assert len(fused_calls) == 1 and len(softmax) == 1
    assert set(want_g) == set(got_g) == set(comp_g)

    def errs(out, grads):
        e = {"out": np.abs(out - want).max()}
        e.update({k: np.abs(grads[k] - want_g[k]).max() for k in want_g})
        return e

    fused, composed = errs(got, got_g), errs(comp, comp_g)
    print("\n[fp32 - float64] {}: composed max {:.3g}, fused max {:.3g}".format(
        "_".join(map(str, cfg)), max(composed.values()), max(fused.values())))
    for k in fused:
        assert composed[k] > 0 or fused[k] == 0, k
        assert fused[k] <= 4 * composed[k], "{}: fused {:.3g} > 4 x composed {:.3g}".format(
            k, fused[k], composed[k])
