"""gnnflow_amd.nn.TemporalAttentionLayer: state-dict names and shapes against the reference's
own (a recorded fixture), and on the GPU its output and parameter gradients against a float64
plain-torch restatement of the reference's formula, fused and composed paths."""
import json
import os

import numpy as np
import pytest

CONFIGS = [(32, 16, 20), (0, 16, 20), (32, 0, 0), (0, 16, 0)]
IDS = ["{}_{}_{}".format(*c) for c in CONFIGS]
DIM_OUT, HEADS = 24, 2
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                       "temporal_attention_state_dict.json")


@pytest.mark.parametrize("cfg", CONFIGS, ids=IDS)
def test_state_dict_matches_the_reference_fixture(cfg):
    import gnnflow_amd
    from gnnflow_amd import nn as gnn
    with open(FIXTURE) as f:
        fix = json.load(f)
    assert (fix["dim_out"], fix["num_head"]) == (DIM_OUT, HEADS)
    assert gnn.TransfomerAttentionLayer is gnn.TemporalAttentionLayer
    assert gnnflow_amd.TemporalAttentionLayer is gnn.TemporalAttentionLayer
    assert gnnflow_amd.TimeEncode is gnn.TimeEncode
    layer = gnn.TemporalAttentionLayer(*cfg, DIM_OUT, HEADS, 0.1, 0.1)
    got = {k: list(v.shape) for k, v in layer.state_dict().items()}
    assert got == fix["configs"]["{}_{}_{}".format(*cfg)]


def test_time_encode_initialisation():
    import torch
    from gnnflow_amd import nn as gnn
    te = gnn.TimeEncode(20)
    want = 1 / 10 ** np.linspace(0, 9, 20, dtype=np.float32)
    assert np.array_equal(te.w.weight.detach().numpy().ravel(), want)
    assert not te.w.bias.detach().numpy().any()
    dt = torch.tensor([0.0, 1.5, 300.0])
    assert torch.equal(te(dt), torch.cos(dt[:, None] * te.w.weight.T + te.w.bias))


def test_layer_without_edges_returns_zeros():
    import torch
    from gnnflow_amd import MFGBlock
    from gnnflow_amd import nn as gnn
    b = MFGBlock(5, 5, torch.zeros(0, dtype=torch.int64), torch.zeros(0, dtype=torch.int64))
    out = gnn.TemporalAttentionLayer(32, 16, 20, DIM_OUT, HEADS, 0.1, 0.1)(b)
    assert out.shape == (5, DIM_OUT) and not out.any()


# ---- GPU ------------------------------------------------------------------------------------------
def _sampled_block():
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


def _reference64(cfg, params, h, f, dt, row, R, G):
    """The reference's forward in float64 plain torch on the CPU; returns (out, {param: grad})."""
    import torch
    import torch.nn.functional as F
    dn, de, dtm = cfg
    p = {k: v.detach().double().cpu().requires_grad_(True) for k, v in params.items()}
    E = len(row)

    def time_enc(x):
        return torch.cos(x.reshape(-1, 1) @ p["time_enc.w.weight"].T + p["time_enc.w.bias"])

    def lin(name, x):
        return x @ p[name + ".weight"].T + p[name + ".bias"]

    empty_e, empty_r = torch.zeros((E, 0), dtype=torch.float64), torch.zeros((R, 0), dtype=torch.float64)
    tgt = h[:R] if dn else (empty_r if dtm else torch.ones((R, DIM_OUT), dtype=torch.float64))
    srcs = h[R:] if dn else empty_e
    ef = f if de else empty_e
    tf = time_enc(dt) if dtm else empty_e
    zf = time_enc(torch.zeros(R, dtype=torch.float64)) if dtm else empty_r
    Q = torch.cat([tgt, zf], 1)
    Q = lin("w_q", Q) if (dn or dtm) else Q
    KV = torch.cat([srcs, ef, tf], 1)
    Q = Q[row].reshape(E, HEADS, -1)
    K = lin("w_k", KV).reshape(E, HEADS, -1)
    V = lin("w_v", KV).reshape(E, HEADS, -1)
    s = F.leaky_relu((Q * K).sum(2), 0.2)
    idx = row[:, None].expand(E, HEADS)
    m = torch.full((R, HEADS), -float("inf"), dtype=torch.float64).scatter_reduce(
        0, idx, s.detach(), "amax")
    ex = torch.exp(s - m[row])
    att = ex / torch.zeros((R, HEADS), dtype=torch.float64).index_add_(0, row, ex)[row]
    agg = torch.zeros((R, DIM_OUT), dtype=torch.float64).index_add_(
        0, row, (V * att[:, :, None]).reshape(E, -1))
    rst = lin("w_out", torch.cat([agg, tgt], 1) if dn else agg)
    out = F.layer_norm(F.relu(rst), (DIM_OUT,), p["layer_norm.weight"], p["layer_norm.bias"])
    (out * G).sum().backward()
    return out.detach().numpy(), {k: v.grad.numpy() for k, v in p.items() if v.grad is not None}


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", CONFIGS, ids=IDS)
def test_layer_matches_float64_reference(cfg, monkeypatch):
    """Tolerance per tensor: 4 x the largest fp32-vs-float64 difference of the COMPOSED path on
    the same inputs (the fused path reorders sums).  Prints both differences."""
    import torch
    from gnnflow_amd import nn as gnn
    from gnnflow_amd import ops
    dn, de, dtm = cfg
    b = _sampled_block()
    R, E, ns = b.num_dst_nodes(), b.num_edges(), b.num_src_nodes()
    rng = np.random.RandomState(60 + dn + de + dtm)
    h = torch.from_numpy(rng.randn(ns, max(dn, 1)).astype(np.float32))
    f = torch.from_numpy(rng.randn(E, max(de, 1)).astype(np.float32))
    G = torch.from_numpy(rng.randn(R, DIM_OUT).astype(np.float32))
    if dn:
        b.srcdata['h'] = h.cuda()
    if de:
        b.edata['f'] = f.cuda()
    torch.manual_seed(61)
    layer = gnn.TemporalAttentionLayer(dn, de, dtm, DIM_OUT, HEADS, 0.0, 0.3).cuda().eval()
    params = dict(layer.named_parameters())
    row = b.edges()[1].cpu()
    want, want_g = _reference64(cfg, params, h.double(), f.double(), b.edata['dt'].double().cpu(),
                                row, R, G.double())

    calls = []
    real = ops.block_attention
    monkeypatch.setattr(ops, "block_attention", lambda *a, **k: calls.append(1) or real(*a, **k))

    def run(fused):
        layer.fused_attention = fused
        layer.zero_grad()
        out = layer(b)
        (out * G.cuda()).sum().backward()
        err = {"out": np.abs(out.detach().cpu().numpy() - want).max()}
        for k, v in params.items():
            err[k] = np.abs(v.grad.cpu().numpy() - want_g[k]).max() if v.grad is not None else 0.0
        return err

    composed = run(False)
    assert not calls
    fused = run(True)                      # eval mode: the fused op
    assert len(calls) == 1
    assert set(want_g) == {k for k, v in params.items() if v.grad is not None}
    print("\n[fp32 - float64] {}: composed max {:.3g}, fused max {:.3g}".format(
        "_".join(map(str, cfg)), max(composed.values()), max(fused.values())))
    for k in fused:
        assert composed[k] > 0 or fused[k] == 0, k
        assert fused[k] <= 4 * composed[k], "{}: fused {:.3g} > 4 x composed {:.3g}".format(
            k, fused[k], composed[k])


@pytest.mark.gpu
def test_training_with_attention_dropout_takes_the_composed_path(monkeypatch):
    import torch
    from gnnflow_amd import nn as gnn
    from gnnflow_amd import ops
    b = _sampled_block()
    b.srcdata['h'] = torch.randn(b.num_src_nodes(), 32, device="cuda")
    b.edata['f'] = torch.randn(b.num_edges(), 16, device="cuda")
    layer = gnn.TemporalAttentionLayer(32, 16, 20, DIM_OUT, HEADS, 0.1, 0.5).cuda()
    fused, softmax = [], []
    real_f, real_s = ops.block_attention, ops.edge_softmax
    monkeypatch.setattr(ops, "block_attention", lambda *a, **k: fused.append(1) or real_f(*a, **k))
    monkeypatch.setattr(ops, "edge_softmax", lambda *a, **k: softmax.append(1) or real_s(*a, **k))
    layer.train()
    out = layer(b)
    assert out.shape == (b.num_dst_nodes(), DIM_OUT) and bool(torch.isfinite(out).all())
    assert not fused and len(softmax) == 1
    layer.eval()
    layer(b)
    assert len(fused) == 1 and len(softmax) == 1
    layer.train()
    layer.att_dropout.p = 0.0              # no attention dropout: fused also in training
    layer(b)
    assert len(fused) == 2 and len(softmax) == 1
