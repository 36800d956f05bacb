"""GPU: ops.patch_project / ops.patch_project_time against the definition in numpy float64, forward
and both gradients, and DyGFormer(fused_patches=True) against the torch route.

The bound is a priori, not tuned: a float32 sum of n products in ANY order (the MFMA's included)
is within (n + 2) * 2^-24 * (sum |terms| + |bias|) of the exact value, |terms| summed in float64;
n = P * d for out and the number of patches for dweight and dbias.  It is asserted per element;
where every term is zero the bound is zero and the result must be exact.  For the time form the
reference's rows are ops.time_encode's own float32 values, widened: the comparison is about the
projection, not about cosf at 1e6 rad.

Lengths: random in [0, L]; with R >= 3 rows 0 and 1 are 0 and L and the last row is L - 1, which
cuts a patch whenever P > 1.  With R == 2 rows 0 and 1 are L and L - 1: 0, L and a cut patch do
not fit into two rows, and the cut is what P == L is there for; no R == 2 shape then has a wholly
padded patch: the patch that is exactly bias is covered by every shape with R >= 3 (row 0) and
by test_exact_properties."""
import numpy as np
import pytest
import torch

from tests import synth

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
SHAPES = [(1, 2, 1, 1, 1), (3, 8, 2, 3, 17), (5, 32, 1, 172, 50), (2, 32, 32, 6, 50),
          (9, 16, 4, 50, 128), (2, 4, 4, 1024, 16), (70, 4, 1, 8, 16), (40, 512, 2, 4, 8)]
CASES = [(s, "table") for s in SHAPES] + [(SHAPES[i], "time") for i in (1, 2, 6)]
TABLE_ROWS = 23


def _inputs(shape, form, seed=0):
    R, L, P, d, C = shape
    rng = np.random.default_rng(seed)
    lengths = rng.integers(0, L + 1, size=R).astype(np.int32)
    if R >= 3:
        lengths[0], lengths[1], lengths[-1] = 0, L, L - 1
    elif R == 2:
        lengths[0], lengths[1] = L, L - 1
    t = dict(lengths=torch.from_numpy(lengths).cuda(),
             weight=torch.from_numpy(rng.standard_normal((C, P * d), np.float32)).cuda(),
             bias=torch.from_numpy(rng.standard_normal(C, np.float32)).cuda(),
             dout=torch.from_numpy(rng.standard_normal((R, L // P, C), np.float32)).cuda())
    if form == "table":
        t["ids"] = torch.from_numpy(rng.integers(-2, TABLE_ROWS + 2, size=(R, L))).cuda()
        t["table"] = torch.from_numpy(rng.standard_normal((TABLE_ROWS, d), np.float32)).cuda()
    else:
        t["delta_t"] = torch.from_numpy(rng.uniform(0, 1e6, size=(R, L)).astype(np.float32)).cuda()
        t["time_weight"] = torch.from_numpy(
            (1 / 10 ** np.linspace(0, 9, d)).astype(np.float32).reshape(d, 1)).cuda()
        t["time_bias"] = torch.from_numpy(rng.standard_normal(d, np.float32)).cuda()
    return t


def _run(t, P, lengths="given", need=(True, True)):
    """(out, dweight, dbias) of the op on the tensors of _inputs"""
    from gnnflow_amd import ops
    w = t["weight"].clone().requires_grad_(need[0])
    b = t["bias"].clone().requires_grad_(need[1])
    lens = t["lengths"] if lengths == "given" else lengths
    if "ids" in t:
        out = ops.patch_project(t["ids"], lens, t["table"], w, b, P)
    else:
        out = ops.patch_project_time(t["delta_t"], lens, t["time_weight"], t["time_bias"], w, b, P)
    out.backward(t["dout"])
    return out.detach(), w.grad, b.grad


def _rows(t):
    """float64 [R, L, d]: the unmasked rows x of the definition"""
    from gnnflow_amd import ops
    if "ids" in t:
        ids, table = t["ids"].cpu().numpy(), t["table"].cpu().numpy().astype(np.float64)
        known = (ids >= 0) & (ids < len(table))
        return table[np.clip(ids, 0, len(table) - 1)] * known[..., None]
    enc = ops.time_encode(t["delta_t"].reshape(-1), t["time_weight"], t["time_bias"])
    return enc.cpu().numpy().astype(np.float64).reshape(tuple(t["delta_t"].shape) + (-1,))


def _worst(got, ref, bound):
    got = got.cpu().numpy().astype(np.float64)
    assert np.isfinite(got).all()
    err = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err == 0, 0.0, err / bound)      # err > 0 on a zero bound: inf
    return float(ratio.max())


@pytest.mark.parametrize("shape,form", CASES, ids=lambda v: "x".join(map(str, v))
                         if isinstance(v, tuple) else v)
def test_against_float64(shape, form):
    from gnnflow_amd import _capi, ops
    R, L, P, d, C = shape
    t = _inputs(shape, form)
    out, gw, gb = _run(t, P)
    assert tuple(out.shape) == (R, L // P, C)
    lengths = t["lengths"].cpu().numpy()
    assert P == 1 or (lengths % P != 0).any()
    filled = np.arange(L)[None, :] < lengths[:, None]
    x = (_rows(t) * filled[..., None]).reshape(R * (L // P), P * d)
    w, b = (t[k].cpu().numpy().astype(np.float64) for k in ("weight", "bias"))
    g = t["dout"].cpu().numpy().astype(np.float64).reshape(-1, C)
    M = len(x)
    worst = {
        "out": _worst(out.reshape(M, C), x @ w.T + b,
                      (P * d + 2) * U * (np.abs(x) @ np.abs(w).T + np.abs(b))),
        "dweight": _worst(gw, g.T @ x, (M + 2) * U * (np.abs(g).T @ np.abs(x))),
        "dbias": _worst(gb, g.sum(0), (M + 2) * U * np.abs(g).sum(0)),
    }
    print("\n[error / bound] " + "  ".join("{} {:.3g}".format(k, v) for k, v in worst.items()))
    assert all(v <= 1.0 for v in worst.values()), worst
    if shape == SHAPES[-1]:
        rows = ops._common._partial_rows(_capi.load().gf_patch_project_backward_partial_rows,
                                         M, C, P * d)
        assert rows > 1


def _bits(tensors):
    return [x.view(torch.int32) for x in tensors]


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(_bits(a), _bits(b)))


def test_exact_properties():
    shape = R, L, P, d, C = (6, 8, 2, 8, 20)
    t = _inputs(shape, "table", seed=3)
    first = _run(t, P)
    assert _same(first, _run(t, P))                               # run to run
    assert int(t["lengths"][0]) == 0                             # wholly past lengths: bias
    assert torch.equal(first[0][0], t["bias"].expand(L // P, C))
    t["table"][5] = 0                                             # no row == a row of zeros
    ids = t["ids"]
    zeroed = dict(t, ids=torch.where((ids < 0) | (ids >= TABLE_ROWS), torch.full_like(ids, 5), ids))
    assert not torch.equal(zeroed["ids"], ids)
    assert _same(_run(t, P), _run(zeroed, P))
    flat = torch.zeros(TABLE_ROWS * d + 4, device="cuda")         # 4 bytes off a 16-byte boundary
    shifted = flat[1:1 + TABLE_ROWS * d].view(TABLE_ROWS, d).copy_(t["table"])
    assert shifted.data_ptr() % 16 == 4 and t["table"].data_ptr() % 16 == 0
    assert _same(_run(t, P), _run(dict(t, table=shifted), P))
    full = torch.full((R,), L, dtype=torch.int32, device="cuda")
    assert _same(_run(t, P, lengths=None), _run(t, P, lengths=full))
    out, gw, gb = _run(t, P)                                      # one gradient at a time
    only_w, only_b = _run(t, P, need=(True, False)), _run(t, P, need=(False, True))
    assert only_w[2] is None and only_b[1] is None
    assert _same((out, gw), only_w[:2]) and _same((out, gb), (only_b[0], only_b[2]))


def test_dygformer_fused_patches_agrees_with_the_torch_route():
    import gnnflow_amd
    from gnnflow_amd.models import DyGFormer
    num_nodes, num_edges, rows = 300, 4000, 120
    src, dst, ts, eid = synth.powerlaw_graph(num_nodes, num_edges, seed=9, tie_levels=500)
    graph = gnnflow_amd.DynamicGraph(1 << 20, 1 << 28, "cuda", 8, 128, "insert")
    synth.ingest_chunks(graph, src, dst, ts, eid, 1500, add_reverse=True)
    q_src, qts = synth.random_roots(num_nodes, rows, 1000.0, seed=4, extra_ids=(-1, num_nodes))
    q_dst, _ = synth.random_roots(num_nodes, rows, 1000.0, seed=5, extra_ids=(3, 4, -2))
    q = [torch.from_numpy(a).cuda() for a in (q_src, q_dst, qts)]
    torch.manual_seed(0)
    tables = (torch.randn(num_nodes - 40, 8, device="cuda"),
              torch.randn(num_edges - 500, 6, device="cuda"))
    kw = dict(dim_node=8, dim_edge=6, dim_time=10, channel_dim=12, patch_size=2, max_length=8,
              dropout=0.0)
    grads = {}
    for fused in (False, True):
        torch.manual_seed(1)
        model = DyGFormer(fused_patches=fused, **kw).cuda()
        score = model.forward_graph(graph, *q, *tables)
        if fused:      # forward()'s fused branch on neighbor_cooccurrence's planes: the same bits
            c = graph.neighbor_cooccurrence(*q, length=8, include_self=True)
            again = model(c.nodes, c.eids, q[2][:, None, None] - c.times, c.counts, c.lengths,
                          *tables)
            assert torch.equal(again.view(torch.int32), score.detach().view(torch.int32))
        score.square().mean().backward()
        grads[fused] = (score.detach(), [model.proj[n].weight.grad for n in model.channels])
    # the derived bound carried through the encoder loosely: O(1) scores, float32 sums
    tol = dict(rtol=1e-4, atol=1e-5)
    assert torch.allclose(grads[True][0], grads[False][0], **tol)
    for a, b in zip(grads[True][1], grads[False][1]):
        assert a.abs().sum() > 0 and torch.allclose(a, b, **tol)
    learn = DyGFormer(fused_patches=True, learn_time=True, **kw).cuda()
    learn.forward_graph(graph, *q, *tables).square().sum().backward()
    for p in learn.time_enc.parameters():
        assert p.grad is not None and p.grad.abs().sum() > 0
