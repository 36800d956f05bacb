"""ops.edge_rank(..., exclude=) (csrc/edge_rank.hip, the MASKED instantiations) on the GPU: exact
equality with tests/edge_rank_exclude_ref.py on integer-valued inputs, for which every float32
summation order gives the float64 value; the empty and the full mask, mask and skip together,
garbage past C, an excluded best candidate, an excluded NaN; nn.EdgePredictor.rank around it, and
the example that filters with DynamicGraph.seen_mask."""
import os
import sys

import numpy as np
import pytest
import torch

from gnnflow_amd import nn as gnn
from gnnflow_amd import ops
from tests import edge_rank_exclude_ref as X
from tests import edge_rank_ref as R
from tests import seen_mask_ref as S

pytestmark = pytest.mark.gpu


def _dev(inp):
    return {n: torch.from_numpy(v).cuda() for n, v in inp.items()}


def _eq(t, a):
    t = t.cpu()
    return np.array_equal(t.double().numpy() if t.dtype.is_floating_point else t.numpy(),
                          np.asarray(a), equal_nan=True)


def _same(out, ref):
    v, i, g, e = ref
    assert _eq(out.values, v) and _eq(out.indices, i)
    assert out.values.dtype == torch.float32 and out.indices.dtype == torch.int64
    if g is None:
        assert out.greater is None and out.equal is None
    else:
        assert _eq(out.greater, g) and _eq(out.equal, e)
        assert out.greater.dtype == out.equal.dtype == torch.int64


@pytest.mark.parametrize("case", X.CASES, ids=X.case_id)
def test_grid_cases_are_exact(case):
    inp, score, mask = X.grid_reference(case)
    B, C, _, k = case
    d = _dev(inp)
    a = (d["src"], d["cand"], d["w"], d["bias"])
    target = inp["target"]
    ref = score[np.arange(B), target]
    d_ref = torch.from_numpy(ref.astype(np.float32)).cuda()
    d_mask = torch.from_numpy(mask).cuda()
    # the mask alone (its bits past C are all set: garbage), with and without a reference score
    _same(ops.edge_rank(*a, k=k, ref_score=d_ref, exclude=d_mask),
          X.rank(inp, k, ref, None, mask, score))
    _same(ops.edge_rank(*a, k=k, exclude=d_mask), X.rank(inp, k, None, None, mask, score))
    # the mask and a skip
    _same(ops.edge_rank(*a, k=k, ref_score=d_ref, skip=d["target"], exclude=d_mask),
          X.rank(inp, k, ref, target, mask, score))
    _same(ops.edge_rank(*a, k=k, skip=d["target"], exclude=d_mask),
          X.rank(inp, k, None, target, mask, score))
    # the same mask without the garbage gives the same bits
    clean = torch.from_numpy(X.random_mask(case, garbage=False)).cuda()
    assert C % 64 == 0 or not torch.equal(clean, d_mask)
    x = ops.edge_rank(*a, k=k, ref_score=d_ref, skip=d["target"], exclude=d_mask)
    y = ops.edge_rank(*a, k=k, ref_score=d_ref, skip=d["target"], exclude=clean)
    assert torch.equal(x.values.view(torch.int32), y.values.view(torch.int32))
    assert torch.equal(x.indices, y.indices)
    assert torch.equal(x.greater, y.greater) and torch.equal(x.equal, y.equal)


@pytest.mark.parametrize("case", X.CASES, ids=X.case_id)
def test_an_empty_mask_changes_nothing_and_a_full_one_leaves_nothing(case):
    inp, score, _ = X.grid_reference(case)
    B, C, _, k = case
    d = _dev(inp)
    a = (d["src"], d["cand"], d["w"], d["bias"])
    d_ref = torch.from_numpy(score[np.arange(B), inp["target"]].astype(np.float32)).cuda()
    zero = torch.zeros((B, (C + 63) // 64), dtype=torch.int64, device="cuda")
    for kw in (dict(ref_score=d_ref, skip=d["target"]), dict(ref_score=d_ref), dict()):
        x = ops.edge_rank(*a, k=k, exclude=zero, **kw)
        y = ops.edge_rank(*a, k=k, **kw)
        assert torch.equal(x.values.view(torch.int32), y.values.view(torch.int32))
        assert torch.equal(x.indices, y.indices)
        if "ref_score" in kw:
            assert torch.equal(x.greater, y.greater) and torch.equal(x.equal, y.equal)
        else:
            assert x.greater is None and x.equal is None
    for garbage in (False, True):
        full = torch.from_numpy(X.full_mask(B, C, garbage)).cuda()
        out = ops.edge_rank(*a, k=k, ref_score=d_ref, exclude=full)
        assert tuple(out.values.shape) == (B, k) == tuple(out.indices.shape)
        assert (out.indices == -1).all() and (out.values == float("-inf")).all()
        assert not out.greater.any() and not out.equal.any()


@pytest.mark.parametrize("D", [100, 7])
def test_full_list_with_exclusions_ends_in_the_fill(D):
    case = (33, 64, D, 64)
    inp, score, mask = X.grid_reference(case)
    d = _dev(inp)
    out = ops.edge_rank(d["src"], d["cand"], d["w"], d["bias"], k=64,
                        exclude=torch.from_numpy(mask).cuda())
    want = X.rank(inp, 64, None, None, mask, score)
    _same(out, want)
    left = X.kept(33, 64, None, mask).sum(1)
    assert 0 < left.min() and left.max() < 64
    idx = out.indices.cpu().numpy()
    for i in range(33):
        assert (idx[i, :left[i]] >= 0).all() and (idx[i, left[i]:] == -1).all()
        assert (out.values[i, left[i]:] == float("-inf")).all()


@pytest.mark.parametrize("case", [(33, 300, 100), (33, 65, 7), (1, 256, 100)], ids=R.case_id)
def test_the_excluded_candidate_is_the_best(case):
    B, C, D = case
    inp, score, _ = X.grid_reference(case)
    d = _dev(inp)
    a = (d["src"], d["cand"], d["w"], d["bias"])
    k = min(C, 10)
    plain = ops.edge_rank(*a, k=k)
    best = plain.indices[:, 0].cpu().numpy()
    assert np.array_equal(best, np.argmax(score, 1))      # argmax: the first among equal scores
    bits = np.zeros((B, (C + 63) // 64 * 64), bool)
    bits[np.arange(B), best] = True
    mask = S.pack(bits)
    ref = score[np.arange(B), best] - 1.0                 # below the best: it counted as greater
    d_ref = torch.from_numpy(ref.astype(np.float32)).cuda()
    out = ops.edge_rank(*a, k=k, ref_score=d_ref, exclude=torch.from_numpy(mask).cuda())
    _same(out, X.rank(inp, k, ref, None, mask, score))
    assert not (out.indices.cpu().numpy() == best[:, None]).any()
    with_best = ops.edge_rank(*a, k=k, ref_score=d_ref)
    assert torch.equal(out.greater, with_best.greater - 1)
    assert torch.equal(out.indices[:, :k - 1], with_best.indices[:, 1:])


@pytest.mark.parametrize("C,D,bad", [(65, 100, 64), (300, 7, 257)])
def test_an_excluded_nan_is_gone(C, D, bad):
    B = 33
    inp = R.make_grid((B, C, D))
    inp["cand"][bad, D // 2] = np.nan
    score = R.scores(inp["src"], inp["cand"], inp["w"], inp["bias"])
    assert np.isnan(score[:, bad]).all() and not np.isnan(np.delete(score, bad, 1)).any()
    d = _dev(inp)
    a = (d["src"], d["cand"], d["w"], d["bias"])
    low = torch.full((B,), float("-inf"), device="cuda")
    bits = np.zeros((B, (C + 63) // 64 * 64), bool)
    bits[::2, bad] = True                                   # every other row excludes the NaN
    bits[:, 0] = True
    mask = S.pack(bits)
    k = min(C, 64)
    out = ops.edge_rank(*a, k=k, ref_score=low, exclude=torch.from_numpy(mask).cuda())
    _same(out, X.rank(inp, k, np.full(B, -np.inf), None, mask, score))
    assert out.greater.tolist() == [C - 2] * B              # the NaN is never counted anyway
    if C <= 65:      # C - 1 or C - 2 are left: the list shows whether the NaN is among them
        idx = out.indices.cpu().numpy()
        assert not (idx[::2] == bad).any() and (idx[::2, -1] == -1).all()
        assert (idx[1::2, C - 2] == bad).all() and torch.isnan(out.values[1::2, C - 2]).all()


def test_row_slices_and_strided_masks():
    case = (33, 300, 100)
    inp, score, mask = X.grid_reference(case)
    d = _dev(inp)
    d_mask = torch.from_numpy(mask).cuda()
    whole = ops.edge_rank(d["src"], d["cand"], d["w"], d["bias"], k=10, exclude=d_mask)
    part = ops.edge_rank(d["src"][5:20], d["cand"], d["w"], d["bias"], k=10, exclude=d_mask[5:20])
    assert torch.equal(part.indices, whole.indices[5:20])
    wide = torch.full((33, 2 * d_mask.shape[1]), -1, dtype=torch.int64, device="cuda")
    wide[:, ::2] = d_mask
    strided = ops.edge_rank(d["src"], d["cand"], d["w"], d["bias"], k=10, exclude=wide[:, ::2])
    assert torch.equal(strided.indices, whole.indices)
    assert torch.equal(strided.values.view(torch.int32), whole.values.view(torch.int32))
    # a shard of the candidates at a multiple of 64 takes the mask's columns from a // 64 on
    a0, b0 = 128, 300
    shard = ops.edge_rank(d["src"], d["cand"][a0:b0], d["w"], d["bias"], k=10,
                          exclude=d_mask[:, a0 // 64:(b0 + 63) // 64])
    sub = np.ascontiguousarray(mask[:, a0 // 64:(b0 + 63) // 64])
    _same(shard, X.rank(None, 10, None, None, sub, score[:, a0:b0]))
    assert np.array_equal(X.kept(33, b0 - a0, None, sub), X.kept(33, 300, None, mask)[:, a0:b0])


def _grid_module(dim, seed):
    g = torch.Generator().manual_seed(seed)
    m = gnn.EdgePredictor(dim)
    with torch.no_grad():
        for p in m.parameters():
            p.copy_(torch.randint(-1, 2, p.shape, generator=g).float())
    return m.cuda()


def test_predictor_rank_with_exclude_fused_and_not(monkeypatch):
    dim, B, C, k = 12, 33, 300, 10
    m = _grid_module(dim, 3)
    g = torch.Generator().manual_seed(4)
    h_src = torch.randint(-2, 3, (B, dim), generator=g).float().cuda()
    h_cand = torch.randint(-2, 3, (C, dim), generator=g).float().cuda()
    target = torch.randint(0, C, (B,), generator=g).cuda()
    mask = X.random_mask((B, C, dim), garbage=True)
    t = target.cpu().numpy()
    mask[np.arange(0, B, 2), t[::2] >> 6] |= np.int64(1) << (t[::2] & 63)    # own bit set too
    d_mask = torch.from_numpy(mask).cuda()
    calls = []
    real = ops.edge_rank
    monkeypatch.setattr(ops, "edge_rank", lambda *a, **kw: calls.append(kw) or real(*a, **kw))
    assert m.fused_score
    fused = m.rank(h_src, h_cand, k=k, target=target, exclude=d_mask)
    assert len(calls) == 1 and calls[0]["exclude"] is d_mask
    m.fused_score = False
    plain = m.rank(h_src, h_cand, k=k, target=target, exclude=d_mask)
    assert len(calls) == 1
    assert torch.equal(fused.indices, plain.indices) and torch.equal(fused.values, plain.values)
    assert torch.equal(fused.greater, plain.greater) and torch.equal(fused.equal, plain.equal)
    # and both are the reference's: the target ranked among the candidates neither excluded nor it
    p = {n: v.double().cpu().numpy() for n, v in m.state_dict().items()}
    inp = dict(src=h_src.double().cpu().numpy() @ p["src_fc.weight"].T + p["src_fc.bias"],
               cand=h_cand.double().cpu().numpy() @ p["dst_fc.weight"].T + p["dst_fc.bias"],
               w=p["out_fc.weight"], bias=p["out_fc.bias"])
    score = R.scores(inp["src"], inp["cand"], inp["w"], inp["bias"])
    _same(fused, X.rank(inp, k, score[np.arange(B), t], t, mask, score))
    unmasked = m.rank(h_src, h_cand, k=k, target=target)
    assert not torch.equal(unmasked.greater, plain.greater)


def test_recommend_edges_filters_what_the_source_has_seen():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "examples"))
    try:
        import recommend_edges
    finally:
        sys.path.pop(0)
    import pandas as pd
    from gnnflow_amd import synthetic
    from gnnflow_amd.utils import build_dynamic_graph
    # the first of the last 30 edges' sources has met some thirty nodes before
    r = recommend_edges.main(batch_size=30, num_candidates=300, num_edges=4000, verbose=False,
                             filter_seen=True)
    assert 0.0 < r["mrr"] <= 1.0 and 0.0 < r["unfiltered_mrr"] <= 1.0
    assert r["mrr"] >= r["unfiltered_mrr"]      # leaving candidates out never worsens a rank
    assert 0.0 < r["seen_share"] < 1.0
    top = r["top5"]
    assert len(top) == 5 and len(set(top)) == 5
    # the first source's history, from the same graph built again
    g = synthetic.reddit_like(seed=42, num_edges=4000)
    df = pd.DataFrame({"src": g["src"], "dst": g["dst"], "time": g["ts"], "eid": g["eid"]})
    graph = build_dynamic_graph(20 << 20, 1000 << 20, "cuda", 62, 1024, "insert",
                                undirected=True, device=0, dataset_df=df)
    assert r["source"] == int(df["src"].to_numpy()[-30])
    dst, ts, _ = graph.get_temporal_neighbors(r["source"])
    earlier = set(dst[ts < np.float32(r["time"])].tolist())
    assert len(earlier) >= 10 and not earlier & set(top)
    plain = recommend_edges.main(batch_size=30, num_candidates=300, num_edges=4000, verbose=False)
    assert set(plain) == {"mrr", "hits@10", "top5", "top5_index", "num_candidates"}
