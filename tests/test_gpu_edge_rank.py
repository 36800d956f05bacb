"""ops.edge_rank (csrc/edge_rank.hip) on the GPU: exact equality with the float64 reference of
tests/edge_rank_ref.py on integer-valued inputs, bit equality with ops.edge_score on drawn ones,
the element-load path, NaN, the (-inf, -1) fill, reproducibility, streams, and
nn.EdgePredictor.rank around it."""
import os
import sys

import numpy as np
import pytest
import torch

from gnnflow_amd import nn as gnn
from gnnflow_amd import ops
from tests import edge_rank_ref as R

pytestmark = pytest.mark.gpu
CH = ops.EDGE_RANK_CHUNK


def _dev(inp):
    return {n: torch.from_numpy(v).cuda() for n, v in inp.items()}


def _eq(t, a):
    t = t.cpu()
    return np.array_equal(t.double().numpy() if t.dtype.is_floating_point else t.numpy(),
                          np.asarray(a), equal_nan=True)


@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_grid_cases_are_exact(case):
    inp, ref = R.grid_reference(case)
    d, k = _dev(inp), case[3]
    refscore = torch.from_numpy(ref.ref.astype(np.float32)).cuda()
    a = (d["src"], d["cand"], d["w"], d["bias"])
    out = ops.edge_rank(*a, k=k, ref_score=refscore, skip=d["target"])
    assert _eq(out.values, ref.values_skip) and _eq(out.indices, ref.indices_skip)
    assert _eq(out.greater, ref.greater_skip) and _eq(out.equal, ref.equal_skip)
    assert out.values.dtype == torch.float32 and out.indices.dtype == torch.int64
    assert out.greater.dtype == out.equal.dtype == torch.int64
    out = ops.edge_rank(*a, k=k, ref_score=refscore)
    assert _eq(out.values, ref.values) and _eq(out.indices, ref.indices)
    assert _eq(out.greater, ref.greater) and _eq(out.equal, ref.equal)
    out = ops.edge_rank(*a, k=k, skip=d["target"])
    assert out.greater is None and out.equal is None
    assert _eq(out.values, ref.values_skip) and _eq(out.indices, ref.indices_skip)
    out = ops.edge_rank(*a, k=0, ref_score=refscore.reshape(-1, 1), skip=d["target"])
    assert tuple(out.values.shape) == (case[0], 0) == tuple(out.indices.shape)
    assert _eq(out.greater, ref.greater_skip) and _eq(out.equal, ref.equal_skip)


def _pairwise(d, B, C):
    """ops.edge_score of every pair as [B, C]."""
    s = ops.edge_score(d["src"], d["cand"].repeat_interleave(B, 0), d["w"], d["bias"])
    return s.reshape(C, B).t().contiguous()


@pytest.mark.parametrize("case", R.DRAWN, ids=R.case_id)
def test_scores_are_edge_score_bit_for_bit(case):
    B, C, D = case
    d = _dev(R.make_drawn(case))
    k = min(C, 64)
    full = _pairwise(d, B, C)
    ref = full[:, C // 2].contiguous()
    out = ops.edge_rank(d["src"], d["cand"], d["w"], d["bias"], k=k, ref_score=ref)
    picked = full.gather(1, out.indices)
    assert torch.equal(out.values.view(torch.int32), picked.view(torch.int32))
    # and they are the k best: sorted by (value descending, index ascending), nothing better left
    order = np.lexsort((np.arange(C)[None, :].repeat(B, 0), -full.cpu().double().numpy()), axis=1)
    assert np.array_equal(out.indices.cpu().numpy(), order[:, :k])
    assert torch.equal(out.greater, (full > ref[:, None]).sum(1))
    assert torch.equal(out.equal, (full == ref[:, None]).sum(1))
    assert (out.equal >= 1).all()      # the reference's own candidate ties exactly


def test_misaligned_rows_take_the_element_path():
    B, C, D = 17, CH + 1, 132
    d = _dev(R.make_drawn((B, C, D)))
    flat = torch.empty(C * D + 1, dtype=torch.float32, device="cuda")
    shifted = flat[1:].view(C, D)      # rows start 4 bytes past a 16-byte boundary
    shifted.copy_(d["cand"])
    assert shifted.data_ptr() % 16 == 4 and shifted.is_contiguous()
    ref = torch.zeros(B, device="cuda")
    a = ops.edge_rank(d["src"], d["cand"], d["w"], d["bias"], k=64, ref_score=ref)
    b = ops.edge_rank(d["src"], shifted, d["w"], d["bias"], k=64, ref_score=ref)
    assert torch.equal(a.values.view(torch.int32), b.values.view(torch.int32))
    assert torch.equal(a.indices, b.indices)
    assert torch.equal(a.greater, b.greater) and torch.equal(a.equal, b.equal)


@pytest.mark.parametrize("C,D,bad", [(5, 100, 2), (CH + 3, 7, CH + 1)])
def test_nan_is_never_counted_and_sorts_last(C, D, bad):
    B = 5
    inp = R.make_grid((B, C, D))
    inp["cand"][bad, D // 2] = np.nan
    ref = R.Reference(inp, min(C, 64), check_ties=False)
    assert np.isnan(ref.score[:, bad]).all()
    d = _dev(inp)
    low = torch.full((B,), float("-inf"), device="cuda")
    out = ops.edge_rank(d["src"], d["cand"], d["w"], d["bias"], k=min(C, 64), ref_score=low)
    assert _eq(out.values, ref.values) and _eq(out.indices, ref.indices)
    assert out.greater.tolist() == [C - 1] * B and out.equal.tolist() == [0] * B
    if C <= 64:      # the whole set is listed: the NaN comes after every other candidate
        assert out.indices[:, -1].tolist() == [bad] * B and torch.isnan(out.values[:, -1]).all()
    else:
        assert not (out.indices == bad).any()
    nan_ref = torch.full((B,), float("nan"), device="cuda")
    out = ops.edge_rank(d["src"], d["cand"], d["w"], d["bias"], ref_score=nan_ref)
    assert out.greater.tolist() == [0] * B and out.equal.tolist() == [0] * B


def test_full_list_with_a_skip_ends_in_the_fill():
    case = (5, 40, 100, 40)
    inp = R.make_grid(case)
    ref = R.Reference(inp, 40)
    d = _dev(inp)
    a = (d["src"], d["cand"], d["w"], d["bias"])
    out = ops.edge_rank(*a, k=40, skip=d["target"])
    assert _eq(out.values, ref.values_skip) and _eq(out.indices, ref.indices_skip)
    assert out.indices[:, -1].tolist() == [-1] * 5
    assert (out.values[:, -1] == float("-inf")).all()
    for far in (-1, 40, 2 ** 40):      # out of range: nothing is excluded
        skip = torch.full((5,), far, dtype=torch.int64, device="cuda")
        out = ops.edge_rank(*a, k=40, skip=skip)
        assert _eq(out.values, ref.values) and _eq(out.indices, ref.indices)


def test_reproducible_streams_and_empty():
    d = _dev(R.make_drawn((33, 2 * CH + 1, 100)))
    ref = torch.zeros(33, device="cuda")
    a = (d["src"], d["cand"], d["w"], d["bias"])
    first = ops.edge_rank(*a, k=64, ref_score=ref)
    again = ops.edge_rank(*a, k=64, ref_score=ref)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        other = ops.edge_rank(*a, k=64, ref_score=ref)
    side.synchronize()
    for o in (again, other):
        assert torch.equal(first.values.view(torch.int32), o.values.view(torch.int32))
        assert torch.equal(first.indices, o.indices)
        assert torch.equal(first.greater, o.greater) and torch.equal(first.equal, o.equal)
    empty = ops.edge_rank(d["src"][:0], d["cand"], d["w"], d["bias"], k=3, ref_score=ref[:0])
    assert tuple(empty.values.shape) == (0, 3) and tuple(empty.greater.shape) == (0,)
    nothing = ops.edge_rank(*a)
    assert tuple(nothing.values.shape) == (33, 0) and nothing.greater is None


def _grid_module(dim, seed):
    g = torch.Generator().manual_seed(seed)
    m = gnn.EdgePredictor(dim)
    with torch.no_grad():
        for p in m.parameters():
            p.copy_(torch.randint(-1, 2, p.shape, generator=g).float())
    return m.cuda()


def test_predictor_rank_fused_and_not(monkeypatch):
    dim, B, C, k = 12, 17, CH + 5, 10
    m = _grid_module(dim, 3)
    g = torch.Generator().manual_seed(4)
    h_src = torch.randint(-2, 3, (B, dim), generator=g).float().cuda()
    h_cand = torch.randint(-2, 3, (C, dim), generator=g).float().cuda()
    target = torch.randint(0, C, (B,), generator=g).cuda()
    calls = []
    real = ops.edge_rank
    monkeypatch.setattr(ops, "edge_rank", lambda *a, **kw: calls.append(1) or real(*a, **kw))
    assert m.fused_score
    fused = m.rank(h_src, h_cand, k=k, target=target)
    assert len(calls) == 1
    m.fused_score = False
    plain = m.rank(h_src, h_cand, k=k, target=target)
    assert len(calls) == 1
    assert torch.equal(fused.values, plain.values) and torch.equal(fused.indices, plain.indices)
    assert torch.equal(fused.greater, plain.greater) and torch.equal(fused.equal, plain.equal)
    # the reference: equal counts the OTHER ties only, never the target itself
    p = {n: v.double().cpu().numpy() for n, v in m.state_dict().items()}
    inp = dict(src=h_src.double().cpu().numpy() @ p["src_fc.weight"].T + p["src_fc.bias"],
               cand=h_cand.double().cpu().numpy() @ p["dst_fc.weight"].T + p["dst_fc.bias"],
               w=p["out_fc.weight"], bias=p["out_fc.bias"], target=target.cpu().numpy())
    ref = R.Reference(inp, k, check_ties=False)
    assert _eq(fused.equal, ref.equal_skip) and _eq(fused.greater, ref.greater_skip)
    assert (fused.equal[torch.from_numpy(ref.equal_skip == 0).cuda()] == 0).all()
    assert _eq(fused.values, ref.values_skip) and _eq(fused.indices, ref.indices_skip)


def test_recommend_edges_example():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "examples"))
    try:
        import recommend_edges
    finally:
        sys.path.pop(0)
    r = recommend_edges.main(batch_size=40, num_candidates=300, num_edges=4000, verbose=False)
    assert 0.0 < r["mrr"] <= 1.0 and 0.0 <= r["hits@10"] <= 1.0
    top = r["top5_index"]
    assert len(top) == 5 and len(set(top)) == 5
    assert all(0 <= i < r["num_candidates"] for i in top)
