"""CPU tests of the edge_rank reference (tests/edge_rank_ref.py) against a hand-worked case, and of
nn.EdgePredictor.rank's torch path against the reference with exact equality on integer-valued
weights and embeddings."""
import numpy as np
import pytest
import torch

from gnnflow_amd import nn as gnn
from gnnflow_amd import ops
from tests import edge_rank_ref as R


def test_reference_on_a_hand_worked_case():
    # relu([1, -1] + cand) . [2, -1] + 1:  c0 (1, 0) -> 3, c1 (2, 1) -> 4, c2 (0, 2) -> -1, c3 = c0
    src = np.array([[1., -1.]])
    cand = np.array([[0., 0.], [1., 2.], [-2., 3.], [0., 0.]])
    s = R.scores(src, cand, [2., -1.], [1.])
    assert s.tolist() == [[3., 4., -1., 3.]]
    assert [a.tolist() for a in R.counts(s, [3.])] == [[1], [2]]
    assert [a.tolist() for a in R.counts(s, [3.], skip=[0])] == [[1], [1]]
    assert [a.tolist() for a in R.counts(s, [np.nan])] == [[0], [0]]
    v, i = R.topk(s, 3)
    assert v.tolist() == [[4., 3., 3.]] and i.tolist() == [[1, 0, 3]]
    v, i = R.topk(s, 4, skip=[0])
    assert v.tolist() == [[4., 3., -1., -np.inf]] and i.tolist() == [[1, 3, 2, -1]]
    s[0, 1] = np.nan      # a NaN is last, below -inf, and never counted
    s[0, 2] = -np.inf
    v, i = R.topk(s, 4)
    assert i.tolist() == [[0, 3, 2, 1]] and np.isnan(v[0, 3]) and v[0, 2] == -np.inf
    assert [a.tolist() for a in R.counts(s, [-np.inf])] == [[2], [1]]


def test_constants_match_the_header():
    assert ops.EDGE_RANK_CHUNK == R.CH and ops.EDGE_RANK_MAX_K == R.MAX_K == 64


def test_every_grid_case_has_its_ties():
    for case in R.CASES:
        R.grid_reference(case)      # Reference asserts them


def _grid_module(dim, seed):
    g = torch.Generator().manual_seed(seed)
    m = gnn.EdgePredictor(dim)
    with torch.no_grad():
        for p in m.parameters():
            p.copy_(torch.randint(-1, 2, p.shape, generator=g).float())
    return m


def _module_reference(m, h_src, h_cand, target, k):
    p = {n: v.detach().double().numpy() for n, v in m.state_dict().items()}
    src = h_src.double().numpy() @ p["src_fc.weight"].T + p["src_fc.bias"]
    cand = h_cand.double().numpy() @ p["dst_fc.weight"].T + p["dst_fc.bias"]
    inp = dict(src=src, cand=cand, w=p["out_fc.weight"], bias=p["out_fc.bias"], target=target)
    return R.Reference(inp, k, check_ties=False)


def _equal(t, a):
    a = np.asarray(a)
    return np.array_equal(t.double().numpy() if t.dtype.is_floating_point else t.numpy(), a,
                          equal_nan=t.dtype.is_floating_point)


@pytest.mark.parametrize("B,C,k", [(5, 9, 4), (3, 7, 7), (4, 70, 64), (2, 1, 1)])
def test_predictor_rank_torch_path_is_exact(B, C, k, monkeypatch):
    dim = 6
    m = _grid_module(dim, 10 * B + C)
    monkeypatch.setattr(m, "_RANK_TORCH_CHUNK", 4)      # several steps of the chunked expression
    g = torch.Generator().manual_seed(B + C)
    h_src = torch.randint(-2, 3, (B, dim), generator=g).float()
    h_cand = torch.randint(-2, 3, (C, dim), generator=g).float()
    if C > 2:
        h_cand[2, 1] = float("nan")      # a NaN candidate row
    target = torch.randint(0, C, (B,), generator=g)
    target[0] = 0
    ref = _module_reference(m, h_src, h_cand, target.numpy(), k)
    out = m.rank(h_src, h_cand, k=k, target=target)      # k == C with a target: the fill
    assert isinstance(out, ops.EdgeRank)
    assert _equal(out.values, ref.values_skip) and _equal(out.indices, ref.indices_skip)
    assert _equal(out.greater, ref.greater_skip) and _equal(out.equal, ref.equal_skip)
    assert _equal(out.rank, 1 + ref.greater_skip + ref.equal_skip / 2)
    if k == C:
        assert out.indices[:, -1].tolist() == [-1] * B
        assert (out.values[:, -1] == float("-inf")).all()
    plain = m.rank(h_src, h_cand, k=k)
    assert plain.greater is None and plain.equal is None and plain.rank is None
    assert _equal(plain.values, ref.values) and _equal(plain.indices, ref.indices)
    if C > 2:      # the NaN row is last wherever it shows, and was never counted
        assert not (plain.indices[:, :min(k, C - 1)] == 2).any()
    counts_only = m.rank(h_src, h_cand, target=target)
    assert tuple(counts_only.values.shape) == (B, 0) == tuple(counts_only.indices.shape)
    assert _equal(counts_only.greater, ref.greater_skip)


def test_predictor_rank_leaves_the_module_alone():
    m = _grid_module(4, 1)
    before = {n: v.clone() for n, v in m.state_dict().items()}
    h = torch.ones(3, 4, requires_grad=True)
    out = m.rank(h, torch.ones(5, 4), k=2)
    assert not out.values.requires_grad
    assert list(m.state_dict()) == list(before)
    assert all(torch.equal(v, before[n]) for n, v in m.state_dict().items())
    with pytest.raises(ValueError):
        m.rank(h, torch.ones(5, 4), k=6)
