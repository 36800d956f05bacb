"""CPU tests of tests/edge_rank_exclude_ref.py on a hand-worked case, and of nn._rank_torch with
`exclude` (the route EdgePredictor.rank takes on the CPU, unfused and under bfloat16) against it."""
import inspect

import numpy as np
import pytest
import torch

from gnnflow_amd import nn as gnn
from gnnflow_amd import ops
from tests import edge_rank_exclude_ref as X
from tests import edge_rank_ref as R
from tests.seen_mask_ref import pack

# the reference restates ops.edge_rank(exclude=): without it there is nothing to restate
assert "exclude" in inspect.signature(ops.edge_rank).parameters


def _mask(rows, C):
    bits = np.zeros((len(rows), (C + 63) // 64 * 64), bool)
    for i, cs in enumerate(rows):
        bits[i, list(cs)] = True
    return pack(bits)


def test_hand_worked_case():
    # scores of the one source: candidate c scores c for c < 4, candidate 4 ties with 3
    score = np.array([[0.0, 1.0, 2.0, 3.0, 3.0]])
    inp = None
    v, i, g, e = X.rank(inp, 3, ref=[2.0], score=score)
    assert i.tolist() == [[3, 4, 2]] and g.tolist() == [2] and e.tolist() == [1]
    v, i, g, e = X.rank(inp, 3, ref=[2.0], exclude=_mask([{3}], 5), score=score)
    assert i.tolist() == [[4, 2, 1]] and v.tolist() == [[3.0, 2.0, 1.0]]
    assert g.tolist() == [1] and e.tolist() == [1]
    v, i, g, e = X.rank(inp, 3, ref=[2.0], skip=[2], exclude=_mask([{3, 4}], 5), score=score)
    assert i.tolist() == [[1, 0, -1]] and v[0, 2] == -np.inf
    assert g.tolist() == [0] and e.tolist() == [0]
    v, i, g, e = X.rank(inp, 2, ref=[2.0], exclude=X.full_mask(1, 5), score=score)
    assert i.tolist() == [[-1, -1]] and g.tolist() == [0] and e.tolist() == [0]
    # bits past C change nothing
    a = X.rank(inp, 3, ref=[2.0], exclude=_mask([{3}], 5), score=score)
    b = X.rank(inp, 3, ref=[2.0], exclude=_mask([{3, 5, 63}], 5), score=score)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


def test_cases_cover_what_they_claim():
    assert {c[0] for c in X.CASES} == {1, 33}
    assert {c[1] for c in X.CASES} == {1, 64, 65, 256, 257, 300}
    assert {c[2] for c in X.CASES} == {100, 7}
    for B in (1, 33):
        for C in (1, 64, 65, 256, 257, 300):
            for D in (100, 7):
                ks = {c[3] for c in X.CASES if c[:3] == (B, C, D)}
                assert ks == {0, 1, min(C, 10)} | ({C} if C <= 64 else set())
    m = X.random_mask((33, 65, 100))
    assert m.shape == (33, 2) and (m[:, 1] >> 1 == -1).all()      # garbage past C is set


def _torch_rank(inp, k, target, exclude, step):
    t = {n: torch.from_numpy(inp[n]) for n in ("src", "cand", "w", "bias")}
    return gnn._rank_torch(t["src"], t["cand"], t["w"], t["bias"], k,
                           None if target is None else torch.from_numpy(target), step,
                           None if exclude is None else torch.from_numpy(exclude))


def _same(out, ref):
    v, i, g, e = ref
    assert np.array_equal(out.values.double().numpy(), v, equal_nan=True)
    assert np.array_equal(out.indices.numpy(), i)
    if g is None:
        assert out.greater is None and out.equal is None
    else:
        assert np.array_equal(out.greater.numpy(), g) and np.array_equal(out.equal.numpy(), e)


@pytest.mark.parametrize("case", [(33, 65, 7, 10), (1, 64, 100, 64), (33, 300, 100, 10),
                                  (33, 257, 7, 1), (1, 1, 7, 1)], ids=X.case_id)
@pytest.mark.parametrize("step", [4096, 100])
def test_rank_torch_with_exclude_equals_the_reference(case, step):
    inp, score, mask = X.grid_reference(case)
    B, C, _, k = case
    target = inp["target"]
    ref = score[np.arange(B), target]
    _same(_torch_rank(inp, k, target, mask, step), X.rank(inp, k, ref, target, mask, score))
    _same(_torch_rank(inp, k, None, mask, step), X.rank(inp, k, None, None, mask, score))
    # the target's own bit set as well: the rank is among the others all the same
    own = mask.copy()
    own[np.arange(B), target >> 6] |= np.int64(1) << (target & 63)
    _same(_torch_rank(inp, k, target, own, step), X.rank(inp, k, ref, target, own, score))
    # everything excluded
    full = X.full_mask(B, C)
    out = _torch_rank(inp, k, target, full, step)
    assert (out.indices == -1).all() and (out.values == float("-inf")).all()
    assert not out.greater.any() and not out.equal.any()
    # no mask and an empty mask agree
    zero = np.zeros_like(mask)
    a, b = _torch_rank(inp, k, target, zero, step), _torch_rank(inp, k, target, None, step)
    assert torch.equal(a.values, b.values) and torch.equal(a.indices, b.indices)
    assert torch.equal(a.greater, b.greater) and torch.equal(a.equal, b.equal)


def test_rank_torch_rejects_a_malformed_mask():
    inp = R.make_grid((4, 70, 8))
    with pytest.raises(ValueError, match="exclude"):
        _torch_rank(inp, 3, None, np.zeros((4, 1), np.int64), 4096)
    with pytest.raises(ValueError, match="exclude"):
        _torch_rank(inp, 3, None, np.zeros((4, 2), np.int32), 4096)


def test_predictor_rank_passes_exclude_on_the_cpu():
    # integer-valued weights and rows: every summation order gives the same float32 score
    g = torch.Generator().manual_seed(0)
    m = gnn.EdgePredictor(6)
    with torch.no_grad():
        for p in m.parameters():
            p.copy_(torch.randint(-1, 2, p.shape, generator=g).float())
    h_src = torch.randint(-2, 3, (3, 6), generator=g).float()
    h_cand = torch.randint(-2, 3, (70, 6), generator=g).float()
    target = torch.tensor([0, 5, 69])
    with torch.no_grad():
        ref = m(torch.cat([h_src, h_cand[target], h_cand[target]]))[0].reshape(-1)
    plain = m.rank(h_src, h_cand, k=64, target=target)
    best = plain.indices[:, 0]
    mask = torch.zeros((3, 2), dtype=torch.int64)
    mask[torch.arange(3), best >> 6] = torch.ones(3, dtype=torch.int64) << (best & 63)
    out = m.rank(h_src, h_cand, k=64, target=target, exclude=mask)
    assert torch.equal(out.indices[:, :63], plain.indices[:, 1:])
    assert not (out.indices == best[:, None]).any() and not (out.indices == target[:, None]).any()
    top = plain.values[:, 0]
    assert torch.equal(out.greater, plain.greater - (top > ref).long())
    assert torch.equal(out.equal, plain.equal - (top == ref).long())
