"""Float64 brute-force reference of ops.edge_rank (csrc/edge_rank.hip) and the seeded inputs that
the CPU and the GPU tests share.  Pure numpy.

    score(i, c) = bias + sum_d w[d] max(src[i, d] + cand[c, d], 0)        a NaN stays a NaN
    greater[i]  = #{c != skip[i] : score(i, c) >  ref[i]}
    equal[i]    = #{c != skip[i] : score(i, c) == ref[i]}
    top k       = the first k of the candidates c != skip[i] ordered by (score is NaN, -score, c),
                  filled with (-inf, -1)

Grid inputs.  src and cand are integers in [-8, 8], w and bias integers in [-4, 4].  With
D <= 257 every partial sum of a score is an integer of magnitude at most 4 + 257 * 4 * 16 < 2^15,
so every float32 summation order is exact and equals the float64 value: the kernels are compared
with EXACT equality, whatever their order of summation.  Integer scores tie often, and make_grid
plants a tie where chance might not: row 0's best candidate is copied over its neighbour, so with
C >= 2 the two best scores of row 0 are equal, and target[0] is one of the two, so that the other
one ties with the reference score after the skip.  `Reference` asserts both for every case where
they are possible (C >= 2; a tie inside the list needs k >= 2).

Drawn inputs (make_drawn) are edge_score_ref._draw's values, for the bit-equality test against
ops.edge_score.
"""
import os
import re

import numpy as np

from tests.edge_score_ref import _draw

_HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include",
                       "gnnflow_hip.h")


def header_constant(name):
    m = re.search(r"#define\s+{}\s+(\d+)".format(name), open(_HEADER).read())
    assert m, name
    return int(m.group(1))


CH = header_constant("GF_EDGE_RANK_CHUNK")
MAX_K = header_constant("GF_EDGE_RANK_MAX_K")


def scores(src, cand, w, bias):
    """float64 [B, C]; np.maximum keeps a NaN."""
    src, cand = np.asarray(src, np.float64), np.asarray(cand, np.float64)
    w = np.asarray(w, np.float64).reshape(-1)
    x = np.maximum(src[:, None, :] + cand[None, :, :], 0.0)
    with np.errstate(invalid="ignore"):
        return float(np.asarray(bias).reshape(-1)[0]) + x @ w


def counts(score, ref, skip=None):
    """(greater, equal) int64 [B] of a score matrix against ref [B]."""
    B, C = score.shape
    keep = np.ones((B, C), bool)
    if skip is not None:
        keep = np.arange(C)[None, :] != np.asarray(skip)[:, None]
    ref = np.asarray(ref, np.float64).reshape(B, 1)
    with np.errstate(invalid="ignore"):
        return ((score > ref) & keep).sum(1).astype(np.int64), \
            ((score == ref) & keep).sum(1).astype(np.int64)


def topk(score, k, skip=None):
    """(values float64 [B, k], indices int64 [B, k]) under the total order of the docstring."""
    B, C = score.shape
    values = np.full((B, k), -np.inf)
    indices = np.full((B, k), -1, np.int64)
    for i in range(B):
        cs = [c for c in range(C) if skip is None or c != int(skip[i])]
        cs.sort(key=lambda c: (1, 0.0, c) if np.isnan(score[i, c]) else (0, -score[i, c], c))
        for t, c in enumerate(cs[:k]):
            values[i, t], indices[i, t] = score[i, c], c
    return values, indices


class Reference:
    """Everything the tests compare with for one case, computed once and left unchanged."""

    def __init__(self, inp, k, check_ties=True):
        self.k = k
        self.score = scores(inp["src"], inp["cand"], inp["w"], inp["bias"])
        B, C = self.score.shape
        target = inp["target"]
        self.ref = self.score[np.arange(B), target] if B else np.zeros(0)
        self.greater_skip, self.equal_skip = counts(self.score, self.ref, target)
        self.greater, self.equal = counts(self.score, self.ref)
        self.values_skip, self.indices_skip = topk(self.score, k, target)
        self.values, self.indices = topk(self.score, k)
        if check_ties and C >= 2:
            assert (self.equal_skip > 0).any(), "no tie with a reference score"
            if k >= 2:
                v = self.values
                assert (v[:, 1:] == v[:, :-1]).any(), "no tie inside a list"


# (B, C, D, k): every B of {1, 5, 17, 33}, every C of {1, 3, CH - 1, CH, CH + 1, 2 CH + 1}, every D
# of {1, 3 (element loads), 4 (one chunk), 60 (fewer chunks than lanes), 64 (one pass), 100 (lanes
# with two chunks and with one), 132 (three and two), 257 (element loads, five passes)} and every
# k of {0, 1, 5, 64, C when C <= 64}, boundary values paired with boundary values.
CASES = [
    (1, 1, 1, 0), (1, 1, 4, 1), (5, 3, 3, 3), (5, 3, 100, 1), (17, CH - 1, 60, 5),
    (17, CH, 64, 64), (33, CH + 1, 100, 5), (33, 2 * CH + 1, 132, 64), (1, 2 * CH + 1, 257, 5),
    (5, CH, 3, 64), (17, CH + 1, 132, 1), (33, 3, 257, 3), (1, CH - 1, 4, 64), (5, CH + 1, 1, 5),
    (17, 3, 64, 0), (33, CH, 60, 1), (5, 2 * CH + 1, 100, 64), (17, 1, 132, 1),
    (33, CH - 1, 257, 5), (1, CH, 100, 0), (17, 40, 4, 40),
]
# (B, C, D) of the bit-equality test, k = min(C, 64)
DRAWN = [(5, 3, 100), (17, CH + 1, 132), (33, 2 * CH + 1, 100), (5, CH, 3)]


def case_id(case):
    return "B{}_C{}_D{}_k{}".format(*case) if len(case) == 4 else "B{}_C{}_D{}".format(*case)


def make_grid(case):
    """Integer-valued float32 src [B, D], cand [C, D], w [D], bias [1] and int64 target [B]."""
    B, C, D = case[:3]
    rng = np.random.RandomState(3000 + B + 7 * C + 31 * D)
    src = rng.randint(-8, 9, size=(B, D)).astype(np.float32)
    cand = rng.randint(-8, 9, size=(C, D)).astype(np.float32)
    w = rng.randint(-4, 5, size=D).astype(np.float32)
    bias = rng.randint(-4, 5, size=1).astype(np.float32)
    target = rng.randint(0, C, size=B).astype(np.int64)
    if C >= 2:      # plant the ties of the module docstring
        best = int(np.argmax(scores(src[:1], cand, w, bias)[0]))
        cand[(best + 1) % C] = cand[best]
        target[0] = best
    return dict(src=src, cand=cand, w=w, bias=bias, target=target)


def make_drawn(case):
    B, C, D = case
    rng = np.random.RandomState(4000 + B + 7 * C + 31 * D)
    return dict(src=_draw(rng, B, D), cand=_draw(rng, C, D), w=_draw(rng, D), bias=_draw(rng, 1))


_cache = {}


def grid_reference(case):
    """(inputs, Reference) of a grid case, shared and left unchanged."""
    if case not in _cache:
        inp = make_grid(case)
        _cache[case] = (inp, Reference(inp, case[3]))
    return _cache[case]
