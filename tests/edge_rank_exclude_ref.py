"""Float64 reference of ops.edge_rank(..., exclude=): tests/edge_rank_ref.scores with the mask
applied in numpy to the counts and the top k.

    kept(i, c)  = c != skip[i]  and  bit c % 64 of exclude[i, c // 64] is clear
    greater[i]  = #{c kept : score(i, c) >  ref[i]}
    equal[i]    = #{c kept : score(i, c) == ref[i]}
    top k       = the first k of the kept candidates ordered by (score is NaN, -score, c), filled
                  with (-inf, -1)

Inputs are edge_rank_ref.make_grid's integer-valued ones, so that every float32 summation order is
exact and the kernel is compared with exact equality.  Pure numpy.
"""
import numpy as np

from tests import edge_rank_ref as R
from tests.seen_mask_ref import pack, unpack

# (B, C, D, k), every combination of: B of {1, 33}; C of {1, 64, 65, 256, 257, 300}: a word, a word
# and a bit, a chunk, a chunk and a bit, sub-tiles of a second chunk; D of {100 (16-byte staging),
# 7 (element-wise)}; k of {0, 1, min(C, 10), C for C <= 64}
CASES = [(B, C, D, k) for B in (1, 33) for C in (1, 64, 65, 256, 257, 300) for D in (100, 7)
         for k in sorted({0, 1, min(C, 10)} | ({C} if C <= 64 else set()))]


def case_id(case):
    return R.case_id(case)


def kept(B, C, skip=None, exclude=None):
    """bool [B, C]: the candidates that take part in row i."""
    keep = np.ones((B, C), bool)
    if skip is not None:
        keep &= np.arange(C)[None, :] != np.asarray(skip)[:, None]
    if exclude is not None:
        assert exclude.shape == (B, (C + 63) // 64) and exclude.dtype == np.int64
        keep &= ~unpack(exclude, C)
    return keep


def counts(score, ref, keep):
    ref = np.asarray(ref, np.float64).reshape(-1, 1)
    with np.errstate(invalid="ignore"):
        return ((score > ref) & keep).sum(1).astype(np.int64), \
            ((score == ref) & keep).sum(1).astype(np.int64)


def topk(score, k, keep):
    B, C = score.shape
    values = np.full((B, k), -np.inf)
    indices = np.full((B, k), -1, np.int64)
    for i in range(B):
        cs = [c for c in range(C) if keep[i, c]]
        cs.sort(key=lambda c: (1, 0.0, c) if np.isnan(score[i, c]) else (0, -score[i, c], c))
        for t, c in enumerate(cs[:k]):
            values[i, t], indices[i, t] = score[i, c], c
    return values, indices


def rank(inp, k, ref=None, skip=None, exclude=None, score=None):
    """(values, indices, greater, equal); greater and equal None without ref."""
    score = R.scores(inp["src"], inp["cand"], inp["w"], inp["bias"]) if score is None else score
    keep = kept(*score.shape, skip, exclude)
    values, indices = topk(score, k, keep)
    greater, equal = counts(score, ref, keep) if ref is not None else (None, None)
    return values, indices, greater, equal


def random_mask(case, density=0.3, garbage=True):
    """int64 [B, W]: each candidate excluded with probability `density`; with `garbage` every bit
    past C is set, which must change nothing."""
    B, C = case[:2]
    rng = np.random.RandomState(5000 + B + 7 * C + 31 * case[2])
    W = (C + 63) // 64
    bits = np.zeros((B, W * 64), bool)
    bits[:, :C] = rng.rand(B, C) < density
    if garbage:
        bits[:, C:] = True
    return pack(bits)


def full_mask(B, C, garbage=False):
    bits = np.zeros((B, (C + 63) // 64 * 64), bool)
    bits[:, :C] = True
    if garbage:
        bits[:] = True
    return pack(bits)


_cache = {}


def grid_reference(case):
    """(inputs, score float64 [B, C], mask int64 [B, W]) of a case's (B, C, D), shared among its
    k and left unchanged."""
    key = tuple(case[:3])
    if key not in _cache:
        inp = R.make_grid(key)
        _cache[key] = (inp, R.scores(inp["src"], inp["cand"], inp["w"], inp["bias"]),
                       random_mask(key))
    return _cache[key]
