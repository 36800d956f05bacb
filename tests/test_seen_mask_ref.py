"""CPU tests of tests/seen_mask_ref.py, the numpy restatement the GPU tests of csrc/seen_mask.hip
compare against, on hand-written cases; and that the package has what it restates."""
import numpy as np
import torch

import gnnflow_amd
from gnnflow_amd.dynamic_graph import check_seen_mask_args
from tests import seen_mask_ref as S

# node 3 met 10, 11, 10 and 12 at times 1, 2, 2, 5; node 4 met 11 at time 3; node 5 nothing
HIST = {
    3: (np.array([10, 11, 10, 12]), np.array([1, 2, 2, 5], np.float32)),
    4: (np.array([11]), np.array([3], np.float32)),
    5: (np.zeros(0, np.int64), np.zeros(0, np.float32)),
}


def _bits(words, C):
    return [[c for c in range(C) if row[c]] for row in S.unpack(words, C)]


def test_restates_what_the_package_offers():
    assert callable(gnnflow_amd.DynamicGraph.seen_mask)
    src, ts, cand = np.array([3, 4]), np.array([9, 9], np.float32), np.arange(70)
    B, C = check_seen_mask_args(torch.from_numpy(src), torch.from_numpy(ts),
                                torch.from_numpy(cand), 0)
    assert S.seen_mask(HIST, src, ts, cand).shape == (B, S.num_words(C)) == (2, 2)


def test_strictly_before_and_unsorted_candidates_with_duplicates():
    cand = np.array([12, 10, 99, 10, 11])      # unsorted, 10 twice, 99 unknown
    src = np.array([3, 3, 3, 3, 3, 4, 4])
    ts = np.array([1, 2, 2.5, 5, 6, 3, 3.5], np.float32)
    m = S.seen_mask(HIST, src, ts, cand)
    assert m.shape == (7, 1) and m.dtype == np.int64
    assert _bits(m, 5) == [[], [1, 3], [1, 3, 4], [1, 3, 4], [0, 1, 3, 4], [], [4]]
    assert m[4, 0] == 0b11011


def test_nan_unknown_negative_and_empty_sources_give_zero_rows():
    cand = np.array([10, 11, 12])
    src = np.array([3, -1, 7, 5, 1 << 40])
    ts = np.array([np.nan, 9, 9, 9, 9], np.float32)
    assert not S.seen_mask(HIST, src, ts, cand).any()


def test_max_history_keeps_the_newest():
    cand = np.array([10, 11, 12])
    src, ts = np.array([3] * 4), np.full(4, 9, np.float32)
    got = [_bits(S.seen_mask(HIST, src[:1], ts[:1], cand, max_history=h), 3)[0]
           for h in (0, 1, 2, 9)]
    assert got == [[0, 1, 2], [2], [0, 2], [0, 1, 2]]
    # the newest of the edges BEFORE t, not of all edges; ties keep the store's order
    assert _bits(S.seen_mask(HIST, [3], [5.0], cand, max_history=1), 3) == [[0]]
    assert _bits(S.seen_mask(HIST, [3], [5.0], cand, max_history=2), 3) == [[0, 1]]


def test_word_borders_and_bits_past_the_end():
    for C in (1, 63, 64, 65, 130):
        cand = np.full(C, 99)
        cand[C - 1] = 12
        cand[0] = 12 if C > 1 else cand[0]
        m = S.seen_mask(HIST, [3], [9.0], cand)
        assert m.shape == (1, (C + 63) // 64)
        assert _bits(m, C) == [sorted({0, C - 1})]
        full = S.unpack(m, m.shape[1] * 64)
        assert not full[:, C:].any()
    # bit 63 is the sign bit of the int64 word
    cand = np.full(64, 12)
    assert S.seen_mask(HIST, [3], [9.0], cand)[0, 0] == -1


def test_pack_and_unpack_are_inverse():
    rng = np.random.RandomState(0)
    bits = rng.rand(5, 192) < 0.5
    assert np.array_equal(S.unpack(S.pack(bits), 192), bits)
