"""CPU tests of tests/common_neighbors_ref.py, the numpy restatement that the GPU tests of
DynamicGraph.common_neighbors, DynamicGraph.temporal_degree and NeighborOverlap compare with:
hand-written histories, answers worked out by hand and written out.

Node 0 (oldest first)   dst  5  6  5  7  5 -2  8      node 1   dst  6  9  5  8  8
                        ts   1  2  3  4  5  6  7               ts   1  3  5  5  9
Node 2 has no edges, node 3 has two at the same time; nodes 5, 6 and 8 have 3, 1 and 2 edges, so
that the common neighbours of 0 and 1 have degrees of their own; 99 is unknown.
"""
import math

import numpy as np
import pytest

from tests import common_neighbors_ref as R

NAN = float("nan")


def _h(dst, ts, eid0):
    return (np.array(dst, np.int64), np.array(ts, np.float32),
            np.arange(eid0, eid0 + len(dst), dtype=np.int64))


HIST = {
    0: _h([5, 6, 5, 7, 5, -2, 8], [1, 2, 3, 4, 5, 6, 7], 0),
    1: _h([6, 9, 5, 8, 8], [1, 3, 5, 5, 9], 10),
    2: _h([], [], 20),
    3: _h([0, 1], [2, 2], 30),
    5: _h([0, 0, 0], [1, 2, 3], 40),
    6: _h([0], [1], 50),
    8: _h([0, 1], [1, 200], 60),
}


def _one(s, d, t, since=None, H=64, K=4):
    out = R.common_neighbors(HIST, [s], [d], [t], None if since is None else [since], H, K)
    assert [x.dtype for x in out] == [np.int32] * 5 + [np.int64, np.int32, np.int32]
    assert [x.shape for x in out] == [(1,)] * 5 + [(1, K)] * 3
    scalars = tuple(int(x[0]) for x in out[:5])
    return scalars, out[5][0].tolist(), out[6][0].tolist(), out[7][0].tolist()


def test_everything_before_the_time_multi_edges_order_and_a_negative_destination():
    # A: 5 x3 (last at position 4), 6 (1), 7 (3), 8 (6); the -2 is an edge and no neighbour
    # B: 6, 9, 5, 8 x2.  common {5, 6, 8} by descending pa: 8, 5, 6
    assert _one(0, 1, 100.0) == ((7, 5, 4, 4, 3), [8, 5, 6, -1], [1, 3, 1, 0], [2, 1, 1, 0])
    # the other way round the order is by the positions in 1's history: 8 (4), 5 (2), 6 (0)
    assert _one(1, 0, 100.0) == ((5, 7, 4, 4, 3), [8, 5, 6, -1], [2, 1, 1, 0], [1, 3, 1, 0])


def test_ties_at_t_are_not_before_t():
    # t = 5: node 0 keeps ts 1 .. 4 = [5, 6, 5, 7], node 1 keeps ts 1, 3 = [6, 9]
    assert _one(0, 1, 5.0) == ((4, 2, 3, 2, 1), [6, -1, -1, -1], [1, 0, 0, 0], [1, 0, 0, 0])
    assert _one(3, 3, 2.0) == ((0, 0, 0, 0, 0), [-1] * 4, [0] * 4, [0] * 4)


def test_since_is_inclusive():
    # ts >= 5: node 0 keeps [5, -2, 8], node 1 keeps [5, 8, 8]
    assert _one(0, 1, 100.0, since=5.0) == ((3, 3, 2, 2, 2), [8, 5, -1, -1], [1, 1, 0, 0],
                                            [2, 1, 0, 0])
    # just above: node 0 keeps [-2, 8], node 1 keeps [8]
    assert _one(0, 1, 100.0, since=5.5) == ((2, 1, 1, 1, 1), [8, -1, -1, -1], [1, 0, 0, 0],
                                            [1, 0, 0, 0])
    assert _one(0, 1, 100.0, since=NAN) == _one(0, 1, 100.0)            # no lower end
    assert _one(0, 1, 100.0, since=-np.inf) == _one(0, 1, 100.0)
    assert _one(0, 1, 6.0, since=50.0)[0] == (0, 0, 0, 0, 0)            # above t: empty


def test_max_history_cuts_a_neighbour_out_of_one_side_only():
    # H = 5: node 0 keeps [5, 7, 5, -2, 8] and loses 6; node 1 keeps all five, 6 among them
    assert _one(0, 1, 100.0, H=5) == ((5, 5, 3, 4, 2), [8, 5, -1, -1], [1, 2, 0, 0],
                                      [2, 1, 0, 0])
    # H = 2: [-2, 8] and [8, 8]
    assert _one(0, 1, 100.0, H=2) == ((2, 2, 1, 1, 1), [8, -1, -1, -1], [1, 0, 0, 0],
                                      [2, 0, 0, 0])
    # H = 1: [8] and [8]
    assert _one(0, 1, 100.0, H=1)[0] == (1, 1, 1, 1, 1)
    # H comes after since and t: of 3 <= ts < 6 the NEWEST 2
    assert _one(0, 1, 6.0, since=3.0, H=2) == ((2, 2, 2, 2, 1), [5, -1, -1, -1], [1, 0, 0, 0],
                                               [1, 0, 0, 0])            # [7, 5] and [5, 8]


def test_truncation_at_k_keeps_the_count():
    assert _one(0, 1, 100.0, K=2) == ((7, 5, 4, 4, 3), [8, 5], [1, 3], [2, 1])
    assert _one(0, 1, 100.0, K=1) == ((7, 5, 4, 4, 3), [8], [1], [2])
    assert _one(0, 1, 100.0, K=0) == ((7, 5, 4, 4, 3), [], [], [])


def test_source_equal_to_destination():
    assert _one(0, 0, 100.0) == ((7, 7, 4, 4, 4), [8, 5, 7, 6], [1, 3, 1, 1], [1, 3, 1, 1])


@pytest.mark.parametrize("v", [2, 99, -1, 1 << 40])
def test_a_node_without_a_history_has_an_empty_window(v):
    assert _one(v, 0, 100.0) == ((0, 7, 0, 4, 0), [-1] * 4, [0] * 4, [0] * 4)
    assert _one(0, v, 100.0) == ((7, 0, 4, 0, 0), [-1] * 4, [0] * 4, [0] * 4)
    assert _one(v, v, 100.0)[0] == (0, 0, 0, 0, 0)


def test_nan_time_and_batches():
    assert _one(0, 1, NAN)[0] == (0, 0, 0, 0, 0)
    out = R.common_neighbors(HIST, [0, 0, 2], [1, 1, 0], [100.0, 5.0, 100.0],
                             [-np.inf, NAN, 5.0], 64, 2)
    assert out[4].tolist() == [3, 1, 0] and out[5].tolist() == [[8, 5], [6, -1], [-1, -1]]
    assert out[1].tolist() == [5, 2, 3]
    scalar = R.common_neighbors(HIST, [0, 0], [1, 1], [100.0, 100.0], 5.0, 64, 2)
    assert scalar[0].tolist() == [3, 3]
    empty = R.common_neighbors(HIST, [], [], [], None, 64, 3)
    assert [x.shape for x in empty] == [(0,)] * 5 + [(0, 3)] * 3


def test_temporal_degree():
    nodes = np.array([[0, 1, -1], [2, 99, 8]], np.int64)
    assert R.temporal_degree(HIST, nodes, np.full((2, 3), 100.0)).tolist() == [[7, 5, 0],
                                                                              [0, 0, 1]]
    assert R.temporal_degree(HIST, nodes, np.full((2, 3), 5.0)).tolist() == [[4, 2, 0], [0, 0, 1]]
    assert R.temporal_degree(HIST, nodes, np.full((2, 3), 1e9), 5.0).tolist() == [[3, 3, 0],
                                                                                [0, 0, 1]]
    assert R.temporal_degree(HIST, nodes, np.full((2, 3), NAN)).tolist() == [[0] * 3] * 2
    assert R.temporal_degree(HIST, nodes, np.full((2, 3), 100.0), NAN).tolist() == \
        [[7, 5, 0], [0, 0, 1]]
    out = R.temporal_degree(HIST, np.zeros((0, 4), np.int64), np.zeros((0, 4), np.float32))
    assert out.shape == (0, 4) and out.dtype == np.int64


def test_the_five_scores():
    # 0 and 1 at t = 100: common 8, 5, 6 of degrees 1, 3, 1 (8's second edge is at 200)
    def s(score, **kw):
        out = R.overlap_scores(HIST, [0], [1], [100.0], score, **kw)
        assert out.dtype == np.float64 and out.shape == (1,)
        return float(out[0])
    assert s("cn") == 3.0
    assert s("pa") == 35.0
    assert s("jaccard") == 3.0 / 5.0                                  # 4 + 4 - 3
    assert s("aa") == 1.0 / math.log(3.0)                             # degree 1 has no term
    assert s("ra") == (1.0 + 1.0 / 3.0) + 1.0                         # in the nodes' order
    # max_common = 1 keeps node 8 alone for aa and ra, and changes nothing else
    assert s("aa", max_common=1) == 0.0 and s("ra", max_common=1) == 1.0
    assert s("cn", max_common=1) == 3.0 and s("jaccard", max_common=0) == 0.6
    # window = 95.5: since = 4.5, node 0 keeps [5, -2, 8], node 1 [5, 8, 8]; no degree counts
    # an edge before 4.5: deg 8 = 0, deg 5 = 0
    assert s("cn", window=95.5) == 2.0 and s("jaccard", window=95.5) == 1.0
    assert s("pa", window=95.5) == 9.0 and s("ra", window=95.5) == 0.0
    assert s("jaccard", window=10.0) == 0.0                           # empty union
    assert R.overlap_scores(HIST, [2, 0], [2, 0], [100.0, 100.0], "jaccard").tolist() == [0, 1]
    with pytest.raises(AssertionError):
        R.overlap_scores(HIST, [0], [1], [100.0], "bogus")
