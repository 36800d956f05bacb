"""CPU tests of tests/pair_history_ref.py, the numpy restatement that the GPU tests of
DynamicGraph.pair_history and EdgeBank compare with: hand-written histories, answers worked out
by hand.

Node 7's history, oldest first:

    position  0   1   2   3   4   5   6
    dst       3   4   3   3   5   3   4
    ts        1   2   2   5   5   5   9
    eid      10  11  12  13  14  15  16

Node 8 has one edge (to 7 at 4, eid 20); node 9 is known and has none."""
import numpy as np
import pytest

from tests import pair_history_ref as P

NINF = np.float32(-np.inf)
NAN = float("nan")

HIST = {
    7: (np.array([3, 4, 3, 3, 5, 3, 4], np.int64),
        np.array([1, 2, 2, 5, 5, 5, 9], np.float32),
        np.array([10, 11, 12, 13, 14, 15, 16], np.int64)),
    8: (np.array([7], np.int64), np.array([4], np.float32), np.array([20], np.int64)),
    9: (np.zeros(0, np.int64), np.zeros(0, np.float32), np.zeros(0, np.int64)),
}


def one(s, d, t, since=None, max_history=0):
    c, lt, le = P.pair_history(HIST, [s], [d], [t], None if since is None else [since],
                               max_history)
    assert c.dtype == np.int64 and lt.dtype == np.float32 and le.dtype == np.int64
    return int(c[0]), lt[0], int(le[0])


def none(got):
    return got[0] == 0 and got[1] == NINF and got[2] == -1


def test_strictly_before_the_tie_is_left_out():
    assert one(7, 3, 5.0) == (2, np.float32(2), 12)        # the three edges AT 5 do not count
    assert one(7, 5, 5.0)[0] == 0 and none(one(7, 5, 5.0))
    assert one(7, 5, 5.5) == (1, np.float32(5), 14)
    assert none(one(7, 3, 1.0)) and none(one(7, 3, -1.0))  # nothing is before the first edge


def test_the_last_among_equal_timestamps_is_the_latest_in_store_order():
    assert one(7, 3, 6.0) == (4, np.float32(5), 15)        # positions 3 and 5 are both at 5
    assert one(7, 4, 2.5) == (1, np.float32(2), 11)
    assert one(7, 3, 2.5) == (2, np.float32(2), 12)
    assert one(7, 4, 1e9) == (2, np.float32(9), 16)


def test_since_is_inclusive():
    assert one(7, 4, 6.0, since=2.0) == (1, np.float32(2), 11)     # the edge AT 2 stays
    assert one(7, 3, 6.0, since=2.0) == (3, np.float32(5), 15)     # position 0 (ts 1) is out
    assert none(one(7, 4, 6.0, since=2.5))
    assert one(7, 3, 6.0, since=5.0) == (2, np.float32(5), 15)


def test_since_above_the_time_is_an_empty_window():
    assert none(one(7, 3, 6.0, since=8.0))
    assert none(one(7, 3, 6.0, since=6.0))                 # lo <= ts < t with lo == t
    assert none(one(7, 3, 6.0, since=np.inf))


def test_nan_since_is_no_lower_end_and_nan_time_is_nothing():
    assert one(7, 3, 6.0, since=NAN) == one(7, 3, 6.0) == (4, np.float32(5), 15)
    assert one(7, 3, 6.0, since=-np.inf) == (4, np.float32(5), 15)
    assert none(one(7, 3, NAN))
    assert none(one(7, 3, NAN, since=0.0)) and none(one(7, 3, NAN, since=NAN))


def test_max_history_is_the_newest_of_the_window_after_since():
    assert one(7, 3, 6.0, max_history=1) == (1, np.float32(5), 15)
    assert none(one(7, 4, 6.0, max_history=4))             # positions 2 .. 5 hold no 4
    assert one(7, 4, 6.0, max_history=5) == (1, np.float32(2), 11)
    assert one(7, 3, 10.0, since=2.0, max_history=2) == (1, np.float32(5), 15)     # 5 and 6
    assert one(7, 4, 10.0, since=2.0, max_history=2) == (1, np.float32(9), 16)
    # the window holds three edges, the bound is wider: all three, nothing older
    assert one(7, 3, 6.0, since=5.0, max_history=5) == (2, np.float32(5), 15)
    assert one(7, 3, 6.0, since=5.0, max_history=1000) == one(7, 3, 6.0, since=5.0)
    assert none(one(7, 5, 10.0, since=2.0, max_history=2))


def test_destinations_that_match_nothing_and_sources_without_a_history():
    for d in (-5, 1000, 7, 0):
        assert none(one(7, d, 1e9))
    for s in (-1, -3, 9, 99, 1 << 40):
        assert none(one(s, 3, 1e9))
    assert one(8, 7, 1e9) == (1, np.float32(4), 20)
    assert none(one(8, 7, 4.0))


def test_rows_are_independent_and_since_broadcasts():
    src = [7, 8, 7, 99, 7]
    dst = [3, 7, 4, 3, 3]
    ts = [6.0, 5.0, 1e9, 5.0, NAN]
    c, lt, le = P.pair_history(HIST, src, dst, ts)
    assert c.tolist() == [4, 1, 2, 0, 0] and le.tolist() == [15, 20, 16, -1, -1]
    assert np.array_equal(lt, np.array([5, 4, 9, -np.inf, -np.inf], np.float32))
    a = P.pair_history(HIST, src, dst, ts, 5.0)
    b = P.pair_history(HIST, src, dst, ts, np.full(5, 5.0, np.float32))
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    assert a[0].tolist() == [2, 0, 1, 0, 0]
    mixed = P.pair_history(HIST, src, dst, ts, [-np.inf, NAN, 9.0, 0.0, 0.0])
    assert mixed[0].tolist() == [4, 1, 1, 0, 0]
    empty = P.pair_history(HIST, [], [], [])
    assert [len(x) for x in empty] == [0, 0, 0]


def test_edge_bank_scores():
    src, dst, ts = [7, 7, 7, 8, 99], [3, 4, 5, 7, 3], [6.0, 6.0, 6.0, 6.0, 6.0]
    s = P.edge_bank_scores(HIST, src, dst, ts)
    assert s.dtype == np.float32 and s.tolist() == [1, 1, 1, 1, 0]
    assert P.edge_bank_scores(HIST, src, dst, ts, min_count=3).tolist() == [1, 0, 0, 0, 0]
    assert P.edge_bank_scores(HIST, src, dst, ts, score="count").tolist() == [4, 1, 1, 1, 0]
    # window 1: since = 5, inclusive
    w = P.edge_bank_scores(HIST, src, dst, ts, mode="time_window", window=1.0, score="count")
    assert w.tolist() == [2, 0, 1, 0, 0]
    assert P.edge_bank_scores(HIST, src, dst, ts, mode="time_window", window=1.0).tolist() == \
        [1, 0, 1, 0, 0]
    big = P.edge_bank_scores(HIST, src, dst, ts, mode="time_window", window=1e6, score="count")
    assert big.tolist() == [4, 1, 1, 1, 0]
    assert P.edge_bank_scores(HIST, src, dst, ts, max_history=1, score="count").tolist() == \
        [1, 0, 0, 1, 0]
    with pytest.raises(AssertionError):
        P.edge_bank_scores(HIST, src, dst, ts, mode="bogus")


class FakeGraph:
    """get_temporal_neighbors returns newest first, as DynamicGraph does."""

    def max_vertex_id(self):
        return 9

    def get_temporal_neighbors(self, v):
        d, t, e = HIST.get(v, HIST[9])
        return d[::-1].copy(), t[::-1].copy(), e[::-1].copy()


def test_from_graph_reverses_to_oldest_first():
    h = P.from_graph(FakeGraph(), [7, 7, 8, 9, 3, -1, 10, 1 << 40])
    assert sorted(h) == [3, 7, 8, 9]
    for v in (7, 8, 9):
        assert all(np.array_equal(a, b) for a, b in zip(h[v], HIST[v]))
    assert len(h[3][0]) == 0
