"""CPU tests of tests/neighbor_cooccurrence_ref.py, the numpy restatement that the GPU tests of
DynamicGraph.neighbor_cooccurrence compare with: hand-written histories (those of
test_common_neighbors_ref.py), answers worked out by hand and written out.

Node 0 (oldest first)   dst  5  6  5  7  5 -2  8      node 1   dst  6  9  5  8  8
                        ts   1  2  3  4  5  6  7               ts   1  3  5  5  9
                        eid  0  1  2  3  4  5  6               eid 10 11 12 13 14
Node 2 has no edges, node 3 has two at the same time, node 8 has met 0 at 1 and 1 at 200; 99 is
unknown.
"""
import numpy as np
import pytest

from tests import neighbor_cooccurrence_ref as R

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


def _one(s, d, t, since=None, L=8, self_slot=True):
    out = R.neighbor_cooccurrence(HIST, [s], [d], [t], None if since is None else [since], L,
                                  self_slot)
    assert [x.dtype for x in out] == [np.int32, np.int64, np.int64, np.float32, np.int32]
    assert [x.shape for x in out] == [(1, 2), (1, 2, L), (1, 2, L), (1, 2, L), (1, 2, L, 2)]
    lengths, nodes, eids, times, counts = (x[0] for x in out)
    return lengths.tolist(), nodes.tolist(), eids.tolist(), times.tolist(), counts.tolist()


def test_self_slot_multi_edges_a_negative_destination_and_padding():
    lengths, nodes, eids, times, counts = _one(0, 1, 100.0)
    assert lengths == [8, 6]
    assert nodes == [[0, 5, 6, 5, 7, 5, -2, 8], [1, 6, 9, 5, 8, 8, -1, -1]]
    assert eids == [[-1, 0, 1, 2, 3, 4, 5, 6], [-1, 10, 11, 12, 13, 14, -1, -1]]
    assert times == [[100, 1, 2, 3, 4, 5, 6, 7], [100, 1, 3, 5, 5, 9, 0, 0]]
    # a: 0 x1, 5 x3, 6, 7, 8 x1; b: 1, 6, 9, 5 x1, 8 x2; the -2 is an element and counts nothing
    assert counts[0] == [[1, 0], [3, 1], [1, 1], [3, 1], [1, 0], [3, 1], [0, 0], [1, 2]]
    assert counts[1] == [[0, 1], [1, 1], [0, 1], [3, 1], [1, 2], [1, 2], [0, 0], [0, 0]]


def test_channel_zero_is_the_sources_sequence_on_both_sides():
    fwd, back = _one(0, 1, 100.0), _one(1, 0, 100.0)
    assert back[1] == fwd[1][::-1] and back[0] == fwd[0][::-1]
    assert back[4] == [[[b, a] for a, b in side] for side in fwd[4][::-1]]


def test_without_the_self_slot_the_bound_is_the_length():
    lengths, nodes, eids, times, counts = _one(0, 1, 100.0, L=4, self_slot=False)
    assert lengths == [4, 4]                       # both cut: the newest four
    assert nodes == [[7, 5, -2, 8], [9, 5, 8, 8]]
    assert eids == [[3, 4, 5, 6], [11, 12, 13, 14]]
    assert times == [[4, 5, 6, 7], [3, 5, 5, 9]]
    assert counts == [[[1, 0], [1, 1], [0, 0], [1, 2]], [[0, 1], [1, 1], [1, 2], [1, 2]]]
    # with it the same length holds one record fewer
    lengths, nodes, _, _, _ = _one(0, 1, 100.0, L=4, self_slot=True)
    assert lengths == [4, 4] and nodes == [[0, 5, -2, 8], [1, 5, 8, 8]]


def test_the_self_slot_is_counted():
    # 8 has met 0 before t = 100: with the self slots 0 and 8 occur on both sides
    lengths, nodes, _, _, counts = _one(0, 8, 100.0)
    assert lengths == [8, 2] and nodes[1] == [8, 0, -1, -1, -1, -1, -1, -1]
    assert counts[0][0] == [1, 1] and counts[0][7] == [1, 1]
    assert counts[1][:2] == [[1, 1], [1, 1]]
    # without them each occurs on one side only
    lengths, nodes, _, _, counts = _one(0, 8, 100.0, self_slot=False)
    assert lengths == [7, 1] and nodes[1][:2] == [0, -1]
    assert counts[0][6] == [1, 0] and counts[1][0] == [0, 1]


def test_ties_at_t_are_not_before_t():
    lengths, nodes, _, _, counts = _one(0, 1, 5.0, self_slot=False)
    assert lengths == [4, 2]
    assert nodes[0][:4] == [5, 6, 5, 7] and nodes[1][:2] == [6, 9]
    assert counts[0][:4] == [[2, 0], [1, 1], [2, 0], [1, 0]] and counts[1][:2] == [[1, 1], [0, 1]]
    assert _one(3, 3, 2.0, self_slot=False)[0] == [0, 0]
    assert _one(3, 3, 2.5, self_slot=False)[0] == [2, 2]


def test_nan_time_keeps_the_self_slot_alone():
    lengths, nodes, eids, times, counts = _one(0, 1, NAN)
    assert lengths == [1, 1] and nodes[0][:2] == [0, -1] and nodes[1][:2] == [1, -1]
    assert eids[0][0] == -1 and np.isnan(times[0][0]) and np.isnan(times[1][0])
    assert times[0][1:] == [0] * 7 and counts[0][0] == [1, 0] and counts[1][0] == [0, 1]
    lengths, nodes, eids, times, counts = _one(0, 1, NAN, self_slot=False)
    assert lengths == [0, 0] and nodes == [[-1] * 8] * 2 and eids == [[-1] * 8] * 2
    assert times == [[0] * 8] * 2 and counts == [[[0, 0]] * 8] * 2


def test_since_is_inclusive_nan_is_none_and_past_t_is_empty():
    lengths, nodes, eids, _, counts = _one(0, 1, 100.0, since=5.0, self_slot=False)
    assert lengths == [3, 3] and nodes[0][:3] == [5, -2, 8] and nodes[1][:3] == [5, 8, 8]
    assert eids[0][:3] == [4, 5, 6] and eids[1][:3] == [12, 13, 14]
    assert counts[0][:3] == [[1, 1], [0, 0], [1, 2]]
    assert _one(0, 1, 100.0, since=NAN) == _one(0, 1, 100.0)
    assert _one(0, 1, 5.0, since=50.0, self_slot=False)[0] == [0, 0]
    assert _one(0, 1, 5.0, since=50.0)[0] == [1, 1]
    # the bound comes after the lower end: the newest two of ts >= 3
    lengths, nodes, _, _, _ = _one(0, 1, 100.0, since=3.0, L=2, self_slot=False)
    assert lengths == [2, 2] and nodes == [[-2, 8], [8, 8]]


def test_both_ends_the_same_node():
    lengths, nodes, eids, times, counts = _one(0, 0, 100.0)
    assert lengths == [8, 8] and nodes[0] == nodes[1] and eids[0] == eids[1]
    assert times[0] == times[1] and counts[0] == counts[1]
    assert counts[0] == [[1, 1], [3, 3], [1, 1], [3, 3], [1, 1], [3, 3], [0, 0], [1, 1]]


@pytest.mark.parametrize("end", [-3, 99, 2])
def test_a_negative_an_unknown_and_an_edgeless_end(end):
    lengths, nodes, eids, times, counts = _one(end, 1, 100.0)
    assert lengths == [1, 6] and nodes[0] == [end] + [-1] * 7 and eids[0] == [-1] * 8
    assert times[0] == [100.0] + [0] * 7
    assert counts[0][0] == ([0, 0] if end < 0 else [1, 0])      # a negative id is not counted
    assert counts[1][:6] == [[0, 1], [0, 1], [0, 1], [0, 1], [0, 2], [0, 2]]
    assert _one(end, 1, 100.0, self_slot=False)[0] == [0, 5]
    # as the second end, and both ends at once
    assert _one(1, end, 100.0)[0] == [6, 1]
    both = _one(end, end, 100.0)
    assert both[0] == [1, 1] and both[4][0][0] == ([0, 0] if end < 0 else [1, 1])


def test_a_larger_length_at_the_same_bound_only_adds_padding():
    """No history here has more than 7 records, so every length from 8 (7 without the self slot)
    leaves the windows whole: the sequences stay, the padding grows."""
    src = [0, 1, 0, 3, 8, -3, 5, 0]
    dst = [1, 0, 0, 8, 0, 1, 99, 2]
    ts = [100.0, 6.0, 5.0, 2.5, 300.0, 100.0, 3.0, NAN]
    for self_slot, since in ((True, None), (False, None), (True, 3.0), (False, [NAN, 1, 2, 3, 4,
                                                                                5, 6, 7])):
        small = 8 if self_slot else 7
        a = R.neighbor_cooccurrence(HIST, src, dst, ts, since, small, self_slot)
        for large in (small + 1, 33, 512):
            b = R.neighbor_cooccurrence(HIST, src, dst, ts, since, large, self_slot)
            assert np.array_equal(a[0], b[0])
            for x, y, pad in zip(a[1:], b[1:], (-1, -1, 0, 0)):
                assert np.array_equal(x, y[:, :, :small], equal_nan=True)
                assert (y[:, :, small:] == pad).all()
    # and a smaller one cuts: not a prefix
    a = R.neighbor_cooccurrence(HIST, src, dst, ts, None, 3, False)
    b = R.neighbor_cooccurrence(HIST, src, dst, ts, None, 7, False)
    assert a[0].max() == 3 and b[0].max() == 7 and not np.array_equal(a[1], b[1][:, :, :3])


def test_length_bounds_and_helpers():
    for L, self_slot in ((1, True), (0, False), (513, True), (513, False)):
        with pytest.raises(AssertionError):
            R.neighbor_cooccurrence(HIST, [0], [1], [9.0], None, L, self_slot)
    out = R.neighbor_cooccurrence(HIST, [0, 2], [1, 99], [100.0, 100.0], None, 2, True)
    assert out[0].tolist() == [[2, 2], [1, 1]]
    assert R.has_cooccurrence(out[1], out[4]).tolist() == [True, False]      # 8 on both sides
    R.same(out, out)
    other = tuple(x.copy() for x in out)
    other[4][1, 1, 0, 1] += 1
    with pytest.raises(AssertionError, match="counts"):
        R.same(out, other)
    out = R.neighbor_cooccurrence(HIST, [], [], [], None, 5, False)
    assert [x.shape for x in out] == [(0, 2), (0, 2, 5), (0, 2, 5), (0, 2, 5), (0, 2, 5, 2)]
