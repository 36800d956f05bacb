"""tests/pair_sequence_ref.py on hand-written histories, every expected value written out by
hand: the GPU tests compare the kernel with this restatement, so it is checked on its own first."""
import numpy as np

from tests import pair_sequence_ref as R

NAN = float("nan")
# node 0, the hub: five edges, two of them at t = 5, the last to a negative destination;
# node 1: two edges; node 2: known, no edges
HIST = {
    0: (np.array([10, 11, 1, 11, -4], np.int64),
        np.array([1.0, 3.0, 5.0, 5.0, 8.0], np.float32),
        np.array([100, 101, 102, 103, 104], np.int64)),
    1: (np.array([0, 11], np.int64), np.array([2.5, 5.0], np.float32), np.array([9, 8], np.int64)),
    2: (np.zeros(0, np.int64), np.zeros(0, np.float32), np.zeros(0, np.int64)),
}


def _one(s, d, t, since=None, length=4, **kw):
    r = R.pair_sequence(HIST, [s], [d], [t], None if since is None else [since], length, **kw)
    L = length
    assert r.lengths.dtype == np.int32 and r.lengths.shape == (1, 2)
    assert r.nodes.dtype == r.eids.dtype == np.int64 and r.counts.dtype == np.int32
    assert r.times.dtype == r.delta_t.dtype == np.float32
    assert r.nodes.shape == r.eids.shape == r.times.shape == r.delta_t.shape == (1, 2, L)
    assert r.counts.shape == (1, 2, L, 2)
    return r


def _planes(r):
    return (r.lengths[0].tolist(), r.nodes[0].tolist(), r.eids[0].tolist(), r.times[0].tolist(),
            r.delta_t[0].tolist(), r.counts[0].tolist())


def test_a_hub_and_a_tie_at_t():
    # at t = 5 the hub's two edges at 5 are not before t; node 1's edge at 5 neither
    assert _planes(_one(0, 1, 5.0)) == (
        [3, 2],
        [[0, 10, 11, -1], [1, 0, -1, -1]],
        [[-1, 100, 101, -1], [-1, 9, -1, -1]],
        [[5, 1, 3, 0], [5, 2.5, 0, 0]],
        [[0, 4, 2, 0], [0, 2.5, 0, 0]],
        [[[1, 1], [1, 0], [1, 0], [0, 0]], [[0, 1], [1, 1], [0, 0], [0, 0]]])
    # just after: the window of the hub is full at the bound L - 1 = 3, the newest three
    r = _planes(_one(0, 1, 5.5))
    assert r[0] == [4, 3] and r[1] == [[0, 11, 1, 11], [1, 0, 11, -1]]
    assert r[2] == [[-1, 101, 102, 103], [-1, 9, 8, -1]]
    assert r[4] == [[0, 2.5, 0.5, 0.5], [0, 3, 0.5, 0]]
    # 11 occurs twice on the hub's side and once on node 1's; 1 is node 1's self slot
    assert r[5] == [[[1, 1], [2, 1], [1, 1], [2, 1]], [[1, 1], [1, 1], [2, 1], [0, 0]]]


def test_empty_nodes_give_the_self_slots_alone():
    for s, d in ((2, 7), (7, 2)):
        assert _planes(_one(s, d, 100.0, length=3)) == (
            [1, 1], [[s, -1, -1], [d, -1, -1]], [[-1] * 3] * 2, [[100, 0, 0]] * 2,
            [[0, 0, 0]] * 2, [[[1, 0], [0, 0], [0, 0]], [[0, 1], [0, 0], [0, 0]]])
    # nothing before t = 1 on the hub either
    assert _planes(_one(0, 0, 1.0, length=2))[0] == [1, 1]


def test_negative_and_unknown_ends_and_src_equal_dst():
    hub = ([0, 11, -4], [-1, 103, 104], [9, 5, 8], [0, 4, 1])
    for other in (-3, 1 << 40):
        own = 0 if other < 0 else 1      # a negative id is nobody's neighbour, not even its own
        lone = ([other, -1, -1], [-1] * 3, [9, 0, 0], [0, 0, 0])
        r = _planes(_one(other, 0, 9.0, length=3))
        assert r[0] == [1, 3] and list(r[1:5]) == [[a, b] for a, b in zip(lone, hub)]
        assert r[5] == [[[own, 0], [0, 0], [0, 0]], [[0, 1], [0, 1], [0, 0]]]
        r = _planes(_one(0, other, 9.0, length=3))
        assert r[0] == [3, 1] and r[1] == [hub[0], lone[0]] and r[4] == [hub[3], lone[3]]
        assert r[5] == [[[1, 0], [1, 0], [0, 0]], [[0, own], [0, 0], [0, 0]]]
    r = _planes(_one(0, 0, 9.0, length=3))
    assert r[0] == [3, 3] and r[1] == [hub[0]] * 2 and r[2] == [hub[1]] * 2
    assert r[5] == [[[1, 1], [1, 1], [0, 0]]] * 2      # the stored -4 is counted nowhere


def test_since_and_nan():
    # since is inclusive and comes before the bound
    r = _planes(_one(0, 1, 9.0, since=5.0))
    assert r[0] == [4, 2] and r[1] == [[0, 1, 11, -4], [1, 11, -1, -1]]
    assert _planes(_one(0, 1, 9.0, since=9.0))[0] == [1, 1]
    assert _planes(_one(0, 1, 9.0, since=NAN)) == _planes(_one(0, 1, 9.0))
    # a NaN time considers nothing; the self slot's time is that NaN and its delta NaN - NaN
    r = _one(0, 1, NAN)
    assert r.lengths.tolist() == [[1, 1]] and np.isnan(r.times[0, :, 0]).all()
    assert np.isnan(r.delta_t[0, :, 0]).all() and not r.delta_t[0, :, 1:].view(np.int32).any()


def test_table_parts_a_short_table_and_the_time_argument():
    node_tab = -np.arange(11 * 3, dtype=np.float32).reshape(11, 3) - 1     # id 11 has no row
    edge_tab = np.arange(104 * 2, dtype=np.float32).reshape(104, 2) + 1    # eid 104 has no row
    w, b = np.array([[1.0], [0.1]], np.float32), np.array([0.5, -1.0], np.float32)
    r = _one(0, 1, 9.0, node_feats=node_tab, edge_feats=edge_tab, weight=w, bias=b)
    assert r.nodes[0].tolist() == [[0, 1, 11, -4], [1, 0, 11, -1]]
    assert r.eids[0].tolist() == [[-1, 102, 103, 104], [-1, 9, 8, -1]]
    assert r.node.shape == (1, 2, 4, 3) and r.edge.shape == (1, 2, 4, 2)
    assert r.arg.shape == (1, 2, 4, 2)
    assert r.node.dtype == r.edge.dtype == r.arg.dtype == np.float32
    zero3, zero2 = [0.0] * 3, [0.0] * 2
    # the self slot has the node's own row; 11 and -4 have none; then the padding
    assert r.node[0].tolist() == [
        [node_tab[0].tolist(), node_tab[1].tolist(), zero3, zero3],
        [node_tab[1].tolist(), node_tab[0].tolist(), zero3, zero3]]
    # the self slot's eid is -1: the zero row; eid 104 has none
    assert r.edge[0].tolist() == [
        [zero2, edge_tab[102].tolist(), edge_tab[103].tolist(), zero2],
        [zero2, edge_tab[9].tolist(), edge_tab[8].tolist(), zero2]]
    assert r.delta_t[0].tolist() == [[0, 4, 4, 1], [0, 6.5, 4, 0]]
    dt = np.array([0, 4, 4, 1, 0, 6.5, 4], np.float32)
    want = np.stack([dt * np.float32(1.0) + np.float32(0.5),
                     (dt * np.float32(0.1)).astype(np.float32) + np.float32(-1.0)], axis=1)
    got = r.arg[0].reshape(8, 2)
    assert np.array_equal(got[:7].view(np.int32), want.astype(np.float32).view(np.int32))
    assert got[0].tolist() == [0.5, -1.0]      # the self slot is encoded: the bias shows
    # a padded slot is +0.0 in every part, the bias does not show
    assert not got[7].view(np.int32).any()
    assert not r.node[0, 1, 3].view(np.int32).any() and not r.edge[0, 1, 3].view(np.int32).any()
    none = _one(0, 1, 9.0)
    assert none.node is None and none.edge is None and none.arg is None


def test_many_rows_and_a_broadcast_since():
    r = R.pair_sequence(HIST, [0, 1, 2], [1, 0, 0], [9.0, 9.0, 4.0], 3.0, 3)
    assert r.lengths.tolist() == [[3, 2], [2, 3], [1, 2]]
    assert r.nodes.tolist() == [[[0, 11, -4], [1, 11, -1]], [[1, 11, -1], [0, 11, -4]],
                                [[2, -1, -1], [0, 11, -1]]]
    assert r.delta_t.tolist() == [[[0, 4, 1], [0, 4, 0]], [[0, 4, 0], [0, 4, 1]],
                                  [[0, 0, 0], [0, 1, 0]]]
