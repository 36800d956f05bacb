"""tests/neighbor_sequence_ref.py on hand-written histories, every expected value written out by
hand: the GPU tests compare the kernel with this restatement, so it is checked on its own first."""
import numpy as np

from tests import neighbor_sequence_ref as R

NAN = float("nan")
# node 0: five edges, two of them at t = 5; node 1: one edge; node 2: known, no edges
HIST = {
    0: (np.array([10, 11, 12, 13, -4], np.int64),
        np.array([1.0, 3.0, 5.0, 5.0, 8.0], np.float32),
        np.array([100, 101, 102, 103, 104], np.int64)),
    1: (np.array([7], np.int64), np.array([2.5], np.float32), np.array([9], np.int64)),
    2: (np.zeros(0, np.int64), np.zeros(0, np.float32), np.zeros(0, np.int64)),
}


def _one(node, t, since=None, length=4, **kw):
    s = R.neighbor_sequence(HIST, [node], [t], None if since is None else [since], length, **kw)
    assert s.lengths.dtype == np.int32 and s.nodes.dtype == s.eids.dtype == np.int64
    assert s.times.dtype == s.delta_t.dtype == np.float32
    assert s.nodes.shape == s.eids.shape == s.times.shape == s.delta_t.shape == (1, length)
    return s


def _planes(s):
    return (int(s.lengths[0]), s.nodes[0].tolist(), s.eids[0].tolist(), s.times[0].tolist(),
            s.delta_t[0].tolist())


def test_empty_histories_give_all_padding():
    for node in (2, 5, -1, 1 << 40):
        assert _planes(_one(node, 100.0)) == (0, [-1] * 4, [-1] * 4, [0.0] * 4, [0.0] * 4)
    assert _planes(_one(0, 1.0)) == (0, [-1] * 4, [-1] * 4, [0.0] * 4, [0.0] * 4)   # nothing < 1


def test_one_edge():
    assert _planes(_one(1, 3.0)) == (1, [7, -1, -1, -1], [9, -1, -1, -1], [2.5, 0, 0, 0],
                                     [0.5, 0, 0, 0])
    assert _planes(_one(1, 2.5))[0] == 0                      # the edge's own time: not before
    assert _planes(_one(1, 3.0, length=1)) == (1, [7], [9], [2.5], [0.5])


def test_a_tie_at_t_is_excluded():
    assert _planes(_one(0, 5.0)) == (2, [10, 11, -1, -1], [100, 101, -1, -1], [1, 3, 0, 0],
                                     [4, 2, 0, 0])
    assert _planes(_one(0, 5.5)) == (4, [10, 11, 12, 13], [100, 101, 102, 103], [1, 3, 5, 5],
                                     [4.5, 2.5, 0.5, 0.5])


def test_since_is_inclusive_and_above_t_is_empty():
    assert _planes(_one(0, 9.0, since=5.0)) == (3, [12, 13, -4, -1], [102, 103, 104, -1],
                                                [5, 5, 8, 0], [4, 4, 1, 0])
    assert _planes(_one(0, 9.0, since=5.5)) == (1, [-4, -1, -1, -1], [104, -1, -1, -1],
                                                [8, 0, 0, 0], [1, 0, 0, 0])
    assert _planes(_one(0, 5.0, since=7.0))[0] == 0           # since above t
    assert _planes(_one(0, 9.0, since=9.0))[0] == 0


def test_nan_t_and_nan_since():
    assert _planes(_one(0, NAN)) == (0, [-1] * 4, [-1] * 4, [0.0] * 4, [0.0] * 4)
    assert _planes(_one(0, NAN, since=0.0))[0] == 0
    assert _planes(_one(0, 4.0, since=NAN)) == _planes(_one(0, 4.0))      # no lower end
    assert _planes(_one(0, 4.0))[0] == 2


def test_length_below_at_and_above_the_window():
    # the window at t = 9 has five edges: the newest `length`, oldest first
    assert _planes(_one(0, 9.0, length=2)) == (2, [13, -4], [103, 104], [5, 8], [4, 1])
    assert _planes(_one(0, 9.0, length=5)) == (5, [10, 11, 12, 13, -4], [100, 101, 102, 103, 104],
                                               [1, 3, 5, 5, 8], [8, 6, 4, 4, 1])
    s = _planes(_one(0, 9.0, length=7))
    assert s[0] == 5 and s[1] == [10, 11, 12, 13, -4, -1, -1] and s[3][5:] == [0, 0]
    # the bound comes after since
    assert _planes(_one(0, 9.0, since=3.0, length=2)) == (2, [13, -4], [103, 104], [5, 8], [4, 1])
    assert _planes(_one(0, 6.0, since=3.0, length=2)) == (2, [12, 13], [102, 103], [5, 5], [1, 1])


def test_table_parts_and_the_time_argument():
    edge_tab = np.arange(104 * 2, dtype=np.float32).reshape(104, 2)      # eid 104 has no row
    node_tab = -np.arange(13 * 3, dtype=np.float32).reshape(13, 3)       # ids 13 and -4 have none
    w, b = np.array([[1.0], [0.1]], np.float32), np.array([0.5, -1.0], np.float32)
    s = _one(0, 9.0, length=6, edge_feats=edge_tab, node_feats=node_tab, weight=w, bias=b)
    assert s.edge.shape == (1, 6, 2) and s.node.shape == (1, 6, 3) and s.arg.shape == (1, 6, 2)
    assert s.edge.dtype == s.node.dtype == s.arg.dtype == np.float32
    assert np.array_equal(s.edge[0, :4], edge_tab[[100, 101, 102, 103]])
    assert not s.edge[0, 4:].any()                            # eid 104, then the padding
    assert np.array_equal(s.node[0, :3], node_tab[[10, 11, 12]])
    assert not s.node[0, 3:].any()                            # 13, -4, then the padding
    dt = np.array([8, 6, 4, 4, 1], np.float32)
    want = np.stack([dt * np.float32(1.0) + np.float32(0.5),
                     (dt * np.float32(0.1)).astype(np.float32) + np.float32(-1.0)], axis=1)
    assert np.array_equal(s.arg[0, :5].view(np.int32), want.astype(np.float32).view(np.int32))
    # a padded slot is +0.0 in every part, the bias does not show
    for part in (s.edge, s.node, s.arg):
        assert not part[0, 5:].view(np.int32).any()
    none = _one(0, 9.0)
    assert none.edge is None and none.node is None and none.arg is None


def test_many_rows_and_a_broadcast_since():
    s = R.neighbor_sequence(HIST, [0, 1, 2, 0], [9.0, 9.0, 9.0, 4.0], 3.0, 3)
    assert s.lengths.tolist() == [3, 0, 0, 1]
    assert s.nodes.tolist() == [[12, 13, -4], [-1] * 3, [-1] * 3, [11, -1, -1]]
    assert s.delta_t.tolist() == [[4, 4, 1], [0] * 3, [0] * 3, [1, 0, 0]]
