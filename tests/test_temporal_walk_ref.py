"""CPU tests of tests/temporal_walk_ref.py, the numpy restatement the GPU tests compare
DynamicGraph.temporal_random_walk and ops.walk_position_counts with: the properties the rule
promises hold for the restatement itself."""
import numpy as np

from tests import hist_negatives_ref as H
from tests import temporal_walk_ref as T

NODES = 24


def _graph(add_reverse=False):
    """About 400 edges among 24 nodes at whole-numbered times in [0, 50): timestamps repeat, so
    nodes have ties; node 23 is only ever a destination."""
    rng = np.random.RandomState(5)
    n = 400
    src = rng.randint(0, NODES - 1, n)
    dst = rng.randint(0, NODES, n)
    ts = np.sort(np.floor(rng.rand(n) * 50)).astype(np.float32)
    return (src, dst, ts), T.from_edges(src, dst, ts, add_reverse=add_reverse)


def _roots(B=40, seed=3):
    """Random nodes at times on and between the edges' times; the first three before every edge."""
    rng = np.random.RandomState(seed)
    ts = np.floor(rng.rand(B) * 60).astype(np.float32) + np.float32(0.5) * (np.arange(B) % 2)
    ts[:3] = 0
    return rng.randint(0, NODES, B).astype(np.int64), ts


def test_every_step_is_an_edge_of_its_history_and_time_strictly_decreases():
    for reverse in (False, True):
        _, (hist, table_len) = _graph(reverse)
        src, ts = _roots()
        for recency, max_history in ((1, 0), (3, 0), (2, 4)):
            nodes, eids, times = T.walks(hist, table_len, src, ts, 5, 6, recency, max_history,
                                         seed=9)
            assert nodes.shape == (40, 6, 6) and eids.shape == times.shape == (40, 6, 5)
            assert (nodes[:, :, 0] == src[:, None]).all()
            taken = T.steps_taken(eids)
            assert taken.min() == 0 and taken.max() == 5
            for i in range(40):
                for w in range(6):
                    v, t = int(src[i]), ts[i]
                    for j in range(taken[i, w]):
                        h_dst, h_ts, h_eid = hist[v]
                        hit = np.flatnonzero((h_dst == nodes[i, w, j + 1]) & (h_eid == eids[i, w, j])
                                             & (h_ts == times[i, w, j]))
                        assert len(hit) >= 1
                        assert times[i, w, j] < t                     # strictly earlier
                        c = T.history_size(h_ts, t)
                        if max_history:                               # among the newest max_history
                            assert hit.max() >= c - max_history
                        assert hit.min() < c
                        v, t = int(nodes[i, w, j + 1]), times[i, w, j]
                    # from the step it ends on: -1, -1, 0
                    assert (nodes[i, w, taken[i, w] + 1:] == -1).all()
                    assert (eids[i, w, taken[i, w]:] == -1).all()
                    assert (times[i, w, taken[i, w]:] == 0).all()
                    if taken[i, w] < 5:                               # and it had to end there
                        assert not 0 <= v < table_len or T.history_size(hist[v][1], t) == 0


def test_a_tie_and_a_nan_start_end_the_walk():
    hist = {0: (np.array([1, 1, 2]), np.array([5, 5, 7], np.float32), np.array([10, 11, 12])),
            1: (np.array([0]), np.array([5], np.float32), np.array([13])),
            2: (np.zeros(0, np.int64), np.zeros(0, np.float32), np.zeros(0, np.int64))}
    src = np.array([0, 0, 0, 0, 1, 2, -1, 3], np.int64)
    ts = np.array([5.0, np.nan, 6.0, 8.0, 6.0, 9.0, 9.0, 9.0], np.float32)
    nodes, eids, times = T.walks(hist, 3, src, ts, 3, 4, seed=1)
    taken = T.steps_taken(eids)
    assert (taken[0] == 0).all()             # both edges of node 0 before 7 are AT 5: a tie
    assert (taken[1] == 0).all()             # NaN
    # from 6: one of the two edges at 5 to node 1, whose only edge is at 5 too: the tie ends it
    assert (taken[2] == 1).all() and (nodes[2, :, 1] == 1).all() and (times[2, :, 0] == 5).all()
    assert set(eids[2, :, 0]) <= {10, 11}
    assert (taken[3] == 1).all()             # 0 -(7)-> 2 has no edge; 0 -(5)-> 1 ends on the tie
    assert (taken[4] == 1).all() and (nodes[4, :, 1] == 0).all() and (nodes[4, :, 2] == -1).all()
    assert (taken[5:] == 0).all()            # no edges, a negative source, one past the table
    assert (nodes[:, :, 0] == src[:, None]).all() and (nodes[5:, :, 1:] == -1).all()


def test_one_draw_is_the_index_hist_negatives_draws_for_the_same_word():
    B, W, L, seed, epoch, first_row = 7, 5, 3, 0x1234, 6, 11
    u = T.words(B, W, L, 1, seed, epoch, first_row)
    c = np.array([1, 2, 3, 5, 64, 300, 2 ** 20], np.uint64)
    for j in range(L):
        # the same key: hist_negatives' attempt 0 under a seed that undoes the two tags, the
        # walk's call word as its epoch, K = W
        h = H.draws(c, first_row, 0, B, W, W, seed ^ T.SEED_TAG ^ H.SEED_TAG, (epoch << 8) + j)[0]
        for i in range(B):
            for w in range(W):
                assert int(T.pick(u[:, i, w, j], int(c[i]))) == h[w, i]
                assert 0 <= h[w, i] < c[i]


def test_walks_are_keyed_by_the_global_row_the_seed_and_the_epoch():
    _, (hist, table_len) = _graph(True)
    src, ts = _roots(30)
    kw = dict(length=4, num_walks=3, recency=2, max_history=0)
    whole = T.walks(hist, table_len, src, ts, seed=7, epoch=2, **kw)
    for a, b in ((0, 11), (11, 30), (29, 30)):
        part = T.walks(hist, table_len, src[a:b], ts[a:b], seed=7, epoch=2, first_row=a, **kw)
        for x, y in zip(part, whole):
            assert np.array_equal(x, y[a:b])
    shifted = T.walks(hist, table_len, src[11:], ts[11:], seed=7, epoch=2, **kw)
    assert not np.array_equal(shifted[1], whole[1][11:])
    for other in (dict(seed=8, epoch=2), dict(seed=7, epoch=3)):
        assert not np.array_equal(T.walks(hist, table_len, src, ts, **other, **kw)[1], whole[1])
    # the documented limit of the keying: at recency 2 a seed that differs by the XOR of the two
    # draws' tags (low bits only) keys the same two draws in the other order
    twin = 7 ^ T.SEED_TAG ^ (T.SEED_TAG + 1)
    assert twin != 7 and twin >> 5 == 7 >> 5
    assert np.array_equal(T.walks(hist, table_len, src, ts, seed=twin, epoch=2, **kw)[1], whole[1])
    # the epoch sits above the step in the call word: epoch e, step j is not epoch 0, step (e << 8) + j
    u = T.words(2, 2, 4, 2, seed=7, epoch=1)
    assert T.tids(5, 2, 3).tolist() == [[15, 16, 17], [18, 19, 20]]
    assert T.tids(2 ** 64 - 1, 2, 3).tolist() == [[2 ** 64 - 3, 2 ** 64 - 2, 2 ** 64 - 1], [0, 1, 2]]
    assert len(np.unique(u)) == u.size


def test_recency_is_the_maximum_of_p_uniform_draws():
    """n = 5 edges, 200 000 draws: every bin within 5 binomial standard deviations of
    ((k + 1)^p - k^p) / n^p.  The modulo-free mapping's bias is below n / 2^32; five sigma over
    ten bins is a false alarm below 1e-5, and the seeds are fixed."""
    n, draws = 5, 200000
    for p, seed in ((1, 101), (3, 103)):
        u = T.words(2000, 100, 1, p, seed=seed)
        x = T.pick(u.reshape(p, -1), n)
        assert x.shape == (draws,) and x.min() == 0 and x.max() == n - 1
        got = np.bincount(x, minlength=n)
        k = np.arange(n, dtype=np.float64)
        prob = ((k + 1) ** p - k ** p) / float(n) ** p
        sigma = np.sqrt(draws * prob * (1 - prob))
        assert (np.abs(got - draws * prob) <= 5 * sigma).all(), (p, got, draws * prob, sigma)
    # recency prefers the newest: the oldest of five edges 1 / 125 of the time
    assert got[0] < got[1] < got[2] < got[3] < got[4]


def test_position_counts_against_a_triple_loop():
    nodes = np.array([[[4, 7, 4], [4, 4, -1], [4, 9, 7]],
                      [[2, -1, -1], [2, 5, 2], [2, 5, 5]]], np.int64)
    ref = np.array([[[7, 4], [9, 4], [7, 7], [-1, -1]],
                    [[5, 2], [2, 2], [-1, 5], [0, 0]]], np.int64)
    for r in (None, ref):
        rr = nodes if r is None else r
        want = np.zeros(nodes.shape + (rr.shape[2],), np.int32)
        for i in range(nodes.shape[0]):
            for w in range(nodes.shape[1]):
                for j in range(nodes.shape[2]):
                    for p in range(rr.shape[2]):
                        if nodes[i, w, j] >= 0:
                            want[i, w, j, p] = sum(rr[i, v, p] == nodes[i, w, j]
                                                   for v in range(rr.shape[1]))
        got = T.position_counts(nodes, r)
        assert got.dtype == np.int32 and np.array_equal(got, want)
    own = T.position_counts(nodes)
    assert own[0, 0, 0].tolist() == [3, 1, 1] and own[0, 1, 2].tolist() == [0, 0, 0]
    assert own[1, 0, 0].tolist() == [3, 0, 1] and own[1, 2, 1].tolist() == [0, 2, 1]
    other = T.position_counts(nodes, ref)
    assert other[0, 0, 1].tolist() == [2, 1] and other[1, 0, 1].tolist() == [0, 0]
