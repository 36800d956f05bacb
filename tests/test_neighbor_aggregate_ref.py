"""tests/neighbor_aggregate_ref.py against a brute-force float64 computation from the raw edge
list, on a 40-node toy and without a device: the reference that the GPU test compares bits with
is itself checked here, by code that shares nothing with it but the edge list.

Counts are exact.  A float32 sum of n terms added left to right differs from the exact sum by at
most gamma_(n-1) * sum|x| <= n * eps32 * sum|x| (Higham, Accuracy and Stability of Numerical
Algorithms, section 4.2; eps32 = 2^-23 is twice the unit roundoff, which covers the higher-order
terms for every n here), and the float64 sum of at most 500 float32 values is exact to far below
that.  The mean adds one correctly rounded division: (n + 1) * eps32 * sum|x| / n."""
import numpy as np
import pytest

from tests import neighbor_aggregate_ref as R

NODES, HUB, TIE = 40, 0, 50.0
EPS32 = float(np.finfo(np.float32).eps)


def _edges():
    rng = np.random.RandomState(5)
    hub_n, rest_n = 300, 260
    src = np.concatenate([[HUB] * hub_n, rng.choice(np.arange(1, 30), rest_n), [HUB] * 5, [30]])
    dst = np.concatenate([rng.choice(np.arange(1, 39), hub_n), rng.choice(np.arange(0, 39), rest_n),
                          [21, 22, 23, 24, 21], [7]])
    t = np.concatenate([np.floor(rng.rand(hub_n + rest_n) * 100), [TIE] * 5, [40.0]])
    order = np.argsort(t, kind="stable")
    return (src[order].astype(np.int64), dst[order].astype(np.int64),
            t[order].astype(np.float32), np.arange(len(t), dtype=np.int64))


def _histories(edges):
    """What the store holds per source: its edges in ingest order (ascending time, stable)."""
    src, dst, t, eid = edges
    return {v: (dst[src == v], t[src == v], eid[src == v]) for v in range(NODES)}


def _brute(edges, v, t, lo, H, table, by_eid):
    """(n, float64 sum [d], float64 sum of |x| [d]) of row (v, t, lo, H), from the edge list."""
    src, dst, ets, eid = edges
    t, keep = np.float32(t), []
    for k in range(len(src)):                      # the list ascends in time
        if src[k] != v or not ets[k] < t:          # NaN t: nothing is before it
            continue
        if lo is not None and not np.isnan(np.float32(lo)) and ets[k] < np.float32(lo):
            continue
        keep.append(k)
    if H:
        keep = keep[-H:] if len(keep) > H else keep
    total = np.zeros(table.shape[1], np.float64)
    mag = np.zeros(table.shape[1], np.float64)
    for k in keep:
        i = eid[k] if by_eid else dst[k]
        if 0 <= i < len(table):
            total += table[i].astype(np.float64)
            mag += np.abs(table[i].astype(np.float64))
    return len(keep), total, mag


@pytest.fixture(scope="module")
def toy():
    edges = _edges()
    rng = np.random.RandomState(1)
    node_tab = rng.randn(25, 5).astype(np.float32)             # ids 25 .. 39 have no row
    edge_tab = rng.randn(len(edges[0]) - 100, 3).astype(np.float32)
    return edges, _histories(edges), node_tab, edge_tab


def _check(toy, nodes, ts, since, H):
    edges, hist, node_tab, edge_tab = toy
    nodes, ts = np.asarray(nodes, np.int64), np.asarray(ts, np.float32)
    lows = None if since is None else np.broadcast_to(np.asarray(since, np.float32), ts.shape)
    for reduce in ("sum", "mean"):
        count, node, edge = R.neighbor_aggregate(hist, nodes, ts, node_tab, edge_tab, since, H,
                                                 reduce)
        assert count.dtype == np.int64 and node.dtype == np.float32 and edge.dtype == np.float32
        for i in range(len(nodes)):
            lo = None if lows is None else lows[i]
            for got, tab, by_eid in ((node[i], node_tab, False), (edge[i], edge_tab, True)):
                n, total, mag = _brute(edges, int(nodes[i]), ts[i], lo, H, tab, by_eid)
                assert count[i] == n
                if n == 0:
                    assert not got.any()
                elif reduce == "sum":
                    assert (np.abs(got - total) <= n * EPS32 * mag).all()
                else:
                    assert (np.abs(got - total / n) <= (n + 1) * EPS32 * mag / n).all()
    return count


def test_every_node_at_four_times(toy):
    nodes = np.tile(np.arange(NODES), 4)
    ts = np.repeat(np.array([-1.0, TIE, 33.5, 1e9], np.float32), NODES)
    count = _check(toy, nodes, ts, None, 0)
    assert count[ts == -1.0].sum() == 0 and count[nodes == HUB].max() == 305
    assert count[nodes == 37].sum() == 0                           # a node without edges


def test_a_tie_at_t_is_not_considered_and_a_nan_time_considers_nothing(toy):
    edges, hist = toy[0], toy[1]
    at_tie = int((hist[HUB][1] == TIE).sum())
    assert at_tie >= 5
    count = _check(toy, [HUB, HUB, HUB], [TIE, np.nextafter(np.float32(TIE), np.float32(100)),
                                         np.nan], None, 0)
    assert count[1] - count[0] == at_tie and count[2] == 0


@pytest.mark.parametrize("since", [np.nan, -np.inf, np.inf, TIE, 1e10])
def test_the_lower_end(toy, since):
    nodes = np.arange(NODES)
    ts = np.full(NODES, 70.0, np.float32)
    count = _check(toy, nodes, ts, since, 0)
    whole = _check(toy, nodes, ts, None, 0)
    if np.isnan(since) or since == -np.inf:
        assert np.array_equal(count, whole)                        # no lower end
    elif since > 70.0:
        assert count.sum() == 0                                    # above t: empty
    else:
        assert 0 < count.sum() < whole.sum()                       # inclusive at the tie
        _, hub_ts, _ = toy[1][HUB]
        assert count[HUB] == int(((hub_ts >= TIE) & (hub_ts < 70.0)).sum())


def test_a_lower_end_per_row(toy):
    nodes = np.tile(np.arange(NODES), 2)
    ts = np.repeat(np.array([TIE, 1e9], np.float32), NODES)
    with np.errstate(invalid="ignore"):
        cols = np.stack([np.full(len(ts), -np.inf), np.full(len(ts), np.nan),
                         np.full(len(ts), TIE), ts + 10.0])
    _check(toy, nodes, ts, cols[np.arange(len(ts)) % 4, np.arange(len(ts))].astype(np.float32), 0)
    _check(toy, nodes, ts, 40.0, 7)


def test_max_history_of_1_n_and_n_plus_1(toy):
    n = len(toy[1][3][0])                                          # node 3's whole history
    assert n >= 3
    for H in (1, n - 1, n, n + 1):
        count = _check(toy, [3, HUB, 30], [1e9, 1e9, 1e9], None, H)
        assert count[0] == min(n, H) and count[1] == min(305, H) and count[2] == 1


def test_missing_rows_count_and_add_nothing(toy):
    edges, hist, node_tab, edge_tab = toy
    count, node, _ = R.neighbor_aggregate(hist, [HUB], [1e9], node_tab, None, None, 0, "sum")
    assert (hist[HUB][0] >= len(node_tab)).any() and count[0] == len(hist[HUB][0])
    ones = np.ones((25, 2), np.float32)
    _, mean, _ = R.neighbor_aggregate(hist, [HUB], [1e9], ones, None, None, 0, "mean")
    known = int((hist[HUB][0] < 25).sum())
    assert mean[0, 0] == np.float32(known) / np.float32(count[0]) < 1
    # out of range on both sides, and a table given alone
    _, none, edge = R.neighbor_aggregate(hist, [-1, NODES, 1 << 40], [1e9] * 3, None, edge_tab)
    assert none is None and not edge.any()


def test_the_sum_is_sequential_not_pairwise():
    """A column on which the order of the float32 additions shows: left to right every 1.0
    next to 1e8 is lost and the sum is 1, any regrouping that pairs the 1e8s keeps more."""
    col = np.array([1e8, 1.0, -1e8, 1.0] * 64, np.float32).reshape(-1, 1)
    want = np.float32(0)
    for x in col[:, 0]:
        want = np.float32(want + x)
    got = R.sequential_sum(col, np.arange(len(col)))
    assert got[0] == want and got.dtype == np.float32
    assert want == 1.0 and col.astype(np.float64).sum() == 128.0
