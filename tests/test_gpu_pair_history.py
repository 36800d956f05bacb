"""DynamicGraph.pair_history (csrc/pair_history.hip) on the GPU against tests/pair_history_ref.py:
all three outputs exactly equal, last_ts bit for bit.

The graph has 40 node ids and about 730 edges at whole-numbered times in [0, 100), so timestamps
repeat: node 0 is a hub with 300 edges to destinations 1 .. 12 and 130 more to node 13 (over 64
lanes some lane holds three or more matches, and the count exceeds 128), and five edges at exactly
t = 50 to 21 .. 24, which it meets at no other time, two of them to 21 (the last among equal
timestamps is told by its edge id); node 30 has one edge; node 38 is only ever a destination and
node 37 is never named (no edges); 39 ends the node table.  The expected values come from
graph.get_temporal_neighbors per node through the numpy restatement, computed once per
(since, max_history) and left unchanged."""
import numpy as np
import pytest
import torch

from tests import pair_history_ref as P

pytestmark = pytest.mark.gpu

NODES, HUB, SINGLE, ONLY_DST, ABSENT = 40, 0, 30, 38, 37
HUB_OFTEN = 13                   # the hub's 130 extra edges lead here
NEVER_DST = 36                   # no edge leads here
TIE = 50.0
TIE_DSTS = [21, 22, 23, 24, 21]  # the hub meets them at t = TIE and never else; 21 twice
TIMES = [-1.0, TIE, 33.5, 1e9]


def _edges():
    rng = np.random.RandomState(11)
    hub_n, often_n, rest_n = 300, 130, 290
    hub_dst = rng.choice(np.arange(1, 13), hub_n)
    hub_t = np.floor(rng.rand(hub_n) * 100)
    often_t = np.floor(rng.rand(often_n) * 100)
    src = rng.choice(np.arange(1, 30), rest_n)
    dst = rng.choice(np.arange(0, 30), rest_n)
    t = np.floor(rng.rand(rest_n) * 100)
    k = len(TIE_DSTS)
    src = np.concatenate([[HUB] * hub_n, [HUB] * often_n, src, [HUB] * k, [SINGLE], [5], [6]])
    dst = np.concatenate([hub_dst, [HUB_OFTEN] * often_n, dst, TIE_DSTS, [7], [ONLY_DST],
                          [NODES - 1]])
    t = np.concatenate([hub_t, often_t, t, [TIE] * k, [40.0], [60.0], [99.0]])
    order = np.argsort(t, kind="stable")
    return src[order].astype(np.int64), dst[order].astype(np.int64), t[order].astype(np.float32)


def _new_graph(edges=None, add_reverse=False):
    import gnnflow_amd
    g = gnnflow_amd.DynamicGraph(1 << 20, 1 << 28, "cuda", 8, 128, "insert")
    if edges is not None:
        g.add_edges(*edges, add_reverse=add_reverse)
    return g


def _queries(edges):
    """Every node before every edge, on the tie, between two times and after every edge, each
    with a destination it meets, one nobody meets, the hub's frequent one, a negative and an
    unknown id; the hub with each tie destination; NaN times; sources that are negative, at and
    past the table's end."""
    e_src, e_dst, _ = edges
    src, dst, ts = [], [], []
    for t in TIMES:
        for v in range(NODES):
            own = e_dst[e_src == v]
            met = int(own[len(own) // 2]) if len(own) else 7
            for d in (met, NEVER_DST, HUB_OFTEN, -5, 1000):
                src.append(v), dst.append(d), ts.append(t)
        for d in TIE_DSTS[:4]:
            src.append(HUB), dst.append(d), ts.append(t)
    for v, d in ((HUB, HUB_OFTEN), (3, 7)):
        src.append(v), dst.append(d), ts.append(np.nan)
    for v in (-3, -1, NODES, 1000, 1 << 40):
        src.append(v), dst.append(HUB_OFTEN), ts.append(1e9)
    return np.array(src, np.int64), np.array(dst, np.int64), np.array(ts, np.float32)


def _since(kind, ts):
    """None, the scalar 40.0, or a tensor's worth: -inf, NaN, the tie's time exactly and a value
    above the row's own time, in turn."""
    if kind == "tensor":
        with np.errstate(invalid="ignore"):
            cols = np.stack([np.full(len(ts), -np.inf), np.full(len(ts), np.nan),
                             np.full(len(ts), TIE), ts + 10.0])
        return cols[np.arange(len(ts)) % 4, np.arange(len(ts))].astype(np.float32)
    return {"none": None, "scalar": 40.0}[kind]


def _row(toy, v, d, t):
    hit = np.flatnonzero((toy.src == v) & (toy.dst == d) & (toy.ts == np.float32(t)))
    assert len(hit) >= 1
    return int(hit[0])


class Toy:
    pass


@pytest.fixture(scope="module")
def toy():
    t = Toy()
    t.edges = _edges()
    t.graph = _new_graph(t.edges)
    t.src, t.dst, t.ts = _queries(t.edges)
    t.hist = P.from_graph(t.graph, t.src)
    t.d_src, t.d_dst, t.d_ts = (torch.from_numpy(x).cuda() for x in (t.src, t.dst, t.ts))
    t.ref = {}
    return t


def _want(toy, kind="none", max_history=0):
    if (kind, max_history) not in toy.ref:
        toy.ref[kind, max_history] = P.pair_history(toy.hist, toy.src, toy.dst, toy.ts,
                                                    _since(kind, toy.ts), max_history)
    return toy.ref[kind, max_history]


def _d_since(kind, ts):
    s = _since(kind, ts)
    return torch.from_numpy(s).cuda() if isinstance(s, np.ndarray) else s


def _host(out, n):
    assert out.count.dtype == torch.int64 and out.last_ts.dtype == torch.float32 and \
        out.last_eid.dtype == torch.int64
    for x in out:
        assert x.is_cuda and x.is_contiguous() and tuple(x.shape) == (n,)
    return tuple(x.cpu().numpy() for x in out)


def _same(got, want, rows=None):
    """count and last_eid equal, last_ts equal bit for bit."""
    if rows is not None:
        want = tuple(w[rows] for w in want)
    assert np.array_equal(got[0], want[0])
    assert np.array_equal(got[1].view(np.int32), want[1].view(np.int32))
    assert np.array_equal(got[2], want[2])


def _call(graph, src, dst, ts, since=None, max_history=0):
    if isinstance(since, np.ndarray):
        since = torch.from_numpy(since).cuda()
    out = graph.pair_history(torch.from_numpy(src).cuda(), torch.from_numpy(dst).cuda(),
                             torch.from_numpy(ts).cuda(), since=since, max_history=max_history)
    return _host(out, len(src))


def test_the_graph_and_the_reference_exercise_every_case(toy):
    """Computed from the store and the reference alone: the comparisons below are not vacuous."""
    h = toy.hist
    assert toy.graph.max_vertex_id() == NODES - 1 and 720 <= toy.graph.num_edges() <= 745
    assert len(h[HUB][0]) >= 430 and len(h[SINGLE][0]) == 1
    assert len(h[ONLY_DST][0]) == 0 and len(h[ABSENT][0]) == 0
    assert np.count_nonzero(h[HUB][1] == TIE) >= 5
    assert not any((hh[0] == NEVER_DST).any() for hh in h.values())
    count, last_ts, last_eid = _want(toy)
    often = _row(toy, HUB, HUB_OFTEN, 1e9)
    assert count[often] == 130 > 128                                # three matches in some lane
    assert 0 < count[_row(toy, HUB, HUB_OFTEN, TIE)] < count[often]
    none = count == 0
    assert none.sum() > 50 and (last_eid[none] == -1).all() and np.isneginf(last_ts[none]).all()
    assert (~none).sum() > 50 and (last_eid[~none] >= 0).all() and \
        np.isfinite(last_ts[~none]).all()
    assert (count[toy.ts == -1.0] == 0).all()                        # before every edge
    assert (count[np.isnan(toy.ts)] == 0).all() and np.isnan(toy.ts).sum() == 2
    assert (count[(toy.src < 0) | (toy.src >= NODES)] == 0).all()
    assert (count[np.isin(toy.dst, [-5, 1000, NEVER_DST])] == 0).all()
    for d in TIE_DSTS[:4]:
        assert count[_row(toy, HUB, d, TIE)] == 0                    # strictly before
        assert count[_row(toy, HUB, d, 1e9)] == TIE_DSTS.count(d)
    # two edges to 21 at the same time: the last is the later one in the store's order
    r21 = _row(toy, HUB, 21, 1e9)
    eids21 = h[HUB][2][(h[HUB][0] == 21)]
    assert len(eids21) == 2 and eids21[0] != eids21[1]
    assert last_eid[r21] == eids21[1] and last_ts[r21] == np.float32(TIE)
    newest_first = toy.graph.get_temporal_neighbors(HUB)
    assert newest_first[2][np.flatnonzero(newest_first[0] == 21)[0]] == last_eid[r21]
    assert count[_row(toy, SINGLE, 7, 1e9)] == 1 and count[_row(toy, SINGLE, 7, 33.5)] == 0
    # the bound is visible: smaller totals with max_history 1 and 5 than with the whole history
    totals = [int(_want(toy, "none", m)[0].sum()) for m in (1, 5, 0)]
    assert 0 < totals[0] < totals[1] < totals[2]
    # and so is the lower end: a row strictly between nothing and everything
    assert 0 < _want(toy, "scalar")[0][often] < count[often]
    mixed = _want(toy, "tensor")[0]
    assert 0 < mixed.sum() < count.sum()


@pytest.mark.parametrize("kind", ["none", "scalar", "tensor"])
@pytest.mark.parametrize("max_history", [0, 1, 5, 1000])
def test_outputs_match_the_reference(toy, max_history, kind):
    out = toy.graph.pair_history(toy.d_src, toy.d_dst, toy.d_ts, since=_d_since(kind, toy.ts),
                                 max_history=max_history)
    got = _host(out, len(toy.src))
    _same(got, _want(toy, kind, max_history))
    if max_history == 1000:                                          # more than any history
        _same(got, _want(toy, kind, 0))


def test_empty_batch_and_repeat_calls(toy):
    empty = toy.graph.pair_history(toy.d_src[:0], toy.d_dst[:0], toy.d_ts[:0])
    assert [tuple(x.shape) for x in empty] == [(0,)] * 3
    assert [x.dtype for x in empty] == [torch.int64, torch.float32, torch.int64]
    a = toy.graph.pair_history(toy.d_src, toy.d_dst, toy.d_ts, since=40.0, max_history=5)
    b = toy.graph.pair_history(toy.d_src, toy.d_dst, toy.d_ts, since=40.0, max_history=5)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    _same(_host(a, len(toy.src)), _want(toy, "scalar", 5))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        c = toy.graph.pair_history(toy.d_src, toy.d_dst, toy.d_ts, since=40.0, max_history=5)
    side.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(a, c))


def test_row_slices_and_strided_views_are_taken_for_what_they_hold(toy):
    d_since = _d_since("tensor", toy.ts)
    a = toy.graph.pair_history(toy.d_src, toy.d_dst, toy.d_ts, since=d_since, max_history=5)
    d = toy.graph.pair_history(toy.d_src[40:280], toy.d_dst[40:280], toy.d_ts[40:280],
                               since=d_since[40:280], max_history=5)
    assert all(torch.equal(x, y[40:280]) for x, y in zip(d, a))
    e = toy.graph.pair_history(toy.d_src[::2], toy.d_dst[::2], toy.d_ts[::2],
                               since=d_since[::2], max_history=5)
    assert all(torch.equal(x, y[::2]) for x, y in zip(e, a))


def test_rows_past_the_grid_limit_are_grid_strided(toy):
    """The launch has at most 4096 workgroups of four rows: more rows than that, the queries
    repeated, so that the expected rows are the reference's rows repeated."""
    rows = 4 * 4096 + 37
    idx = torch.arange(rows, device="cuda") % len(toy.src)
    out = toy.graph.pair_history(toy.d_src[idx], toy.d_dst[idx], toy.d_ts[idx],
                                 since=_d_since("tensor", toy.ts)[idx], max_history=5)
    _same(_host(out, rows), _want(toy, "tensor", 5), idx.cpu().numpy())


def test_arguments_are_checked_on_the_gpu_too(toy):
    with pytest.raises(ValueError, match="the graph is on device"):
        toy.graph.pair_history(toy.d_src.cpu(), toy.d_dst.cpu(), toy.d_ts.cpu())
    with pytest.raises(ValueError, match="dst is on"):
        toy.graph.pair_history(toy.d_src, toy.d_dst.cpu(), toy.d_ts)
    with pytest.raises(ValueError, match="since is on"):
        toy.graph.pair_history(toy.d_src, toy.d_dst, toy.d_ts, since=toy.d_ts.cpu())
    with pytest.raises(ValueError, match="ts has"):
        toy.graph.pair_history(toy.d_src, toy.d_dst, toy.d_ts[:-1])
    with pytest.raises(TypeError, match="max_history"):
        toy.graph.pair_history(toy.d_src, toy.d_dst, toy.d_ts, max_history=True)
    with pytest.raises(TypeError, match="dst"):
        toy.graph.pair_history(toy.d_src, toy.d_dst.int(), toy.d_ts)


def test_a_graph_without_nodes_fills_its_outputs():
    graph = _new_graph()
    src = np.array([0, 5, -1], np.int64)
    got = _call(graph, src, src, np.array([1e9, 0.0, np.nan], np.float32), since=0.0)
    assert got[0].tolist() == [0, 0, 0] and got[2].tolist() == [-1, -1, -1]
    assert np.isneginf(got[1]).all()


def test_edges_added_later_are_seen(toy):
    src, dst, t = toy.edges
    cut = 400
    graph = _new_graph((src[:cut], dst[:cut], t[:cut]))
    first = _call(graph, toy.src, toy.dst, toy.ts)
    _same(first, P.pair_history(P.from_graph(graph, toy.src), toy.src, toy.dst, toy.ts))
    torch.cuda.synchronize()      # add_edges moves segments: the launch above has completed
    graph.add_edges(src[cut:], dst[cut:], t[cut:])
    second = _call(graph, toy.src, toy.dst, toy.ts)
    _same(second, _want(toy))                                   # the same store as in one piece
    assert (second[0] >= first[0]).all() and second[0].sum() > first[0].sum()
    torch.cuda.synchronize()
    # and a burst that makes the hub's and a new node's segments grow, to a destination of the
    # queries that nobody had met
    graph.add_edges(np.array([HUB] * 40 + [31] * 9), np.full(49, NEVER_DST),
                    np.full(49, 200.0, np.float32))
    hist = P.from_graph(graph, toy.src)
    third = _call(graph, toy.src, toy.dst, toy.ts)
    _same(third, P.pair_history(hist, toy.src, toy.dst, toy.ts))
    r = _row(toy, HUB, NEVER_DST, 1e9)
    assert second[0][r] == 0 and third[0][r] == 40 and third[1][r] == np.float32(200.0)
    assert third[0][_row(toy, 31, NEVER_DST, 1e9)] == 9
    for kind, m in (("scalar", 5), ("tensor", 0)):
        s = _since(kind, toy.ts)
        _same(_call(graph, toy.src, toy.dst, toy.ts, s, m),
              P.pair_history(hist, toy.src, toy.dst, toy.ts, s, m))


def test_after_offload_only_live_edges_count(toy):
    src, dst, t = toy.edges
    graph = _new_graph((src[:400], dst[:400], t[:400]))
    graph.add_edges(src[400:], dst[400:], t[400:])
    before = _call(graph, toy.src, toy.dst, toy.ts)
    _same(before, _want(toy))
    torch.cuda.synchronize()
    edges_before = graph.num_edges()
    assert graph.offload_old_blocks(60.0) > 0 and graph.num_edges() < edges_before
    hist = P.from_graph(graph, toy.src)
    assert sum(len(h[0]) for h in hist.values()) < sum(len(h[0]) for h in toy.hist.values())
    for kind, m in (("none", 0), ("none", 5), ("tensor", 0), ("scalar", 5)):
        s = _since(kind, toy.ts)
        _same(_call(graph, toy.src, toy.dst, toy.ts, s, m),
              P.pair_history(hist, toy.src, toy.dst, toy.ts, s, m))
    after = _call(graph, toy.src, toy.dst, toy.ts)
    assert (after[0] <= before[0]).all() and after[0].sum() < before[0].sum()


def test_undirected_graph_counts_both_directions(toy):
    graph = _new_graph(toy.edges, add_reverse=True)
    hist = P.from_graph(graph, toy.src)
    assert len(hist[ONLY_DST][0]) == 1 and int(hist[ONLY_DST][0][0]) == 5
    for kind, m in (("none", 0), ("none", 5), ("tensor", 0)):
        s = _since(kind, toy.ts)
        _same(_call(graph, toy.src, toy.dst, toy.ts, s, m),
              P.pair_history(hist, toy.src, toy.dst, toy.ts, s, m))
    got = _call(graph, toy.src, toy.dst, toy.ts)
    assert (got[0] >= _want(toy)[0]).all() and got[0].sum() > _want(toy)[0].sum()
    # the bank is symmetric: (u, v) and (v, u) have the same count and the same last time (the
    # last edge id too where one edge is the last; among equal times each side has its own order)
    u = np.array([5, ONLY_DST, HUB, HUB_OFTEN, HUB, 21], np.int64)
    v = np.array([ONLY_DST, 5, HUB_OFTEN, HUB, 21, HUB], np.int64)
    sym = _call(graph, u, v, np.full(6, 1e9, np.float32))
    assert np.array_equal(sym[0][0::2], sym[0][1::2]) and sym[0][0] == 1
    assert sym[0][2] >= 130 and sym[0][4] >= 2
    assert np.array_equal(sym[1][0::2], sym[1][1::2])
    assert sym[2][0] == sym[2][1] >= 0
