"""DynamicGraph.temporal_random_walk (csrc/temporal_walk.hip) on the GPU against
tests/temporal_walk_ref.py, bit for bit.

The graph is the toy of tests/test_gpu_seen_mask.py, rebuilt here: 40 node ids and about 600
edges at whole-numbered times in [0, 100), so timestamps repeat: node 0 is a hub with about 300
edges and four edges at exactly t = 50 to destinations it meets at no other time; node 30 has one
edge; node 38 is only ever a destination and node 37 is never named (no edges); 39 ends the node
table.  It is built with and without reverse edges.  The histories come from
graph.get_temporal_neighbors per node and, a second time, from the edge arrays in numpy; the
expected walks are computed once per case and left unchanged."""
import numpy as np
import pytest
import torch

from tests import temporal_walk_ref as T

pytestmark = pytest.mark.gpu

NODES, HUB, SINGLE, ONLY_DST, ABSENT = 40, 0, 30, 38, 37
TIE = 50.0
TIE_DSTS = [21, 22, 23, 24]      # the hub meets them at t = TIE and never else

# (B, W, L): one walk; not multiples of 64 and a wave that spans roots; W above one wave
SHAPES = [(1, 1, 1), (67, 3, 4), (167, 70, 2)]
SEED, EPOCH = 0x5EED0123456789AB, 3


def _edges():
    rng = np.random.RandomState(11)
    hub_n, rest_n = 300, 290
    hub_dst = rng.choice(np.arange(1, 13), hub_n)
    hub_t = np.floor(rng.rand(hub_n) * 100)
    src = rng.choice(np.arange(1, 30), rest_n)
    dst = rng.choice(np.arange(0, 30), rest_n)
    t = np.floor(rng.rand(rest_n) * 100)
    src = np.concatenate([[HUB] * hub_n, src, [HUB] * 4, [SINGLE], [5], [6]])
    dst = np.concatenate([hub_dst, dst, TIE_DSTS, [7], [ONLY_DST], [NODES - 1]])
    t = np.concatenate([hub_t, t, [TIE] * 4, [40.0], [60.0], [99.0]])
    order = np.argsort(t, kind="stable")
    return src[order].astype(np.int64), dst[order].astype(np.int64), t[order].astype(np.float32)


def _new_graph(edges=None, add_reverse=False):
    import gnnflow_amd
    g = gnnflow_amd.DynamicGraph(1 << 20, 1 << 28, "cuda", 8, 128, "insert")
    if edges is not None:
        g.add_edges(*edges, add_reverse=add_reverse)
    return g


def _queries():
    """Every node before every edge, on the tie, between two times and after every edge; a NaN
    time; sources that are negative, at and past the table's end."""
    nodes = np.arange(NODES)
    src = np.concatenate([nodes, nodes, nodes, nodes, [HUB, 3], [-3, -1, NODES, 1000, 1 << 40]])
    ts = np.concatenate([np.full(NODES, -1.0), np.full(NODES, TIE), np.full(NODES, 33.5),
                         np.full(NODES, 1e9), [np.nan, np.nan], np.full(5, 1e9)])
    return src.astype(np.int64), ts.astype(np.float32)


def _rows(B):
    """The queries a shape walks from: the hub after every edge; the last 67 (between times, after
    every edge, NaN, the unknown sources); all 167."""
    n = len(_queries()[0])
    return {1: slice(3 * NODES + HUB, 3 * NODES + HUB + 1), 67: slice(n - 67, n), n: slice(0, n)}[B]


class Toy:
    pass


@pytest.fixture(scope="module")
def toy():
    t = Toy()
    t.edges = _edges()
    t.graph = {r: _new_graph(t.edges, add_reverse=r) for r in (False, True)}
    t.hist = {r: T.from_graph(t.graph[r]) for r in (False, True)}
    t.src, t.ts = _queries()
    t.d_src, t.d_ts = torch.from_numpy(t.src).cuda(), torch.from_numpy(t.ts).cuda()
    t.ref = {}
    return t


def _want(toy, reverse, shape, recency=1, max_history=0):
    key = (reverse, shape, recency, max_history)
    if key not in toy.ref:
        B, W, L = shape
        hist, table_len = toy.hist[reverse]
        toy.ref[key] = T.walks(hist, table_len, toy.src[_rows(B)], toy.ts[_rows(B)], L, W, recency,
                               max_history, SEED, EPOCH)
    return toy.ref[key]


def _call(graph, src, ts, L, W, **kw):
    out = graph.temporal_random_walk(torch.from_numpy(src).cuda(), torch.from_numpy(ts).cuda(),
                                     L, W, **kw)
    return _host(out, len(src), W, L)


def _host(out, B, W, L):
    import gnnflow_amd
    assert isinstance(out, gnnflow_amd.TemporalWalks)
    assert out.nodes.dtype == torch.int64 and tuple(out.nodes.shape) == (B, W, L + 1)
    assert out.eids.dtype == torch.int64 and tuple(out.eids.shape) == (B, W, L)
    assert out.times.dtype == torch.float32 and tuple(out.times.shape) == (B, W, L)
    assert all(x.is_cuda and x.is_contiguous() for x in out)
    return tuple(x.cpu().numpy() for x in out)


def _same(got, want):
    """Bit for bit: the times as their words."""
    return np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and \
        np.array_equal(got[2].view(np.uint32), want[2].view(np.uint32))


@pytest.mark.parametrize("reverse", [False, True])
def test_the_two_ways_to_the_histories_agree(toy, reverse):
    """get_temporal_neighbors reversed is the store's order, ties in the order they were given."""
    hist, table_len = toy.hist[reverse]
    want, want_len = T.from_edges(*toy.edges, add_reverse=reverse)
    assert table_len == want_len == NODES and sorted(hist) == sorted(want) == list(range(NODES))
    for v in range(NODES):
        for a, b in zip(hist[v], want[v]):
            assert a.dtype == b.dtype and np.array_equal(a, b), v
    assert np.count_nonzero(hist[HUB][1] == TIE) >= 4 and len(hist[ABSENT][0]) == 0
    assert len(hist[ONLY_DST][0]) == (1 if reverse else 0)


def test_the_graph_and_the_reference_exercise_every_case(toy):
    """Computed from the store and the reference alone: the comparisons below are not vacuous."""
    for reverse in (False, True):
        hist, table_len = toy.hist[reverse]
        hub_newest = hist[HUB][1][-1]
        assert len(hist[HUB][0]) >= 300 and len(hist[SINGLE][0]) >= 1
        ended_at, searched, on_tie = set(), 0, 0
        for shape in SHAPES[1:]:
            B, W, L = shape
            src, ts = toy.src[_rows(B)], toy.ts[_rows(B)]
            nodes, eids, times = _want(toy, reverse, shape)
            taken = T.steps_taken(eids)
            if L == 4:
                ended_at |= set(np.unique(taken).tolist())
            # the time a step started from
            start = np.concatenate([np.broadcast_to(ts[:, None, None], (B, W, 1)), times[:, :, :-1]], 2)
            step = eids >= 0
            # a step out of the hub that the last_ts_bits shortcut does not resolve
            searched += np.count_nonzero(step & (nodes[:, :, :-1] == HUB) & (start <= hub_newest))
            for i, w in zip(*np.nonzero(taken < L)):
                j = taken[i, w]
                v, t = int(nodes[i, w, j]), start[i, w, j]
                if 0 <= v < table_len and (hist[v][1] == t).any():
                    assert T.history_size(hist[v][1], t) == 0
                    on_tie += 1
            # the unknown sources keep their id in slot 0 and go nowhere
            assert nodes[-5:, :, 0].tolist() == [[s] * W for s in (-3, -1, NODES, 1000, 1 << 40)]
            assert (taken[-7:] == 0).all()                                  # NaN too
            assert (times[step][:] < start[step]).all()                     # strictly earlier
        assert ended_at == {0, 1, 2, 3, 4}, ended_at                        # 4: a full-length walk
        assert searched > 0 and on_tie > 0
    # the hub on the tie never takes a tie edge, the hub after every edge does
    nodes = _want(toy, False, SHAPES[2])[0]
    assert not np.isin(nodes[NODES + HUB, :, 1], TIE_DSTS).any()
    assert np.isin(nodes[3 * NODES + HUB, :, 1], TIE_DSTS).any()
    # the options are visible: other walks for another recency and another bound
    base = _want(toy, False, SHAPES[2])[1]
    assert not np.array_equal(base, _want(toy, False, SHAPES[2], 4, 0)[1])
    assert not np.array_equal(base, _want(toy, False, SHAPES[2], 1, 5)[1])
    newest = toy.hist[True][0][HUB][2][-1]
    assert (_want(toy, True, SHAPES[2], 1, 1)[1][3 * NODES + HUB, :, 0] == newest).all()


@pytest.mark.parametrize("max_history", [0, 1, 5])
@pytest.mark.parametrize("recency", [1, 2, 4])
@pytest.mark.parametrize("shape", SHAPES)
def test_walks_match_the_reference(toy, shape, recency, max_history):
    B, W, L = shape
    for reverse in (False, True):
        out = toy.graph[reverse].temporal_random_walk(
            toy.d_src[_rows(B)], toy.d_ts[_rows(B)], L, W, recency=recency,
            max_history=max_history, seed=SEED, epoch=EPOCH)
        assert _same(_host(out, B, W, L), _want(toy, reverse, shape, recency, max_history))


def test_empty_batch_repeat_calls_and_a_side_stream(toy):
    g = toy.graph[True]
    B, W, L = SHAPES[1]
    src, ts = toy.d_src[_rows(B)], toy.d_ts[_rows(B)]
    kw = dict(recency=2, max_history=5, seed=SEED, epoch=EPOCH)
    _host(g.temporal_random_walk(src[:0], ts[:0], L, W, **kw), 0, W, L)
    a = g.temporal_random_walk(src, ts, L, W, **kw)
    b = g.temporal_random_walk(src, ts, L, W, **kw)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert _same(_host(a, B, W, L), _want(toy, True, SHAPES[1], 2, 5))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        c = g.temporal_random_walk(src, ts, L, W, **kw)
    side.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(a, c))
    # a strided view is taken for what it holds; another seed or epoch gives other walks
    d = g.temporal_random_walk(toy.d_src[::2], toy.d_ts[::2], 2, 3, seed=SEED)
    e = g.temporal_random_walk(toy.d_src[::2].clone(), toy.d_ts[::2].clone(), 2, 3, seed=SEED)
    assert all(torch.equal(x, y) for x, y in zip(d, e))
    # (SEED + 1 would not do at recency 2: it swaps the keys seed ^ (TAG + 0) and seed ^ (TAG + 1)
    # of the two draws, whose maximum is the same; seeds are told apart above their low five bits)
    for other in (dict(kw, seed=SEED ^ (1 << 40)), dict(kw, epoch=EPOCH + 1)):
        assert not torch.equal(g.temporal_random_walk(src, ts, L, W, **other).eids, a.eids)


def test_first_row_slices_reproduce_the_whole(toy):
    g = toy.graph[True]
    B, W, L = SHAPES[2]
    kw = dict(recency=2, seed=SEED, epoch=EPOCH)
    whole = g.temporal_random_walk(toy.d_src, toy.d_ts, L, W, **kw)
    assert _same(_host(whole, B, W, L), _want(toy, True, SHAPES[2], 2, 0))
    for a, b in ((0, 60), (60, 167), (166, 167)):
        part = g.temporal_random_walk(toy.d_src[a:b], toy.d_ts[a:b], L, W, first_row=a, **kw)
        assert all(torch.equal(x, y[a:b]) for x, y in zip(part, whole))
    moved = g.temporal_random_walk(toy.d_src[60:], toy.d_ts[60:], L, W, **kw)
    assert not torch.equal(moved.eids, whole.eids[60:])
    # first_row wraps mod 2^64 with the row, as the reference's tids do
    hist, table_len = toy.hist[True]
    top = 2 ** 64 - 2
    got = _host(g.temporal_random_walk(toy.d_src[117:123], toy.d_ts[117:123], 3, 5,
                                       first_row=top, **kw), 6, 5, 3)
    assert _same(got, T.walks(hist, table_len, toy.src[117:123], toy.ts[117:123], 3, 5, 2, 0,
                              SEED, EPOCH, top))


def test_walks_past_the_grid_limit_are_grid_strided(toy):
    """The launch has at most 8192 workgroups of 64 walks: more walks than that in one call are
    the walks of two calls below the limit, by the keying the test above compares with the
    reference."""
    g = toy.graph[False]
    W = 3200
    assert len(toy.src) * W > 8192 * 64 > 90 * W
    kw = dict(recency=2, max_history=5, seed=SEED)
    whole = g.temporal_random_walk(toy.d_src, toy.d_ts, 1, W, **kw)
    for a, b in ((0, 80), (80, 167)):
        part = g.temporal_random_walk(toy.d_src[a:b], toy.d_ts[a:b], 1, W, first_row=a, **kw)
        assert all(torch.equal(x, y[a:b]) for x, y in zip(part, whole))
    assert (whole.nodes[:, :, 0] == toy.d_src[:, None]).all()
    assert (whole.eids[3 * NODES + HUB] >= 0).all() and (whole.eids[:NODES] == -1).all()


def test_arguments_are_checked_on_the_gpu_too(toy):
    g = toy.graph[False]
    with pytest.raises(ValueError, match="the graph is on device"):
        g.temporal_random_walk(toy.d_src.cpu(), toy.d_ts.cpu(), 2)
    with pytest.raises(ValueError, match="ts is on"):
        g.temporal_random_walk(toy.d_src, toy.d_ts.cpu(), 2)
    with pytest.raises(ValueError, match="length"):
        g.temporal_random_walk(toy.d_src, toy.d_ts, 33)
    with pytest.raises(TypeError, match="recency"):
        g.temporal_random_walk(toy.d_src, toy.d_ts, 2, recency=True)


def test_an_empty_graph_gives_walks_that_all_end(toy):
    graph = _new_graph()
    hist, table_len = T.from_graph(graph)
    assert table_len == 0 and hist == {}
    got = _call(graph, toy.src, toy.ts, 3, 2, seed=SEED)
    assert _same(got, T.walks(hist, table_len, toy.src, toy.ts, 3, 2, seed=SEED))
    assert (got[0][:, :, 0] == toy.src[:, None]).all() and (got[0][:, :, 1:] == -1).all()
    assert (got[1] == -1).all() and (got[2] == 0).all()


def test_edges_added_later_are_walked(toy):
    src, dst, t = toy.edges
    cut = 350
    graph = _new_graph((src[:cut], dst[:cut], t[:cut]), add_reverse=True)
    kw = dict(recency=2, seed=SEED, epoch=EPOCH)
    first = _call(graph, toy.src, toy.ts, 3, 5, **kw)
    hist, table_len = T.from_graph(graph)
    assert _same(first, T.walks(hist, table_len, toy.src, toy.ts, 3, 5, 2, 0, SEED, EPOCH))
    torch.cuda.synchronize()      # add_edges moves segments: the launch above has completed
    graph.add_edges(src[cut:], dst[cut:], t[cut:], add_reverse=True)
    # and a burst that makes the hub's and a new node's segments grow
    graph.add_edges(np.array([HUB] * 40 + [31] * 9), np.full(49, 33), np.full(49, 200.0, np.float32))
    hist2, table_len2 = T.from_graph(graph)
    assert len(hist2[HUB][0]) >= len(hist[HUB][0]) + 40 and len(hist2[31][0]) == 9
    for m in (0, 5):
        second = _call(graph, toy.src, toy.ts, 3, 5, max_history=m, **kw)
        assert _same(second, T.walks(hist2, table_len2, toy.src, toy.ts, 3, 5, 2, m, SEED, EPOCH))
    assert not _same(first, second)
    assert (second[0][3 * NODES + HUB, :, 1] == 33).any()       # the burst is the hub's newest


def test_after_offload_only_live_edges_are_walked(toy):
    src, dst, t = toy.edges
    graph = _new_graph((src[:350], dst[:350], t[:350]))
    graph.add_edges(src[350:], dst[350:], t[350:])
    kw = dict(recency=1, seed=SEED, epoch=EPOCH)
    before = _call(graph, toy.src, toy.ts, 4, 3, **kw)
    hist, table_len = toy.hist[False]
    assert _same(before, T.walks(hist, table_len, toy.src, toy.ts, 4, 3, 1, 0, SEED, EPOCH))
    torch.cuda.synchronize()
    edges_before = graph.num_edges()
    assert graph.offload_old_blocks(60.0) > 0 and graph.num_edges() < edges_before
    live, live_len = T.from_graph(graph)
    assert sum(len(h[0]) for h in live.values()) < sum(len(h[0]) for h in hist.values())
    for m in (0, 5):
        after = _call(graph, toy.src, toy.ts, 4, 3, max_history=m, **kw)
        assert _same(after, T.walks(live, live_len, toy.src, toy.ts, 4, 3, 1, m, SEED, EPOCH))
    assert not _same(before, after)
