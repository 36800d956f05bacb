"""DynamicGraph.seen_mask (csrc/seen_mask.hip) on the GPU against tests/seen_mask_ref.py, bit for
bit.

The graph has 40 node ids and about 600 edges at whole-numbered times in [0, 100), so timestamps
repeat: node 0 is a hub with about 300 edges to few destinations (lanes take several strides,
destinations repeat) and four edges at exactly t = 50 to destinations it meets at no other time;
node 30 has one edge; node 38 is only ever a destination and node 37 is never named (no edges);
39 ends the node table.  The expected bits come from graph.get_temporal_neighbors per node through
the numpy restatement, computed once per (candidate list, max_history) and left unchanged."""
import numpy as np
import pytest
import torch

from tests import seen_mask_ref as S

pytestmark = pytest.mark.gpu

NODES, HUB, SINGLE, ONLY_DST, ABSENT = 40, 0, 30, 38, 37
TIE = 50.0
TIE_DSTS = [21, 22, 23, 24]      # the hub meets them at t = TIE and never else


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


def _cands(C):
    """Unsorted ids with duplicates, ids the graph never saw (40 .. 44, 1000) and a negative one."""
    if C == 1:
        return np.array([TIE_DSTS[0]], np.int64)
    rng = np.random.RandomState(100 + C)
    pool = np.concatenate([np.arange(45), [1000, -5]])
    ids = rng.choice(pool, C)      # with replacement: duplicates from C = 63 on by pigeonhole
    ids[:2] = TIE_DSTS[1]          # a duplicate for certain
    ids[2:8] = [40, 1000, -5, 5, 7, TIE_DSTS[0]]
    ids[-1] = 33                   # the last bit of the last word
    return ids.astype(np.int64)


class Toy:
    pass


@pytest.fixture(scope="module")
def toy():
    t = Toy()
    t.edges = _edges()
    t.graph = _new_graph(t.edges)
    t.src, t.ts = _queries()
    t.hist = S.from_graph(t.graph, t.src)
    t.d_src, t.d_ts = torch.from_numpy(t.src).cuda(), torch.from_numpy(t.ts).cuda()
    t.ref = {}
    return t


def _want(toy, C, max_history):
    if (C, max_history) not in toy.ref:
        toy.ref[C, max_history] = S.seen_mask(toy.hist, toy.src, toy.ts, _cands(C), max_history)
    return toy.ref[C, max_history]


def _call(graph, src, ts, cand, max_history=0):
    out = graph.seen_mask(torch.from_numpy(src).cuda(), torch.from_numpy(ts).cuda(),
                          torch.from_numpy(cand).cuda(), max_history)
    assert out.dtype == torch.int64 and out.is_cuda and out.is_contiguous()
    assert tuple(out.shape) == (len(src), (len(cand) + 63) // 64)
    return out.cpu().numpy()


def test_the_graph_and_the_reference_exercise_every_case(toy):
    """Computed from the store and the reference alone: the comparisons below are not vacuous."""
    h = toy.hist
    assert toy.graph.max_vertex_id() == NODES - 1 and 590 <= toy.graph.num_edges() <= 610
    assert len(h[HUB][0]) >= 300 and len(h[SINGLE][0]) == 1
    assert len(h[ONLY_DST][0]) == 0 and len(h[ABSENT][0]) == 0
    assert len(np.unique(h[HUB][0])) <= 16                         # destinations repeat
    assert np.count_nonzero(h[HUB][1] == TIE) >= 4                 # several edges on the tie
    assert np.count_nonzero(h[HUB][1] < TIE) > 64 and np.count_nonzero(h[HUB][1] > TIE) > 64
    cand = _cands(130)
    assert len(np.unique(cand)) < 130 and (np.diff(cand) < 0).any()
    assert np.isin([40, 1000, -5], cand).all()
    want = S.unpack(_want(toy, 130, 0), 130)
    n = NODES
    assert not want[:n].any()                                      # before every edge
    assert want[n:2 * n].any() and want[3 * n:4 * n].any()
    assert not want[4 * n:].any()                                  # NaN and unknown sources
    tie_cols = np.isin(cand, TIE_DSTS)
    assert tie_cols.sum() >= 3
    assert not want[n + HUB, tie_cols].any()                       # strictly before
    assert want[3 * n + HUB, tie_cols].all()
    assert want[3 * n + SINGLE].sum() == np.count_nonzero(cand == 7) >= 1
    assert not want[3 * n + ABSENT].any() and not want[3 * n + ONLY_DST].any()
    # the bound is visible: fewer bits with max_history 1 and 5 than with the whole history
    bits = [int(S.unpack(_want(toy, 130, m), 130).sum()) for m in (1, 5, 0)]
    assert 0 < bits[0] < bits[1] < bits[2]


@pytest.mark.parametrize("max_history", [0, 1, 5, 1000])
@pytest.mark.parametrize("C", [1, 63, 64, 65, 130])
def test_bits_match_the_reference(toy, C, max_history):
    cand = _cands(C)
    got = toy.graph.seen_mask(toy.d_src, toy.d_ts, torch.from_numpy(cand).cuda(), max_history)
    assert got.dtype == torch.int64 and tuple(got.shape) == (len(toy.src), (C + 63) // 64)
    got = got.cpu().numpy()
    assert np.array_equal(got, _want(toy, C, max_history))
    assert not S.unpack(got, got.shape[1] * 64)[:, C:].any()       # bits past C are zero
    if max_history == 1000:                                        # more than any history
        assert np.array_equal(got, _want(toy, C, 0))


def test_empty_batch_and_repeat_calls(toy):
    cand = torch.from_numpy(_cands(65)).cuda()
    empty = toy.graph.seen_mask(toy.d_src[:0], toy.d_ts[:0], cand)
    assert tuple(empty.shape) == (0, 2) and empty.dtype == torch.int64
    a = toy.graph.seen_mask(toy.d_src, toy.d_ts, cand, 5)
    b = toy.graph.seen_mask(toy.d_src, toy.d_ts, cand, 5)
    assert torch.equal(a, b)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        c = toy.graph.seen_mask(toy.d_src, toy.d_ts, cand, 5)
    side.synchronize()
    assert torch.equal(a, c)
    # a row slice and a strided view are taken for what they hold
    d = toy.graph.seen_mask(toy.d_src[40:80], toy.d_ts[40:80], cand, 5)
    assert torch.equal(d, a[40:80])
    e = toy.graph.seen_mask(toy.d_src[::2], toy.d_ts[::2], cand, 5)
    assert torch.equal(e, a[::2])


def test_rows_past_the_grid_limit_are_grid_strided(toy):
    """The launch has at most 4096 workgroups of four rows: more rows than that, the queries
    repeated, so that the expected rows are the reference's rows repeated."""
    rows = 4 * 4096 + 37
    idx = torch.arange(rows, device="cuda") % len(toy.src)
    got = toy.graph.seen_mask(toy.d_src[idx], toy.d_ts[idx],
                              torch.from_numpy(_cands(65)).cuda(), 5)
    assert np.array_equal(got.cpu().numpy(), _want(toy, 65, 5)[idx.cpu().numpy()])


def test_arguments_are_checked_on_the_gpu_too(toy):
    cand = torch.from_numpy(_cands(65)).cuda()
    with pytest.raises(ValueError, match="the graph is on device"):
        toy.graph.seen_mask(toy.d_src.cpu(), toy.d_ts.cpu(), cand.cpu())
    with pytest.raises(ValueError, match="cand_ids is on"):
        toy.graph.seen_mask(toy.d_src, toy.d_ts, cand.cpu())
    with pytest.raises(ValueError, match="candidate"):
        toy.graph.seen_mask(toy.d_src, toy.d_ts, cand[:0])
    with pytest.raises(TypeError, match="max_history"):
        toy.graph.seen_mask(toy.d_src, toy.d_ts, cand, True)


def test_edges_added_later_are_seen(toy):
    src, dst, t = toy.edges
    cut = 350
    graph = _new_graph((src[:cut], dst[:cut], t[:cut]))
    q_src, q_ts = _queries()
    cand = _cands(130)
    first = _call(graph, q_src, q_ts, cand)
    assert np.array_equal(first, S.seen_mask(S.from_graph(graph, q_src), q_src, q_ts, cand))
    torch.cuda.synchronize()      # add_edges moves segments: the launch above has completed
    graph.add_edges(src[cut:], dst[cut:], t[cut:])
    # and a burst that makes the hub's and a new node's segments grow, to a destination unseen so far
    graph.add_edges(np.array([HUB] * 40 + [31] * 9), np.full(49, 33), np.full(49, 200.0, np.float32))
    second = _call(graph, q_src, q_ts, cand)
    assert np.array_equal(second, _want(toy, 130, 0) | second)     # nothing of the full graph lost
    hist = S.from_graph(graph, q_src)
    assert np.array_equal(second, S.seen_mask(hist, q_src, q_ts, cand))
    col = int(np.flatnonzero(cand == 33)[0])
    seen33 = S.unpack(second, 130)[:, col]
    assert seen33[3 * NODES + HUB] and seen33[3 * NODES + 31] and not S.unpack(first, 130)[:, col].any()
    assert not np.array_equal(first, second)
    assert np.array_equal(_call(graph, q_src, q_ts, cand, 5),
                          S.seen_mask(hist, q_src, q_ts, cand, 5))


def test_after_offload_only_live_edges_count(toy):
    src, dst, t = toy.edges
    graph = _new_graph((src[:350], dst[:350], t[:350]))
    graph.add_edges(src[350:], dst[350:], t[350:])
    q_src, q_ts = _queries()
    cand = _cands(130)
    before = _call(graph, q_src, q_ts, cand)
    assert np.array_equal(before, _want(toy, 130, 0))
    torch.cuda.synchronize()
    edges_before = graph.num_edges()
    assert graph.offload_old_blocks(60.0) > 0 and graph.num_edges() < edges_before
    hist = S.from_graph(graph, q_src)
    assert sum(len(h[0]) for h in hist.values()) < sum(len(h[0]) for h in toy.hist.values())
    for m in (0, 5):
        assert np.array_equal(_call(graph, q_src, q_ts, cand, m),
                              S.seen_mask(hist, q_src, q_ts, cand, m))
    after = _call(graph, q_src, q_ts, cand)
    assert np.array_equal(after & before, after) and not np.array_equal(after, before)


def test_undirected_graph_sees_who_pointed_at_the_source(toy):
    graph = _new_graph(toy.edges, add_reverse=True)
    q_src, q_ts = _queries()
    cand = _cands(130)
    hist = S.from_graph(graph, q_src)
    assert len(hist[ONLY_DST][0]) == 1 and int(hist[ONLY_DST][0][0]) == 5
    for m in (0, 5):
        got = _call(graph, q_src, q_ts, cand, m)
        assert np.array_equal(got, S.seen_mask(hist, q_src, q_ts, cand, m))
    got = S.unpack(_call(graph, q_src, q_ts, cand), 130)
    assert got[3 * NODES + ONLY_DST, cand == 5].all() and got[3 * NODES + ONLY_DST].sum() == \
        np.count_nonzero(cand == 5) >= 1
    directed = S.unpack(_want(toy, 130, 0), 130)
    assert (got | directed == got).all() and got.sum() > directed.sum()
