"""DynamicGraph.neighbor_aggregate (csrc/neighbor_aggregate.hip) on the GPU against
tests/neighbor_aggregate_ref.py: count equal, and the two feature outputs equal BIT FOR BIT to the
sequential float32 loop, compared through .view(torch.int32).

The graph is test_gpu_pair_history.py's toy (its construction is copied here): 40 node ids and
about 730 edges at whole-numbered times in [0, 100), so timestamps repeat; node 0 is a hub with 435
edges, five of them at exactly t = 50; node 30 has one edge; node 38 is only ever a destination,
node 37 is never named, 39 ends the node table.  Every node is asked at times before every edge,
on the tie, between two times and after every edge; two rows have NaN times; five have sources
that are negative, at and past the table's end.  The expected values come from
graph.get_temporal_neighbors per node through the numpy restatement, computed once per
combination and left unchanged.

Widths: 1 (a single lane), 3 (not a multiple of four), 64 and 65 (a wave of scalar columns and one
more: a second tile), 172 (the workload's own, float4 columns), 260 and 1024 (more than 64 float4
columns: tiles of those too).  One test has more rows than the launch has waves, which is more
than any other case needs, because the grid-stride loop is a path of its own."""
import numpy as np
import pytest
import torch

from tests import neighbor_aggregate_ref as R

pytestmark = pytest.mark.gpu

NODES, HUB, SINGLE, ONLY_DST, ABSENT = 40, 0, 30, 38, 37
HUB_OFTEN = 13
TIE = 50.0
TIE_DSTS = [21, 22, 23, 24, 21]
TIMES = [-1.0, TIE, 33.5, 1e9]
NODE_ROWS = 20                   # ids 20 .. 39 have no row in the short node table


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


def _queries():
    nodes, ts = [], []
    for t in TIMES:
        for v in range(NODES):
            nodes.append(v), ts.append(t)
    for v in (HUB, 3):
        nodes.append(v), ts.append(np.nan)
    for v in (-3, -1, NODES, 1000, 1 << 40):
        nodes.append(v), ts.append(1e9)
    return np.array(nodes, np.int64), np.array(ts, np.float32)


def _since(kind, ts):
    """None, the scalar 40.0, or a tensor's worth: -inf, NaN, the tie's time exactly and a value
    above the row's own time, in turn."""
    if kind == "tensor":
        with np.errstate(invalid="ignore"):
            cols = np.stack([np.full(len(ts), -np.inf), np.full(len(ts), np.nan),
                             np.full(len(ts), TIE), ts + 10.0])
        return cols[np.arange(len(ts)) % 4, np.arange(len(ts))].astype(np.float32)
    return {"none": None, "scalar": 40.0}[kind]


def _d_since(kind, ts):
    s = _since(kind, ts)
    return torch.from_numpy(s).cuda() if isinstance(s, np.ndarray) else s


class Toy:
    pass


@pytest.fixture(scope="module")
def toy():
    t = Toy()
    t.edges = _edges()
    t.graph = _new_graph(t.edges)
    t.nodes, t.ts = _queries()
    t.hist = R.from_graph(t.graph, t.nodes)
    t.d_nodes, t.d_ts = torch.from_numpy(t.nodes).cuda(), torch.from_numpy(t.ts).cuda()
    t.num_edges = t.graph.num_edges()
    rng = np.random.RandomState(3)
    # one table per width, random normal; the node tables cover every id, the edge tables every eid
    t.node_tab = {d: rng.randn(NODES, d).astype(np.float32) for d in (1, 3, 64, 65, 172)}
    t.edge_tab = {d: rng.randn(t.num_edges, d).astype(np.float32) for d in (4, 172)}
    t.dev = {}
    t.ref = {}
    return t


def _dev(toy, tab):
    """The device copy of a host table, made once."""
    if tab is None:
        return None
    if id(tab) not in toy.dev:
        toy.dev[id(tab)] = (tab, torch.from_numpy(tab).cuda())
    return toy.dev[id(tab)][1]


def _want(toy, node_tab, edge_tab, kind, max_history, reduce, hist=None):
    key = (id(node_tab), id(edge_tab), kind, max_history, reduce, id(hist))
    if key not in toy.ref:
        toy.ref[key] = R.neighbor_aggregate(toy.hist if hist is None else hist, toy.nodes, toy.ts,
                                            node_tab, edge_tab, _since(kind, toy.ts), max_history,
                                            reduce) + (node_tab, edge_tab, hist)   # keep ids alive
    return toy.ref[key][:3]


def _same(out, want, n, dn, de, rows=None):
    """count equal; node and edge equal bit for bit."""
    assert out.count.dtype == torch.int64 and tuple(out.count.shape) == (n,)
    count = want[0] if rows is None else want[0][rows]
    assert np.array_equal(out.count.cpu().numpy(), count)
    for got, exp, d in ((out.node, want[1], dn), (out.edge, want[2], de)):
        if d == 0:
            assert got is None and exp is None
            continue
        assert got.dtype == torch.float32 and got.is_cuda and got.is_contiguous() and \
            tuple(got.shape) == (n, d) and not got.requires_grad
        exp = exp if rows is None else exp[rows]
        assert np.array_equal(got.view(torch.int32).cpu().numpy(), exp.view(np.int32))


def _run(toy, node_tab, edge_tab, kind="none", max_history=0, reduce="mean", graph=None,
         hist=None):
    out = (toy.graph if graph is None else graph).neighbor_aggregate(
        toy.d_nodes, toy.d_ts, node_feats=_dev(toy, node_tab), edge_feats=_dev(toy, edge_tab),
        since=_d_since(kind, toy.ts), max_history=max_history, reduce=reduce)
    _same(out, _want(toy, node_tab, edge_tab, kind, max_history, reduce, hist), len(toy.nodes),
          0 if node_tab is None else node_tab.shape[1],
          0 if edge_tab is None else edge_tab.shape[1])
    return out


def test_the_graph_and_the_reference_exercise_every_case(toy):
    """Computed from the store and the reference alone: the comparisons below are not vacuous."""
    h = toy.hist
    assert toy.graph.max_vertex_id() == NODES - 1 and 720 <= toy.num_edges <= 745
    assert len(h[HUB][0]) == 435 and len(h[SINGLE][0]) == 1
    assert len(h[ONLY_DST][0]) == 0 and len(h[ABSENT][0]) == 0
    assert np.count_nonzero(h[HUB][1] == TIE) >= 5
    count, node, edge = _want(toy, toy.node_tab[172], toy.edge_tab[4], "none", 0, "sum")
    assert count[(toy.nodes == HUB) & (toy.ts == np.float32(1e9))] == 435
    assert (count[toy.ts == -1.0] == 0).all() and (count[np.isnan(toy.ts)] == 0).all()
    assert np.isnan(toy.ts).sum() == 2
    assert (count[(toy.nodes < 0) | (toy.nodes >= NODES)] == 0).all()
    assert (count == 0).sum() > 40 and (count > 64).sum() >= 2 and (count == 1).sum() >= 1
    assert not node[count == 0].any() and not edge[count == 0].any()
    assert node[count > 0].any(axis=1).all()
    # the tie is strictly before nothing of itself: the hub's window at t = 50 ends before it
    at = {t: int(count[(toy.nodes == HUB) & (toy.ts == np.float32(t))][0]) for t in TIMES}
    assert at[-1.0] == 0 < at[33.5] < at[TIE] < at[1e9]
    assert at[TIE] == int((h[HUB][1] < TIE).sum())
    # the bound and the lower end are visible
    totals = [int(_want(toy, toy.node_tab[172], toy.edge_tab[4], "none", m, "sum")[0].sum())
              for m in (1, 64, 65, 0)]
    assert 0 < totals[0] < totals[1] < totals[2] < totals[3]
    for kind in ("scalar", "tensor"):
        assert 0 < _want(toy, toy.node_tab[172], toy.edge_tab[4], kind, 0, "sum")[0].sum() < \
            count.sum()
    # sum and mean differ, and the mean is the sum over the count in float32
    mean = _want(toy, toy.node_tab[172], toy.edge_tab[4], "none", 0, "mean")[1]
    big = count > 1
    assert (mean[big] != node[big]).any()
    assert np.array_equal(mean[big], node[big] / count[big].astype(np.float32)[:, None])


@pytest.mark.parametrize("reduce", ["sum", "mean"])
@pytest.mark.parametrize("kind", ["none", "scalar", "tensor"])
@pytest.mark.parametrize("max_history", [0, 1, 64, 65])
def test_both_tables_match_the_reference(toy, max_history, kind, reduce):
    _run(toy, toy.node_tab[172], toy.edge_tab[4], kind, max_history, reduce)


@pytest.mark.parametrize("reduce", ["sum", "mean"])
@pytest.mark.parametrize("dn", [1, 3, 64, 65, 172])
def test_node_table_alone_at_every_width(toy, dn, reduce):
    out = _run(toy, toy.node_tab[dn], None, "tensor", 64, reduce)
    assert out.edge is None
    _run(toy, toy.node_tab[dn], None, "none", 0, reduce)


@pytest.mark.parametrize("reduce", ["sum", "mean"])
@pytest.mark.parametrize("de", [4, 172])
def test_edge_table_alone_at_every_width(toy, de, reduce):
    out = _run(toy, None, toy.edge_tab[de], "tensor", 64, reduce)
    assert out.node is None
    _run(toy, None, toy.edge_tab[de], "none", 0, reduce)


@pytest.mark.parametrize("dn,de", [(1, 172), (3, 4), (64, 172), (65, 4), (172, 172)])
def test_both_tables_at_mixed_widths(toy, dn, de):
    for reduce in ("sum", "mean"):
        _run(toy, toy.node_tab[dn], toy.edge_tab[de], "scalar", 65, reduce)


@pytest.mark.parametrize("d", [260, 1024])
def test_tables_wider_than_a_wave_of_float4_columns(toy, d):
    rng = np.random.RandomState(d)
    node_tab = rng.randn(NODES, d).astype(np.float32)
    edge_tab = rng.randn(toy.num_edges, d).astype(np.float32)
    for reduce in ("sum", "mean"):
        _run(toy, node_tab, edge_tab, "none", 64, reduce)


def test_a_table_that_is_not_16_byte_aligned_takes_scalar_columns(toy):
    """A contiguous table one float into its storage: its width is a multiple of four and float4
    loads would be misaligned."""
    tab = toy.node_tab[172]
    flat = torch.zeros(tab.size + 1, dtype=torch.float32, device="cuda")
    flat[1:] = torch.from_numpy(tab).cuda().reshape(-1)
    view = flat[1:].view(NODES, 172)
    assert view.is_contiguous() and view.data_ptr() % 16 == 4
    for reduce in ("sum", "mean"):
        out = toy.graph.neighbor_aggregate(toy.d_nodes, toy.d_ts, node_feats=view,
                                           max_history=65, reduce=reduce)
        _same(out, _want(toy, tab, None, "none", 65, reduce), len(toy.nodes), 172, 0)


def test_ids_without_a_row_add_nothing_and_still_count(toy):
    node_short = toy.node_tab[172][:NODE_ROWS].copy()
    edge_short = toy.edge_tab[172][:toy.num_edges - 200].copy()
    h = toy.hist
    assert (h[HUB][0] >= NODE_ROWS).any() and (h[HUB][2] >= len(edge_short)).any()
    full = _want(toy, toy.node_tab[172], toy.edge_tab[172], "none", 0, "mean")
    for reduce in ("sum", "mean"):
        for kind, m in (("none", 0), ("tensor", 64)):
            _run(toy, node_short, edge_short, kind, m, reduce)
    short = _want(toy, node_short, edge_short, "none", 0, "mean")
    assert np.array_equal(short[0], full[0])                         # the count is unchanged
    assert (short[1] != full[1]).any() and (short[2] != full[2]).any()
    # an all-ones table: the mean is the share of the considered edges that have a row
    ones = np.ones((NODE_ROWS, 3), np.float32)
    out = _run(toy, ones, None, "none", 0, "mean")
    got = out.node[:, 0].cpu().numpy()
    for i in np.flatnonzero(full[0] > 0):
        a, c = R.window(h[int(toy.nodes[i])][1], toy.ts[i])
        known = int((h[int(toy.nodes[i])][0][a:c] < NODE_ROWS).sum())
        assert got[i] == np.float32(known) / np.float32(c - a)


@pytest.mark.parametrize("d", [1, 4, 172])
def test_the_mean_of_an_all_ones_table_is_exactly_one(toy, d):
    ones_n = torch.ones((NODES, d), device="cuda")
    ones_e = torch.ones((toy.num_edges, d), device="cuda")
    for kind, m in (("none", 0), ("tensor", 65)):
        out = toy.graph.neighbor_aggregate(toy.d_nodes, toy.d_ts, node_feats=ones_n,
                                           edge_feats=ones_e, since=_d_since(kind, toy.ts),
                                           max_history=m)
        want = (out.count > 0).float()[:, None].expand(-1, d)
        assert (out.count > 0).any() and (out.count == 0).any()
        assert torch.equal(out.node, want) and torch.equal(out.edge, want)
        total = toy.graph.neighbor_aggregate(toy.d_nodes, toy.d_ts, node_feats=ones_n,
                                             since=_d_since(kind, toy.ts), max_history=m,
                                             reduce="sum")
        assert torch.equal(total.node, out.count.float()[:, None].expand(-1, d))


def test_undirected_graph(toy):
    graph = _new_graph(toy.edges, add_reverse=True)
    hist = R.from_graph(graph, toy.nodes)
    assert len(hist[ONLY_DST][0]) == 1 and int(hist[ONLY_DST][0][0]) == 5
    for reduce, kind, m in (("mean", "none", 0), ("sum", "tensor", 64), ("mean", "scalar", 1)):
        out = _run(toy, toy.node_tab[172], toy.edge_tab[4], kind, m, reduce, graph=graph,
                   hist=hist)
    got = graph.neighbor_aggregate(toy.d_nodes, toy.d_ts, node_feats=_dev(toy, toy.node_tab[3]))
    assert (got.count.cpu().numpy() >= _want(toy, toy.node_tab[3], None, "none", 0, "mean")[0]).all()
    assert out.count.sum() > 0


def test_empty_batch_and_a_graph_without_edges(toy):
    nf, ef = _dev(toy, toy.node_tab[65]), _dev(toy, toy.edge_tab[4])
    empty = toy.graph.neighbor_aggregate(toy.d_nodes[:0], toy.d_ts[:0], node_feats=nf,
                                         edge_feats=ef)
    assert tuple(empty.count.shape) == (0,) and empty.count.dtype == torch.int64
    assert tuple(empty.node.shape) == (0, 65) and tuple(empty.edge.shape) == (0, 4)
    assert empty.node.dtype == empty.edge.dtype == torch.float32
    only = toy.graph.neighbor_aggregate(toy.d_nodes[:0], toy.d_ts[:0], edge_feats=ef)
    assert only.node is None and tuple(only.edge.shape) == (0, 4)
    graph = _new_graph()
    for reduce in ("sum", "mean"):
        out = graph.neighbor_aggregate(toy.d_nodes, toy.d_ts, node_feats=nf, edge_feats=ef,
                                       since=0.0, reduce=reduce)
        assert not out.count.any() and not out.node.any() and not out.edge.any()
        assert tuple(out.node.shape) == (len(toy.nodes), 65)


def test_repeat_calls_give_the_same_bits_on_any_stream(toy):
    nf, ef = _dev(toy, toy.node_tab[172]), _dev(toy, toy.edge_tab[172])

    def call():
        return toy.graph.neighbor_aggregate(toy.d_nodes, toy.d_ts, node_feats=nf, edge_feats=ef,
                                            since=40.0, max_history=65)
    a, b = call(), call()
    assert all(torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x,
                           y.view(torch.int32) if y.dtype == torch.float32 else y)
               for x, y in zip(a, b))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        c = call()
    side.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(a, c))
    _same(a, _want(toy, toy.node_tab[172], toy.edge_tab[172], "scalar", 65, "mean"),
          len(toy.nodes), 172, 172)


def test_every_output_element_is_written(toy):
    """torch's allocator hands back the blocks just freed: fill blocks of the outputs' sizes with
    NaN, free them, and no NaN may be left after the call."""
    n = len(toy.nodes)
    nf, ef = _dev(toy, toy.node_tab[65]), _dev(toy, toy.edge_tab[4])
    for kind, m in (("none", 0), ("tensor", 1)):
        torch.cuda.synchronize()
        junk = [torch.full((n, 65), float("nan"), device="cuda"),
                torch.full((n, 4), float("nan"), device="cuda"),
                torch.full((n,), -1, dtype=torch.int64, device="cuda")]
        del junk
        out = toy.graph.neighbor_aggregate(toy.d_nodes, toy.d_ts, node_feats=nf, edge_feats=ef,
                                           since=_d_since(kind, toy.ts), max_history=m)
        assert not torch.isnan(out.node).any() and not torch.isnan(out.edge).any()
        assert (out.count >= 0).all()
        _same(out, _want(toy, toy.node_tab[65], toy.edge_tab[4], kind, m, "mean"), n, 65, 4)


@pytest.mark.parametrize("kind", ["none", "scalar", "tensor"])
def test_count_agrees_with_temporal_degree_and_common_neighbors(toy, kind):
    nf = _dev(toy, toy.node_tab[1])
    since = _d_since(kind, toy.ts)
    degree = toy.graph.temporal_degree(toy.d_nodes, toy.d_ts, since=since)
    for m in (0, 1, 64, 65):
        out = toy.graph.neighbor_aggregate(toy.d_nodes, toy.d_ts, node_feats=nf, since=since,
                                           max_history=m)
        assert torch.equal(out.count, degree.clamp(max=m) if m else degree)
        if m == 64:
            cn = toy.graph.common_neighbors(toy.d_nodes, toy.d_nodes, toy.d_ts, since=since,
                                            max_history=64)
            assert torch.equal(out.count, cn.n_src.long())


def test_row_slices_and_strided_views_are_taken_for_what_they_hold(toy):
    nf = _dev(toy, toy.node_tab[172])
    d_since = _d_since("tensor", toy.ts)
    a = toy.graph.neighbor_aggregate(toy.d_nodes, toy.d_ts, node_feats=nf, since=d_since,
                                     max_history=64)
    b = toy.graph.neighbor_aggregate(toy.d_nodes[40:140], toy.d_ts[40:140], node_feats=nf,
                                     since=d_since[40:140], max_history=64)
    assert torch.equal(b.count, a.count[40:140]) and torch.equal(b.node, a.node[40:140])
    c = toy.graph.neighbor_aggregate(toy.d_nodes[::2], toy.d_ts[::2], node_feats=nf,
                                     since=d_since[::2], max_history=64)
    assert torch.equal(c.count, a.count[::2]) and torch.equal(c.node, a.node[::2])
    # a row slice of a table is the table without its other rows
    d = toy.graph.neighbor_aggregate(toy.d_nodes, toy.d_ts, node_feats=nf[:NODE_ROWS],
                                     since=d_since, max_history=64)
    want = _want(toy, toy.node_tab[172][:NODE_ROWS].copy(), None, "tensor", 64, "mean")
    _same(d, want, len(toy.nodes), 172, 0)


def test_rows_past_the_grid_limit_are_grid_strided(toy):
    """The launch has at most 4096 workgroups of four rows: more rows than that, the queries
    repeated, so that the expected rows are the reference's rows repeated."""
    rows = 4 * 4096 + 37
    idx = torch.arange(rows, device="cuda") % len(toy.nodes)
    out = toy.graph.neighbor_aggregate(toy.d_nodes[idx], toy.d_ts[idx],
                                       node_feats=_dev(toy, toy.node_tab[3]),
                                       edge_feats=_dev(toy, toy.edge_tab[4]),
                                       since=_d_since("tensor", toy.ts)[idx], max_history=5)
    _same(out, _want(toy, toy.node_tab[3], toy.edge_tab[4], "tensor", 5, "mean"), rows, 3, 4,
          idx.cpu().numpy())


def test_tables_are_detached_and_arguments_checked_on_the_gpu_too(toy):
    nf = _dev(toy, toy.node_tab[3]).clone().requires_grad_(True)
    out = toy.graph.neighbor_aggregate(toy.d_nodes, toy.d_ts, node_feats=nf)
    assert not out.node.requires_grad and out.node.grad_fn is None
    with pytest.raises(ValueError, match="the graph is on device"):
        toy.graph.neighbor_aggregate(toy.d_nodes.cpu(), toy.d_ts.cpu(), node_feats=nf.cpu())
    with pytest.raises(ValueError, match="node_feats is on"):
        toy.graph.neighbor_aggregate(toy.d_nodes, toy.d_ts, node_feats=nf.detach().cpu())
    with pytest.raises(ValueError, match="contiguous"):
        toy.graph.neighbor_aggregate(toy.d_nodes, toy.d_ts,
                                     node_feats=_dev(toy, toy.node_tab[64])[:, :32])
    with pytest.raises(TypeError, match="float32"):
        toy.graph.neighbor_aggregate(toy.d_nodes, toy.d_ts, node_feats=nf.detach().half())
    with pytest.raises(ValueError, match="1 to 1024"):
        toy.graph.neighbor_aggregate(toy.d_nodes, toy.d_ts,
                                     node_feats=torch.zeros(2, 1025, device="cuda"))
