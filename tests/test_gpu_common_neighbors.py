"""DynamicGraph.common_neighbors and DynamicGraph.temporal_degree (csrc/common_neighbors.hip) on
the GPU against tests/common_neighbors_ref.py: all eight outputs exactly equal.

The graph is test_gpu_pair_history.py's kind, with whole-numbered times in [0, 100) so that
timestamps repeat: node 0 is a hub with 430 edges over destinations 1 .. 13; nodes 40 and 41 are
wide, 560 edges each to 560 distinct nodes (100 .. 619 and 1000 .. 1519) of which they share 40
(2000 .. 2039); nodes 1 .. 29 have 290 edges among themselves and the hub; node 30 has one edge;
node 2046 is only ever a destination, 2045 is never named and 2050 ends the node table.  Built
once directed and once with reverse edges, where the wide nodes' leaves get histories of their
own.  The expected values come from graph.get_temporal_neighbors per node through the numpy
restatement, computed once per (graph, since, max_history) with max_common = 512 and left
unchanged; a smaller max_common is its first columns (test_common_neighbors_ref.py checks that on
the restatement)."""
import numpy as np
import pytest
import torch

from tests import common_neighbors_ref as R
from tests import pair_history_ref as P

pytestmark = pytest.mark.gpu

HUB, WIDE_A, WIDE_B, SINGLE = 0, 40, 41, 30
ONLY_DST, ABSENT, LAST = 2046, 2045, 2050
SHARED = np.arange(2000, 2040)
TIE = 50.0
TIMES = [-1.0, TIE, 33.5, 1e9]
HS = [1, 32, 33, 128, 129, 512]
KS = [0, 1, 3, 512]
KINDS = ["none", "scalar", "tensor"]
# every kind of node: the hub, both wide ones, two small ones, the single edge, the destination
# only, the absent one, a shared leaf, a leaf of one wide node, a negative id, the table's end,
# past it and far past it
ENDS = [HUB, WIDE_A, WIDE_B, 3, 5, SINGLE, ONLY_DST, ABSENT, 2000, 100, -3, LAST, LAST + 1, 1 << 40]


def _edges():
    rng = np.random.RandomState(23)
    hub_n, wide_n, rest_n = 430, 520, 290
    parts = [(np.full(hub_n, HUB), rng.choice(np.arange(1, 14), hub_n)),
             (np.full(wide_n, WIDE_A), np.arange(100, 100 + wide_n)),
             (np.full(wide_n, WIDE_B), np.arange(1000, 1000 + wide_n)),
             (np.full(len(SHARED), WIDE_A), SHARED), (np.full(len(SHARED), WIDE_B), SHARED),
             (rng.choice(np.arange(1, 30), rest_n), rng.choice(np.arange(0, 30), rest_n))]
    src = np.concatenate([p[0] for p in parts] + [[SINGLE], [5], [6]])
    dst = np.concatenate([p[1] for p in parts] + [[7], [ONLY_DST], [LAST]])
    t = np.floor(rng.rand(len(src)) * 100)
    t[-3:] = [40.0, 60.0, 99.0]
    order = np.argsort(t, kind="stable")
    return src[order].astype(np.int64), dst[order].astype(np.int64), t[order].astype(np.float32)


def _new_graph(edges=None, add_reverse=False):
    import gnnflow_amd
    g = gnnflow_amd.DynamicGraph(1 << 20, 1 << 28, "cuda", 8, 128, "insert")
    if edges is not None:
        g.add_edges(*edges, add_reverse=add_reverse)
    return g


def _queries():
    """Every kind of node with every kind, itself included, before every edge, on a tie, between
    two times and after every edge; and NaN times."""
    src, dst, ts = [], [], []
    for t in TIMES:
        for s in ENDS:
            for d in ENDS:
                src.append(s), dst.append(d), ts.append(t)
    for s, d in ((HUB, 3), (WIDE_A, WIDE_B), (5, 5)):
        src.append(s), dst.append(d), ts.append(np.nan)
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


def _d_since(kind, ts):
    s = _since(kind, ts)
    return torch.from_numpy(s).cuda() if isinstance(s, np.ndarray) else s


class Toy:
    pass


@pytest.fixture(scope="module")
def toys():
    out = {}
    edges = _edges()
    src, dst, ts = _queries()
    for reverse in (False, True):
        t = Toy()
        t.edges, t.src, t.dst, t.ts = edges, src, dst, ts
        t.graph = _new_graph(edges, add_reverse=reverse)
        assert t.graph.max_vertex_id() == LAST
        t.hist = P.from_graph(t.graph, np.arange(LAST + 1))      # the neighbours' degrees too
        t.d_src, t.d_dst, t.d_ts = (torch.from_numpy(x).cuda() for x in (src, dst, ts))
        t.ref = {}
        out[reverse] = t
    return out


def _want(toy, kind, H, K=512):
    if (kind, H) not in toy.ref:
        toy.ref[kind, H] = R.common_neighbors(toy.hist, toy.src, toy.dst, toy.ts,
                                              _since(kind, toy.ts), H, 512)
    return tuple(x if x.ndim == 1 else x[:, :K] for x in toy.ref[kind, H])


def _host(out, n, K):
    assert type(out).__name__ == "CommonNeighbors"
    assert [x.dtype for x in out] == [torch.int32] * 5 + [torch.int64] + [torch.int32] * 2
    assert [tuple(x.shape) for x in out] == [(n,)] * 5 + [(n, K)] * 3
    assert all(x.is_cuda and x.is_contiguous() for x in out)
    return tuple(x.cpu().numpy() for x in out)


def _same(got, want, rows=None):
    for name, g, w in zip(("n_src", "n_dst", "u_src", "u_dst", "common", "nodes", "cnt_src",
                           "cnt_dst"), got, want):
        if rows is not None:
            w = w[rows]
        bad = np.flatnonzero((g != w).reshape(len(g), -1).any(1)) if g.size else []
        assert g.shape == w.shape and len(bad) == 0, \
            "{}: rows {} got {} want {}".format(name, bad[:5], g[bad[:5]], w[bad[:5]])


def test_the_graph_and_the_reference_exercise_every_case(toys):
    """Computed from the stores and the restatement alone: the comparisons below are not
    vacuous."""
    toy, rev = toys[False], toys[True]
    h = toy.hist
    assert len(h[HUB][0]) == 430 and len(np.unique(h[HUB][0])) == 13
    for v in (WIDE_A, WIDE_B):
        assert len(np.unique(h[v][0])) >= 520
    assert len(np.intersect1d(h[WIDE_A][0], h[WIDE_B][0])) == 40
    assert len(h[ONLY_DST][0]) == 0 and len(h[ABSENT][0]) == 0 and len(h[SINGLE][0]) == 1
    assert len(rev.hist[ONLY_DST][0]) == 1 and len(rev.hist[2000][0]) == 2
    assert len(toy.src) == 4 * len(ENDS) ** 2 + 3 and np.isnan(toy.ts).sum() == 3
    assert (toy.src == toy.dst).sum() >= 4 * len(ENDS)
    for t in (toy, rev):
        n_src, n_dst, u_src, u_dst, common, nodes, cnt_src, cnt_dst = _want(t, "none", 512)
        for K in (0, 1, 3):
            assert (common > K).any()                                   # truncated rows
        assert ((n_src > 0) & (n_dst > 0) & (common == 0)).any()        # disjoint, not empty
        assert cnt_src.max() >= 3 and cnt_dst.max() >= 3                # multi-edges
        union = u_src + u_dst - common
        assert union.max() >= 2 * 512 - 64                              # the table's design load
        wide = (t.src == WIDE_A) & (t.dst == WIDE_B) & (t.ts == np.float32(1e9))
        assert wide.sum() == 1 and 20 <= common[wide][0] <= 40          # most of the shared 40
        assert (common[np.isnan(t.ts)] == 0).all() and (n_src[t.ts == -1.0] == 0).all()
        assert ((t.src == t.dst) & (common == u_src) & (common > 3)).any()
        assert (n_src[(t.src < 0) | (t.src > LAST)] == 0).all()
        c = R.temporal_degree(t.hist, t.src, t.ts)
        for H in HS:
            n_h = _want(t, "none", H)[0]
            assert ((n_h == H) & (c > H)).any(), H                      # n_src == H < c
        # max_history cuts neighbours out: fewer common ones at 32 than at 512, and the lower
        # end and the tie do too
        assert 0 < _want(t, "none", 32)[4].sum() < common.sum()
        assert 0 < _want(t, "scalar", 512)[4].sum() < common.sum()
        assert 0 < _want(t, "tensor", 512)[4].sum() < common.sum()
        tie, late = t.ts == np.float32(TIE), t.ts == np.float32(1e9)
        assert 0 < n_src[tie].sum() < n_src[late].sum()
    assert rev.ref["none", 512][4].sum() > toy.ref["none", 512][4].sum()


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("H", HS)
def test_outputs_match_the_reference(toys, H, kind, reverse):
    toy = toys[reverse]
    for K in KS:
        out = toy.graph.common_neighbors(toy.d_src, toy.d_dst, toy.d_ts,
                                         since=_d_since(kind, toy.ts), max_history=H,
                                         max_common=K)
        _same(_host(out, len(toy.src), K), _want(toy, kind, H, K))


def test_defaults_empty_batch_repeat_calls_and_another_stream(toys):
    toy = toys[True]
    n = len(toy.src)
    _same(_host(toy.graph.common_neighbors(toy.d_src, toy.d_dst, toy.d_ts), n, 32),
          R.common_neighbors(toy.hist, toy.src, toy.dst, toy.ts))      # 64 and 32
    empty = toy.graph.common_neighbors(toy.d_src[:0], toy.d_dst[:0], toy.d_ts[:0], max_common=5)
    _host(empty, 0, 5)
    kw = dict(since=40.0, max_history=129, max_common=7)
    a = toy.graph.common_neighbors(toy.d_src, toy.d_dst, toy.d_ts, **kw)
    b = toy.graph.common_neighbors(toy.d_src, toy.d_dst, toy.d_ts, **kw)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        c = toy.graph.common_neighbors(toy.d_src, toy.d_dst, toy.d_ts, **kw)
    side.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(a, c))
    # slices and strided views are taken for what they hold
    d_since = _d_since("tensor", toy.ts)
    whole = toy.graph.common_neighbors(toy.d_src, toy.d_dst, toy.d_ts, since=d_since,
                                       max_history=33, max_common=3)
    part = toy.graph.common_neighbors(toy.d_src[1::3], toy.d_dst[1::3], toy.d_ts[1::3],
                                      since=d_since[1::3], max_history=33, max_common=3)
    assert all(torch.equal(x, y[1::3]) for x, y in zip(part, whole))


@pytest.mark.parametrize("H", [32, 128, 512])
def test_rows_past_the_grid_limit_are_grid_strided(toys, H):
    """A launch has at most 4096 workgroups, of one row each in the largest bucket and of four in
    the others: more rows than either covers in a pass, the queries repeated."""
    toy = toys[True]
    rows = 4 * 4096 + 37
    idx = torch.arange(rows, device="cuda") % len(toy.src)
    out = toy.graph.common_neighbors(toy.d_src[idx], toy.d_dst[idx], toy.d_ts[idx],
                                     since=_d_since("tensor", toy.ts)[idx], max_history=H,
                                     max_common=3)
    _same(_host(out, rows, 3), _want(toy, "tensor", H, 3), idx.cpu().numpy())


def test_a_graph_without_nodes_gives_zeros_and_padding():
    graph = _new_graph()
    src = torch.tensor([0, 5, -1], dtype=torch.int64, device="cuda")
    ts = torch.tensor([1e9, 0.0, float("nan")], device="cuda")
    for H in (1, 64, 512):
        got = _host(graph.common_neighbors(src, src.flip(0), ts, since=0.0, max_history=H,
                                           max_common=4), 3, 4)
        assert all((x == 0).all() for x in got[:5] + got[6:]) and (got[5] == -1).all()
    assert graph.temporal_degree(src, ts).tolist() == [0, 0, 0]


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("H", [33, 512])
def test_the_counts_are_pair_historys(toys, H, reverse):
    """Needs no restatement: under the same window, pair_history of (src, nodes[:, k]) counts
    cnt_src[:, k] and of (dst, nodes[:, k]) cnt_dst[:, k]; the -1 padding counts 0."""
    toy = toys[reverse]
    K = 40
    d_since = _d_since("tensor", toy.ts)
    out = toy.graph.common_neighbors(toy.d_src, toy.d_dst, toy.d_ts, since=d_since,
                                     max_history=H, max_common=K)
    assert (out.common > 0).sum() >= 15 and (out.nodes == -1).any() and \
        (out.common >= min(H, K)).any()
    for k in range(K):
        z = out.nodes[:, k].contiguous()
        for end, cnt in ((toy.d_src, out.cnt_src), (toy.d_dst, out.cnt_dst)):
            count = toy.graph.pair_history(end, z, toy.d_ts, since=d_since, max_history=H).count
            assert torch.equal(count, cnt[:, k].long()), k
        assert ((z >= 0) == (out.cnt_src[:, k] > 0)).all()
        assert ((z >= 0) == (out.cnt_dst[:, k] > 0)).all()
    filled = (out.nodes >= 0).sum(1)
    assert torch.equal(filled, out.common.clamp(max=K).long())


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("kind", KINDS)
def test_temporal_degree(toys, kind, reverse):
    toy = toys[reverse]
    K = 6
    nodes = toy.graph.common_neighbors(toy.d_src, toy.d_dst, toy.d_ts, max_history=129,
                                       max_common=K).nodes
    assert (nodes == -1).any() and (nodes >= 0).any()
    since = _since(kind, toy.ts)
    d_since = _d_since(kind, toy.ts)
    if isinstance(since, np.ndarray):
        since, d_since = since[:, None].repeat(K, 1), d_since[:, None].expand(-1, K)
    got = toy.graph.temporal_degree(nodes, toy.d_ts[:, None].expand(-1, K), since=d_since)
    assert got.dtype == torch.int64 and tuple(got.shape) == (len(toy.src), K) and got.is_cuda
    want = R.temporal_degree(toy.hist, nodes.cpu().numpy(), toy.ts[:, None], since)
    assert np.array_equal(got.cpu().numpy(), want)
    assert (want[nodes.cpu().numpy() < 0] == 0).all() and want.max() > 100
    # the queries' own ends, 1-D: negative, absent and past-the-table ids among them
    got = toy.graph.temporal_degree(toy.d_src, toy.d_ts, since=_d_since(kind, toy.ts))
    assert np.array_equal(got.cpu().numpy(),
                          R.temporal_degree(toy.hist, toy.src, toy.ts, _since(kind, toy.ts)))
    empty = toy.graph.temporal_degree(nodes[:0], toy.d_ts[:0, None].expand(-1, K))
    assert tuple(empty.shape) == (0, K) and empty.dtype == torch.int64


def test_arguments_are_checked_on_the_gpu_too(toys):
    toy = toys[False]
    with pytest.raises(ValueError, match="the graph is on device"):
        toy.graph.common_neighbors(toy.d_src.cpu(), toy.d_dst.cpu(), toy.d_ts.cpu())
    with pytest.raises(ValueError, match="dst is on"):
        toy.graph.common_neighbors(toy.d_src, toy.d_dst.cpu(), toy.d_ts)
    with pytest.raises(ValueError, match="max_history"):
        toy.graph.common_neighbors(toy.d_src, toy.d_dst, toy.d_ts, max_history=513)
    with pytest.raises(ValueError, match="max_common"):
        toy.graph.common_neighbors(toy.d_src, toy.d_dst, toy.d_ts, max_common=513)
    with pytest.raises(ValueError, match="the graph is on device"):
        toy.graph.temporal_degree(toy.d_src.cpu(), toy.d_ts.cpu())
    # and by the native entry itself, with nothing launched
    from gnnflow_amd import _capi
    p = toy.d_src.data_ptr()
    for H, K in ((0, 4), (513, 4), (64, 513)):
        rc = toy.graph._lib.gf_graph_common_neighbors(
            toy.graph._h, p, p, p, None, 4, H, K, p, p, p, p, p, p, p, p, 0, None)
        assert rc == _capi.GF_ERR_INVALID_ARGUMENT
    rc = toy.graph._lib.gf_graph_common_neighbors(
        toy.graph._h, p, p, p, None, 2 ** 31, 64, 4, p, p, p, p, p, p, p, p, 0, None)
    assert rc == _capi.GF_ERR_INVALID_ARGUMENT
    rc = toy.graph._lib.gf_graph_common_neighbors(
        toy.graph._h, p, None, p, None, 4, 64, 4, p, p, p, p, p, p, p, p, 0, None)
    assert rc == _capi.GF_ERR_INVALID_ARGUMENT
