"""DynamicGraph.neighbor_cooccurrence (csrc/neighbor_cooccurrence.hip) on the GPU against
tests/neighbor_cooccurrence_ref.py: all five outputs exactly equal, the times by their bits.

The graph is test_gpu_common_neighbors.py's, built again here, with whole-numbered times in
[0, 100) so that timestamps repeat: node 0 is a hub with 430 edges over destinations 1 .. 13; nodes
40 and 41 are wide, 560 edges each to 560 distinct nodes (100 .. 619 and 1000 .. 1519) of which
they share 40 (2000 .. 2039); nodes 1 .. 29 have 290 edges among themselves and the hub; node 30
has one edge; node 2046 is only ever a destination, 2045 is never named and 2050 ends the node
table.  Built once directed and once with reverse edges.  The expected values come from
graph.get_temporal_neighbors per node through the numpy restatement, computed once per (graph,
since, length, include_self) and left unchanged.  The lengths are both sides of every bucket edge
of the kernel (32 | 33, 128 | 129), the largest and the smallest legal ones."""
import numpy as np
import pytest
import torch

from tests import neighbor_cooccurrence_ref as R

pytestmark = pytest.mark.gpu

HUB, WIDE_A, WIDE_B, SINGLE = 0, 40, 41, 30
ONLY_DST, ABSENT, LAST = 2046, 2045, 2050
SHARED = np.arange(2000, 2040)
TIE = 50.0
TIMES = [-1.0, TIE, 33.5, 1e9]
LENGTHS = [1, 2, 32, 33, 128, 129, 512]
KINDS = ["none", "scalar", "tensor"]
ENDS = [HUB, WIDE_A, WIDE_B, 3, 5, SINGLE, ONLY_DST, ABSENT, 2000, 100, -3, LAST, LAST + 1, 1 << 40]
CASES = [(L, s) for L in LENGTHS for s in (False, True) if L >= 1 + s]


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
        t.hist = R.from_graph(t.graph, np.arange(LAST + 1))
        t.d_src, t.d_dst, t.d_ts = (torch.from_numpy(x).cuda() for x in (src, dst, ts))
        t.ref = {}
        out[reverse] = t
    return out


def _want(toy, kind, L, self_slot):
    key = (kind, L, self_slot)
    if key not in toy.ref:
        toy.ref[key] = R.neighbor_cooccurrence(toy.hist, toy.src, toy.dst, toy.ts,
                                               _since(kind, toy.ts), L, self_slot)
    return toy.ref[key]


def _host(out, n, L):
    assert type(out).__name__ == "NeighborCooccurrence" and out._fields == R.FIELDS
    assert [x.dtype for x in out] == [torch.int32, torch.int64, torch.int64, torch.float32,
                                      torch.int32]
    assert [tuple(x.shape) for x in out] == [(n, 2), (n, 2, L), (n, 2, L), (n, 2, L),
                                             (n, 2, L, 2)]
    assert all(x.is_cuda and x.is_contiguous() for x in out)
    return tuple(x.cpu().numpy() for x in out)


def test_the_graph_and_the_reference_exercise_every_case(toys):
    """Computed from the stores and the restatement alone: the comparisons below are not
    vacuous."""
    toy, rev = toys[False], toys[True]
    h = toy.hist
    assert len(h[HUB][0]) == 430 and len(np.unique(h[HUB][0])) == 13
    assert len(np.intersect1d(h[WIDE_A][0], h[WIDE_B][0])) == 40
    assert len(h[ONLY_DST][0]) == 0 and len(h[ABSENT][0]) == 0 and len(h[SINGLE][0]) == 1
    assert len(toy.src) == 4 * len(ENDS) ** 2 + 3 and np.isnan(toy.ts).sum() == 3
    assert (toy.src == toy.dst).sum() >= 4 * len(ENDS)
    for t in (toy, rev):
        for L, self_slot in CASES:
            lengths, nodes, eids, times, counts = _want(t, "none", L, self_slot)
            s = int(self_slot)
            assert lengths.min() == s and (lengths == L).any(), (L, s)      # empty, full to L
            assert (lengths.max(1) == s).any() and (lengths.min(1) == L).any(), (L, s)
            if L >= 32:
                # counts >= 2 on both channels of one element; and rows with some co-occurrence
                assert ((counts[..., 0] >= 2) & (counts[..., 1] >= 2)).any(), (L, s)
            assert R.has_cooccurrence(nodes, counts).sum() >= 8, (L, s)
            assert not R.has_cooccurrence(nodes, counts).all()
            if self_slot:
                assert (nodes[:, :, 0] < 0).any() and (counts[nodes < 0] == 0).all()
                assert np.isnan(times[np.isnan(t.ts)][:, :, 0]).all()
        # rows cut by the bound: the hub has 430 edges and the wide nodes 560, every length cuts
        # some window, and the lower end and the tie cut too
        full = _want(t, "none", 512, False)[0]
        assert (full == 512).any() and 430 <= full[t.src == HUB, 0].max() < 512
        for L in (1, 32, 128):
            assert ((_want(t, "none", L, False)[0] == L) & (full > L)).any(), L
        assert 0 < _want(t, "scalar", 512, False)[0].sum() < full.sum()
        assert 0 < _want(t, "tensor", 512, False)[0].sum() < full.sum()
        tie, late = t.ts == np.float32(TIE), t.ts == np.float32(1e9)
        assert 0 < full[tie].sum() < full[late].sum()
        assert (full[t.ts == -1.0] == 0).all() and (full[np.isnan(t.ts)] == 0).all()
        # a row's keys at the table's design load: two full sides of distinct nodes
        wide = (t.src == WIDE_A) & (t.dst == WIDE_B) & late
        nodes = _want(t, "none", 512, False)[1][wide][0]
        assert len(np.unique(nodes)) >= 2 * 512 - 64
    # negative stored destinations do not occur in this graph; the fuzz stores have none either:
    # the rule for them is the self slot's (z < 0), which the rows with a negative end exercise
    assert (toy.edges[1] >= 0).all()


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("L,self_slot", CASES)
def test_outputs_match_the_reference(toys, L, self_slot, kind, reverse):
    toy = toys[reverse]
    out = toy.graph.neighbor_cooccurrence(toy.d_src, toy.d_dst, toy.d_ts,
                                          since=_d_since(kind, toy.ts), length=L,
                                          include_self=self_slot)
    R.same(_host(out, len(toy.src), L), _want(toy, kind, L, self_slot))


def test_defaults_empty_batch_repeat_calls_and_views(toys):
    toy = toys[True]
    n = len(toy.src)
    R.same(_host(toy.graph.neighbor_cooccurrence(toy.d_src, toy.d_dst, toy.d_ts), n, 32),
           _want(toy, "none", 32, True))
    empty = toy.graph.neighbor_cooccurrence(toy.d_src[:0], toy.d_dst[:0], toy.d_ts[:0], length=5)
    _host(empty, 0, 5)
    kw = dict(since=40.0, length=129, include_self=False)
    a = toy.graph.neighbor_cooccurrence(toy.d_src, toy.d_dst, toy.d_ts, **kw)
    b = toy.graph.neighbor_cooccurrence(toy.d_src, toy.d_dst, toy.d_ts, **kw)
    assert all(torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x,
                           y.view(torch.int32) if y.dtype == torch.float32 else y)
               for x, y in zip(a, b))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        c = toy.graph.neighbor_cooccurrence(toy.d_src, toy.d_dst, toy.d_ts, **kw)
    side.synchronize()
    R.same(tuple(x.cpu().numpy() for x in c), tuple(x.cpu().numpy() for x in a))
    # a non-contiguous src (and the rest) is taken for what it holds
    d_since = _d_since("tensor", toy.ts)
    whole = toy.graph.neighbor_cooccurrence(toy.d_src, toy.d_dst, toy.d_ts, since=d_since,
                                            length=33)
    assert not toy.d_src[1::3].is_contiguous()
    part = toy.graph.neighbor_cooccurrence(toy.d_src[1::3], toy.d_dst[1::3], toy.d_ts[1::3],
                                           since=d_since[1::3], length=33)
    R.same(tuple(x.cpu().numpy() for x in part),
           tuple(x[1::3].contiguous().cpu().numpy() for x in whole))


@pytest.mark.parametrize("L,rows", [(8, 4 * 4096 + 37), (40, 4 * 4096 + 37), (129, 4096 + 37)])
def test_rows_past_the_grid_limit_are_grid_strided(toys, L, rows):
    """A launch has at most 4096 workgroups, of four rows each in the two smaller buckets and of
    one in the largest: more rows than a pass covers, the queries repeated (at most 37 MB of
    outputs; well under a second)."""
    toy = toys[True]
    idx = torch.arange(rows, device="cuda") % len(toy.src)
    out = toy.graph.neighbor_cooccurrence(toy.d_src[idx], toy.d_dst[idx], toy.d_ts[idx],
                                          since=_d_since("tensor", toy.ts)[idx], length=L)
    want = R.neighbor_cooccurrence(toy.hist, toy.src, toy.dst, toy.ts, _since("tensor", toy.ts),
                                   L, True)
    R.same(_host(out, rows, L), want, idx.cpu().numpy())


def test_a_graph_without_nodes_gives_the_self_slots_alone():
    graph = _new_graph()
    src = torch.tensor([0, 5, -1], dtype=torch.int64, device="cuda")
    ts = torch.tensor([1e9, 0.0, float("nan")], device="cuda")
    for L in (2, 64, 512):
        got = _host(graph.neighbor_cooccurrence(src, src.flip(0), ts, since=0.0, length=L), 3, L)
        want = R.neighbor_cooccurrence({}, [0, 5, -1], [-1, 5, 0], ts.cpu().numpy(), 0.0, L, True)
        R.same(got, want)
        assert (got[0] == 1).all() and got[4][1, :, 0].tolist() == [[1, 1], [1, 1]]
    for L in (1, 64, 512):
        got = _host(graph.neighbor_cooccurrence(src, src.flip(0), ts, length=L,
                                                include_self=False), 3, L)
        assert (got[0] == 0).all() and (got[1] == -1).all() and (got[2] == -1).all()
        assert (got[3] == 0).all() and (got[4] == 0).all()


def test_arguments_are_checked_on_the_gpu_too(toys):
    toy = toys[False]
    with pytest.raises(ValueError, match="the graph is on device"):
        toy.graph.neighbor_cooccurrence(toy.d_src.cpu(), toy.d_dst.cpu(), toy.d_ts.cpu())
    with pytest.raises(ValueError, match="dst is on"):
        toy.graph.neighbor_cooccurrence(toy.d_src, toy.d_dst.cpu(), toy.d_ts)
    with pytest.raises(ValueError, match="length"):
        toy.graph.neighbor_cooccurrence(toy.d_src, toy.d_dst, toy.d_ts, length=513)
    with pytest.raises(ValueError, match="length"):
        toy.graph.neighbor_cooccurrence(toy.d_src, toy.d_dst, toy.d_ts, length=1)
    # and by the native entry itself, with nothing launched: a bound of 0 never reaches the kernel
    from gnnflow_amd import _capi
    p = toy.d_src.data_ptr()
    fn = toy.graph._lib.gf_graph_neighbor_cooccurrence
    for L, self_slot in ((0, 0), (1, 1), (513, 0), (513, 1)):
        assert fn(toy.graph._h, p, p, p, None, 4, L, self_slot, p, p, p, p, p, 0, None) == \
            _capi.GF_ERR_INVALID_ARGUMENT
    assert fn(toy.graph._h, p, p, p, None, 2 ** 31, 32, 1, p, p, p, p, p, 0, None) == \
        _capi.GF_ERR_INVALID_ARGUMENT
    assert fn(toy.graph._h, p, None, p, None, 4, 32, 1, p, p, p, p, p, 0, None) == \
        _capi.GF_ERR_INVALID_ARGUMENT
    assert fn(toy.graph._h, p, p, p, None, 4, 32, 1, p, p, p, p, None, 0, None) == \
        _capi.GF_ERR_INVALID_ARGUMENT
    assert fn(toy.graph._h, p, p, p, None, 4, 32, 1, p, p, p, p, p + 4, 0, None) == \
        _capi.GF_ERR_INVALID_ARGUMENT
    assert fn(toy.graph._h, None, None, None, None, 0, 32, 1, None, None, None, None, None, 0,
              None) == _capi.GF_OK
