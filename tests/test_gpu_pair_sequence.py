"""DynamicGraph.pair_sequence (csrc/pair_sequence.hip) on the GPU against
tests/pair_sequence_ref.py: lengths, nodes, eids and counts equal; times, delta_t and the table
parts equal BIT FOR BIT, compared through .view(torch.int32); the time part of the filled slots
equal bit for bit to ops.time_encode on the reader's own delta_t (and within 1e-6 of the float64
cosine of the reference's float32 argument: the precise cosf is good to 2 ulp of a result of
magnitude <= 1, 2.4e-7); every element of a padded slot the bits of +0.0.

The graph is test_gpu_neighbor_sequence.py's toy (40 node ids, about 730 edges at whole-numbered
times, node 0 a hub with 435 edges, five of them at exactly t = 50).  Every node is a source once
per time -- before every edge, on the tie, between two times, after every edge -- paired with
another node, with itself every seventh row; two rows have NaN times; the ends of eight rows are
negative or at and past the table's end.  The expected values come from
graph.get_temporal_neighbors per node through the numpy restatement, computed once per combination
and left unchanged.

Lengths: 2 (the self slot and one edge), 3, 32 and 33 (the first bucket's edge), 128 and 129 (the
second's, 129 being the first with four waves on a row), 512 (the limit).  Widths: 1 and 3 (scalar
chunks), 4 (one float4), 64 and 65, 172, 1024 (the limit), alone and mixed; the chunk type is
decided per part, so a mix has float4 parts next to scalar ones."""
import numpy as np
import pytest
import torch

from tests import pair_sequence_ref as R
from tests import test_gpu_neighbor_sequence as T

pytestmark = pytest.mark.gpu

NODES, HUB = T.NODES, T.HUB
LENGTHS = [2, 3, 32, 33, 128, 129, 512]
KINDS = T.KINDS
FIELDS = ("lengths", "nodes", "eids", "times", "delta_t", "counts")


def _queries():
    src, dst, ts = [], [], []
    for t in T.TIMES:
        for v in range(NODES):
            src.append(v), ts.append(t)
            dst.append(v if v % 7 == 3 else (v * 11 + 5) % NODES)
    for s, d in ((HUB, 3), (3, HUB)):
        src.append(s), dst.append(d), ts.append(np.nan)
    for s, d in ((-3, HUB), (HUB, -1), (NODES, 1), (1, 1000), (1 << 40, -7), (-1, -1),
                 (HUB, HUB), (T.HUB_OFTEN, HUB)):
        src.append(s), dst.append(d), ts.append(1e9)
    return np.array(src, np.int64), np.array(dst, np.int64), np.array(ts, np.float32)


@pytest.fixture(scope="module")
def toy():
    t = T.Toy()
    t.edges = T._edges()
    t.graph = T._new_graph(t.edges)
    t.src, t.dst, t.ts = _queries()
    t.hist = R.from_graph(t.graph, np.concatenate([t.src, t.dst]))
    t.d_src, t.d_dst = torch.from_numpy(t.src).cuda(), torch.from_numpy(t.dst).cuda()
    t.d_ts = torch.from_numpy(t.ts).cuda()
    t.num_edges = t.graph.num_edges()
    t.tabs, t.encs, t.dev, t.ref = {}, {}, {}, {}
    return t


def _want(toy, kind, length, node_tab=None, edge_tab=None, enc=None, hist=None):
    key = (kind, length, id(node_tab), id(edge_tab), id(enc), id(hist))
    if key not in toy.ref:
        w, b = (None, None) if enc is None else enc
        toy.ref[key] = (R.pair_sequence(toy.hist if hist is None else hist, toy.src, toy.dst,
                                        toy.ts, T._since(kind, toy.ts), length, node_tab,
                                        edge_tab, w, b),
                        node_tab, edge_tab, enc, hist)                 # keep the ids alive
    return toy.ref[key][0]


_bits = T._bits


def _same(out, want, n, length, d_enc=None, rows=None):
    """Every output against the reference (its rows `rows` when given)."""
    from gnnflow_amd import ops
    pick = (lambda x: x) if rows is None else (lambda x: x[rows])
    assert out.lengths.dtype == torch.int32 and tuple(out.lengths.shape) == (n, 2)
    assert out.counts.dtype == torch.int32 and tuple(out.counts.shape) == (n, 2, length, 2)
    for x, dtype in ((out.nodes, torch.int64), (out.eids, torch.int64),
                     (out.times, torch.float32), (out.delta_t, torch.float32)):
        assert x.dtype == dtype and tuple(x.shape) == (n, 2, length)
    for x in out:
        assert x is None or (x.is_cuda and x.is_contiguous() and not x.requires_grad and
                             x.grad_fn is None)
    lengths = pick(want.lengths)
    for name in ("lengths", "nodes", "eids", "counts"):
        assert np.array_equal(getattr(out, name).cpu().numpy(), pick(getattr(want, name))), name
    assert np.array_equal(_bits(out.times), _bits(pick(want.times)))
    assert np.array_equal(_bits(out.delta_t), _bits(pick(want.delta_t)))
    padding = np.arange(length)[None, None, :] >= lengths[:, :, None]
    for name, got, ref in (("node", out.node, want.node), ("edge", out.edge, want.edge)):
        if ref is None:
            assert got is None, name
            continue
        assert got.dtype == torch.float32 and tuple(got.shape) == (n, 2, length, ref.shape[3])
        assert np.array_equal(_bits(got), _bits(pick(ref))), name
        assert not _bits(got)[padding].any()
    if want.arg is None:
        assert out.time is None
        return
    dT = want.arg.shape[3]
    assert out.time.dtype == torch.float32 and tuple(out.time.shape) == (n, 2, length, dT)
    got = _bits(out.time)
    assert not got[padding].any()                               # +0.0, whatever the bias
    enc_out = ops.time_encode(out.delta_t.reshape(-1), d_enc[0], d_enc[1])
    assert np.array_equal(got[~padding], _bits(enc_out).reshape(n, 2, length, dT)[~padding])
    arg = pick(want.arg)[~padding].astype(np.float64)
    part = out.time.cpu().numpy()[~padding]
    known = np.isfinite(arg)                                    # a NaN time: NaN - NaN
    assert np.isnan(part[~known]).all()
    assert np.abs(part[known] - np.cos(arg[known])).max(initial=0.0) <= 1e-6


def _run(toy, kind="none", length=32, dn=0, de=0, dT=0, fixed=True, graph=None, hist=None):
    node_tab, edge_tab = T._tab(toy, "node", dn), T._tab(toy, "edge", de)
    enc = T._enc(toy, dT, fixed)
    d_enc = T._d_enc(toy, enc)
    out = (toy.graph if graph is None else graph).pair_sequence(
        toy.d_src, toy.d_dst, toy.d_ts, since=T._d_since(kind, toy.ts), length=length,
        node_feats=T._dev(toy, node_tab), edge_feats=T._dev(toy, edge_tab), time_encoder=d_enc)
    _same(out, _want(toy, kind, length, node_tab, edge_tab, enc, hist), len(toy.src), length,
          d_enc)
    return out


def test_the_graph_and_the_reference_exercise_every_case(toy):
    """Computed from the store and the reference alone: the comparisons below are not vacuous."""
    assert len(toy.hist[HUB][0]) == 435
    assert (toy.src == toy.dst).sum() > 20 and np.isnan(toy.ts).sum() == 2
    for L in LENGTHS:
        w = _want(toy, "none", L)
        n = w.lengths
        assert n.min() == 1 and n.max() == min(L, 436)          # the self slot is always there
        assert (n == 1).sum() > 80 and ((n == L).sum() >= 1 or L > 436)
        assert (n[toy.ts == -1.0] == 1).all() and (n[np.isnan(toy.ts)] == 1).all()
        assert (w.eids[:, :, 0] == -1).all() and np.array_equal(w.nodes[:, 0, 0], toy.src)
        assert np.array_equal(w.nodes[:, 1, 0], toy.dst)
        self_t = w.times[:, :, 0]
        assert np.array_equal(self_t.view(np.int32), np.stack([toy.ts, toy.ts], 1).view(np.int32))
        assert L < 32 or (w.counts > 1).any()                    # a neighbour met more than once
        both = (w.counts[..., 0] > 0) & (w.counts[..., 1] > 0)
        assert both.any() and (~both & (w.nodes >= 0)).any()
        pad = np.arange(L)[None, None, :] >= n[:, :, None]
        assert (w.nodes[pad] == -1).all() and not w.counts[pad].any()
        assert not w.delta_t[pad].view(np.int32).any()
    # a negative end is in its self slot and counted nowhere
    w = _want(toy, "none", 33)
    neg = toy.src < 0
    assert neg.sum() >= 2 and not w.counts[neg, 0, 0].any()
    for kind in ("scalar", "tensor"):
        cut = _want(toy, kind, 512).lengths
        assert cut.sum() < _want(toy, "none", 512).lengths.sum()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("length", LENGTHS)
def test_planes_and_parts_match_the_reference(toy, length, kind):
    out = _run(toy, kind, length)                                # the planes alone
    assert out.node is None and out.edge is None and out.time is None
    _run(toy, kind, length, dn=4, de=4, dT=4)                    # float4 chunks in every part
    _run(toy, kind, length, dn=3, de=4, dT=1)                    # one float4 part, two scalar


@pytest.mark.parametrize("dn,de,dT", [(4, 0, 0), (3, 0, 1), (4, 172, 100), (65, 3, 4),
                                      (0, 1024, 0), (1024, 0, 0), (1, 0, 0), (0, 1, 0),
                                      (0, 3, 0), (64, 0, 0), (0, 64, 0), (65, 0, 0), (0, 65, 0),
                                      (172, 0, 0), (0, 0, 1), (0, 0, 3), (0, 0, 4), (0, 0, 64),
                                      (0, 0, 65), (0, 0, 172), (0, 0, 1024), (172, 64, 4),
                                      (1, 1, 1), (172, 172, 172), (4, 3, 4), (3, 4, 3)])
def test_every_width_alone_and_mixed(toy, dn, de, dT):
    _run(toy, "tensor", 33, dn, de, dT)
    _run(toy, "none", 3, dn, de, dT)


@pytest.mark.parametrize("length", [129, 512])
def test_wide_parts_with_four_waves_on_a_row(toy, length):
    """The largest bucket's stride is 256 threads: widths below, at and above it."""
    _run(toy, "scalar", length, dn=65, de=172, dT=3)
    _run(toy, "none", length, dn=0, de=64, dT=100)


@pytest.mark.parametrize("dT", [1, 4, 100])
def test_time_part_with_a_random_weight_and_a_non_zero_bias(toy, dT):
    """The padding stays +0.0 where cos(bias) is not 0, the self slot is cos(bias)'s encoding of
    its own delta, and the filled slots are ops.time_encode's bits."""
    w, b = T._enc(toy, dT, fixed=False)
    assert (np.cos(b.astype(np.float64)) != 0).all()
    for length, kind in ((3, "none"), (33, "scalar"), (129, "tensor")):
        out = _run(toy, kind, length, dT=dT, fixed=False)
        _run(toy, kind, length, de=4, dT=dT, fixed=False)
    known = ~np.isnan(toy.ts)
    self_part = out.time[:, :, 0].cpu().numpy()[known]
    assert np.abs(self_part - np.cos(b.astype(np.float64))).max() <= 1e-6


def test_time_encoder_given_as_a_module(toy):
    from gnnflow_amd.nn import FixedTimeEncode, TimeEncode
    for module in (FixedTimeEncode(8).cuda(), TimeEncode(8).cuda()):
        holder = module if hasattr(module, "weight") else module.w
        pair = (holder.weight.detach(), holder.bias.detach())
        a = toy.graph.pair_sequence(toy.d_src, toy.d_dst, toy.d_ts, length=8,
                                    time_encoder=module)
        b = toy.graph.pair_sequence(toy.d_src, toy.d_dst, toy.d_ts, length=8, time_encoder=pair)
        assert not a.time.requires_grad and a.time.grad_fn is None
        assert torch.equal(a.time.view(torch.int32), b.time.view(torch.int32))
        filled = torch.arange(8, device="cuda") < a.lengths.unsqueeze(2)
        want = module(a.delta_t).detach().reshape(a.time.shape)
        assert filled.any() and not filled.all()
        assert torch.equal(a.time[filled].view(torch.int32), want[filled].view(torch.int32))
        assert not a.time[~filled].view(torch.int32).any()


def test_ids_without_a_row_give_a_zero_part(toy):
    node_short = T._tab(toy, "node", 172)[:T.NODE_ROWS].copy()
    edge_short = T._tab(toy, "edge", 4)[:toy.num_edges - 200].copy()
    enc = T._enc(toy, 4)
    for kind, length in (("none", 33), ("tensor", 3), ("scalar", 129)):
        out = toy.graph.pair_sequence(
            toy.d_src, toy.d_dst, toy.d_ts, since=T._d_since(kind, toy.ts), length=length,
            node_feats=T._dev(toy, node_short), edge_feats=T._dev(toy, edge_short),
            time_encoder=T._d_enc(toy, enc))
        want = _want(toy, kind, length, node_short, edge_short, enc)
        _same(out, want, len(toy.src), length, T._d_enc(toy, enc))
        full = _want(toy, kind, length, T._tab(toy, "node", 172), T._tab(toy, "edge", 4), enc)
        assert (want.node != full.node).any()
        assert np.array_equal(_bits(want.arg), _bits(full.arg))      # by bits: a NaN time's row
        no_row = want.nodes >= T.NODE_ROWS
        assert no_row[:, :, 0].any() and no_row[:, :, 1:].any()      # self slots and records
        assert not out.node.cpu().numpy()[no_row].any()
        # the self slot: the node's own row in `node`, the zero row in `edge`
        own = (toy.src >= 0) & (toy.src < T.NODE_ROWS)
        assert np.array_equal(out.node[:, 0, 0].cpu().numpy()[own], node_short[toy.src[own]])
        assert not out.edge[:, :, 0].view(torch.int32).any()


def test_a_table_that_is_not_16_byte_aligned_takes_scalar_chunks(toy):
    """A contiguous table one float into its storage: its width is a multiple of four and float4
    loads would be misaligned; the other parts keep their float4 chunks.  The same bits as the
    aligned call."""
    enc = T._enc(toy, 4)
    node_tab, edge_tab = T._tab(toy, "node", 172), T._tab(toy, "edge", 4)
    for which, tab in (("node", node_tab), ("edge", edge_tab)):
        flat = torch.zeros(tab.size + 1, dtype=torch.float32, device="cuda")
        flat[1:] = T._dev(toy, tab).reshape(-1)
        view = flat[1:].view(tab.shape)
        assert view.is_contiguous() and view.data_ptr() % 16 == 4
        kw = {"node_feats": T._dev(toy, node_tab), "edge_feats": T._dev(toy, edge_tab)}
        for length in (33, 129):
            aligned = toy.graph.pair_sequence(toy.d_src, toy.d_dst, toy.d_ts, length=length,
                                              time_encoder=T._d_enc(toy, enc), **kw)
            kw2 = dict(kw)
            kw2[which + "_feats"] = view
            out = toy.graph.pair_sequence(toy.d_src, toy.d_dst, toy.d_ts, length=length,
                                          time_encoder=T._d_enc(toy, enc), **kw2)
            _same(out, _want(toy, "none", length, node_tab, edge_tab, enc), len(toy.src), length,
                  T._d_enc(toy, enc))
            assert T._equal_bits(out, aligned)


def test_undirected_graph(toy):
    graph = T._new_graph(toy.edges, add_reverse=True)
    hist = R.from_graph(graph, np.concatenate([toy.src, toy.dst]))
    assert len(hist[T.ONLY_DST][0]) == 1 and int(hist[T.ONLY_DST][0][0]) == 5
    for kind, length in (("none", 512), ("tensor", 33), ("scalar", 2)):
        out = _run(toy, kind, length, dn=172, de=4, dT=4, graph=graph, hist=hist)
    both = graph.pair_sequence(toy.d_src, toy.d_dst, toy.d_ts, length=512)
    assert (both.lengths.cpu().numpy() >= _want(toy, "none", 512).lengths).all()
    assert both.lengths.sum() > out.lengths.sum()


def test_empty_batch_and_a_graph_without_edges(toy):
    nf, ef = T._dev(toy, T._tab(toy, "node", 65)), T._dev(toy, T._tab(toy, "edge", 4))
    enc = T._enc(toy, 4, fixed=False)
    d_enc = T._d_enc(toy, enc)
    empty = toy.graph.pair_sequence(toy.d_src[:0], toy.d_dst[:0], toy.d_ts[:0], length=7,
                                    node_feats=nf, edge_feats=ef, time_encoder=d_enc)
    assert tuple(empty.lengths.shape) == (0, 2) and empty.lengths.dtype == torch.int32
    for x, dtype in ((empty.nodes, torch.int64), (empty.eids, torch.int64),
                     (empty.times, torch.float32), (empty.delta_t, torch.float32)):
        assert tuple(x.shape) == (0, 2, 7) and x.dtype == dtype and x.is_cuda
    assert tuple(empty.counts.shape) == (0, 2, 7, 2) and empty.counts.dtype == torch.int32
    assert tuple(empty.node.shape) == (0, 2, 7, 65) and tuple(empty.edge.shape) == (0, 2, 7, 4)
    assert tuple(empty.time.shape) == (0, 2, 7, 4) and empty.time.dtype == torch.float32
    none = toy.graph.pair_sequence(toy.d_src[:0], toy.d_dst[:0], toy.d_ts[:0])
    assert none.node is None and none.edge is None and none.time is None
    assert tuple(none.nodes.shape) == (0, 2, 32)
    # a graph without nodes gives the self slots alone
    graph = T._new_graph()
    out = graph.pair_sequence(toy.d_src, toy.d_dst, toy.d_ts, since=0.0, length=7,
                              node_feats=nf, edge_feats=ef, time_encoder=d_enc)
    want = R.pair_sequence({}, toy.src, toy.dst, toy.ts, 0.0, 7, T._tab(toy, "node", 65),
                           T._tab(toy, "edge", 4), *enc)
    _same(out, want, len(toy.src), 7, d_enc)
    assert (out.lengths == 1).all() and (out.nodes[:, :, 1:] == -1).all()
    assert not out.edge.view(torch.int32).any() and out.node[:, :, 0].any()


def test_repeat_calls_give_the_same_bits_on_any_stream(toy):
    nf, ef = T._dev(toy, T._tab(toy, "node", 4)), T._dev(toy, T._tab(toy, "edge", 172))
    enc = T._enc(toy, 100)
    for length in (33, 129):
        def call():
            return toy.graph.pair_sequence(toy.d_src, toy.d_dst, toy.d_ts, since=40.0,
                                           length=length, node_feats=nf, edge_feats=ef,
                                           time_encoder=T._d_enc(toy, enc))
        a, b = call(), call()
        assert T._equal_bits(a, b)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            c = call()
        side.synchronize()
        assert T._equal_bits(a, c)
        _same(a, _want(toy, "scalar", length, T._tab(toy, "node", 4), T._tab(toy, "edge", 172),
                       enc), len(toy.src), length, T._d_enc(toy, enc))


def test_every_output_element_is_written(toy):
    """torch's allocator hands back the blocks just freed: fill blocks of the nine outputs' sizes
    with NaN (float) and a value no output holds (int), free them, and none may be left."""
    n = len(toy.src)
    nf, ef = T._dev(toy, T._tab(toy, "node", 65)), T._dev(toy, T._tab(toy, "edge", 4))
    enc = T._enc(toy, 3, fixed=False)
    junk_id = -(1 << 50)
    for kind, length in (("none", 33), ("tensor", 2), ("scalar", 512), ("none", 129)):
        torch.cuda.synchronize()
        junk = [torch.full((n, 2, length, d), float("nan"), device="cuda") for d in (65, 4, 3)]
        junk += [torch.full((n, 2, length), float("nan"), device="cuda") for _ in range(2)]
        junk += [torch.full((n, 2, length), junk_id, dtype=torch.int64, device="cuda")
                 for _ in range(2)]
        junk += [torch.full((n, 2, length, 2), -7, dtype=torch.int32, device="cuda"),
                 torch.full((n, 2), -7, dtype=torch.int32, device="cuda")]
        del junk
        out = toy.graph.pair_sequence(toy.d_src, toy.d_dst, toy.d_ts,
                                      since=T._d_since(kind, toy.ts), length=length,
                                      node_feats=nf, edge_feats=ef,
                                      time_encoder=T._d_enc(toy, enc))
        known = ~torch.isnan(toy.d_ts)                          # a NaN time is in its own row
        for x in (out.node, out.edge, out.time, out.times, out.delta_t):
            assert not torch.isnan(x[known]).any()
        assert (out.nodes != junk_id).all() and (out.eids != junk_id).all()
        assert (out.lengths >= 1).all() and (out.counts >= 0).all()
        _same(out, _want(toy, kind, length, T._tab(toy, "node", 65), T._tab(toy, "edge", 4), enc),
              n, length, T._d_enc(toy, enc))


def test_row_slices_and_strided_views_are_taken_for_what_they_hold(toy):
    ef = T._dev(toy, T._tab(toy, "edge", 172))
    enc = T._d_enc(toy, T._enc(toy, 4))
    d_since = T._d_since("tensor", toy.ts)

    def call(rows, **kw):
        return toy.graph.pair_sequence(toy.d_src[rows], toy.d_dst[rows], toy.d_ts[rows],
                                       since=d_since[rows], length=33, time_encoder=enc, **kw)
    a = call(slice(None), edge_feats=ef)
    for rows in (slice(40, 140), slice(None, None, 2), slice(1, None, 3)):
        assert T._equal_bits(call(rows, edge_feats=ef),
                             [None if x is None else x[rows] for x in a])
    # a row slice of a table is the table without its other rows
    short = toy.num_edges - 200
    d = call(slice(None), edge_feats=ef[:short])
    want = _want(toy, "tensor", 33, None, T._tab(toy, "edge", 172)[:short].copy(),
                 T._enc(toy, 4))
    _same(d, want, len(toy.src), 33, enc)


def test_before_and_after_add_edges_and_offload(toy):
    src, dst, t = toy.edges
    nodes = np.concatenate([toy.src, toy.dst])
    nf, ef = T._tab(toy, "node", 4), T._tab(toy, "edge", 3)
    enc = T._enc(toy, 4)

    def check(graph, hist, kind, length):
        out = graph.pair_sequence(toy.d_src, toy.d_dst, toy.d_ts,
                                  since=T._d_since(kind, toy.ts), length=length,
                                  node_feats=T._dev(toy, nf), edge_feats=T._dev(toy, ef),
                                  time_encoder=T._d_enc(toy, enc))
        w, b = enc
        want = R.pair_sequence(hist, toy.src, toy.dst, toy.ts, T._since(kind, toy.ts), length,
                               nf, ef, w, b)
        _same(out, want, len(toy.src), length, T._d_enc(toy, enc))
        return out

    graph = T._new_graph((src[:400], dst[:400], t[:400]))
    first = check(graph, R.from_graph(graph, nodes), "none", 33)
    torch.cuda.synchronize()      # add_edges moves segments: the launch above has completed
    graph.add_edges(src[400:], dst[400:], t[400:])
    second = check(graph, toy.hist, "none", 33)                 # the same store as in one piece
    assert (second.lengths >= first.lengths).all() and second.lengths.sum() > first.lengths.sum()
    check(graph, toy.hist, "tensor", 129)
    torch.cuda.synchronize()
    edges_before = graph.num_edges()
    assert graph.offload_old_blocks(60.0) > 0 and graph.num_edges() < edges_before
    hist = R.from_graph(graph, nodes)
    third = check(graph, hist, "none", 33)
    check(graph, hist, "scalar", 129)
    big_before = check(T._new_graph(toy.edges), toy.hist, "none", 512)
    big_after = check(graph, hist, "none", 512)
    assert (big_after.lengths <= big_before.lengths).all()
    assert big_after.lengths.sum() < big_before.lengths.sum() and third.lengths.sum() > 0


@pytest.mark.parametrize("length,rows", [(2, 4 * 4096 + 1), (129, 4096 + 1)])
def test_rows_past_the_grid_limit_are_grid_strided(toy, length, rows):
    """A launch has at most 4096 workgroups, of four rows each in the two smaller buckets and of
    one in the largest: one row more than a pass covers, the queries repeated, so that the
    expected rows are the reference's rows repeated.  Width 1 keeps the outputs small."""
    idx = torch.arange(rows, device="cuda") % len(toy.src)
    d_since = T._d_since("tensor", toy.ts)[idx]
    node_tab, edge_tab, enc = T._tab(toy, "node", 1), T._tab(toy, "edge", 1), T._enc(toy, 1)
    out = toy.graph.pair_sequence(toy.d_src[idx], toy.d_dst[idx], toy.d_ts[idx], since=d_since,
                                  length=length, node_feats=T._dev(toy, node_tab),
                                  edge_feats=T._dev(toy, edge_tab),
                                  time_encoder=T._d_enc(toy, enc))
    _same(out, _want(toy, "tensor", length, node_tab, edge_tab, enc), rows, length,
          T._d_enc(toy, enc), idx.cpu().numpy())


def test_inputs_are_detached_and_arguments_checked_on_the_gpu_too(toy):
    ef = T._dev(toy, T._tab(toy, "edge", 3)).clone().requires_grad_(True)
    w = T._dev(toy, T._enc(toy, 4)[0]).clone().reshape(-1, 1).requires_grad_(True)
    b = T._dev(toy, T._enc(toy, 4)[1]).clone().requires_grad_(True)
    ts = toy.d_ts.clone().requires_grad_(True)
    out = toy.graph.pair_sequence(toy.d_src, toy.d_dst, ts, length=8, edge_feats=ef,
                                  time_encoder=(w, b))
    for x in out:
        assert x is None or (not x.requires_grad and x.grad_fn is None)
    assert out.node is None and out.edge is not None
    with pytest.raises(ValueError, match="the graph is on device"):
        toy.graph.pair_sequence(toy.d_src.cpu(), toy.d_dst.cpu(), toy.d_ts.cpu())
    with pytest.raises(ValueError, match="edge_feats is on"):
        toy.graph.pair_sequence(toy.d_src, toy.d_dst, toy.d_ts, edge_feats=ef.detach().cpu())
    with pytest.raises(ValueError, match="contiguous"):
        toy.graph.pair_sequence(toy.d_src, toy.d_dst, toy.d_ts,
                                node_feats=T._dev(toy, T._tab(toy, "node", 64))[:, :32])
    with pytest.raises(TypeError, match="float32"):
        toy.graph.pair_sequence(toy.d_src, toy.d_dst, toy.d_ts, edge_feats=ef.detach().half())
    with pytest.raises(ValueError, match="length"):
        toy.graph.pair_sequence(toy.d_src, toy.d_dst, toy.d_ts, length=1)
