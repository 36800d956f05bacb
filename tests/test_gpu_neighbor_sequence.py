"""DynamicGraph.neighbor_sequence (csrc/neighbor_sequence.hip) on the GPU against
tests/neighbor_sequence_ref.py: lengths, nodes and eids equal; times, delta_t and the table parts
of the tokens equal BIT FOR BIT, compared through .view(torch.int32); the time part of the filled
slots equal bit for bit to ops.time_encode on the reader's own delta_t (and within 1e-6 of the
float64 cosine of the reference's float32 argument: the precise cosf is good to 2 ulp of a result
of magnitude <= 1, 2.4e-7); every element of a padded slot the bits of +0.0.

The graph is test_gpu_neighbor_aggregate.py's toy (its construction is copied here): 40 node ids
and about 730 edges at whole-numbered times in [0, 100), so timestamps repeat; node 0 is a hub with
435 edges, five of them at exactly t = 50; node 30 has one edge; node 38 is only ever a
destination, node 37 is never named, 39 ends the node table.  Every node is asked at times before
every edge, on the tie, between two times and after every edge; two rows have NaN times; five have
nodes that are negative, at and past the table's end.  The expected values come from
graph.get_temporal_neighbors per node through the numpy restatement, computed once per
combination and left unchanged.

Lengths: 1, 2, 8 (a few lanes), 64 and 65 (a wave of positions and one more), 512 (the limit).
Widths: 1 and 3 (scalar chunks), 4 (one float4), 64 and 65, 172 and 100 (the workload's own), 1024
(the limit), alone and mixed; a mix with a width that is no multiple of four takes scalar chunks
for every part."""
import numpy as np
import pytest
import torch

from tests import neighbor_sequence_ref as R

pytestmark = pytest.mark.gpu

NODES, HUB, SINGLE, ONLY_DST, ABSENT = 40, 0, 30, 38, 37
HUB_OFTEN = 13
TIE = 50.0
TIE_DSTS = [21, 22, 23, 24, 21]
TIMES = [-1.0, TIE, 33.5, 1e9]
NODE_ROWS = 20                   # ids 20 .. 39 have no row in the short node table
LENGTHS = [1, 2, 8, 64, 65, 512]
KINDS = ["none", "scalar", "tensor"]


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
    t.tabs, t.encs, t.dev, t.ref = {}, {}, {}, {}
    return t


def _tab(toy, which, d):
    """The host table of one kind ("node": a row per node id, "edge": a row per edge id) and
    width, random normal, made once; None for width 0."""
    if d == 0:
        return None
    if (which, d) not in toy.tabs:
        rng = np.random.RandomState(1000 * (which == "edge") + d)
        rows = NODES if which == "node" else toy.num_edges
        toy.tabs[which, d] = rng.randn(rows, d).astype(np.float32)
    return toy.tabs[which, d]


def _enc(toy, dT, fixed=True):
    """(weight [dT], bias [dT]) on the host: FixedTimeEncode's, or random with a non-zero bias."""
    if dT == 0:
        return None
    if (dT, fixed) not in toy.encs:
        if fixed:
            from gnnflow_amd.nn import FixedTimeEncode
            m = FixedTimeEncode(dT)
            toy.encs[dT, fixed] = (m.weight.reshape(-1).numpy().copy(), m.bias.numpy().copy())
        else:
            rng = np.random.RandomState(77 + dT)
            toy.encs[dT, fixed] = (rng.randn(dT).astype(np.float32),
                                   (rng.rand(dT) + 0.25).astype(np.float32))
    return toy.encs[dT, fixed]


def _dev(toy, arr):
    """The device copy of a host array, made once."""
    if arr is None:
        return None
    if id(arr) not in toy.dev:
        toy.dev[id(arr)] = (arr, torch.from_numpy(arr).cuda())
    return toy.dev[id(arr)][1]


def _d_enc(toy, enc):
    return None if enc is None else (_dev(toy, enc[0]).reshape(-1, 1), _dev(toy, enc[1]))


def _want(toy, kind, length, edge_tab=None, node_tab=None, enc=None, hist=None):
    key = (kind, length, id(edge_tab), id(node_tab), id(enc), id(hist))
    if key not in toy.ref:
        w, b = (None, None) if enc is None else enc
        toy.ref[key] = (R.neighbor_sequence(toy.hist if hist is None else hist, toy.nodes, toy.ts,
                                            _since(kind, toy.ts), length, edge_tab, node_tab, w, b),
                        edge_tab, node_tab, enc, hist)                 # keep the ids alive
    return toy.ref[key][0]


def _bits(x):
    return x.view(torch.int32).cpu().numpy() if isinstance(x, torch.Tensor) else x.view(np.int32)


def _same(out, want, n, length, enc=None, d_enc=None, rows=None):
    """Every output against the reference (its rows `rows` when given)."""
    from gnnflow_amd import ops
    pick = (lambda x: x) if rows is None else (lambda x: x[rows])
    assert out.lengths.dtype == torch.int32 and tuple(out.lengths.shape) == (n,)
    for x, dtype in ((out.nodes, torch.int64), (out.eids, torch.int64),
                     (out.times, torch.float32), (out.delta_t, torch.float32)):
        assert x.dtype == dtype and tuple(x.shape) == (n, length) and x.is_contiguous()
        assert x.is_cuda and not x.requires_grad
    lengths = pick(want.lengths)
    assert np.array_equal(out.lengths.cpu().numpy(), lengths)
    assert np.array_equal(out.nodes.cpu().numpy(), pick(want.nodes))
    assert np.array_equal(out.eids.cpu().numpy(), pick(want.eids))
    assert np.array_equal(_bits(out.times), _bits(pick(want.times)))
    assert np.array_equal(_bits(out.delta_t), _bits(pick(want.delta_t)))
    de = 0 if want.edge is None else want.edge.shape[2]
    dn = 0 if want.node is None else want.node.shape[2]
    dT = 0 if want.arg is None else want.arg.shape[2]
    if de + dn + dT == 0:
        assert out.tokens is None
        return
    tok = out.tokens
    assert tok.dtype == torch.float32 and tuple(tok.shape) == (n, length, de + dn + dT)
    assert tok.is_cuda and tok.is_contiguous() and not tok.requires_grad and tok.grad_fn is None
    padding = np.arange(length)[None, :] >= lengths[:, None]
    got = _bits(tok)
    assert not got[padding].any()                               # +0.0, the time part included
    if de:
        assert np.array_equal(got[..., :de], _bits(pick(want.edge)))
    if dn:
        assert np.array_equal(got[..., de:de + dn], _bits(pick(want.node)))
    if dT:
        enc_out = ops.time_encode(out.delta_t.reshape(-1), d_enc[0], d_enc[1])
        enc_bits = _bits(enc_out).reshape(n, length, dT)
        assert np.array_equal(got[..., de + dn:][~padding], enc_bits[~padding])
        arg = pick(want.arg)[~padding].astype(np.float64)
        part = tok[..., de + dn:].cpu().numpy()[~padding]
        assert np.isfinite(part).all() and np.abs(part - np.cos(arg)).max(initial=0.0) <= 1e-6


def _run(toy, kind="none", length=32, de=0, dn=0, dT=0, fixed=True, graph=None, hist=None):
    edge_tab, node_tab, enc = _tab(toy, "edge", de), _tab(toy, "node", dn), _enc(toy, dT, fixed)
    d_enc = _d_enc(toy, enc)
    out = (toy.graph if graph is None else graph).neighbor_sequence(
        toy.d_nodes, toy.d_ts, since=_d_since(kind, toy.ts), length=length,
        edge_feats=_dev(toy, edge_tab), node_feats=_dev(toy, node_tab), time_encoder=d_enc)
    _same(out, _want(toy, kind, length, edge_tab, node_tab, enc, hist), len(toy.nodes), length,
          enc, d_enc)
    return out


def test_the_graph_and_the_reference_exercise_every_case(toy):
    """Computed from the store and the reference alone: the comparisons below are not vacuous."""
    h = toy.hist
    assert toy.graph.max_vertex_id() == NODES - 1 and 720 <= toy.num_edges <= 745
    assert len(h[HUB][0]) == 435 and len(h[SINGLE][0]) == 1
    assert len(h[ONLY_DST][0]) == 0 and len(h[ABSENT][0]) == 0
    assert np.count_nonzero(h[HUB][1] == TIE) >= 5
    assert np.isnan(toy.ts).sum() == 2
    for L in LENGTHS:
        n = _want(toy, "none", L).lengths
        assert (n == 0).sum() > 40 and n.max() == min(L, 435)
        assert (n == L).sum() >= 1 or L > 435                    # 512 is longer than any window
        assert (n[toy.ts == -1.0] == 0).all() and (n[np.isnan(toy.ts)] == 0).all()
        assert (n[(toy.nodes < 0) | (toy.nodes >= NODES)] == 0).all()
    full = _want(toy, "none", 512)
    n = full.lengths
    assert (n == 1).sum() >= 1 and (n > 64).sum() >= 2 and (n == 0).sum() > 40
    hub_after = int(np.flatnonzero((toy.nodes == HUB) & (toy.ts == np.float32(1e9)))[0])
    assert n[hub_after] == 435
    # rows that fill, overflow and do not fill a length: n == L is also "cut by the length"
    assert (_want(toy, "none", 64).lengths == 64).sum() >= 2
    assert 0 < (_want(toy, "none", 8).lengths < 8).sum() < len(n)
    # the tie is excluded: the hub's sequence at t = 50 ends strictly before it
    hub_tie = int(np.flatnonzero((toy.nodes == HUB) & (toy.ts == np.float32(TIE)))[0])
    assert n[hub_tie] == int((h[HUB][1] < TIE).sum()) < int((h[HUB][1] <= TIE).sum())
    assert full.times[hub_tie, :n[hub_tie]].max() < TIE
    assert (full.delta_t[hub_tie, :n[hub_tie]] > 0).all()
    # length cuts visibly: the newest L of the window, oldest first
    totals = [int(_want(toy, "none", L).lengths.sum()) for L in LENGTHS]
    assert all(a < b for a, b in zip(totals, totals[1:]))
    short = _want(toy, "none", 8)
    assert np.array_equal(short.eids[hub_after], full.eids[hub_after, 435 - 8:435])
    assert (np.diff(full.times[hub_after, :435]) >= 0).all()
    # since cuts visibly, both as a scalar and as a tensor
    for kind in ("scalar", "tensor"):
        cut = _want(toy, kind, 512).lengths
        assert 0 < cut.sum() < n.sum() and (cut <= n).all()
    assert (_want(toy, "scalar", 512).times[_want(toy, "scalar", 512).eids >= 0] >= 40.0).all()
    # the padding is what the contract says
    pad = np.arange(512)[None, :] >= n[:, None]
    assert (full.nodes[pad] == -1).all() and (full.eids[pad] == -1).all()
    assert not full.times[pad].any() and not full.delta_t[pad].any()
    assert (full.eids[~pad] >= 0).all()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("length", LENGTHS)
def test_planes_and_tokens_match_the_reference(toy, length, kind):
    out = _run(toy, kind, length)                                # the planes alone
    assert out.tokens is None
    _run(toy, kind, length, de=4, dT=4)                          # float4 chunks
    _run(toy, kind, length, de=4, dn=3, dT=1)                    # scalar chunks


@pytest.mark.parametrize("de,dn,dT", [(4, 0, 0), (0, 3, 1), (172, 4, 100), (3, 65, 4),
                                      (1024, 0, 0), (1, 0, 0), (0, 1, 0), (3, 0, 0), (0, 4, 0),
                                      (64, 0, 0), (0, 64, 0), (65, 0, 0), (0, 65, 0),
                                      (0, 172, 0), (172, 0, 0), (0, 0, 1), (0, 0, 3), (0, 0, 4),
                                      (0, 0, 64), (0, 0, 65), (0, 0, 172), (64, 172, 4),
                                      (1, 1, 1), (172, 172, 172)])
def test_every_width_alone_and_mixed(toy, de, dn, dT):
    _run(toy, "tensor", 65, de, dn, dT)
    _run(toy, "none", 8, de, dn, dT)


@pytest.mark.parametrize("dT", [1, 4, 100])
def test_time_part_with_a_random_weight_and_a_non_zero_bias(toy, dT):
    """The padding stays +0.0 where cos(bias) is not 0, and the filled slots are ops.time_encode's
    bits, with FixedTimeEncode's frequencies and with random ones."""
    w, b = _enc(toy, dT, fixed=False)
    assert (np.cos(b.astype(np.float64)) != 0).all()
    for length, kind in ((8, "none"), (65, "scalar")):
        _run(toy, kind, length, dT=dT, fixed=False)
        _run(toy, kind, length, de=4, dT=dT, fixed=False)
        _run(toy, kind, length, dT=dT, fixed=True)


def test_time_encoder_given_as_a_module(toy):
    from gnnflow_amd.nn import FixedTimeEncode, TimeEncode
    for module in (FixedTimeEncode(8).cuda(), TimeEncode(8).cuda()):
        holder = module if hasattr(module, "weight") else module.w
        pair = (holder.weight.detach(), holder.bias.detach())
        a = toy.graph.neighbor_sequence(toy.d_nodes, toy.d_ts, length=8, time_encoder=module)
        b = toy.graph.neighbor_sequence(toy.d_nodes, toy.d_ts, length=8, time_encoder=pair)
        assert not a.tokens.requires_grad and a.tokens.grad_fn is None
        assert torch.equal(a.tokens.view(torch.int32), b.tokens.view(torch.int32))
        filled = torch.arange(8, device="cuda")[None, :] < a.lengths[:, None]
        want = module(a.delta_t).detach().reshape(a.tokens.shape)
        assert filled.any() and not filled.all()
        assert torch.equal(a.tokens[filled].view(torch.int32), want[filled].view(torch.int32))
        assert not a.tokens[~filled].view(torch.int32).any()


def test_ids_without_a_row_give_a_zero_part_and_the_time_part_is_intact(toy):
    node_short = _tab(toy, "node", 172)[:NODE_ROWS].copy()
    edge_short = _tab(toy, "edge", 4)[:toy.num_edges - 200].copy()
    enc = _enc(toy, 4)
    h = toy.hist
    assert (h[HUB][0] >= NODE_ROWS).any() and (h[HUB][2] >= len(edge_short)).any()
    for kind, length in (("none", 65), ("tensor", 8)):
        out = toy.graph.neighbor_sequence(
            toy.d_nodes, toy.d_ts, since=_d_since(kind, toy.ts), length=length,
            edge_feats=_dev(toy, edge_short), node_feats=_dev(toy, node_short),
            time_encoder=_d_enc(toy, enc))
        want = _want(toy, kind, length, edge_short, node_short, enc)
        _same(out, want, len(toy.nodes), length, enc, _d_enc(toy, enc))
        full = _want(toy, kind, length, _tab(toy, "edge", 4), _tab(toy, "node", 172), enc)
        assert np.array_equal(want.lengths, full.lengths) and np.array_equal(want.arg, full.arg)
        assert (want.node != full.node).any() and (want.edge != full.edge).any()
        no_row = (want.nodes >= NODE_ROWS)
        assert no_row.any() and not out.tokens[..., 4:176].cpu().numpy()[no_row].any()


def test_a_table_that_is_not_16_byte_aligned_takes_scalar_chunks(toy):
    """A contiguous table one float into its storage: every width is a multiple of four and
    float4 loads would be misaligned.  The same bits as the aligned call."""
    for which, d in (("node", 172), ("edge", 4)):
        tab = _tab(toy, which, d)
        flat = torch.zeros(tab.size + 1, dtype=torch.float32, device="cuda")
        flat[1:] = _dev(toy, tab).reshape(-1)
        view = flat[1:].view(tab.shape)
        assert view.is_contiguous() and view.data_ptr() % 16 == 4
        enc = _enc(toy, 4)
        kw = {which + "_feats": view}
        out = toy.graph.neighbor_sequence(toy.d_nodes, toy.d_ts, length=65,
                                          time_encoder=_d_enc(toy, enc), **kw)
        want = _want(toy, "none", 65, tab if which == "edge" else None,
                     tab if which == "node" else None, enc)
        _same(out, want, len(toy.nodes), 65, enc, _d_enc(toy, enc))
        aligned = toy.graph.neighbor_sequence(
            toy.d_nodes, toy.d_ts, length=65, time_encoder=_d_enc(toy, enc),
            **{which + "_feats": _dev(toy, tab)})
        assert torch.equal(out.tokens.view(torch.int32), aligned.tokens.view(torch.int32))


def test_undirected_graph(toy):
    graph = _new_graph(toy.edges, add_reverse=True)
    hist = R.from_graph(graph, toy.nodes)
    assert len(hist[ONLY_DST][0]) == 1 and int(hist[ONLY_DST][0][0]) == 5
    for kind, length in (("none", 512), ("tensor", 64), ("scalar", 1)):
        out = _run(toy, kind, length, de=4, dn=172, dT=4, graph=graph, hist=hist)
    assert out.lengths.sum() > 0
    both = graph.neighbor_sequence(toy.d_nodes, toy.d_ts, length=512)
    assert (both.lengths.cpu().numpy() >= _want(toy, "none", 512).lengths).all()


def test_empty_batch_and_a_graph_without_edges(toy):
    ef, nf = _dev(toy, _tab(toy, "edge", 4)), _dev(toy, _tab(toy, "node", 65))
    enc = _d_enc(toy, _enc(toy, 4, fixed=False))
    empty = toy.graph.neighbor_sequence(toy.d_nodes[:0], toy.d_ts[:0], length=7, edge_feats=ef,
                                        node_feats=nf, time_encoder=enc)
    assert tuple(empty.lengths.shape) == (0,) and empty.lengths.dtype == torch.int32
    for x, dtype in ((empty.nodes, torch.int64), (empty.eids, torch.int64),
                     (empty.times, torch.float32), (empty.delta_t, torch.float32)):
        assert tuple(x.shape) == (0, 7) and x.dtype == dtype and x.is_cuda
    assert tuple(empty.tokens.shape) == (0, 7, 73) and empty.tokens.dtype == torch.float32
    assert toy.graph.neighbor_sequence(toy.d_nodes[:0], toy.d_ts[:0]).tokens is None
    graph = _new_graph()
    out = graph.neighbor_sequence(toy.d_nodes, toy.d_ts, since=0.0, length=7, edge_feats=ef,
                                  node_feats=nf, time_encoder=enc)
    assert not out.lengths.any() and (out.nodes == -1).all() and (out.eids == -1).all()
    assert not out.times.view(torch.int32).any() and not out.delta_t.view(torch.int32).any()
    assert tuple(out.tokens.shape) == (len(toy.nodes), 7, 73)
    assert not out.tokens.view(torch.int32).any()


def _equal_bits(a, b):
    return all((x is None and y is None) or torch.equal(
        x.view(torch.int32) if x.dtype == torch.float32 else x,
        y.view(torch.int32) if y.dtype == torch.float32 else y) for x, y in zip(a, b))


def test_repeat_calls_give_the_same_bits_on_any_stream(toy):
    ef, nf = _dev(toy, _tab(toy, "edge", 172)), _dev(toy, _tab(toy, "node", 4))
    enc = _enc(toy, 100)

    def call():
        return toy.graph.neighbor_sequence(toy.d_nodes, toy.d_ts, since=40.0, length=65,
                                           edge_feats=ef, node_feats=nf,
                                           time_encoder=_d_enc(toy, enc))
    a, b = call(), call()
    assert _equal_bits(a, b)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        c = call()
    side.synchronize()
    assert _equal_bits(a, c)
    _same(a, _want(toy, "scalar", 65, _tab(toy, "edge", 172), _tab(toy, "node", 4), enc),
          len(toy.nodes), 65, enc, _d_enc(toy, enc))


def test_every_output_element_is_written(toy):
    """torch's allocator hands back the blocks just freed: fill blocks of the six outputs' sizes
    with NaN (float) and a value no output holds (int), free them, and none may be left."""
    n = len(toy.nodes)
    ef, nf = _dev(toy, _tab(toy, "edge", 4)), _dev(toy, _tab(toy, "node", 65))
    enc = _enc(toy, 3, fixed=False)
    junk_id = -(1 << 50)
    for kind, length in (("none", 65), ("tensor", 2), ("scalar", 512)):
        torch.cuda.synchronize()
        junk = [torch.full((n, length, 72), float("nan"), device="cuda"),
                torch.full((n, length), float("nan"), device="cuda"),
                torch.full((n, length), float("nan"), device="cuda"),
                torch.full((n, length), junk_id, dtype=torch.int64, device="cuda"),
                torch.full((n, length), junk_id, dtype=torch.int64, device="cuda"),
                torch.full((n,), -7, dtype=torch.int32, device="cuda")]
        del junk
        out = toy.graph.neighbor_sequence(toy.d_nodes, toy.d_ts, since=_d_since(kind, toy.ts),
                                          length=length, edge_feats=ef, node_feats=nf,
                                          time_encoder=_d_enc(toy, enc))
        assert not torch.isnan(out.tokens).any() and not torch.isnan(out.times).any()
        assert not torch.isnan(out.delta_t).any()
        assert (out.nodes != junk_id).all() and (out.eids != junk_id).all()
        assert (out.lengths >= 0).all()
        _same(out, _want(toy, kind, length, _tab(toy, "edge", 4), _tab(toy, "node", 65), enc), n,
              length, enc, _d_enc(toy, enc))


def test_row_slices_and_strided_views_are_taken_for_what_they_hold(toy):
    ef = _dev(toy, _tab(toy, "edge", 172))
    enc = _d_enc(toy, _enc(toy, 4))
    d_since = _d_since("tensor", toy.ts)

    def call(rows, **kw):
        return toy.graph.neighbor_sequence(toy.d_nodes[rows], toy.d_ts[rows],
                                           since=d_since[rows], length=64, time_encoder=enc, **kw)
    a = call(slice(None), edge_feats=ef)
    for rows in (slice(40, 140), slice(None, None, 2), slice(1, None, 3)):
        assert _equal_bits(call(rows, edge_feats=ef), [x[rows] for x in a])
    # a row slice of a table is the table without its other rows
    short = toy.num_edges - 200
    d = call(slice(None), edge_feats=ef[:short])
    want = _want(toy, "tensor", 64, _tab(toy, "edge", 172)[:short].copy(), None, _enc(toy, 4))
    _same(d, want, len(toy.nodes), 64, _enc(toy, 4), enc)


def test_rows_past_the_grid_limit_are_grid_strided(toy):
    """The launch has at most 4096 workgroups of four rows, a wave per row: more rows than those
    16 384, the queries repeated, so that the expected rows are the reference's rows repeated.
    length = 4 and narrow widths keep the outputs at a few megabytes."""
    rows = 4 * 4096 + 37
    idx = torch.arange(rows, device="cuda") % len(toy.nodes)
    d_since = _d_since("tensor", toy.ts)[idx]
    for de, dn, dT in ((4, 0, 4), (4, 3, 1)):
        edge_tab, node_tab, enc = _tab(toy, "edge", de), _tab(toy, "node", dn), _enc(toy, dT)
        out = toy.graph.neighbor_sequence(toy.d_nodes[idx], toy.d_ts[idx], since=d_since,
                                          length=4, edge_feats=_dev(toy, edge_tab),
                                          node_feats=_dev(toy, node_tab),
                                          time_encoder=_d_enc(toy, enc))
        _same(out, _want(toy, "tensor", 4, edge_tab, node_tab, enc), rows, 4, enc,
              _d_enc(toy, enc), idx.cpu().numpy())


def test_inputs_are_detached_and_arguments_checked_on_the_gpu_too(toy):
    ef = _dev(toy, _tab(toy, "edge", 3)).clone().requires_grad_(True)
    w = _dev(toy, _enc(toy, 4)[0]).clone().reshape(-1, 1).requires_grad_(True)
    b = _dev(toy, _enc(toy, 4)[1]).clone().requires_grad_(True)
    ts = toy.d_ts.clone().requires_grad_(True)
    out = toy.graph.neighbor_sequence(toy.d_nodes, ts, length=8, edge_feats=ef,
                                      time_encoder=(w, b))
    for x in out:
        assert not x.requires_grad and x.grad_fn is None
    with pytest.raises(ValueError, match="the graph is on device"):
        toy.graph.neighbor_sequence(toy.d_nodes.cpu(), toy.d_ts.cpu(), edge_feats=ef.cpu())
    with pytest.raises(ValueError, match="edge_feats is on"):
        toy.graph.neighbor_sequence(toy.d_nodes, toy.d_ts, edge_feats=ef.detach().cpu())
    with pytest.raises(ValueError, match="time_encoder's bias is on"):
        toy.graph.neighbor_sequence(toy.d_nodes, toy.d_ts, time_encoder=(w, b.detach().cpu()))
    with pytest.raises(ValueError, match="contiguous"):
        toy.graph.neighbor_sequence(toy.d_nodes, toy.d_ts,
                                    node_feats=_dev(toy, _tab(toy, "node", 64))[:, :32])
    with pytest.raises(TypeError, match="float32"):
        toy.graph.neighbor_sequence(toy.d_nodes, toy.d_ts, edge_feats=ef.detach().half())
    with pytest.raises(ValueError, match="1 to 1024"):
        toy.graph.neighbor_sequence(toy.d_nodes, toy.d_ts,
                                    node_feats=torch.zeros(2, 1025, device="cuda"))
    with pytest.raises(ValueError, match="length"):
        toy.graph.neighbor_sequence(toy.d_nodes, toy.d_ts, length=513)
