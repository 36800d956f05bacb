"""gf_batch_hist_negatives and DeviceBatchStream(graph=, hist_ratio=) on the GPU against
tests/hist_negatives_ref.py, bit for bit.

The toy graph has 64 node ids and about 2 000 Zipf edges at 400 distinct times (so timestamps
repeat), ingested in two add_edges calls.  The stream is those edges plus eight rows put in at
position 7: a source whose only destination is the positive one (at two times), a source id the
graph never saw, ids at and past the node table's end and a negative one, a NaN time, and a time
later than every edge (the kernel's shortcut past the search).  The reference takes every node's
history from graph.get_temporal_neighbors, reversed to oldest first, and is computed ONCE per K
over the whole stream: a draw is keyed by the edge's global row, so every batch of every test
below is a slice of it."""
import numpy as np
import pytest

from tests import batch_stream_ref as R
from tests import hist_negatives_ref as H

pytestmark = pytest.mark.gpu

CANARY_I, CANARY_F, PAD = -0x0123456789ABCDEF, -12345.5, 67
SEED = 0x5EEDC0FFEE123457      # above 2^32: both key words of the generator are in play
EPOCH, FIRST_ROW = 5, 77
NODES, SPECIAL_AT = 64, 7
LONER, LONER_DST, ABSENT = 60, 7, 61      # 60 only ever pointed at 7; 61 and 62 have no edge


def _graph_edges():
    rng = np.random.RandomState(5)
    E = 2000
    p = 1.0 / np.arange(1, 57)
    p /= p.sum()
    src = rng.choice(56, E, p=p)
    dst = rng.permutation(60)[rng.choice(56, E, p=p)]
    time = np.floor(rng.rand(E) * 400)
    src = np.concatenate([src, [LONER] * 3, [59]])
    dst = np.concatenate([dst, [LONER_DST] * 3, [NODES - 1]])      # 63 ends the node table
    time = np.concatenate([time, [50, 150, 250], [399]])
    order = np.argsort(time, kind="stable")
    return (src[order].astype(np.int64), dst[order].astype(np.int64),
            time[order].astype(np.float32))


def _new_graph():
    import gnnflow_amd
    return gnnflow_amd.DynamicGraph(1 << 20, 1 << 28, "cuda", 8, 128, "insert")


def _histories(graph):
    """({node: (destinations, timestamps) oldest first}, table_len) as the graph stands."""
    table_len = graph.max_vertex_id() + 1
    out = {}
    for v in range(table_len):
        d, t, _ = graph.get_temporal_neighbors(v)
        if len(d):
            out[v] = (d[::-1].copy(), t[::-1].copy())
    return out, table_len


class Toy:
    pass


def _reference(toy, hist, table_len, K, lo=0, hi=None, epoch=EPOCH, first_row=FIRST_ROW):
    """(random negatives [K, B], with the historical ones written [K, B], classes [K, B], ts)"""
    hi = toy.rows if hi is None else hi
    B = hi - lo
    roots, ts = R.assemble(toy.src, toy.dst, toy.time, lo, hi, K, toy.dl, seed=SEED, epoch=epoch,
                           first_row=first_row)
    got, classes = H.overwrite(roots, toy.src, toy.dst, toy.time, lo, hi, K, K, hist, table_len,
                               seed=SEED, epoch=epoch, first_row=first_row)
    assert np.array_equal(got[:2 * B], roots[:2 * B])
    return roots[2 * B:].reshape(K, B), got[2 * B:].reshape(K, B), classes, ts[:B]


@pytest.fixture(scope="module")
def toy():
    from gnnflow_amd import DeviceDstSet
    t = Toy()
    g_src, g_dst, g_time = _graph_edges()
    t.graph_edges = (g_src, g_dst, g_time)
    t.graph = _new_graph()
    cut = 1200
    t.graph.add_edges(g_src[:cut], g_dst[:cut], g_time[:cut])
    t.graph.add_edges(g_src[cut:], g_dst[cut:], g_time[cut:])
    nan = np.float32("nan")
    special = [(LONER, LONER_DST, 300.0), (LONER, LONER_DST, 100.0), (ABSENT, 5, 200.0),
               (1000, 5, 200.0), (-3, 5, 200.0), (NODES, 5, 200.0), (0, 5, nan), (0, 5, 1e9)]
    t.src = np.insert(g_src, SPECIAL_AT, [s[0] for s in special])
    t.dst = np.insert(g_dst, SPECIAL_AT, [s[1] for s in special])
    t.time = np.insert(g_time, SPECIAL_AT, np.array([s[2] for s in special], np.float32))
    t.rows = len(t.src)
    t.eid = np.arange(t.rows, dtype=np.int64) + 11
    t.dl = np.unique(t.dst)
    t.dst_set = DeviceDstSet(NODES, "cuda:0", t.dst)
    t.hist, t.table_len = _histories(t.graph)
    assert t.table_len == NODES and ABSENT not in t.hist
    assert len(np.unique(g_time)) < len(g_time) // 3               # timestamps repeat
    assert set(t.hist[LONER][0].tolist()) == {LONER_DST}
    t.ref = {K: _reference(t, t.hist, t.table_len, K) for K in (1, 3)}
    return t


def _stream(toy, batch_size, K, Kh, graph=None, **kw):
    from gnnflow_amd import DeviceBatchStream
    kw.setdefault("seed", SEED)
    kw.setdefault("first_row", FIRST_ROW)
    rows = kw.pop("rows", slice(None))
    s = DeviceBatchStream(toy.src[rows], toy.dst[rows], toy.time[rows], toy.eid[rows], batch_size,
                          toy.dst_set, neg_ratio=K, graph=(graph or toy.graph) if Kh else None,
                          hist_ratio=Kh, **kw)
    s.set_epoch(EPOCH)
    return s


def _want_roots(toy, ref, lo, hi, K, Kh):
    """The batch [lo, hi) with Kh historical planes, from a whole-stream reference of K."""
    base, hist = ref[0], ref[1]
    planes = [toy.src[lo:hi], toy.dst[lo:hi]]
    planes += [hist[k, lo:hi] for k in range(Kh)] + [base[k, lo:hi] for k in range(Kh, K)]
    return np.concatenate(planes)


def _bits(a):
    return a.view(np.int32)


def test_the_reference_exercises_every_case(toy):
    """Computed from the reference alone: the comparisons below cannot pass vacuously."""
    for K in (1, 3):
        base, hist, classes, _ = toy.ref[K]
        assert np.mean(classes == H.HISTORICAL) >= 0.5
        for keep in (H.UNKNOWN_SOURCE, H.NO_HISTORY, H.ALL_REJECTED):
            assert np.any(classes == keep), keep
        assert np.array_equal(hist[classes != H.HISTORICAL], base[classes != H.HISTORICAL])
        assert np.mean(hist != base) > 0.4                        # the overwrite is visible
    classes = toy.ref[3][2][0]
    at = SPECIAL_AT
    assert classes[at:at + 8].tolist() == [H.ALL_REJECTED] * 2 + [H.NO_HISTORY] + \
        [H.UNKNOWN_SOURCE] * 3 + [H.NO_HISTORY, H.HISTORICAL]
    # rows on a tie: another edge of the source carries the row's time and is not its history,
    # although earlier edges are
    ties = [(s, t) for s, t in zip(toy.src[20:600].tolist(), toy.time[20:600])
            if np.count_nonzero(toy.hist[s][1] == t) >= 2 and H.history_size(toy.hist[s][1], t)]
    assert len(ties) >= 10


@pytest.mark.parametrize("K,Kh", [(1, 1), (3, 1), (3, 3)])
@pytest.mark.parametrize("B", [1, 2, 63, 64, 65, 257])
def test_batches_match_reference(toy, B, K, Kh):
    """Three batches of B rows from row 7 on (the special rows first) against the reference;
    everything but the first Kh negative planes against a stream without historical negatives."""
    import torch
    borders = np.minimum(SPECIAL_AT + B * np.arange(4), toy.rows)
    s = _stream(toy, B, K, Kh, borders=borders)
    s0 = _stream(toy, B, K, 0, borders=borders)
    assert s0.hist_filled is None and s.hist_filled.dtype == torch.int64
    want_filled = 0
    for b in range(3):
        lo, hi = int(borders[b]), int(borders[b + 1])
        n = hi - lo
        roots, ts, eids = (x.cpu().numpy() for x in s.batch(b))
        roots0, ts0, _ = (x.cpu().numpy() for x in s0.batch(b))
        assert roots.dtype == np.int64 and ts.dtype == np.float32
        assert np.array_equal(roots, _want_roots(toy, toy.ref[K], lo, hi, K, Kh))
        assert np.array_equal(roots[:2 * n], roots0[:2 * n])
        assert np.array_equal(roots[(2 + Kh) * n:], roots0[(2 + Kh) * n:])
        assert np.array_equal(_bits(ts), _bits(ts0))
        assert np.array_equal(_bits(ts), _bits(np.tile(toy.time[lo:hi], 2 + K)))
        assert np.array_equal(eids, toy.eid[lo:hi])
        want_filled += H.filled(toy.ref[K][2][:Kh, lo:hi])
    assert int(s.hist_filled.item()) == want_filled
    s.reset_hist_filled()
    assert int(s.hist_filled.item()) == 0


def test_whole_stream_materialize_equals_single_batches(toy):
    import torch
    K = Kh = 3
    s = _stream(toy, 257, K, Kh)
    many = s.materialize()
    torch.cuda.synchronize()
    total = H.filled(toy.ref[K][2])
    assert int(s.hist_filled.item()) == total and total >= toy.rows * Kh // 2
    s.reset_hist_filled()
    assert len(many) == len(s) == (toy.rows + 256) // 257
    for b, (roots, ts, eids) in enumerate(many):
        lo, hi = int(s.borders[b]), int(s.borders[b + 1])
        assert roots.storage_offset() == (2 + K) * lo
        one = s.batch(b)
        for x, y in zip(one, (roots, ts, eids)):      # by bits: one row's time is NaN
            assert np.array_equal(x.cpu().numpy().view(np.int32), y.cpu().numpy().view(np.int32))
        assert np.array_equal(roots.cpu().numpy(), _want_roots(toy, toy.ref[K], lo, hi, K, Kh))
    assert int(s.hist_filled.item()) == total                  # accumulated over the launches
    part = s.materialize(first=2, count=3)
    for b in range(3):
        assert np.array_equal(part[b][0].cpu().numpy(), many[2 + b][0].cpu().numpy())
    assert s.materialize(first=len(s)) == []


def _raw(toy, borders, rows, capacity, K, Kh, filled=True):
    """gf_batch_assemble_many then gf_batch_hist_negatives on canary-guarded buffers, one
    element off 16-byte alignment; returns (roots, ts, filled) after the canary check."""
    import torch
    from gnnflow_amd import _capi
    lib = _capi.load()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()      # noqa: E731
    d_src, d_dst, d_time, d_dl = dev(toy.src), dev(toy.dst), dev(toy.time), dev(toy.dl)
    d_count = torch.tensor([len(toy.dl)], dtype=torch.int64, device="cuda")
    d_b = dev(np.asarray(borders, dtype=np.int64))
    shift, n = 1, capacity
    roots = torch.full((shift + n + PAD,), CANARY_I, dtype=torch.int64, device="cuda")
    ts = torch.full((shift + n + PAD,), CANARY_F, dtype=torch.float32, device="cuda")
    count = torch.full((1 + PAD,), 0, dtype=torch.int64, device="cuda")
    count[1:] = CANARY_I
    stream = _capi.current_stream(torch.device("cuda", 0))
    _capi.check(lib.gf_batch_assemble_many(
        d_src.data_ptr(), d_dst.data_ptr(), d_time.data_ptr(), rows, d_b.data_ptr(),
        len(borders) - 1, 8, K, d_dl.data_ptr(), d_count.data_ptr(), SEED, EPOCH, FIRST_ROW,
        roots.data_ptr() + 8 * shift, ts.data_ptr() + 4 * shift, n, 0, stream))
    _capi.check(lib.gf_batch_hist_negatives(
        toy.graph._h, d_src.data_ptr(), d_dst.data_ptr(), d_time.data_ptr(), rows, d_b.data_ptr(),
        len(borders) - 1, 8, K, Kh, SEED, EPOCH, FIRST_ROW, roots.data_ptr() + 8 * shift, n,
        count.data_ptr() if filled else None, 0, stream))
    torch.cuda.synchronize()
    r, t, c = roots.cpu().numpy(), ts.cpu().numpy(), count.cpu().numpy()
    assert np.all(r[:shift] == CANARY_I) and np.all(r[shift + n:] == CANARY_I)
    assert np.all(t[:shift] == np.float32(CANARY_F)) and np.all(t[shift + n:] == np.float32(CANARY_F))
    assert np.all(c[1:] == CANARY_I)
    return r[shift:shift + n], t[shift:shift + n], int(c[0])


def test_raw_call_leaves_canaries_and_skips_bad_borders(toy):
    K, Kh = 3, 2
    borders = [3, 10, 10, 300]      # max_batch_rows = 8 undersizes the grid: still done in full
    full = 5 * (300 - 3)
    classes = toy.ref[K][2]

    def want(b):
        return _want_roots(toy, toy.ref[K], borders[b], borders[b + 1], K, Kh)

    roots, ts, filled = _raw(toy, borders, toy.rows, full, K, Kh)
    assert np.array_equal(roots[:35], want(0)) and np.array_equal(roots[35:], want(2))
    assert np.array_equal(_bits(ts[:35]), _bits(np.tile(toy.time[3:10], 5)))
    assert filled == H.filled(classes[:Kh, 3:300])
    # no counter asked for: the same batches
    again, _, zero = _raw(toy, borders, toy.rows, full, K, Kh, filled=False)
    assert np.array_equal(again, roots) and zero == 0
    # the stream is said to end at row 200: batch 2 (10..300) writes nothing, batch 0 does
    roots, _, filled = _raw(toy, borders, 200, full, K, Kh)
    assert np.array_equal(roots[:35], want(0)) and np.all(roots[35:] == CANARY_I)
    assert filled == H.filled(classes[:Kh, 3:10])
    # capacity for the first batch only
    roots, _, filled = _raw(toy, borders, toy.rows, 35, K, Kh)
    assert np.array_equal(roots, want(0)) and filled == H.filled(classes[:Kh, 3:10])


def test_raw_argument_errors(toy):
    import torch
    from gnnflow_amd import _capi
    lib = _capi.load()
    x = torch.zeros(64, dtype=torch.int64, device="cuda")
    t = torch.zeros(64, dtype=torch.float32, device="cuda")
    b = torch.tensor([0, 4], dtype=torch.int64, device="cuda")
    s = _capi.current_stream(torch.device("cuda", 0))
    g, p, q, bp = toy.graph._h, x.data_ptr(), t.data_ptr(), b.data_ptr()

    def call(graph=g, src=p, dst=p, time=q, rows=4, borders=bp, batches=1, K=2, Kh=1, roots=p):
        return lib.gf_batch_hist_negatives(graph, src, dst, time, rows, borders, batches, 4, K, Kh,
                                           0, 0, 0, roots, 16, None, 0, s)

    bad = _capi.GF_ERR_INVALID_ARGUMENT
    assert call(graph=None) == bad and b"null graph" in lib.gf_last_error()
    for null in ("src", "dst", "time", "borders", "roots"):
        assert call(**{null: None}) == bad, null
    assert call(K=2, Kh=3) == bad and b"hist_ratio" in lib.gf_last_error()
    assert call(K=1 << 16, Kh=1) == bad
    assert call(rows=1 << 44) == bad
    assert call(batches=1 << 31) == bad
    # nothing to do is not an error, whatever the buffers
    assert call(Kh=0, src=None, roots=None) == 0 and call(batches=0, borders=None) == 0
    torch.cuda.synchronize()
    assert int(x.abs().sum().item()) == 0


def test_same_edge_same_negatives_whatever_the_batches(toy):
    """Another batch size, and a slice of the stream that says where it starts (what a rank
    does), give every edge the negatives of the whole-stream reference."""
    K, Kh = 3, 3
    hist = toy.ref[K][1]
    for batch_size, start in ((100, 0), (64, 500)):
        s = _stream(toy, batch_size, K, Kh, rows=slice(start, None), first_row=FIRST_ROW + start)
        got = np.concatenate([r.cpu().numpy()[2 * len(e):].reshape(K, len(e))
                              for r, _, e in s], axis=1)
        assert np.array_equal(got, hist[:, start:])


def test_two_runs_are_bit_equal_and_the_epoch_changes_the_draws(toy):
    K, Kh = 3, 3
    lo, hi = 300, 365
    s = _stream(toy, 65, K, Kh, borders=[lo, hi])
    a, b = s.batch(0)[0].cpu().numpy(), s.batch(0)[0].cpu().numpy()
    assert np.array_equal(a, b) and np.array_equal(a, _want_roots(toy, toy.ref[K], lo, hi, K, Kh))
    # high words of the epoch and of the global row
    epoch, first_row = (1 << 32) + EPOCH, (1 << 63) - 5
    s = _stream(toy, 65, K, Kh, borders=[lo, hi], first_row=first_row)
    s.set_epoch(epoch)
    c = s.batch(0)[0].cpu().numpy()
    _, want, classes, _ = _reference(toy, toy.hist, toy.table_len, K, lo, hi, epoch=epoch,
                                     first_row=first_row)
    assert np.array_equal(c[2 * 65:], want.reshape(-1))
    assert np.mean(classes == H.HISTORICAL) > 0.5
    assert np.mean(c[2 * 65:] != a[2 * 65:]) > 0.3


def test_side_stream(toy):
    import torch
    K, Kh = 3, 2
    s = _stream(toy, 600, K, Kh)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    roots, _, _ = s.batch(1, stream=side)
    side.synchronize()
    assert np.array_equal(roots.cpu().numpy(), _want_roots(toy, toy.ref[K], 600, 1200, K, Kh))
    assert int(s.hist_filled.item()) == H.filled(toy.ref[K][2][:Kh, 600:1200])


def test_edges_added_later_are_drawn_from(toy):
    """A graph that holds the first 1 200 edges when the stream is built: batches launched after
    add_edges returns draw from the new edges too (the launch reads the store as it stands)."""
    import torch
    K, lo, hi = 3, 1500, 1757
    g_src, g_dst, g_time = toy.graph_edges
    graph = _new_graph()
    graph.add_edges(g_src[:1200], g_dst[:1200], g_time[:1200])
    s = _stream(toy, 257, K, K, graph=graph, borders=[lo, hi])
    before = s.batch(0)[0].cpu().numpy()
    early = _reference(toy, *_histories(graph), K, lo, hi)
    assert np.array_equal(before[2 * 257:], early[1].reshape(-1))
    torch.cuda.synchronize()                                   # the rule: launches done first
    graph.add_edges(g_src[1200:], g_dst[1200:], g_time[1200:])
    after = s.batch(0)[0].cpu().numpy()
    late = _reference(toy, *_histories(graph), K, lo, hi)
    assert np.array_equal(after, _want_roots(toy, toy.ref[K], lo, hi, K, K))
    assert np.array_equal(after[2 * 257:], late[1].reshape(-1))
    assert np.mean(late[1] != early[1]) > 0.3                  # the histories did grow


def test_after_offload_only_live_edges_are_drawn(toy):
    import torch
    K, lo, hi = 3, 1500, 1757
    g_src, g_dst, g_time = toy.graph_edges
    graph = _new_graph()
    graph.add_edges(g_src[:1000], g_dst[:1000], g_time[:1000])
    graph.add_edges(g_src[1000:], g_dst[1000:], g_time[1000:])
    s = _stream(toy, 257, K, K, graph=graph, borders=[lo, hi])
    s.batch(0)
    torch.cuda.synchronize()
    edges_before = graph.num_edges()
    assert graph.offload_old_blocks(200.0) > 0 and graph.num_edges() < edges_before
    hist, table_len = _histories(graph)
    assert sum(len(h[0]) for h in hist.values()) < sum(len(h[0]) for h in toy.hist.values())
    s.reset_hist_filled()
    got = s.batch(0)[0].cpu().numpy()
    _, want, classes, _ = _reference(toy, hist, table_len, K, lo, hi)
    assert np.array_equal(got[2 * 257:], want.reshape(-1))
    assert int(s.hist_filled.item()) == H.filled(classes)
    assert not np.array_equal(want, toy.ref[K][1][:, lo:hi])   # the dropped edges were drawn before
    live = {v: set(h[0].tolist()) for v, h in hist.items()}
    picked = classes == H.HISTORICAL
    for k, i in zip(*np.nonzero(picked)):
        assert want[k, i] in live[int(toy.src[lo + i])]


def test_evaluation_example_prints_the_historical_share(capsys):
    import importlib.util
    import math
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location(
        "evaluate_edge_prediction", os.path.join(root, "examples", "evaluate_edge_prediction.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    result = mod.main(num_batches=2, hist_negatives=2)
    line = [l for l in capsys.readouterr().out.splitlines() if l.startswith("ap ")][-1]
    share = float(re.search(r"historical negatives (\S+)% of 2 per edge", line).group(1)) / 100
    assert result["batches"] == 2 and result["mrr_batches"] == 2 and result["nonfinite"] == 0
    assert all(math.isfinite(result[k]) for k in ("ap", "auc", "mrr"))
    assert 0 < result["hist_share"] <= 1 and abs(result["hist_share"] - share) < 1e-3


def test_link_metrics_takes_the_k_major_result(toy):
    """Scores of a batch's positives and of its negatives as they lie in roots, fed to
    LinkMetrics: the MRR is that of each positive among ITS negatives at stride B, rank =
    1 + #greater + #equal / 2, summed in float64 (257 terms: far inside 1e-12)."""
    import torch
    from gnnflow_amd.metrics import LinkMetrics
    K, Kh, lo, hi = 3, 2, 7, 264
    B = hi - lo
    s = _stream(toy, B, K, Kh, borders=[lo, hi])
    roots, _, _ = s.batch(0)
    score = ((torch.arange(-8, 1200, device="cuda") * 37) % 101).to(torch.float32)
    pos, neg = score[roots[B:2 * B] + 8], score[roots[2 * B:] + 8]
    m = LinkMetrics("cuda:0")
    m.update(pos.reshape(B, 1), neg.reshape(K * B, 1), sigmoid=False)
    got = m.compute()
    want_roots = _want_roots(toy, toy.ref[K], lo, hi, K, Kh)
    table = ((np.arange(-8, 1200) * 37) % 101).astype(np.float32)
    p, n = table[want_roots[B:2 * B] + 8], table[want_roots[2 * B:] + 8].reshape(K, B)
    rank = 1 + (n > p).sum(axis=0) + (n == p).sum(axis=0) / 2
    assert got["mrr_batches"] == 1 and got["nonfinite"] == 0
    assert abs(got["mrr"] - np.mean(1 / rank)) <= 1e-12
