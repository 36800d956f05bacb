"""gf_batch_assemble / gf_batch_assemble_many and DeviceBatchStream on the GPU against
tests/batch_stream_ref.py, bit for bit.

Shapes: B around the quad (4 rows), the wave (64) and the workgroup (256 lanes of quads) edges;
lo = 3 (nothing aligned), 2 (the int64 columns aligned, time not) and 8 (all aligned); outputs
at an aligned and at a shifted address; so every 16-byte / scalar path and the partial last
quad run.  Every raw call writes into buffers with a canary region behind them."""
import numpy as np
import pandas as pd
import pytest

from tests import batch_stream_ref as R

pytestmark = pytest.mark.gpu

CANARY_I, CANARY_F, PAD = -0x0123456789ABCDEF, -12345.5, 67
SEED = 0x5EEDC0FFEE123457      # above 2^32: both key words of the generator are in play


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _stream_arrays(E, seed):
    rng = np.random.RandomState(seed)
    return (rng.randint(0, 1 << 40, E).astype(np.int64), rng.randint(0, 1 << 40, E).astype(np.int64),
            rng.rand(E).astype(np.float32) * 1000)


def _dl(M):
    return (np.arange(M, dtype=np.int64) * 3 + 11)


def _buffers(n, shift):
    """roots / ts views of n elements starting `shift` elements into canary-filled storage."""
    import torch
    roots = torch.full((shift + n + PAD,), CANARY_I, dtype=torch.int64, device="cuda")
    ts = torch.full((shift + n + PAD,), CANARY_F, dtype=torch.float32, device="cuda")
    return roots, ts


def _check_canaries(roots, ts, shift, n):
    r, t = roots.cpu().numpy(), ts.cpu().numpy()
    assert np.all(r[:shift] == CANARY_I) and np.all(r[shift + n:] == CANARY_I)
    assert np.all(t[:shift] == np.float32(CANARY_F)) and np.all(t[shift + n:] == np.float32(CANARY_F))
    return r[shift:shift + n], t[shift:shift + n]


def _raw(src, dst, time, lo, hi, K, dl, seed=0, epoch=0, first_row=0, shift=0, count=None):
    """One gf_batch_assemble call on device copies; returns (roots, ts) after the canary check."""
    import torch
    from gnnflow_amd import _capi
    lib = _capi.load()
    n = (2 + K) * (hi - lo)
    d_src, d_dst, d_time = _dev(src), _dev(dst), _dev(time)
    d_dl = _dev(dl) if K else None
    d_count = torch.tensor([len(dl) if count is None else count], dtype=torch.int64,
                           device="cuda") if K else None
    roots, ts = _buffers(n, shift)
    _capi.check(lib.gf_batch_assemble(
        d_src.data_ptr(), d_dst.data_ptr(), d_time.data_ptr(), len(src), lo, hi, K,
        d_dl.data_ptr() if K else None, d_count.data_ptr() if K else None, seed, epoch, first_row,
        roots.data_ptr() + 8 * shift, ts.data_ptr() + 4 * shift, 0,
        _capi.current_stream(torch.device("cuda", 0))))
    torch.cuda.synchronize()
    return _check_canaries(roots, ts, shift, n)


def _equal(got, want):
    assert got[0].dtype == np.int64 and got[1].dtype == np.float32
    assert np.array_equal(got[0], want[0])
    assert np.array_equal(got[1].view(np.int32), want[1].view(np.int32))


@pytest.mark.parametrize("K", [0, 1, 3, 9])
@pytest.mark.parametrize("B", [1, 2, 63, 64, 65, 257, 600])
def test_batch_matches_reference(B, K):
    E = B + 13
    src, dst, time = _stream_arrays(E, B * 16 + K)
    for M in ([1, 2, 7, 1000] if K else [1]):
        dl = _dl(M)
        for lo, shift in ((3, 0), (2, 1), (8, 0), (8, 1)):
            want = R.assemble(src, dst, time, lo, lo + B, K, dl, seed=SEED, epoch=5, first_row=77)
            got = _raw(src, dst, time, lo, lo + B, K, dl, seed=SEED, epoch=5, first_row=77,
                       shift=shift)
            _equal(got, want)


@pytest.mark.parametrize("epoch", [0, (1 << 32) + 1])
@pytest.mark.parametrize("first_row", [3 * 10 ** 9, (1 << 63) - 5])
def test_high_words_of_row_and_epoch(first_row, epoch):
    B, K = 65, 3
    src, dst, time = _stream_arrays(B + 4, 3)
    dl = _dl(1000)
    want = R.assemble(src, dst, time, 4, 4 + B, K, dl, seed=SEED, epoch=epoch, first_row=first_row)
    _equal(_raw(src, dst, time, 4, 4 + B, K, dl, seed=SEED, epoch=epoch, first_row=first_row),
           want)
    if epoch:      # the high word matters: epoch 1 draws something else
        other = R.assemble(src, dst, time, 4, 4 + B, K, dl, seed=SEED, epoch=1, first_row=first_row)
        assert not np.array_equal(other[0], want[0])


def test_two_runs_are_bit_equal():
    src, dst, time = _stream_arrays(300, 8)
    a = _raw(src, dst, time, 1, 298, 9, _dl(7), seed=SEED, epoch=2)
    b = _raw(src, dst, time, 1, 298, 9, _dl(7), seed=SEED, epoch=2)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.int32), b[1].view(np.int32))


def test_count_is_read_from_device_memory():
    """The list's length comes from d_dl_count: a longer buffer behind it is never drawn from,
    and a count that allows no draw gives -1."""
    src, dst, time = _stream_arrays(70, 9)
    dl = _dl(1000)
    got = _raw(src, dst, time, 0, 70, 2, dl, seed=3, count=7)
    _equal(got, R.assemble(src, dst, time, 0, 70, 2, dl[:7], seed=3))
    for count in (0, -4, 1 << 32):
        roots, _ = _raw(src, dst, time, 0, 70, 2, dl, seed=3, count=count)
        assert np.array_equal(roots[:140], np.concatenate([src, dst])) and np.all(roots[140:] == -1)


def test_raw_argument_errors():
    import torch
    from gnnflow_amd import _capi
    lib = _capi.load()
    x = torch.zeros(16, dtype=torch.int64, device="cuda")
    t = torch.zeros(16, dtype=torch.float32, device="cuda")
    s = _capi.current_stream(torch.device("cuda", 0))
    p, q = x.data_ptr(), t.data_ptr()
    assert lib.gf_batch_assemble(p, p, q, 4, 3, 2, 0, None, None, 0, 0, 0, p, q, 0, s) == 1
    assert lib.gf_batch_assemble(p, p, q, 4, 0, 5, 0, None, None, 0, 0, 0, p, q, 0, s) == 1
    assert lib.gf_batch_assemble(p, p, q, 4, 0, 4, 1, None, None, 0, 0, 0, p, q, 0, s) == 1
    assert lib.gf_batch_assemble(p, None, q, 4, 0, 4, 0, None, None, 0, 0, 0, p, q, 0, s) == 1
    assert lib.gf_batch_assemble(p, p, q, 4, 2, 2, 0, None, None, 0, 0, 0, None, None, 0, s) == 0
    torch.cuda.synchronize()


# ---- the Python class --------------------------------------------------------------------
@pytest.fixture(scope="module")
def toy():
    """A 1 000-row stream, its destination set on the device, and the reference's list."""
    from gnnflow_amd import DeviceDstSet
    rng = np.random.RandomState(21)
    E = 1000
    src, dst = rng.randint(0, 300, E), rng.randint(300, 500, E)
    time = np.sort(rng.rand(E) * 5000)
    df = pd.DataFrame({"src": src, "dst": dst, "time": time, "eid": np.arange(E) + 7})
    dst_set = DeviceDstSet(500, "cuda:0", dst)
    return df, dst_set, np.unique(dst)


def _np(batch):
    return tuple(x.cpu().numpy() for x in batch)


def test_stream_batches(toy):
    from gnnflow_amd import DeviceBatchStream
    df, dst_set, dl = toy
    s = DeviceBatchStream(df.src.values, df.dst.values, df.time.values, df.eid.values, 300,
                          dst_set, neg_ratio=3, seed=SEED, first_row=50)
    assert len(s) == 4 and s.borders.tolist() == [0, 300, 600, 900, 1000]
    s.set_epoch(6)
    got = [_np(b) for b in s]
    assert len(got) == 4
    for i, (roots, ts, eids) in enumerate(got):
        lo, hi = s.borders[i], s.borders[i + 1]
        want = R.assemble(df.src.values, df.dst.values, df.time.values, lo, hi, 3, dl, seed=SEED,
                          epoch=6, first_row=50)
        _equal((roots, ts), want)
        assert np.array_equal(eids, df.eid.values[lo:hi])
    _equal(_np(s[-1])[:2], got[3][:2])
    with pytest.raises(IndexError):
        s[4]
    # a view, not a copy
    assert s[1][2].data_ptr() == s.eid.data_ptr() + 8 * 300
    # neg_ratio = 0 is get_batch_no_neg
    from gnnflow_amd import utils as U
    s0 = DeviceBatchStream.from_dataframe(df, 256, None, neg_ratio=0, device="cuda:0")
    want0 = list(U.get_batch_no_neg(df, 256))
    assert len(s0) == len(want0)
    for b, w in zip(s0, want0):
        for x, y in zip(_np(b), w):
            assert x.dtype == y.dtype and np.array_equal(x, y)


def test_batch_on_a_side_stream(toy):
    import torch
    from gnnflow_amd import DeviceBatchStream
    df, dst_set, dl = toy
    s = DeviceBatchStream(df.src.values, df.dst.values, df.time.values, df.eid.values, 600, dst_set)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    roots, ts, _ = s.batch(1, stream=side)
    side.synchronize()
    _equal((roots.cpu().numpy(), ts.cpu().numpy()),
           R.assemble(df.src.values, df.dst.values, df.time.values, 600, 1000, 1, dl))


def test_materialize_equals_single_launches(toy):
    import torch
    from gnnflow_amd import DeviceBatchStream
    df, dst_set, dl = toy
    borders = [5, 6, 71, 71, 328, 929]      # 1, 65, 0, 257 and 601 rows
    s = DeviceBatchStream(df.src.values, df.dst.values, df.time.values, df.eid.values, 300,
                          dst_set, neg_ratio=2, seed=11, first_row=1 << 40, borders=borders)
    many = s.materialize()
    torch.cuda.synchronize()
    assert len(many) == 5 and many[2][0].numel() == 0 and many[2][2].numel() == 0
    # views of one buffer, batch b at (2 + K) * (borders[b] - borders[0])
    for b, (roots, ts, _) in enumerate(many):
        assert roots.storage_offset() == 4 * (borders[b] - 5) == ts.storage_offset()
        assert roots.numel() == 4 * (borders[b + 1] - borders[b]) == ts.numel()
    assert many[4][0].data_ptr() == many[0][0].data_ptr() + 8 * 4 * (borders[4] - 5)
    for b in range(5):
        one, got = _np(s.batch(b)), _np(many[b])
        for x, y in zip(one, got):
            assert np.array_equal(x, y)
        _equal(got[:2], R.assemble(df.src.values, df.dst.values, df.time.values, borders[b],
                                   borders[b + 1], 2, dl, seed=11, first_row=1 << 40))
    part = s.materialize(first=3, count=2)
    assert len(part) == 2
    for b in range(2):
        for x, y in zip(_np(part[b]), _np(many[3 + b])):
            assert np.array_equal(x, y)
    assert s.materialize(first=5) == [] and s.materialize(count=0) == []


def test_many_leaves_canaries_and_skips_bad_borders(toy):
    """Raw gf_batch_assemble_many: nothing is written past each buffer, and a batch whose
    borders reach past the stream or whose slices would pass `capacity` writes nothing."""
    import torch
    from gnnflow_amd import _capi
    df, _, dl = toy
    lib = _capi.load()
    src, dst = df.src.values.astype(np.int64), df.dst.values.astype(np.int64)
    time = df.time.values.astype(np.float32)
    d_src, d_dst, d_time, d_dl = _dev(src), _dev(dst), _dev(time), _dev(dl)
    d_count = torch.tensor([len(dl)], dtype=torch.int64, device="cuda")
    K = 1

    def run(borders, rows, capacity):
        n = 3 * (borders[-1] - borders[0]) if capacity is None else capacity
        roots, ts = _buffers(max(n, 0), 0)
        d_b = _dev(np.asarray(borders, dtype=np.int64))
        _capi.check(lib.gf_batch_assemble_many(
            d_src.data_ptr(), d_dst.data_ptr(), d_time.data_ptr(), rows, d_b.data_ptr(),
            len(borders) - 1, 8, K, d_dl.data_ptr(), d_count.data_ptr(), 5, 0, 0,
            roots.data_ptr(), ts.data_ptr(), n, 0, _capi.current_stream(torch.device("cuda", 0))))
        torch.cuda.synchronize()
        return _check_canaries(roots, ts, 0, n)

    borders = [3, 10, 10, 300]       # max_batch_rows = 8 undersizes the grid: still written in full
    roots, ts = run(borders, 1000, None)
    for b in range(3):
        lo, hi = borders[b], borders[b + 1]
        at = 3 * (lo - 3)
        want = R.assemble(src, dst, time, lo, hi, K, dl, seed=5)
        _equal((roots[at:at + 3 * (hi - lo)], ts[at:at + 3 * (hi - lo)]), want)
    # the stream is said to end at row 200: batch 2 (10..300) writes nothing, batch 0 does
    roots, _ = run(borders, 200, None)
    assert np.array_equal(roots[:21], R.assemble(src, dst, time, 3, 10, K, dl, seed=5)[0])
    assert np.all(roots[21:] == CANARY_I)
    # capacity for the first batch only
    roots, _ = run(borders, 1000, 21)
    assert np.array_equal(roots, R.assemble(src, dst, time, 3, 10, K, dl, seed=5)[0])


def test_sampler_takes_device_batches(toy):
    """A DeviceBatchStream batch fed to TemporalSampler.sample gives the blocks the same arrays
    give as numpy."""
    import gnnflow_amd
    from gnnflow_amd import DeviceBatchStream
    df, dst_set, _ = toy
    g = gnnflow_amd.DynamicGraph(1 << 20, 1 << 28, "cuda", 8, 128, "insert")
    g.add_edges(df.src.values.astype(np.int64), df.dst.values.astype(np.int64),
                df.time.values.astype(np.float32), df.eid.values.astype(np.int64),
                add_reverse=True)
    sampler = gnnflow_amd.TemporalSampler(g, [5, 5])
    s = DeviceBatchStream(df.src.values, df.dst.values, df.time.values, df.eid.values, 400,
                          dst_set, seed=2)
    roots, ts, _ = s.batch(1)
    assert roots.is_cuda and ts.is_cuda
    got = sampler.sample(roots, ts)
    want = sampler.sample(roots.cpu().numpy(), ts.cpu().numpy())
    for gl, wl in zip(got, want):
        for gb, wb in zip(gl, wl):
            assert gb.num_edges() == wb.num_edges() and gb.num_edges() > 0
            for key in ("ID", "ts"):
                assert np.array_equal(gb.srcdata[key].cpu().numpy(), wb.srcdata[key].cpu().numpy())
            for key in ("ID", "dt"):
                assert np.array_equal(gb.edata[key].cpu().numpy(), wb.edata[key].cpu().numpy())
            assert np.array_equal(gb.edges()[1].cpu().numpy(), wb.edges()[1].cpu().numpy())


def test_from_dataframe_equals_get_batch(monkeypatch):
    """1 000 rows whose index starts off a multiple of the batch size, with a random start: src,
    dst, ts and eid of every batch equal utils.get_batch's; the negatives equal the reference's."""
    import torch
    from gnnflow_amd import DeviceBatchStream, DeviceDstSet
    from gnnflow_amd import utils as U
    monkeypatch.setenv("LOCAL_RANK", "0")
    rng = np.random.RandomState(4)
    E = 1000
    df = pd.DataFrame({"src": rng.randint(0, 300, E), "dst": rng.randint(300, 500, E),
                       "time": np.sort(rng.rand(E) * 100), "eid": np.arange(E) + 130},
                      index=np.arange(130, 130 + E))
    dl = np.unique(df.dst.values)
    dst_set = DeviceDstSet(500, "cuda:0", df.dst.values)
    host_neg = U.DstRandEdgeSampler(df.dst.values, seed=0)
    starts = set()
    for seed in range(4):
        torch.manual_seed(seed)
        want = list(U.get_batch(df, 100, 4, host_neg))
        torch.manual_seed(seed)
        s = DeviceBatchStream.from_dataframe(df, 100, dst_set, num_chunks=4, seed=seed,
                                             first_row=10 ** 6)
        starts.add(int(s.borders[0]))
        assert len(s) == len(want)
        for i, (roots, ts, eids) in enumerate(s):
            roots, ts, eids = roots.cpu().numpy(), ts.cpu().numpy(), eids.cpu().numpy()
            w_roots, w_ts, w_eid = want[i]
            B = len(w_eid)
            lo = int(s.borders[i])
            assert int(s.borders[i + 1]) - lo == B
            assert np.array_equal(roots[:2 * B], w_roots[:2 * B])
            assert ts.dtype == w_ts.dtype and np.array_equal(ts, w_ts)
            assert np.array_equal(eids, w_eid)
            assert np.array_equal(roots[2 * B:], R.negatives(dl, 10 ** 6, lo, B, 1, seed, 0))
    assert starts <= {0, 25, 50, 75}
