"""CPU tests of tests/batch_stream_ref.py, the numpy restatement the GPU tests of
csrc/batch_stream.hip compare against: hand-computed values, the keying property, the layout,
the borders of DeviceBatchStream.from_dataframe's rule against utils.get_batch, and the
uniformity of the multiply-shift draw."""
import numpy as np
import pandas as pd
import torch

from gnnflow_amd import utils as U
from tests import batch_stream_ref as R
from tests.attention_dropout_ref import philox_first


def test_hand_computed_batch():
    """B = 2, K = 2, M = 3.  seed 1, epoch 3, first_row 10, lo 1: rows 11 and 12 of the stream,
    tid = row * 2 + k = 22, 23 (row 11), 24, 25 (row 12).  The four draws below were computed
    with include/gnnflow_rng.h compiled as C; index = (u * 3) >> 32:
        1571206142 * 3 =  4713618426 -> 1      3596903265 * 3 = 10790709795 -> 2
        1095638226 * 3 =  3286914678 -> 0      4080721168 * 3 = 12242163504 -> 2"""
    u = philox_first(1, np.array([22, 23, 24, 25], dtype=np.uint64), 3)
    assert u.tolist() == [1571206142, 3596903265, 1095638226, 4080721168]
    src = [100, 101, 102, 103]
    dst = [200, 201, 202, 203]
    time = [0.5, 1.5, 2.5, 3.5]
    roots, ts = R.assemble(src, dst, time, 1, 3, 2, [5, 8, 13], seed=1, epoch=3, first_row=10)
    #                  src       dst       k = 0: tid 22, 24   k = 1: tid 23, 25
    assert roots.tolist() == [101, 102, 201, 202, 8, 5, 13, 13]
    assert roots.dtype == np.int64 and ts.dtype == np.float32
    assert ts.tolist() == [1.5, 2.5] * 4


def test_tid_wraps_like_uint64():
    t = R.tids((1 << 63) - 5, 0, 8, 3)
    want = [[(((1 << 63) - 5 + i) * 3 + k) % (1 << 64) for i in range(8)] for k in range(3)]
    assert t.tolist() == want
    assert ((1 << 63) - 5) * 3 > (1 << 64)      # the product does wrap: 3 * 2^63 - 15 -> 2^63 - 15
    assert want[0][0] == (1 << 63) - 15


def test_same_negatives_whatever_the_batch_size():
    rng = np.random.RandomState(0)
    E, K = 50, 3
    src, dst = rng.randint(0, 40, E), rng.randint(40, 90, E)
    time = np.arange(E, dtype=np.float32)
    dl = np.unique(dst)

    def per_edge(batch):
        neg = np.empty((E, K), np.int64)
        for lo in range(0, E, batch):
            hi = min(lo + batch, E)
            roots, _ = R.assemble(src, dst, time, lo, hi, K, dl, seed=9, epoch=2, first_row=1000)
            neg[lo:hi] = roots[2 * (hi - lo):].reshape(K, hi - lo).T
        return neg

    a, b = per_edge(7), per_edge(50)
    assert np.array_equal(a, b)
    assert len(np.unique(a)) > 1
    # another epoch, another first_row: other draws
    roots, _ = R.assemble(src, dst, time, 0, E, K, dl, seed=9, epoch=3, first_row=1000)
    assert not np.array_equal(roots[2 * E:].reshape(K, E).T, b)
    # a rank that owns rows 20.. and says so draws what the one process drew for them
    roots, _ = R.assemble(src[20:], dst[20:], time[20:], 0, 30, K, dl, seed=9, epoch=2,
                          first_row=1020)
    assert np.array_equal(roots[60:].reshape(K, 30).T, b[20:])


def test_layout_is_k_major():
    B, K = 5, 4
    dl = np.arange(1000, 1100)
    roots, ts = R.assemble(np.arange(B), np.arange(B) + 10, np.arange(B) * 0.25, 0, B, K, dl,
                           seed=4)
    assert roots[:B].tolist() == list(range(B)) and roots[B:2 * B].tolist() == list(range(10, 15))
    neg = roots[2 * B:]
    for k in range(K):
        for i in range(B):
            u = int(philox_first(4, i * K + k, 0))
            assert neg[k * B + i] == dl[(u * len(dl)) >> 32]      # positive i's k-th: stride B
    assert np.array_equal(ts.reshape(2 + K, B), np.tile(np.arange(B, dtype=np.float32) * 0.25,
                                                        (2 + K, 1)))


def test_no_negatives_is_get_batch_no_neg():
    roots, ts = R.assemble([1, 2, 3], [4, 5, 6], [7, 8, 9], 0, 3, 0, [])
    assert roots.tolist() == [1, 2, 3, 4, 5, 6] and ts.tolist() == [7, 8, 9, 7, 8, 9]


def _frame(first_index, rows):
    rng = np.random.RandomState(first_index)
    return pd.DataFrame({"src": rng.randint(0, 50, rows), "dst": rng.randint(50, 99, rows),
                         "time": np.arange(rows, dtype=np.float64),
                         "eid": np.arange(first_index, first_index + rows)},
                        index=np.arange(first_index, first_index + rows))


def _borders(df, batch_size, skip):
    """The rule DeviceBatchStream.from_dataframe applies."""
    borders = [int(pos[0]) for pos in U._row_groups(df, batch_size, skip)]
    return borders + [len(df)]


def test_borders_match_get_batch_off_a_multiple():
    df = _frame(130, 1000)               # index 130..1129, batches of 100: 70, 100 x 9, 30
    borders = _borders(df, 100, 0)
    assert np.diff(borders).tolist() == [70] + [100] * 9 + [30]
    neg = U.DstRandEdgeSampler(df["dst"].values, seed=0)
    got = list(U.get_batch(df, 100, 0, neg))
    assert len(got) == len(borders) - 1
    for (roots, ts, eid), lo, hi in zip(got, borders[:-1], borders[1:]):
        want_roots, want_ts = R.assemble(df["src"].values, df["dst"].values, df["time"].values,
                                         lo, hi, 0, [])
        assert np.array_equal(roots[:2 * (hi - lo)], want_roots)
        assert np.array_equal(ts[:2 * (hi - lo)], want_ts)
        assert np.array_equal(eid, df["eid"].values[lo:hi])


def test_borders_match_get_batch_random_start(monkeypatch):
    monkeypatch.setenv("LOCAL_RANK", "0")
    df = _frame(0, 1000)
    neg = U.DstRandEdgeSampler(df["dst"].values, seed=0)
    seen = set()
    for seed in range(6):
        torch.manual_seed(seed)
        got = list(U.get_batch(df, 100, 4, neg))
        torch.manual_seed(seed)
        skip = U._random_start(4, 100, 1)
        seen.add(skip)
        borders = _borders(df, 100, skip)
        assert borders[0] == skip and len(got) == len(borders) - 1
        for (roots, _, eid), lo, hi in zip(got, borders[:-1], borders[1:]):
            assert np.array_equal(roots[:hi - lo], df["src"].values[lo:hi])
            assert np.array_equal(eid, df["eid"].values[lo:hi])
    assert len(seen) > 1 and seen <= {0, 25, 50, 75}


def test_draws_are_uniform():
    """M = 7, 70 000 draws: every count within 5 sigma of 10 000,
    sigma = sqrt(70000 * (1/7) * (6/7)) = 92.6."""
    n, M = 70000, 7
    draws = R.sample(np.arange(M), n, seed=12345)
    counts = np.bincount(draws, minlength=M)
    sigma = np.sqrt(n * (1 / 7) * (6 / 7))
    assert counts.sum() == n
    assert np.all(np.abs(counts - n / M) <= 5 * sigma), counts


def test_union_is_np_unique():
    ids, bad = R.union(10, [3, 9, 3, 0], [], [10, -1, 4])
    assert ids.tolist() == [0, 3, 4, 9] and bad == 2
