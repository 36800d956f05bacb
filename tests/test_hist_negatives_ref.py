"""CPU tests of tests/hist_negatives_ref.py, the numpy restatement the GPU tests of
csrc/hist_negatives.hip compare against: the published constants, the separation of the
historical draws from the random ones, strict time comparison, the three ways a slot is kept,
and the words of first_row and epoch that enter a draw."""
import os
import re

import numpy as np

from tests import batch_stream_ref as B
from tests import hist_negatives_ref as H
from tests.attention_dropout_ref import philox_first

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 0x5EEDC0FFEE123457


def test_constants_are_the_headers():
    text = open(os.path.join(ROOT, "include", "gnnflow_hip.h")).read()
    tag = re.search(r"#define\s+GF_HIST_NEG_SEED_TAG\s+(0x[0-9A-Fa-f]+)ULL", text)
    attempts = re.search(r"#define\s+GF_HIST_NEG_ATTEMPTS\s+(\d+)", text)
    assert tag and int(tag.group(1), 16) == H.SEED_TAG
    assert attempts and int(attempts.group(1)) == H.ATTEMPTS == 4
    assert H.SEED_TAG >> 32 and H.SEED_TAG & 0xFFFFFFFF      # both key words of Philox change


def test_attempt_seed_wraps_and_differs():
    seeds = {H.attempt_seed(SEED, a) for a in range(H.ATTEMPTS)}
    assert len(seeds) == H.ATTEMPTS and SEED not in seeds
    assert H.attempt_seed(0, 0) == H.SEED_TAG and H.attempt_seed(0, 3) == H.SEED_TAG + 3
    assert H.attempt_seed((1 << 64) - 1, 1) == ((1 << 64) - 1) ^ (H.SEED_TAG + 1)


def test_historical_draws_are_not_the_random_draws():
    """Same seed, same tid, same epoch: the 32-bit draw behind a historical negative differs
    from the one behind the random negative, for every attempt (4 000 pairs of 32-bit words:
    a coincidence has probability 1e-6).  With the history equal to the destination list, the
    negatives themselves differ too."""
    K, rows = 3, 1000
    tid = B.tids(77, 5, rows, K)
    random_u = philox_first(SEED, tid, 9)
    for a in range(H.ATTEMPTS):
        assert not np.any(philox_first(H.attempt_seed(SEED, a), tid, 9) == random_u)
    dl = np.arange(500, 900, dtype=np.int64)
    src, dst = np.zeros(rows + 5, np.int64), np.full(rows + 5, -7, np.int64)
    time = np.full(rows + 5, 10.0, np.float32)
    roots, _ = B.assemble(src, dst, time, 5, 5 + rows, K, dl, seed=SEED, epoch=9, first_row=77)
    hist = {0: (dl, np.zeros(len(dl), np.float32))}
    got, classes = H.overwrite(roots, src, dst, time, 5, 5 + rows, K, K, hist, 1, seed=SEED,
                               epoch=9, first_row=77)
    assert np.all(classes == H.HISTORICAL)
    assert np.mean(got[2 * rows:] != roots[2 * rows:]) > 0.98      # equal by chance: 1 in 400
    # Kh = 0 draws exactly what the stream draws today
    same, _ = H.overwrite(roots, src, dst, time, 5, 5 + rows, K, 0, hist, 1, seed=SEED, epoch=9)
    assert np.array_equal(same, roots)


def test_time_comparison_is_strict():
    ts = np.array([1.0, 2.0, 2.0, 2.0, 3.0], np.float32)
    assert H.history_size(ts, 2.0) == 1            # the three ties are not history
    assert H.history_size(ts, np.nextafter(np.float32(2.0), np.float32(3.0))) == 4
    assert H.history_size(ts, 1.0) == 0 and H.history_size(ts, 3.5) == 5
    assert H.history_size(ts, np.float32("nan")) == 0
    assert H.history_size([], 1.0) == 0
    # a value that float64 tells apart from 2 but float32 does not is a tie
    assert H.history_size(ts, 2.0 + 1e-9) == 1


def _one_row(hist_dst, hist_ts, d, t, K=3, Kh=2, s=4, table_len=8):
    src, dst = np.array([s], np.int64), np.array([d], np.int64)
    time = np.array([t], np.float32)
    roots, _ = B.assemble(src, dst, time, 0, 1, K, [900, 901, 902], seed=SEED)
    hist = {4: (np.asarray(hist_dst, np.int64), np.asarray(hist_ts, np.float32))}
    got, classes = H.overwrite(roots, src, dst, time, 0, 1, K, Kh, hist, table_len, seed=SEED)
    return roots, got, classes


def test_tie_only_history_keeps_the_slot():
    roots, got, classes = _one_row([10, 11], [5.0, 5.0], 12, 5.0)
    assert np.array_equal(got, roots) and np.all(classes == H.NO_HISTORY)
    roots, got, classes = _one_row([10, 11], [5.0, 5.0], 12, 5.5)
    assert np.all(classes == H.HISTORICAL) and set(got[2:4]) <= {10, 11}
    assert got[4] == roots[4] and np.array_equal(got[:2], roots[:2])      # plane k >= Kh stays


def test_only_edges_before_t_are_drawn():
    # 11 is in the history but not before t: with c == 1 every draw is index 0
    _, got, classes = _one_row([10, 11], [1.0, 9.0], 12, 5.0, Kh=3)
    assert got[2:].tolist() == [10, 10, 10] and np.all(classes == H.HISTORICAL)


def test_unknown_sources_keep_the_slot():
    for s, table_len in ((-1, 8), (8, 8), (1 << 40, 8), (4, 0)):
        roots, got, classes = _one_row([10], [1.0], 12, 5.0, s=s, table_len=table_len)
        assert np.array_equal(got, roots) and np.all(classes == H.UNKNOWN_SOURCE)
    # inside the table but without an edge: no history
    roots, got, classes = _one_row([10], [1.0], 12, 5.0, s=5)
    assert np.array_equal(got, roots) and np.all(classes == H.NO_HISTORY)


def test_history_of_the_positive_alone_is_rejected_four_times():
    roots, got, classes = _one_row([12, 12, 12], [1.0, 2.0, 3.0], 12, 5.0)
    assert np.array_equal(got, roots) and np.all(classes == H.ALL_REJECTED)
    assert H.filled(classes) == 0


def test_first_attempt_that_differs_wins():
    """History [d, x]: attempt a is taken when attempts 0 .. a - 1 drew index 0.  Over 400 slots
    every attempt number occurs, and so does rejection of all four."""
    rows, K = 400, 1
    src, dst = np.full(rows, 2, np.int64), np.full(rows, 50, np.int64)
    time = np.full(rows, 3.0, np.float32)
    roots, _ = B.assemble(src, dst, time, 0, rows, K, [900], seed=1)
    hist = {2: (np.array([50, 60]), np.array([1.0, 2.0], np.float32))}
    got, classes = H.overwrite(roots, src, dst, time, 0, rows, K, K, hist, 3, seed=1)
    j = H.draws(np.full(rows, 2), 0, 0, rows, K, K, 1, 0)[:, 0, :]      # [4, rows] of 0 / 1
    first = np.where(j.any(axis=0), j.argmax(axis=0), -1)
    assert set(first.tolist()) == {-1, 0, 1, 2, 3}
    assert np.array_equal(classes[0] == H.ALL_REJECTED, first < 0)
    assert np.all(got[2 * rows:][first >= 0] == 60) and np.all(got[2 * rows:][first < 0] == 900)
    assert H.filled(classes) == int(np.count_nonzero(first >= 0))


def test_high_words_of_first_row_and_epoch_enter_the_draw():
    rows, K = 64, 2
    src, dst = np.zeros(rows, np.int64), np.full(rows, -1, np.int64)
    time = np.full(rows, 1.0, np.float32)
    c = np.full(rows, 1000)

    def j(first_row, epoch):
        return H.draws(c, first_row, 0, rows, K, K, SEED, epoch)

    base = j(3, 1)
    assert not np.array_equal(j(3 + (1 << 33), 1), base)       # tid's high word (K = 2: bit 34)
    assert not np.array_equal(j(3, 1 + (1 << 32)), base)       # epoch's high word
    assert not np.array_equal(j(3, 2), base) and np.array_equal(j(3, 1), base)
    # the key is the global row: rows 10.. of a slice that says first_row = 13 draw the same
    assert np.array_equal(H.draws(c[10:], 13, 0, rows - 10, K, K, SEED, 1), base[:, :, 10:])
    # tid wraps like the kernel's uint64
    wrapped = H.draws(c, (1 << 63) - 5, 0, rows, K, K, SEED, 1)
    tid = B.tids((1 << 63) - 5, 0, rows, K)
    u = philox_first(H.attempt_seed(SEED, 2), tid, 1).astype(np.uint64)
    assert np.array_equal(wrapped[2], ((u * np.uint64(1000)) >> np.uint64(32)).astype(np.int64))
