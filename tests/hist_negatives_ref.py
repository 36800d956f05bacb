"""Numpy restatement of csrc/hist_negatives.hip (include/gnnflow_hip.h,
gf_batch_hist_negatives): the historical negatives written over the first Kh negative planes of
a batch that `batch_stream_ref.assemble` has laid out.  Integers only: the kernel must match bit
for bit.

    slot (i, k), k < Kh:  s, d, t = src, dst, time of row lo + i;  g = first_row + lo + i
    history of s, oldest first: destinations h_dst[0:n], timestamps h_ts[0:n]
    c    = #{x in h_ts : x < t}          float32 <, strict: a tie is not history, NaN t gives 0
    u_a  = philox_first(seed ^ (SEED_TAG + a), tid, epoch)    a < 4,  tid = g * K + k  mod 2^64
    cand = h_dst[(u_a * c) >> 32]
    roots[2B + k*B + i] = the first cand != d

A slot is KEPT (holds what it held) when s is outside [0, table_len), when c == 0, or when all
four attempts drew d.
"""
import numpy as np

from tests.attention_dropout_ref import philox_first
from tests.batch_stream_ref import MASK64, tids
from tests.history_window_ref import count_before

SEED_TAG = 0x484953544E454730      # GF_HIST_NEG_SEED_TAG, "HISTNEG0"
ATTEMPTS = 4                       # GF_HIST_NEG_ATTEMPTS

# what became of a slot
HISTORICAL, UNKNOWN_SOURCE, NO_HISTORY, ALL_REJECTED = 0, 1, 2, 3


def attempt_seed(seed, a):
    return (int(seed) ^ ((SEED_TAG + a) & MASK64)) & MASK64


def history_size(h_ts, t):
    """c: elements of the node's timestamps strictly below t, compared as float32."""
    return count_before(h_ts, t)


def draws(c, first_row, lo, B, K, Kh, seed, epoch):
    """int64 [ATTEMPTS, Kh, B]: the index (u * c[i]) >> 32 every attempt of every slot draws
    (0 where c[i] == 0: no draw is defined there)."""
    t = tids(first_row, lo, B, K)[:Kh]
    c = np.asarray(c, dtype=np.uint64)
    out = np.empty((ATTEMPTS, Kh, B), dtype=np.int64)
    for a in range(ATTEMPTS):
        u = philox_first(attempt_seed(seed, a), t, epoch).astype(np.uint64)
        out[a] = ((u * c[None, :]) >> np.uint64(32)).astype(np.int64)      # u c < 2^64
    return out


def overwrite(roots, src, dst, time, lo, hi, K, Kh, histories, table_len, seed=0, epoch=0,
              first_row=0):
    """(roots with the historical negatives written, classes int8 [Kh, B]) of the batch
    [lo, hi).  `roots` is the assembled batch, int64 [(2 + K) * B], and is not modified.
    `histories` maps a node id to (destinations, timestamps) of its live edges, oldest first; a
    node below table_len that is not in it has no edge."""
    assert 0 <= Kh <= K
    src, dst = np.asarray(src, dtype=np.int64), np.asarray(dst, dtype=np.int64)
    time = np.asarray(time, dtype=np.float32)
    B = hi - lo
    out = np.array(roots, dtype=np.int64, copy=True)
    assert out.shape == ((2 + K) * B,)
    classes = np.zeros((Kh, B), dtype=np.int8)
    if Kh == 0 or B == 0:
        return out, classes
    c = np.zeros(B, dtype=np.uint64)
    known = np.zeros(B, dtype=bool)
    for i in range(B):
        s = int(src[lo + i])
        known[i] = 0 <= s < table_len
        if known[i] and s in histories:
            c[i] = history_size(histories[s][1], time[lo + i])
    j = draws(c, first_row, lo, B, K, Kh, seed, epoch)
    for i in range(B):
        if not known[i] or c[i] == 0:
            classes[:, i] = UNKNOWN_SOURCE if not known[i] else NO_HISTORY
            continue
        h_dst = np.asarray(histories[int(src[lo + i])][0], dtype=np.int64)
        d = dst[lo + i]
        for k in range(Kh):
            classes[k, i] = ALL_REJECTED
            for a in range(ATTEMPTS):
                cand = h_dst[j[a, k, i]]
                if cand != d:
                    out[2 * B + k * B + i] = cand
                    classes[k, i] = HISTORICAL
                    break
    return out, classes


def filled(classes):
    return int(np.count_nonzero(classes == HISTORICAL))
