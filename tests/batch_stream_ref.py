"""Numpy restatement of csrc/batch_stream.hip: the batch `gf_batch_assemble` writes and the
destination set `gf_dst_set_mark` / `gf_dst_set_compact` keep.  Integers and copied floats only:
the kernels must match bit for bit.

    roots[0:B]          = src[lo:hi]
    roots[B:2B]         = dst[lo:hi]
    roots[2B + k*B + i] = dl[(uint64(u) * M) >> 32]     u = philox_first(seed, tid, epoch)
    ts[j*B + i]         = time[lo + i],  j < 2 + K      tid = (first_row + lo + i) * K + k  mod 2^64
"""
import numpy as np

from tests.attention_dropout_ref import philox_first

MASK64 = (1 << 64) - 1


def tids(first_row, lo, B, K):
    """uint64 [K, B]: the Philox counter of negative k of row lo + i, wrapping like the kernel."""
    first_row, lo, B, K = int(first_row), int(lo), int(B), int(K)      # numpy integers would wrap
    out = np.empty((K, B), dtype=np.uint64)
    for k in range(K):
        for i in range(B):
            out[k, i] = ((first_row + lo + i) * K + k) & MASK64      # Python integers: exact
    return out


def negatives(dl, first_row, lo, B, K, seed, epoch):
    """int64 [K * B], k-major."""
    dl = np.asarray(dl, dtype=np.int64)
    M = len(dl)
    assert 0 < M < (1 << 32)
    if K == 0 or B == 0:
        return np.empty(0, np.int64)
    u = philox_first(seed, tids(first_row, lo, B, K), epoch).astype(np.uint64)
    return dl[((u * np.uint64(M)) >> np.uint64(32)).astype(np.int64)].reshape(-1)      # u M < 2^64


def assemble(src, dst, time, lo, hi, K, dl, seed=0, epoch=0, first_row=0):
    """(roots int64 [(2 + K) B], ts float32 [(2 + K) B]) of the batch [lo, hi)."""
    src, dst = np.asarray(src, dtype=np.int64), np.asarray(dst, dtype=np.int64)
    t = np.asarray(time, dtype=np.float32)[lo:hi]
    B = hi - lo
    neg = negatives(dl, first_row, lo, B, K, seed, epoch) if K else np.empty(0, np.int64)
    return np.concatenate([src[lo:hi], dst[lo:hi], neg]), np.concatenate([t] * (2 + K))


def sample(dl, size, seed, first=0, call=0):
    """DeviceDstSet.sample: K = 1 and tid = first + i."""
    return negatives(dl, first, 0, size, 1, seed, call)


def union(num_nodes, *adds):
    """(ascending ids inside [0, num_nodes), number of ids outside) after adding every array."""
    every = np.concatenate([np.asarray(a, dtype=np.int64).reshape(-1) for a in adds] +
                           [np.empty(0, np.int64)])
    inside = (every >= 0) & (every < num_nodes)
    return np.unique(every[inside]), int((~inside).sum())


def default_borders(rows, batch_size):
    return np.append(np.arange(0, rows, batch_size, dtype=np.int64), rows)
