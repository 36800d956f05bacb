"""Numpy restatement of DynamicGraph.seen_mask (csrc/seen_mask.hip, include/gnnflow_hip.h,
gf_graph_seen_mask): from per-node chronological histories to the [B, W] mask words.

    considered(i) = the entries (dst, t') of history[src[i]] with t' < ts[i]   (float32 <: a NaN
                    ts[i] gives none), and with max_history > 0 only the newest max_history of them
    bit c % 64 of word [i, c // 64] is set  iff  cand_ids[c] == dst for a considered entry

A history is (dst int64 [n], ts float32 [n]), OLDEST FIRST, the live edges of the node in the
store's order; `from_graph` reads them with get_temporal_neighbors (which returns newest first)
for every node a query names.  A source without a history (negative, unknown, no live edges) gives
a zero row; bits at positions >= C are 0.  Words are returned as int64, the type torch holds them
in (bit 63 is the sign).  Pure numpy.
"""
import numpy as np

from tests import history_window_ref


def num_words(C):
    return (C + 63) // 64


def considered(history, t, max_history=0):
    """The dst of the considered entries of one history (oldest first) for a query at time t."""
    dst, ts = history
    a, c = history_window_ref.window(ts, t, None, max_history)
    return np.asarray(dst, np.int64)[a:c]


def seen_mask(histories, src, ts, cand_ids, max_history=0):
    """int64 [B, W].  histories: {node: (dst, ts)}, oldest first."""
    src, ts = np.asarray(src, np.int64), np.asarray(ts, np.float32)
    cand_ids = np.asarray(cand_ids, np.int64)
    B, C = len(src), len(cand_ids)
    assert C >= 1 and len(ts) == B and max_history >= 0
    bits = np.zeros((B, num_words(C) * 64), bool)
    for i in range(B):
        h = histories.get(int(src[i]))
        if h is None or len(h[0]) == 0:
            continue
        bits[i, :C] = np.isin(cand_ids, considered(h, ts[i], max_history))
    return pack(bits)


def pack(bits):
    """bool [B, 64 W] -> int64 [B, W], bit b of word w = bits[:, 64 w + b]."""
    B = bits.shape[0]
    weights = np.uint64(1) << np.arange(64, dtype=np.uint64)
    words = (bits.reshape(B, -1, 64).astype(np.uint64) * weights).sum(-1, dtype=np.uint64)
    return words.view(np.int64).reshape(B, -1)


def unpack(words, C):
    """int64 [B, W] -> bool [B, C]."""
    w = np.asarray(words, np.int64).view(np.uint64)
    ids = np.arange(C)
    return ((w[:, ids >> 6] >> (ids & 63).astype(np.uint64)) & np.uint64(1)).astype(bool)


def from_graph(graph, nodes):
    """{node: (dst, ts)} oldest first, for every distinct valid node of `nodes`."""
    return {v: h[:2] for v, h in history_window_ref.from_graph(graph, nodes).items()}
