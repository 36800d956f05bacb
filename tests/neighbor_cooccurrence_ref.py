"""Numpy restatement of DynamicGraph.neighbor_cooccurrence (csrc/neighbor_cooccurrence.hip,
include/gnnflow_hip.h: gf_graph_neighbor_cooccurrence).

Histories as in tests/pair_history_ref.py: {node: (dst int64 [m], ts float32 [m], eid int64 [m])},
OLDEST FIRST.  For row i with s = src[i], d = dst[i], t = ts[i] and, when `since` is given,
lo = since[i], with L = length and self = 1 if include_self else 0, the window of a node v over
h = histories[v] is common_neighbors' at the bound H = L - self (1 .. MAX_LENGTH - self),
tests/history_window_ref.py's c and n:

    records c - n .. c - 1 of h, oldest first

and empty for a node without a history.  seq(v) = [v itself if self] + the records' dst.  For
z >= 0, a(z) and b(z) are how often z occurs in seq(s) and in seq(d); a negative id is not counted
and its own counts are 0, 0.

    lengths[i]          = len(seq(s)), len(seq(d))
    nodes[i, side]      = seq(v), then -1                      side 0: v = s, side 1: v = d
    eids[i, side]       = the records' eid; -1 for the self slot and the padding
    times[i, side]      = the records' ts; t for the self slot; 0 in the padding
    counts[i, side, p]  = a(z), b(z) of z = nodes[i, side, p]; 0, 0 in the padding

Pure numpy, dictionaries and loops: nothing here is shaped like the kernel's table.
"""
import numpy as np

from tests.history_window_ref import count_before, from_graph, window  # noqa: F401  (re-exported)

MAX_LENGTH = 512                   # GF_COOC_MAX_LENGTH


def sequence(histories, v, t, lo, length, include_self):
    """(nodes, eids, times) of seq(v) as three lists, the self slot first, then oldest first."""
    nodes, eids, times = [], [], []
    if include_self:
        nodes.append(int(v)), eids.append(-1), times.append(np.float32(t))
    H = length - (1 if include_self else 0)
    assert H >= 1
    h = histories.get(int(v))
    if h is not None and len(h[0]):
        for p in range(*window(h[1], t, lo, H)):
            nodes.append(int(h[0][p])), eids.append(int(h[2][p])), times.append(np.float32(h[1][p]))
    return nodes, eids, times


def neighbor_cooccurrence(histories, src, dst, ts, since=None, length=32, include_self=True):
    """(lengths int32 [N, 2]; nodes, eids int64 [N, 2, L]; times float32 [N, 2, L]; counts int32
    [N, 2, L, 2]).  since: None, a scalar, or an array [N]."""
    src, dst = np.asarray(src, np.int64), np.asarray(dst, np.int64)
    ts = np.asarray(ts, np.float32)
    N, L = len(src), length
    assert len(dst) == N and len(ts) == N and isinstance(include_self, bool)
    assert 1 + include_self <= L <= MAX_LENGTH
    if since is not None:
        since = np.broadcast_to(np.asarray(since, np.float32), (N,))
    lengths = np.zeros((N, 2), np.int32)
    nodes = np.full((N, 2, L), -1, np.int64)
    eids = np.full((N, 2, L), -1, np.int64)
    times = np.zeros((N, 2, L), np.float32)
    counts = np.zeros((N, 2, L, 2), np.int32)
    for i in range(N):
        lo = since[i] if since is not None else None
        sides = [sequence(histories, v, ts[i], lo, L, include_self) for v in (src[i], dst[i])]
        occurs = [{}, {}]
        for side in (0, 1):
            for z in sides[side][0]:
                if z >= 0:
                    occurs[side][z] = occurs[side].get(z, 0) + 1
        for side in (0, 1):
            seq_nodes, seq_eids, seq_times = sides[side]
            lengths[i, side] = len(seq_nodes)
            for p, z in enumerate(seq_nodes):
                nodes[i, side, p], eids[i, side, p] = z, seq_eids[p]
                times[i, side, p] = seq_times[p]
                counts[i, side, p, 0] = occurs[0].get(z, 0)
                counts[i, side, p, 1] = occurs[1].get(z, 0)
    return lengths, nodes, eids, times, counts


FIELDS = ("lengths", "nodes", "eids", "times", "counts")


def same(got, want, rows=None):
    """Assert five outputs equal, floats by their bits (the times are copies, NaN included)."""
    for name, g, w in zip(FIELDS, got, want):
        if rows is not None:
            w = w[rows]
        assert g.dtype == w.dtype and g.shape == w.shape, (name, g.dtype, w.dtype, g.shape, w.shape)
        if g.dtype == np.float32:
            g, w = g.view(np.uint32), w.view(np.uint32)
        bad = np.flatnonzero((g != w).reshape(len(g), -1).any(1)) if g.size else []
        assert len(bad) == 0, "{}: rows {} got {} want {}".format(name, bad[:5], g[bad[:5]],
                                                                  w[bad[:5]])


def has_cooccurrence(nodes, counts):
    """bool [N]: some element of either side is a node >= 0 with both counts > 0."""
    both = (nodes >= 0) & (counts[..., 0] > 0) & (counts[..., 1] > 0)
    return both.reshape(len(nodes), -1).any(1)
