"""Numpy restatement of DynamicGraph.common_neighbors and DynamicGraph.temporal_degree
(csrc/common_neighbors.hip, include/gnnflow_hip.h: gf_graph_common_neighbors,
gf_graph_temporal_degree) and of gnnflow_amd.NeighborOverlap's scores on top of them.

Histories as in tests/pair_history_ref.py: {node: (dst int64 [m], ts float32 [m], eid int64 [m])},
OLDEST FIRST.  For row i with s = src[i], d = dst[i], t = ts[i] and, when `since` is given,
lo = since[i], the window of a node v over h = histories[v] is pair_history's
(tests/history_window_ref.py: c, c0, n) at the bound H = max_history, 1 .. MAX_HISTORY:

    records h.dst[c - n : c], at positions 0 .. n - 1

and empty for a node without a history.  A = window(s), B = window(d).  For z >= 0: a(z), b(z) =
the records of A, of B equal to z, pa(z) = the largest position in A that holds z.

    n_src, n_dst = |A|, |B|;  u_src, u_dst = #{z : a(z) > 0}, #{z : b(z) > 0}
    common       = #{z : a(z) > 0 and b(z) > 0}
    nodes[i]     = those z by descending pa(z), the first min(common, K), then -1
    cnt_src[i, k], cnt_dst[i, k] = a(z), b(z) of z = nodes[i, k]; 0 in the padding

temporal_degree is c - c0 of one node's window.  Pure numpy, dictionaries and loops: nothing here
is shaped like the kernel's table.
"""
import numpy as np

from tests import history_window_ref
from tests.history_window_ref import count_before, from_graph  # noqa: F401  (re-exported)

MAX_HISTORY = 512                  # GF_CN_MAX_HISTORY, also the bound of max_common
SCORES = ("cn", "jaccard", "aa", "ra", "pa")


def _bounds(h, t, lo):
    """(c0, c) of a history at time t and lower end lo (None: no lower end)."""
    if h is None or len(h[0]) == 0:
        return 0, 0
    return history_window_ref.window(h[1], t, lo)      # without a bound c - n is c0


def window(histories, v, t, lo, max_history):
    """The destinations of node v's window, oldest first (int64 [n]).  max_history is a bound
    here, 0 included: 0 records, not "no bound"."""
    h = histories.get(int(v))
    if h is None or len(h[0]) == 0 or max_history == 0:
        return np.zeros(0, np.int64)
    a, c = history_window_ref.window(h[1], t, lo, max_history)
    return np.asarray(h[0][a:c], np.int64)


def common_neighbors(histories, src, dst, ts, since=None, max_history=64, max_common=32):
    """(n_src, n_dst, u_src, u_dst, common int32 [N]; nodes int64 [N, K]; cnt_src, cnt_dst int32
    [N, K]).  since: None, a scalar, or an array [N]."""
    src, dst = np.asarray(src, np.int64), np.asarray(dst, np.int64)
    ts = np.asarray(ts, np.float32)
    N, H, K = len(src), max_history, max_common
    assert len(dst) == N and len(ts) == N and 1 <= H <= MAX_HISTORY and 0 <= K <= MAX_HISTORY
    if since is not None:
        since = np.broadcast_to(np.asarray(since, np.float32), (N,))
    n_src, n_dst, u_src, u_dst, common = (np.zeros(N, np.int32) for _ in range(5))
    nodes = np.full((N, K), -1, np.int64)
    cnt_src, cnt_dst = np.zeros((N, K), np.int32), np.zeros((N, K), np.int32)
    for i in range(N):
        lo = since[i] if since is not None else None
        A = window(histories, src[i], ts[i], lo, H)
        B = window(histories, dst[i], ts[i], lo, H)
        a, b, pa = {}, {}, {}
        for p, z in enumerate(A.tolist()):
            if z >= 0:
                a[z] = a.get(z, 0) + 1
                pa[z] = p                      # p ascends: the last one stays
        for z in B.tolist():
            if z >= 0:
                b[z] = b.get(z, 0) + 1
        both = sorted((z for z in a if z in b), key=lambda z: -pa[z])
        n_src[i], n_dst[i], u_src[i], u_dst[i], common[i] = len(A), len(B), len(a), len(b), \
            len(both)
        for k, z in enumerate(both[:K]):
            nodes[i, k], cnt_src[i, k], cnt_dst[i, k] = z, a[z], b[z]
    return n_src, n_dst, u_src, u_dst, common, nodes, cnt_src, cnt_dst


def temporal_degree(histories, nodes, ts, since=None):
    """int64 of nodes' shape: c - c0 of each node's window; 0 for a node without a history."""
    nodes = np.asarray(nodes, np.int64)
    ts = np.broadcast_to(np.asarray(ts, np.float32), nodes.shape)
    if since is not None:
        since = np.broadcast_to(np.asarray(since, np.float32), nodes.shape)
    out = np.zeros(nodes.shape, np.int64)
    for idx in np.ndindex(*nodes.shape):
        c0, c = _bounds(histories.get(int(nodes[idx])), ts[idx],
                        since[idx] if since is not None else None)
        out[idx] = c - c0
    return out


def overlap_scores(histories, src, dst, ts, score="cn", max_history=64, max_common=64,
                   window=None):
    """float64 [N]: NeighborOverlap's score before its one rounding to float32.  window: since =
    ts - window in float32, as EdgeBank's.  aa and ra sum over the returned nodes only, in their
    order, one term after the other."""
    assert score in SCORES
    ts = np.asarray(ts, np.float32)
    since = ts - np.float32(window) if window is not None else None
    n_src, n_dst, u_src, u_dst, common, nodes, _, _ = common_neighbors(
        histories, src, dst, ts, since, max_history, max_common)
    N = len(ts)
    out = np.zeros(N, np.float64)
    if score == "cn":
        return common.astype(np.float64)
    if score == "pa":
        return n_src.astype(np.float64) * n_dst.astype(np.float64)
    if score == "jaccard":
        union = u_src.astype(np.int64) + u_dst - common
        for i in range(N):
            out[i] = float(common[i]) / float(union[i]) if union[i] > 0 else 0.0
        return out
    deg = temporal_degree(histories, nodes, ts[:, None], None if since is None else since[:, None])
    for i in range(N):
        for k in range(nodes.shape[1]):
            g = int(deg[i, k])
            if score == "aa" and g >= 2:
                out[i] += 1.0 / np.log(np.float64(g))
            elif score == "ra" and g >= 1:
                out[i] += 1.0 / np.float64(g)
    return out
