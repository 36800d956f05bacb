"""Numpy restatement of DynamicGraph.pair_history (csrc/pair_history.hip, include/gnnflow_hip.h,
gf_graph_pair_history) and of gnnflow_amd.EdgeBank's scores on top of it.

A history is (dst int64 [m], ts float32 [m], eid int64 [m]), OLDEST FIRST, the live edges of a node
in the store's order; `from_graph` reads them with get_temporal_neighbors (which returns newest
first) for every node a query names.  For row i with s = src[i], d = dst[i], t = ts[i] and, when
`since` is given, lo = since[i], over h = histories[s]:

    considered  = the window of h at (t, lo, max_history), tests/history_window_ref.py
    count[i]    = #{p considered : h.dst[p] == d}
    last_ts[i]  = h.ts[p*],  last_eid[i] = h.eid[p*]    p* the largest such p;  -inf, -1 for none

A source without a history (negative, unknown, no live edges) gives (0, -inf, -1).  Pure numpy.
"""
import numpy as np

from tests.history_window_ref import count_before, from_graph, window  # noqa: F401  (re-exported)


def pair_history(histories, src, dst, ts, since=None, max_history=0):
    """(count int64 [N], last_ts float32 [N], last_eid int64 [N]).  histories: {node: (dst, ts,
    eid)}, oldest first.  since: None, a scalar, or an array [N]."""
    src, dst = np.asarray(src, np.int64), np.asarray(dst, np.int64)
    ts = np.asarray(ts, np.float32)
    N = len(src)
    assert len(dst) == N and len(ts) == N and max_history >= 0
    if since is not None:
        since = np.broadcast_to(np.asarray(since, np.float32), (N,))
    count = np.zeros(N, np.int64)
    last_ts = np.full(N, -np.inf, np.float32)
    last_eid = np.full(N, -1, np.int64)
    for i in range(N):
        h = histories.get(int(src[i]))
        if h is None or len(h[0]) == 0:
            continue
        h_dst, h_ts, h_eid = h
        a, c = window(h_ts, ts[i], None if since is None else since[i], max_history)
        hits = np.flatnonzero(np.asarray(h_dst[a:c], np.int64) == dst[i]) + a
        count[i] = len(hits)
        if len(hits):
            last_ts[i] = np.float32(h_ts[hits[-1]])
            last_eid[i] = int(h_eid[hits[-1]])
    return count, last_ts, last_eid


def edge_bank_scores(histories, src, dst, ts, mode="unlimited", window=None, min_count=1,
                     max_history=0, score="seen"):
    """float32 [N]: EdgeBank.score_pairs.  time_window: since = ts - window, in float32."""
    ts = np.asarray(ts, np.float32)
    since = None
    if mode == "time_window":
        since = ts - np.float32(window)
    else:
        assert mode == "unlimited"
    count = pair_history(histories, src, dst, ts, since, max_history)[0]
    if score == "seen":
        return (count >= min_count).astype(np.float32)
    assert score == "count"
    return count.astype(np.float32)
