"""Numpy restatement of DynamicGraph.neighbor_aggregate (csrc/neighbor_aggregate.hip,
include/gnnflow_hip.h, gf_graph_neighbor_aggregate).

A history is (dst int64 [m], ts float32 [m], eid int64 [m]), OLDEST FIRST, the live edges of a node
in the store's order; `from_graph` reads them with get_temporal_neighbors (which returns newest
first) for every node a query names.  For row i with v = nodes[i], t = ts[i] and, when `since` is
given, lo = since[i], over h = histories[v]:

    considered = positions c - n .. c - 1, the window of h at (t, lo, max_history),
                 tests/history_window_ref.py, oldest first
    count[i]   = n
    node[i, :] = (((0 + N[h.dst[c - n]]) + N[h.dst[c - n + 1]]) + ...) + N[h.dst[c - 1]]
    edge[i, :] = the same over E[h.eid[p]]

one float32 addition per considered position, in that order; N[id] and E[id] are the zero row
for an id without a row in the table (negative, >= len(table)), which still counts in n.
reduce="mean" divides the finished sum once by float32(n); zeros where n == 0.  np.sum is pairwise
and is not used: the sum is np.cumsum(..., dtype=float32)[-1], a sequential float32 loop per
column.  A node without a history (negative, unknown, no live edges) gives 0 and zero rows.
Pure numpy.
"""
import numpy as np

from tests.history_window_ref import count_before, from_graph, window   # noqa: F401  (re-exported)


def sequential_sum(table, ids):
    """float32 [d]: 0 + table[ids[0]] + table[ids[1]] + ... left to right, a missing id adding
    the zero row."""
    table = np.asarray(table, np.float32)
    ids = np.asarray(ids, np.int64)
    rows = np.zeros((len(ids) + 1, table.shape[1]), np.float32)      # rows[0]: the +0.0 start
    known = (ids >= 0) & (ids < len(table))
    rows[1:][known] = table[ids[known]]
    return np.cumsum(rows, axis=0, dtype=np.float32)[-1]


def neighbor_aggregate(histories, nodes, ts, node_feats=None, edge_feats=None, since=None,
                       max_history=0, reduce="mean"):
    """(count int64 [N], node float32 [N, dn] or None, edge float32 [N, de] or None).
    histories: {node: (dst, ts, eid)}, oldest first.  since: None, a scalar, or an array [N]."""
    nodes, ts = np.asarray(nodes, np.int64), np.asarray(ts, np.float32)
    N = len(nodes)
    assert len(ts) == N and max_history >= 0 and reduce in ("sum", "mean")
    assert node_feats is not None or edge_feats is not None
    if since is not None:
        since = np.broadcast_to(np.asarray(since, np.float32), (N,))
    count = np.zeros(N, np.int64)
    outs = [None if tab is None else np.zeros((N, np.shape(tab)[1]), np.float32)
            for tab in (node_feats, edge_feats)]
    for i in range(N):
        h = histories.get(int(nodes[i]))
        if h is None or len(h[0]) == 0:
            continue
        h_dst, h_ts, h_eid = h
        a, c = window(h_ts, ts[i], None if since is None else since[i], max_history)
        n = c - a
        count[i] = n
        if n == 0:
            continue
        for out, tab, ids in ((outs[0], node_feats, h_dst), (outs[1], edge_feats, h_eid)):
            if tab is None:
                continue
            total = sequential_sum(tab, ids[a:c])
            out[i] = total / np.float32(n) if reduce == "mean" else total
            assert out[i].dtype == np.float32
    return count, outs[0], outs[1]
