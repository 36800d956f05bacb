"""Numpy restatement of DynamicGraph.neighbor_sequence (csrc/neighbor_sequence.hip,
include/gnnflow_hip.h, gf_graph_neighbor_sequence).

A history is (dst int64 [m], ts float32 [m], eid int64 [m]), OLDEST FIRST, the live edges of a node
in the store's order (pair_history_ref.from_graph).  For row i with v = nodes[i], t = ts[i] and,
when `since` is given, lo = since[i], over h = histories[v], with L = length:

    (a, c)  = neighbor_aggregate_ref.window(h.ts, t, lo, L)      lo <= ts < t, the newest L
    n       = c - a,  lengths[i] = n
    nodes[i, p], eids[i, p], times[i, p] = h.dst[a + p], h.eid[a + p], h.ts[a + p]      p < n
    delta_t[i, p] = float32(t) - h.ts[a + p], one float32 subtraction                   p < n
    -1, -1, 0, 0 for p >= n
    edge[i, p, :] = E[eids[i, p], :],  node[i, p, :] = N[nodes[i, p], :]                p < n
                    the zero row for an id without a row in the table (negative, >= len(table))
    arg[i, p, j]  = float32(w[j] * delta_t[i, p]) + b[j], two float32 roundings         p < n
    edge, node, arg = +0.0 for p >= n

The kernel's tokens are [edge | node | cosf(arg)].  The cosine is not restated: it is
time_encode.hip's, and the GPU test compares the time part with ops.time_encode; `arg` is what goes
into it, and a padded slot's time part is +0.0, not cos of anything.  A node without a history
(negative, unknown, no live edges) gives an all-padding row.  Pure numpy.
"""
from typing import NamedTuple, Optional

import numpy as np

from tests.neighbor_aggregate_ref import window
from tests.pair_history_ref import count_before, from_graph      # noqa: F401  (re-exported)


class Sequence(NamedTuple):
    lengths: np.ndarray              # int32 [N]
    nodes: np.ndarray                # int64 [N, L]
    eids: np.ndarray                 # int64 [N, L]
    times: np.ndarray                # float32 [N, L]
    delta_t: np.ndarray              # float32 [N, L]
    edge: Optional[np.ndarray]       # float32 [N, L, de] or None
    node: Optional[np.ndarray]       # float32 [N, L, dn] or None
    arg: Optional[np.ndarray]        # float32 [N, L, dT] or None


def rows_of(table, ids):
    """float32 [len(ids), d]: table[ids], the zero row for an id without a row."""
    table = np.asarray(table, np.float32)
    ids = np.asarray(ids, np.int64)
    out = np.zeros((len(ids), table.shape[1]), np.float32)
    known = (ids >= 0) & (ids < len(table))
    out[known] = table[ids[known]]
    return out


def neighbor_sequence(histories, nodes, ts, since=None, length=32, edge_feats=None,
                      node_feats=None, weight=None, bias=None):
    """Sequence(...).  histories: {node: (dst, ts, eid)}, oldest first.  since: None, a scalar, or
    an array [N].  weight [dT] or [dT, 1] and bias [dT] are given together."""
    nodes, ts = np.asarray(nodes, np.int64), np.asarray(ts, np.float32)
    N, L = len(nodes), int(length)
    assert len(ts) == N and L >= 1 and (weight is None) == (bias is None)
    if since is not None:
        since = np.broadcast_to(np.asarray(since, np.float32), (N,))
    lengths = np.zeros(N, np.int32)
    out_nodes = np.full((N, L), -1, np.int64)
    eids = np.full((N, L), -1, np.int64)
    times = np.zeros((N, L), np.float32)
    delta_t = np.zeros((N, L), np.float32)
    edge = None if edge_feats is None else np.zeros((N, L, np.shape(edge_feats)[1]), np.float32)
    node = None if node_feats is None else np.zeros((N, L, np.shape(node_feats)[1]), np.float32)
    arg = None
    if weight is not None:
        w = np.asarray(weight, np.float32).reshape(-1)
        b = np.asarray(bias, np.float32).reshape(-1)
        assert w.shape == b.shape
        arg = np.zeros((N, L, len(w)), np.float32)
    for i in range(N):
        h = histories.get(int(nodes[i]))
        if h is None or len(h[0]) == 0:
            continue
        h_dst, h_ts, h_eid = h
        a, c = window(h_ts, ts[i], None if since is None else since[i], L)
        n = c - a
        assert 0 <= n <= L
        lengths[i] = n
        if n == 0:
            continue
        out_nodes[i, :n] = h_dst[a:c]
        eids[i, :n] = h_eid[a:c]
        times[i, :n] = np.asarray(h_ts[a:c], np.float32)
        delta_t[i, :n] = ts[i] - times[i, :n]
        assert delta_t.dtype == np.float32
        if edge is not None:
            edge[i, :n] = rows_of(edge_feats, h_eid[a:c])
        if node is not None:
            node[i, :n] = rows_of(node_feats, h_dst[a:c])
        if arg is not None:
            with np.errstate(over="ignore", invalid="ignore"):
                prod = (w[None, :] * delta_t[i, :n, None]).astype(np.float32)
                arg[i, :n] = prod + b[None, :]
    return Sequence(lengths, out_nodes, eids, times, delta_t, edge, node, arg)
