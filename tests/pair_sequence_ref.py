"""Numpy restatement of DynamicGraph.pair_sequence (csrc/pair_sequence.hip, include/gnnflow_hip.h:
gf_graph_pair_sequence).

Histories as in tests/history_window_ref.py: {node: (dst int64 [m], ts float32 [m], eid int64 [m])},
OLDEST FIRST.  For row i with s = src[i], d = dst[i], t = ts[i] and, when `since` is given,
lo = since[i], with L = length (2 .. MAX_LENGTH):

    lengths, nodes, eids, times, counts = neighbor_cooccurrence_ref.neighbor_cooccurrence(...,
                          length=L, include_self=True): the self slot at position 0 (eid -1, time
                          t, counted), then the window at the bound L - 1, oldest first, then the
                          padding -1, -1, 0, (0, 0)
    delta_t[i, side, p] = float32(t) - times[i, side, p], one float32 subtraction, for
                          p < lengths[i, side] (the self slot: t - t); +0.0 for p >= lengths
    node[i, side, p, :] = N[nodes[i, side, p], :],  edge[i, side, p, :] = E[eids[i, side, p], :]
                          for p < lengths, the zero row for an id without a row in the table
                          (neighbor_sequence_ref.rows_of): the self slot has the node's own row in
                          `node` and the zero row in `edge`
    arg[i, side, p, j]  = float32(w[j] * delta_t[i, side, p]) + b[j], two float32 roundings, for
                          p < lengths
    node, edge, arg     = +0.0 for p >= lengths

The kernel's time part is cosf(arg).  As in neighbor_sequence_ref.py the cosine is not restated: it
is time_encode.hip's, and the GPU test compares the time part with ops.time_encode on the reader's
delta_t; `arg` is what goes into it, and a padded slot's time part is +0.0, not cos of anything.
Pure numpy.
"""
from typing import NamedTuple, Optional

import numpy as np

from tests.history_window_ref import count_before, from_graph, window      # noqa: F401
from tests.neighbor_cooccurrence_ref import neighbor_cooccurrence
from tests.neighbor_sequence_ref import rows_of

MAX_LENGTH = 512                   # GF_PAIRSEQ_MAX_LENGTH


class PairSequence(NamedTuple):
    lengths: np.ndarray              # int32 [N, 2]
    nodes: np.ndarray                # int64 [N, 2, L]
    eids: np.ndarray                 # int64 [N, 2, L]
    times: np.ndarray                # float32 [N, 2, L]
    delta_t: np.ndarray              # float32 [N, 2, L]
    counts: np.ndarray               # int32 [N, 2, L, 2]
    node: Optional[np.ndarray]       # float32 [N, 2, L, dn] or None
    edge: Optional[np.ndarray]       # float32 [N, 2, L, de] or None
    arg: Optional[np.ndarray]        # float32 [N, 2, L, dT] or None


def pair_sequence(histories, src, dst, ts, since=None, length=32, node_feats=None,
                  edge_feats=None, weight=None, bias=None):
    """PairSequence(...).  histories: {node: (dst, ts, eid)}, oldest first.  since: None, a
    scalar, or an array [N].  weight [dT] or [dT, 1] and bias [dT] are given together."""
    ts = np.asarray(ts, np.float32)
    N, L = len(ts), int(length)
    assert 2 <= L <= MAX_LENGTH and (weight is None) == (bias is None)
    lengths, nodes, eids, times, counts = neighbor_cooccurrence(
        histories, src, dst, ts, since, L, True)
    filled = np.arange(L)[None, None, :] < lengths[:, :, None]              # [N, 2, L]
    with np.errstate(invalid="ignore"):                                     # inf - inf, NaN
        delta_t = np.where(filled, ts[:, None, None] - times, np.float32(0)).astype(np.float32)
    assert (ts[:, None, None] - times).dtype == np.float32

    def part(table, ids):
        if table is None:
            return None
        rows = rows_of(table, ids.reshape(-1)).reshape(N, 2, L, -1)
        return np.where(filled[..., None], rows, np.float32(0)).astype(np.float32)

    arg = None
    if weight is not None:
        w = np.asarray(weight, np.float32).reshape(-1)
        b = np.asarray(bias, np.float32).reshape(-1)
        assert w.shape == b.shape
        with np.errstate(over="ignore", invalid="ignore"):
            prod = (w * delta_t[..., None]).astype(np.float32)
            arg = np.where(filled[..., None], prod + b, np.float32(0)).astype(np.float32)
    return PairSequence(lengths, nodes, eids, times, delta_t, counts, part(node_feats, nodes),
                        part(edge_feats, eids), arg)
