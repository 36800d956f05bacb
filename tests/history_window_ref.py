"""Numpy restatement of the history window that the edge-history readers share
(csrc/history_window.hpp's header comment); the readers' references are built on it.

A history is (dst int64 [m], ts float32 [m], eid int64 [m]), OLDEST FIRST, the live edges of a node
in the store's order.  For time t, optional lower end lo and bound H (max_history, 0: none):

    c  = #{x in h.ts : x < t}                    float32 <: a NaN t gives 0
    c0 = min(c, #{x in h.ts : x < lo})           float32 <: a NaN lo gives 0; 0 without lo
    n  = min(c - c0, H) if H else c - c0
    considered = positions c - n .. c - 1        lo <= ts < t, the newest n, oldest first
"""
import numpy as np


def count_before(ts, t):
    """#{x in ts : x < t} in float32; the history ascends, so these are a prefix.  NaN goes
    through < as it is: nothing is below NaN."""
    with np.errstate(invalid="ignore"):
        before = np.asarray(ts, np.float32) < np.float32(t)
    c = int(before.sum())
    assert before[:c].all()
    return c


def window(h_ts, t, lo=None, max_history=0):
    """(c - n, c): the considered positions of a history with timestamps h_ts."""
    c = count_before(h_ts, t)
    c0 = min(c, count_before(h_ts, lo)) if lo is not None else 0
    n = min(c - c0, max_history) if max_history else c - c0
    return c - n, c


def from_graph(graph, nodes):
    """{node: (dst, ts, eid)} oldest first, for every distinct valid node of `nodes`."""
    out = {}
    for v in np.unique(np.asarray(nodes, np.int64)):
        if 0 <= v <= graph.max_vertex_id():
            d, t, e = graph.get_temporal_neighbors(int(v))
            out[int(v)] = (d[::-1].copy(), t[::-1].copy(), e[::-1].copy())
    return out
