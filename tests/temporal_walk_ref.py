"""Numpy restatement of DynamicGraph.temporal_random_walk (csrc/temporal_walk.hip,
include/gnnflow_hip.h, gf_graph_temporal_walks) and of ops.walk_position_counts
(csrc/walk_positions.hip, gf_walk_position_counts).  Integers only: the kernels must match bit
for bit.

    walk (i, w):  v_0 = src[i], t_0 = ts[i], nodes[i, w, 0] = src[i];  for step j = 0 .. L - 1
    v_j outside [0, table_len): the walk has ended
    history of v_j, oldest first: h_dst[0:m], h_ts[0:m], h_eid[0:m]
    c    = #{x in h_ts : x < t_j}        float32 <, strict: a tie is not history, NaN t_j gives 0
    n    = min(c, max_history) if max_history else c                n == 0: the walk has ended
    u_a  = philox_first(seed ^ (SEED_TAG + a), tid, (epoch << 8) + j)     a < recency
    x    = max over a of (u_a * n) >> 32
    k    = (c - n) + x;  nodes[i, w, j + 1], eids[i, w, j], times[i, w, j] = h_dst[k], h_eid[k], h_ts[k]
    v_{j+1}, t_{j+1} = h_dst[k], h_ts[k]           tid = (first_row + i) * W + w  mod 2^64

Every slot from the step a walk ends on holds nodes = -1, eids = -1, times = 0.

A history is (dst int64 [m], ts float32 [m], eid int64 [m]), OLDEST FIRST, the live edges of the
node in the store's order; `from_graph` reads them with get_temporal_neighbors (which returns
newest first), `from_edges` builds them from the edge arrays the graph was given in one call,
`from_chunks` from those of successive calls.

    position_counts:  out[i, w, j, p] = #{w' : ref[i, w', p] == nodes[i, w, j]} if nodes[i, w, j] >= 0 else 0
"""
import numpy as np

from tests.attention_dropout_ref import philox_first
from tests.history_window_ref import count_before

MASK64 = (1 << 64) - 1
SEED_TAG = 0x54454D5057414C4B      # GF_WALK_SEED_TAG, "TEMPWALK"
MAX_LENGTH = 32                    # GF_WALK_MAX_LENGTH
MAX_RECENCY = 8                    # GF_WALK_MAX_RECENCY


def draw_seed(seed, a):
    return (int(seed) ^ ((SEED_TAG + a) & MASK64)) & MASK64


def tids(first_row, B, W):
    """uint64 [B, W]: (first_row + i) * W + w mod 2^64."""
    out = np.empty((B, W), dtype=np.uint64)
    for i in range(B):
        for w in range(W):
            out[i, w] = ((first_row + i) * W + w) & MASK64      # Python integers: exact
    return out


def words(B, W, L, recency, seed=0, epoch=0, first_row=0):
    """uint64 [recency, B, W, L]: the Philox word u_a of every draw of every step."""
    t = tids(first_row, B, W)[:, :, None]
    call = np.array([((int(epoch) << 8) + j) & MASK64 for j in range(L)], dtype=np.uint64)
    out = np.empty((recency, B, W, L), dtype=np.uint64)
    for a in range(recency):
        out[a] = philox_first(draw_seed(seed, a), t, call[None, None, :]).astype(np.uint64)
    return out


def pick(u, n):
    """x: the maximum over the draws u (uint64 words below 2^32, any shape, first axis the draws)
    of (u * n) >> 32.  0 <= x < n."""
    u = np.asarray(u, dtype=np.uint64)
    return ((u * np.uint64(n)) >> np.uint64(32)).max(axis=0).astype(np.int64)      # u n < 2^64


def history_size(h_ts, t):
    """c: elements of the node's timestamps strictly below t, compared as float32."""
    return count_before(h_ts, t)


def walks(histories, table_len, src, ts, length, num_walks=1, recency=1, max_history=0, seed=0,
          epoch=0, first_row=0):
    """(nodes int64 [B, W, L + 1], eids int64 [B, W, L], times float32 [B, W, L]).  histories:
    {node: (dst, ts, eid)}, oldest first; a node below table_len that is not in it has no edge."""
    src, ts = np.asarray(src, dtype=np.int64), np.asarray(ts, dtype=np.float32)
    B, W, L = len(src), num_walks, length
    assert len(ts) == B and 1 <= L <= MAX_LENGTH and 1 <= W < 2 ** 16
    assert 1 <= recency <= MAX_RECENCY and max_history >= 0
    nodes = np.full((B, W, L + 1), -1, dtype=np.int64)
    eids = np.full((B, W, L), -1, dtype=np.int64)
    times = np.zeros((B, W, L), dtype=np.float32)
    u = words(B, W, L, recency, seed, epoch, first_row)
    for i in range(B):
        nodes[i, :, 0] = src[i]
        for w in range(W):
            v, t = int(src[i]), ts[i]
            for j in range(L):
                if not 0 <= v < table_len or v not in histories:
                    break
                h_dst, h_ts, h_eid = histories[v]
                c = history_size(h_ts, t)
                n = min(c, max_history) if max_history else c
                if n == 0:
                    break
                k = (c - n) + int(pick(u[:, i, w, j], n))
                nodes[i, w, j + 1], eids[i, w, j], times[i, w, j] = h_dst[k], h_eid[k], h_ts[k]
                v, t = int(h_dst[k]), np.float32(h_ts[k])
    return nodes, eids, times


def steps_taken(eids):
    """int64 [B, W]: the steps a walk took before it ended (edge ids are >= 0 in the tests)."""
    return (np.asarray(eids) >= 0).sum(-1)


def position_counts(nodes, ref=None):
    """int32 [B, W, L + 1, Lr + 1]."""
    nodes = np.asarray(nodes, dtype=np.int64)
    ref = nodes if ref is None else np.asarray(ref, dtype=np.int64)
    assert nodes.ndim == 3 and ref.ndim == 3 and ref.shape[0] == nodes.shape[0]
    out = np.zeros(nodes.shape + (ref.shape[2],), dtype=np.int32)
    for i in range(nodes.shape[0]):
        # [W, L + 1, Wr, Lr + 1] summed over the walks of ref
        eq = nodes[i][:, :, None, None] == ref[i][None, None, :, :]
        out[i] = eq.sum(2) * (nodes[i] >= 0)[:, :, None]
    return out


def from_graph(graph):
    """({node: (dst, ts, eid)} oldest first for every id the node table holds, table_len)."""
    table_len = graph.max_vertex_id() + 1 if graph.num_vertices() else 0
    out = {}
    for v in range(table_len):
        d, t, e = graph.get_temporal_neighbors(int(v))
        out[v] = (d[::-1].copy(), t[::-1].copy(), e[::-1].copy())
    return out, table_len


def from_edges(src, dst, ts, eid=None, add_reverse=False):
    """The same from the edge arrays of ONE add_edges call on an empty graph: a node's edges in
    the order given, stable-sorted by time (ties keep the order given; with add_reverse the
    reversed copies follow all forward edges, as DynamicGraph.add_edges concatenates them)."""
    src, dst = np.asarray(src, dtype=np.int64), np.asarray(dst, dtype=np.int64)
    ts = np.asarray(ts, dtype=np.float32)
    eid = np.arange(len(src), dtype=np.int64) if eid is None else np.asarray(eid, dtype=np.int64)
    if add_reverse:
        src, dst = np.concatenate([src, dst]), np.concatenate([dst, src])
        ts, eid = np.concatenate([ts, ts]), np.concatenate([eid, eid])
    table_len = int(max(src.max(), dst.max())) + 1 if len(src) else 0
    out = {}
    for v in range(table_len):
        idx = np.flatnonzero(src == v)
        idx = idx[np.argsort(ts[idx], kind="stable")]
        out[v] = (dst[idx], ts[idx], eid[idx])
    return out, table_len


def from_chunks(src, dst, ts, eid, chunk, add_reverse=False):
    """The same from the edge arrays given to an empty graph in successive add_edges calls of
    `chunk` edges each (tests/synth.py ingest_chunks), under either block policy and before any
    offload, where no call holds a time below an earlier call's: a node's edges call after call,
    inside a call stable-sorted by time in the order given (with add_reverse a call's reversed
    copies follow all its forward edges).  Only the nodes that have an edge are in the result, so
    that a sparse far id costs nothing."""
    src, dst = np.asarray(src, dtype=np.int64), np.asarray(dst, dtype=np.int64)
    ts, eid = np.asarray(ts, dtype=np.float32), np.asarray(eid, dtype=np.int64)
    call = np.arange(len(src)) // chunk
    given = np.arange(len(src))
    if add_reverse:
        src, dst = np.concatenate([src, dst]), np.concatenate([dst, src])
        ts, eid, call = np.concatenate([ts, ts]), np.concatenate([eid, eid]), np.tile(call, 2)
        given = np.concatenate([given, given + len(given)])
    table_len = int(max(src.max(), dst.max())) + 1 if len(src) else 0
    order = np.lexsort((given, ts, call, src))      # by node, then call, then time, then as given
    starts = np.flatnonzero(np.append(True, src[order][1:] != src[order][:-1]))
    out = {}
    for a, b in zip(starts, np.append(starts[1:], len(order))):
        idx = order[a:b]
        out[int(src[idx[0]])] = (dst[idx], ts[idx], eid[idx])
    return out, table_len
