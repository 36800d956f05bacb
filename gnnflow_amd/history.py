"""The edge-history readers of DynamicGraph (seen_mask, pair_history, common_neighbors,
temporal_degree, neighbor_cooccurrence, neighbor_aggregate, neighbor_sequence, pair_sequence,
temporal_random_walk): their argument checkers, result types and limits, and HistoryReaders, the
base class that gives DynamicGraph the methods.  dynamic_graph.py re-exports the public names."""
from typing import NamedTuple, Optional

import numpy as np
import torch

from . import _capi


# The checkers of the edge-history readers are built from the helpers below.  Each checker calls
# them in the order in which its errors are reported when several arguments are wrong, which is
# part of its contract (tests/test_history_checkers.py).

def _typed_tensors(tensors, since=None):
    """The (name, tensor, dtype) triples, `since` appended when it is a tensor, after the type
    checks the history readers share."""
    tensors = list(tensors)
    if isinstance(since, torch.Tensor):
        tensors.append(("since", since, torch.float32))
    for name, x, dtype in tensors:
        if not isinstance(x, torch.Tensor):
            raise TypeError("{} must be a tensor, got {}".format(name, type(x).__name__))
        if x.dtype != dtype:
            raise TypeError("{} must be {}, got {}".format(name, dtype, x.dtype))
    if since is not None and not isinstance(since, torch.Tensor) and (
            isinstance(since, bool) or not isinstance(since, (int, float))):
        raise TypeError("since must be None, a float or a tensor, got {}".format(
            type(since).__name__))
    return tensors


def _one_dim(tensors):
    for name, x, _ in tensors:
        if x.dim() != 1:
            raise ValueError("{} must be 1-D, got shape {}".format(name, tuple(x.shape)))


def _equal_rows(tensors):
    """N of 1-D tensors of one length; the first of them is the one the message measures by."""
    first, N = tensors[0][0], int(tensors[0][1].shape[0])
    for name, x, _ in tensors[1:]:
        if int(x.shape[0]) != N:
            raise ValueError("{} has {} rows, {} has {}".format(first, N, name, int(x.shape[0])))
    return N


def _below_2_31(n, what, unit):
    if n >= 2 ** 31:
        raise ValueError("{} takes fewer than 2**31 {}, got {}".format(what, unit, n))


def _rows(tensors, what):
    """N of 1-D tensors of one length, fewer than 2**31."""
    _one_dim(tensors)
    N = _equal_rows(tensors)
    _below_2_31(N, what, "rows")
    return N


def _same_device(tensors):
    first, x0, _ = tensors[0]
    for name, x, _ in tensors[1:]:
        if x.device != x0.device:
            raise ValueError("{} is on {}, {} on {}".format(name, x.device, first, x0.device))


def _int_arg(value, name, lo, hi):
    if isinstance(value, bool) or not isinstance(value, (int, np.integer)):
        raise TypeError("{} must be an int, got {}".format(name, type(value).__name__))
    value = int(value)
    if not lo <= value < hi:
        raise ValueError("{} must be in [{}, {}), got {}".format(name, lo, hi, value))
    return value


# seen_mask and pair_history report max_history in two steps: its type with the other type
# errors, ahead of the shapes, and its sign after the shapes.  A numpy integer is not an int here.

def _history_type(max_history):
    if isinstance(max_history, bool) or not isinstance(max_history, int):
        raise TypeError("max_history must be an int, got {}".format(type(max_history).__name__))


def _history_sign(max_history):
    if max_history < 0:
        raise ValueError("max_history must be >= 0, got {}".format(max_history))


def _pair_tensors(src, dst, ts):
    return [("src", src, torch.int64), ("dst", dst, torch.int64), ("ts", ts, torch.float32)]


def _given_tables(named):
    """The (name, tensor, dtype) triples of a table reader's (name, table) pairs that are not None.
    Refuses a half-precision one ahead of _typed_tensors: this message names what is supported."""
    tables = [(name, x, torch.float32) for name, x in named if x is not None]
    for name, x, _ in tables:
        if isinstance(x, torch.Tensor) and x.dtype in (torch.float16, torch.bfloat16):
            raise TypeError("{} must be float32, got {}: half-precision tables are not "
                            "supported".format(name, x.dtype))
    return tables


def _feature_tables(tables, max_width):
    """{name: width} of the given tables, each [rows >= 1, 1 .. max_width] and contiguous."""
    width = {}
    for name, x, _ in tables:
        if x.dim() != 2:
            raise ValueError("{} must be 2-D, got shape {}".format(name, tuple(x.shape)))
        if int(x.shape[0]) == 0:      # no storage to point the kernel at
            raise ValueError("{} has no rows".format(name))
        if not 1 <= int(x.shape[1]) <= max_width:
            raise ValueError("{} must have 1 to {} columns, got {}".format(
                name, max_width, int(x.shape[1])))
        if not x.is_contiguous():
            raise ValueError("{} must be contiguous (a table is never copied); got strides "
                             "{}".format(name, tuple(x.stride())))
        width[name] = int(x.shape[1])
    return width


def _table_rows(tensors, what):
    """_rows of a table reader's 1-D tensors: nodes, ts and, when it is a tensor, since."""
    return _rows([t for t in tensors if t[0] in ("nodes", "ts", "since")], what)


def check_seen_mask_args(src, ts, cand_ids, max_history=0):
    """Arguments of DynamicGraph.seen_mask, checked before anything is launched: the kernel takes
    raw pointers and trusts them.  Needs no device.  Returns (B, C)."""
    tensors = _typed_tensors([("src", src, torch.int64), ("ts", ts, torch.float32),
                              ("cand_ids", cand_ids, torch.int64)])
    _history_type(max_history)
    _one_dim(tensors)
    B, Cn = _equal_rows(tensors[:2]), int(cand_ids.shape[0])
    if Cn == 0:
        raise ValueError("seen_mask needs at least one candidate")
    _below_2_31(Cn, "seen_mask", "candidates")
    _below_2_31(B, "seen_mask", "rows")
    _history_sign(max_history)
    _same_device(tensors)
    return B, Cn


class PairHistory(NamedTuple):
    """What DynamicGraph.pair_history returns, one entry per (src, dst, ts) row."""
    count: torch.Tensor      # int64 [N]; considered edges of src that lead to dst
    last_ts: torch.Tensor    # float32 [N]; time of the latest of them, -inf where count == 0
    last_eid: torch.Tensor   # int64 [N]; its edge id, -1 where count == 0


def check_pair_history_args(src, dst, ts, since=None, max_history=0):
    """Arguments of DynamicGraph.pair_history, checked before anything is launched: the kernel
    takes raw pointers and trusts them.  Needs no device.  Returns N."""
    tensors = _typed_tensors(_pair_tensors(src, dst, ts), since)
    _history_type(max_history)
    N = _rows(tensors, "pair_history")
    _history_sign(max_history)
    _same_device(tensors)
    return N


CN_MAX_HISTORY = 512      # GF_CN_MAX_HISTORY


class CommonNeighbors(NamedTuple):
    """What DynamicGraph.common_neighbors returns, one row per (src, dst, ts) row; A and B are the
    considered edges of src and of dst."""
    n_src: torch.Tensor      # int32 [N]; |A|, multi-edges counted
    n_dst: torch.Tensor      # int32 [N]; |B|
    u_src: torch.Tensor      # int32 [N]; distinct neighbours in A
    u_dst: torch.Tensor      # int32 [N]; distinct neighbours in B
    common: torch.Tensor     # int32 [N]; neighbours in both, not capped by max_common
    nodes: torch.Tensor      # int64 [N, K]; the common ones, src's most recent first, then -1
    cnt_src: torch.Tensor    # int32 [N, K]; edges of A that lead to nodes[i, k], 0 in the padding
    cnt_dst: torch.Tensor    # int32 [N, K]; edges of B that lead to nodes[i, k], 0 in the padding


def check_common_neighbors_args(src, dst, ts, since=None, max_history=64, max_common=32):
    """Arguments of DynamicGraph.common_neighbors, checked before anything is launched or
    allocated: the kernel takes raw pointers and trusts them.  Needs no device.
    Returns (N, H, K)."""
    tensors = _typed_tensors(_pair_tensors(src, dst, ts), since)
    H = _int_arg(max_history, "max_history", 1, CN_MAX_HISTORY + 1)
    K = _int_arg(max_common, "max_common", 0, CN_MAX_HISTORY + 1)
    N = _rows(tensors, "common_neighbors")
    _same_device(tensors)
    return N, H, K


def check_temporal_degree_args(nodes, ts, since=None):
    """Arguments of DynamicGraph.temporal_degree, checked before anything is launched.  Needs no
    device.  Returns the number of elements."""
    tensors = _typed_tensors([("nodes", nodes, torch.int64), ("ts", ts, torch.float32)], since)
    for name, x, _ in tensors[1:]:
        if tuple(x.shape) != tuple(nodes.shape):
            raise ValueError("nodes has shape {}, {} has {}".format(
                tuple(nodes.shape), name, tuple(x.shape)))
    _below_2_31(nodes.numel(), "temporal_degree", "elements")
    _same_device(tensors)
    return int(nodes.numel())


COOC_MAX_LENGTH = 512      # GF_COOC_MAX_LENGTH


class NeighborCooccurrence(NamedTuple):
    """What DynamicGraph.neighbor_cooccurrence returns, one row per (src, dst, ts) row; side 0 is
    src's sequence, side 1 dst's, L = length slots each, oldest first after the self slot."""
    lengths: torch.Tensor    # int32 [N, 2]; filled slots of each side, the self slot included
    nodes: torch.Tensor      # int64 [N, 2, L]; the sequence's nodes, then -1
    eids: torch.Tensor       # int64 [N, 2, L]; the edges' ids; -1 for the self slot and the padding
    times: torch.Tensor      # float32 [N, 2, L]; the edges' times; ts for the self slot; 0 padding
    counts: torch.Tensor     # int32 [N, 2, L, 2]; occurrences in src's, in dst's sequence


def check_neighbor_cooccurrence_args(src, dst, ts, since=None, length=32, include_self=True):
    """Arguments of DynamicGraph.neighbor_cooccurrence, checked before anything is launched or
    allocated: the kernel takes raw pointers and trusts them.  Needs no device.
    Returns (N, L, self)."""
    tensors = _typed_tensors(_pair_tensors(src, dst, ts), since)
    if not isinstance(include_self, bool):
        raise TypeError("include_self must be a bool, got {}".format(type(include_self).__name__))
    # length - include_self bounds the window, and a bound of 0 would be "no bound"
    L = _int_arg(length, "length", 1 + int(include_self), COOC_MAX_LENGTH + 1)
    N = _rows(tensors, "neighbor_cooccurrence")
    _same_device(tensors)
    return N, L, int(include_self)


AGG_MAX_WIDTH = 1024      # GF_AGG_MAX_WIDTH


class NeighborAggregate(NamedTuple):
    """What DynamicGraph.neighbor_aggregate returns, one row per (node, ts) row."""
    count: torch.Tensor              # int64 [N]; the considered edges of the node
    node: Optional[torch.Tensor]     # float32 [N, dn]; their destinations' rows reduced, or None
    edge: Optional[torch.Tensor]     # float32 [N, de]; their own rows reduced, or None


def check_neighbor_aggregate_args(nodes, ts, node_feats=None, edge_feats=None, since=None,
                                  max_history=0, reduce="mean"):
    """Arguments of DynamicGraph.neighbor_aggregate, checked before anything is launched or
    allocated: the kernel takes raw pointers and trusts them.  Needs no device.
    Returns (N, dn, de), a width of 0 for a table that is not given."""
    rows = [("nodes", nodes, torch.int64), ("ts", ts, torch.float32)]
    tables = _given_tables((("node_feats", node_feats), ("edge_feats", edge_feats)))
    tensors = _typed_tensors(rows + tables, since)
    _history_type(max_history)
    if not isinstance(reduce, str):
        raise TypeError("reduce must be a str, got {}".format(type(reduce).__name__))
    N = _table_rows(tensors, "neighbor_aggregate")
    if not tables:
        raise ValueError("neighbor_aggregate needs node_feats or edge_feats")
    width = _feature_tables(tables, AGG_MAX_WIDTH)
    if reduce not in ("sum", "mean"):
        raise ValueError("reduce must be 'sum' or 'mean', got {!r}".format(reduce))
    _history_sign(max_history)
    _same_device(tensors)
    return N, width.get("node_feats", 0), width.get("edge_feats", 0)


SEQ_MAX_LENGTH = 512      # GF_SEQ_MAX_LENGTH
SEQ_MAX_WIDTH = 1024      # GF_SEQ_MAX_WIDTH


class NeighborSequence(NamedTuple):
    """What DynamicGraph.neighbor_sequence returns, one row per (node, ts) row; L = length slots,
    oldest first, the slots p >= lengths[i] are padding."""
    lengths: torch.Tensor            # int32 [N]; filled slots
    nodes: torch.Tensor              # int64 [N, L]; the edges' destinations, then -1
    eids: torch.Tensor               # int64 [N, L]; the edges' ids, then -1
    times: torch.Tensor              # float32 [N, L]; the edges' times, then 0
    delta_t: torch.Tensor            # float32 [N, L]; ts[i] - times[i, p], then 0
    tokens: Optional[torch.Tensor]   # float32 [N, L, de + dn + dT], zeros in the padding, or None


def _encoder_tensors(time_encoder):
    """(weight, bias) of a time encoder: a (weight, bias) pair, or a module that holds them as
    `weight` and `bias` (nn.FixedTimeEncode) or as those of its Linear `w` (nn.TimeEncode)."""
    if isinstance(time_encoder, (tuple, list)):
        if len(time_encoder) != 2:
            raise TypeError("time_encoder must be a module or a (weight, bias) pair, got {} "
                            "elements".format(len(time_encoder)))
        return time_encoder[0], time_encoder[1]
    for holder in (time_encoder, getattr(time_encoder, "w", None)):
        if hasattr(holder, "weight") and hasattr(holder, "bias"):
            return holder.weight, holder.bias
    raise TypeError("time_encoder must be a module with weight and bias or a (weight, bias) pair, "
                    "got {}".format(type(time_encoder).__name__))


def check_neighbor_sequence_args(nodes, ts, since=None, length=32, edge_feats=None,
                                 node_feats=None, time_encoder=None):
    """Arguments of DynamicGraph.neighbor_sequence, checked before anything is launched or
    allocated: the kernel takes raw pointers and trusts them.  Needs no device.
    Returns (N, L, de, dn, dT), a width of 0 for a part that is not given."""
    rows = [("nodes", nodes, torch.int64), ("ts", ts, torch.float32)]
    tables = _given_tables((("edge_feats", edge_feats), ("node_feats", node_feats)))
    encoder = []
    if time_encoder is not None:
        weight, bias = _encoder_tensors(time_encoder)
        encoder = [("time_encoder's weight", weight, torch.float32),
                   ("time_encoder's bias", bias, torch.float32)]
    tensors = _typed_tensors(rows + tables + encoder, since)
    L = _int_arg(length, "length", 1, SEQ_MAX_LENGTH + 1)
    N = _table_rows(tensors, "neighbor_sequence")
    width = _feature_tables(tables, SEQ_MAX_WIDTH)
    dT = _encoder_width(encoder, SEQ_MAX_WIDTH)
    _same_device(tensors)
    return N, L, width.get("edge_feats", 0), width.get("node_feats", 0), dT


PAIRSEQ_MAX_LENGTH = 512      # GF_PAIRSEQ_MAX_LENGTH
PAIRSEQ_MAX_WIDTH = 1024      # GF_PAIRSEQ_MAX_WIDTH


class PairSequence(NamedTuple):
    """What DynamicGraph.pair_sequence returns, one row per (src, dst, ts) row; side 0 is src's
    sequence, side 1 dst's, L = length slots each: the self slot, then oldest first, then padding."""
    lengths: torch.Tensor            # int32 [N, 2]; filled slots of each side, the self slot included
    nodes: torch.Tensor              # int64 [N, 2, L]; the sequence's nodes, then -1
    eids: torch.Tensor               # int64 [N, 2, L]; the edges' ids; -1 for the self slot, padding
    times: torch.Tensor              # float32 [N, 2, L]; the edges' times; ts for the self slot; then 0
    delta_t: torch.Tensor            # float32 [N, 2, L]; ts[i] - times on a filled slot, then 0
    counts: torch.Tensor             # int32 [N, 2, L, 2]; occurrences in src's, in dst's sequence
    node: Optional[torch.Tensor]     # float32 [N, 2, L, dn], zeros in the padding, or None
    edge: Optional[torch.Tensor]     # float32 [N, 2, L, de], zeros in the padding, or None
    time: Optional[torch.Tensor]     # float32 [N, 2, L, dT], zeros in the padding, or None


def _encoder_width(encoder, max_width):
    """dT of the (name, tensor, dtype) triples of a time encoder's weight and bias; 0 without."""
    if not encoder:
        return 0
    weight, bias = encoder[0][1], encoder[1][1]
    if bias.dim() != 1:
        raise ValueError("time_encoder's bias must be [dT], got shape {}".format(
            tuple(bias.shape)))
    dT = int(bias.shape[0])
    if not 1 <= dT <= max_width:
        raise ValueError("time_encoder must have 1 to {} columns, got {}".format(max_width, dT))
    if tuple(weight.shape) not in ((dT, 1), (dT,)):
        raise ValueError("time_encoder's weight must be [dT, 1] or [dT] with dT = {}, got "
                         "shape {}".format(dT, tuple(weight.shape)))
    return dT


def check_pair_sequence_args(src, dst, ts, since=None, length=32, node_feats=None,
                             edge_feats=None, time_encoder=None):
    """Arguments of DynamicGraph.pair_sequence, checked before anything is launched or
    allocated: the kernel takes raw pointers and trusts them.  Needs no device.
    Returns (N, L, dn, de, dT), a width of 0 for a part that is not given."""
    tables = _given_tables((("node_feats", node_feats), ("edge_feats", edge_feats)))
    encoder = []
    if time_encoder is not None:
        weight, bias = _encoder_tensors(time_encoder)
        encoder = [("time_encoder's weight", weight, torch.float32),
                   ("time_encoder's bias", bias, torch.float32)]
    tensors = _typed_tensors(_pair_tensors(src, dst, ts) + tables + encoder, since)
    # length - 1 bounds the window behind the self slot, and a bound of 0 would be "no bound"
    L = _int_arg(length, "length", 2, PAIRSEQ_MAX_LENGTH + 1)
    N = _rows([t for t in tensors if t[0] in ("src", "dst", "ts", "since")], "pair_sequence")
    width = _feature_tables(tables, PAIRSEQ_MAX_WIDTH)
    dT = _encoder_width(encoder, PAIRSEQ_MAX_WIDTH)
    _same_device(tensors)
    return N, L, width.get("node_feats", 0), width.get("edge_feats", 0), dT


WALK_MAX_LENGTH = 32      # GF_WALK_MAX_LENGTH
WALK_MAX_RECENCY = 8      # GF_WALK_MAX_RECENCY


class TemporalWalks(NamedTuple):
    """What DynamicGraph.temporal_random_walk returns: B roots, W walks each, L steps.  Slots from
    the step a walk ends on hold nodes = -1, eids = -1, times = 0."""
    nodes: torch.Tensor      # int64 [B, W, L + 1]; nodes[:, :, 0] is the root
    eids: torch.Tensor       # int64 [B, W, L]; the edge step j took
    times: torch.Tensor      # float32 [B, W, L]; its timestamp


def check_temporal_walk_args(src, ts, length, num_walks=1, recency=1, max_history=0, seed=0,
                             epoch=0, first_row=0):
    """Arguments of DynamicGraph.temporal_random_walk, checked before anything is launched or
    allocated: the kernel takes raw pointers and trusts them.  Needs no device.
    Returns (B, W, L)."""
    tensors = _typed_tensors([("src", src, torch.int64), ("ts", ts, torch.float32)])
    L = _int_arg(length, "length", 1, WALK_MAX_LENGTH + 1)
    W = _int_arg(num_walks, "num_walks", 1, 2 ** 16)
    _int_arg(recency, "recency", 1, WALK_MAX_RECENCY + 1)
    _int_arg(max_history, "max_history", 0, 2 ** 64)
    for name, x in (("seed", seed), ("epoch", epoch), ("first_row", first_row)):
        _int_arg(x, name, 0, 2 ** 64)
    _one_dim(tensors)
    B = _equal_rows(tensors)
    if B * W >= 2 ** 31:
        raise ValueError("temporal_random_walk takes fewer than 2**31 walks per call, got "
                         "{} x {}".format(B, W))
    _same_device(tensors)
    return B, W, L


def _row_tensors(*xs):
    """The row tensors as a kernel reads them; the caller holds them until the launch."""
    return [x.detach().contiguous() for x in xs]


def _ptr(x):
    return None if x is None else x.data_ptr()


def _table(x, width):
    """(pointer, rows, width) of an optional table; width 0: it is not given."""
    return (x.data_ptr(), x.shape[0], width) if width else (None, 0, 0)


class HistoryReaders:
    """The edge-history readers of a graph over the C ABI, which DynamicGraph inherits; uses its
    self._lib, self._h and self._device.  Every reader checks its arguments, allocates its
    outputs and launches one kernel on the current stream."""

    def _check_on_device(self, dev):
        if dev.type != "cuda" or (dev.index is not None and dev.index != self._device):
            raise ValueError("the graph is on device cuda:{}, the inputs on {}".format(
                self._device, dev))
        return dev

    @staticmethod
    def _since_tensor(since, shape, dev):
        if since is None:
            return None
        if isinstance(since, torch.Tensor):
            return since.detach().contiguous()
        return torch.full(shape, float(since), dtype=torch.float32, device=dev)

    def _launch(self, fn, *args):
        """fn(graph, *args, device, the current stream), checked"""
        _capi.check(fn(self._h, *args, self._device,
                       _capi.current_stream(torch.device("cuda", self._device))))

    def seen_mask(self, src: torch.Tensor, ts: torch.Tensor, cand_ids: torch.Tensor,
                  max_history: int = 0) -> torch.Tensor:
        """Which of the candidates has each source already met: an int64 tensor [B, W],
        W = (C + 63) // 64, in which bit c % 64 of word [i, c // 64] is set iff one of the
        considered edges of src[i] leads to cand_ids[c].  The considered edges are the live edges
        of src[i] in the store whose timestamp is strictly below ts[i] (float <: a NaN time gives
        no bits) and, when max_history > 0, only the newest max_history of them.  "Strictly
        before" and "live" as for DeviceBatchStream's historical negatives: edges that
        offload_old_blocks took are gone, and on a graph built with reverse edges the history
        includes the nodes that pointed at the source.  Bits at positions >= C are 0; a source
        that is negative, past the node table or without live edges gives a zero row.

        src: int64 [B], ts: float32 [B], cand_ids: int64 [C] in any order, duplicates and ids
        unknown to the graph allowed; all on the graph's device.  B == 0 returns [0, W];
        C == 0 is a ValueError.  The result is ops.edge_rank's `exclude`
        (EdgePredictor.rank(..., exclude=)): recommendation without the nodes already known,
        filtered MRR / Hits@k.

        One sort of the candidates and one kernel (csrc/seen_mask.hip) on the current stream,
        memory from torch, never synchronises.  Edges added to the graph are seen by calls made
        after add_edges returns; add_edges and offload_old_blocks move and free segments:
        synchronise the streams that calls were launched on before calling either, as for
        DeviceBatchStream(hist_ratio=).

        The cost is proportional to the histories considered: a wave reads every considered edge
        of its row and looks it up among the sorted candidates, so a hub with 10^6 earlier edges
        is 10^6 record reads for its row.  max_history is what bounds it."""
        B, Cn = check_seen_mask_args(src, ts, cand_ids, max_history)
        dev = self._check_on_device(src.device)
        W = (Cn + 63) // 64
        with torch.cuda.device(self._device):
            mask = torch.zeros((B, W), dtype=torch.int64, device=dev)
            if B:
                sorted_ids, perm = torch.sort(cand_ids.detach())
                s, t = _row_tensors(src, ts)
                self._launch(self._lib.gf_graph_seen_mask, s.data_ptr(), t.data_ptr(), B,
                             sorted_ids.data_ptr(), perm.data_ptr(), Cn, max_history,
                             mask.data_ptr())
        return mask

    def pair_history(self, src: torch.Tensor, dst: torch.Tensor, ts: torch.Tensor, *,
                     since=None, max_history: int = 0) -> PairHistory:
        """Has each pair interacted before, how often, and when last:
        PairHistory(count int64 [N], last_ts float32 [N], last_eid int64 [N]).

        The considered edges of row i are the live edges of src[i] in the store whose timestamp
        is strictly below ts[i] (float <: a NaN time gives none) and, with `since`, not below
        since[i] -- the lower end is inclusive, and a NaN since[i] is no lower end -- and, when
        max_history > 0, only the newest max_history of that window (the bound comes after
        `since`).  count[i] is the number of them that lead to dst[i]; last_ts[i] and last_eid[i]
        are the timestamp and the edge id of the latest of those in the store's order, the first
        match in get_temporal_neighbors' newest-first list, so that equal timestamps are told
        apart; -inf and -1 where count[i] == 0.  "Strictly before" and "live" as for seen_mask:
        edges that offload_old_blocks took are gone, and on a graph built with reverse edges the
        history includes the edges that pointed at the source.  Any dst is legal (negative,
        unknown to the graph) and matches nothing; a source that is negative, past the node table
        or without live edges gives (0, -inf, -1).  The exact rule is in include/gnnflow_hip.h
        (gf_graph_pair_history), the window in csrc/history_window.hpp, and it is restated in
        numpy in tests/pair_history_ref.py.

        src, dst: int64 [N], ts: float32 [N]; since: None, a float (the same lower end for every
        row) or a float32 tensor [N]; all tensors on the graph's device.  N == 0 returns three
        empty tensors without a launch.  These are EdgeBank's inputs (gnnflow_amd.EdgeBank) and
        the usual pair features: times seen, time since the last contact, the last edge's id.

        One kernel (csrc/pair_history.hip, a wave per row) on the current stream, memory from
        torch, never synchronises.  Edges added to the graph are seen by calls made after
        add_edges returns; add_edges and offload_old_blocks move and free segments: synchronise
        the streams that calls were launched on before calling either, as for seen_mask.

        The cost is proportional to the edges considered: a wave reads every considered edge of
        its row, so a hub with 10^6 earlier edges is 10^6 record reads for each of its rows.
        max_history and since are what bound it."""
        N = check_pair_history_args(src, dst, ts, since, max_history)
        dev = self._check_on_device(src.device)
        with torch.cuda.device(self._device):
            count = torch.empty(N, dtype=torch.int64, device=dev)
            last_ts = torch.empty(N, dtype=torch.float32, device=dev)
            last_eid = torch.empty(N, dtype=torch.int64, device=dev)
            if N:
                s, d, t = _row_tensors(src, dst, ts)
                lo = self._since_tensor(since, (N,), dev)
                self._launch(self._lib.gf_graph_pair_history, s.data_ptr(), d.data_ptr(),
                             t.data_ptr(), _ptr(lo), N, max_history, count.data_ptr(),
                             last_ts.data_ptr(), last_eid.data_ptr())
        return PairHistory(count, last_ts, last_eid)

    def common_neighbors(self, src: torch.Tensor, dst: torch.Tensor, ts: torch.Tensor, *,
                         since=None, max_history: int = 64,
                         max_common: int = 32) -> CommonNeighbors:
        """Which nodes have both ends of each pair met before the row's time:
        CommonNeighbors(n_src, n_dst, u_src, u_dst, common int32 [N]; nodes int64 [N, K];
        cnt_src, cnt_dst int32 [N, K]), K = max_common.

        The considered edges of a node are pair_history's: its live edges in the store whose
        timestamp is strictly below ts[i] (float <: a NaN time gives none) and, with `since`, not
        below since[i] -- the lower end is inclusive, a NaN since[i] is no lower end -- and of
        that window only the newest max_history.  max_history is required here, 1 .. 512: it
        bounds the table a row is intersected in.  A is that set for src[i], B for dst[i], both
        at the same time and lower end.  An edge whose stored destination is negative counts as
        an edge but is nobody's neighbour.

        - n_src, n_dst: the edges in A and in B, multi-edges counted.
        - u_src, u_dst: the distinct neighbours in A and in B.
        - common: the neighbours in both, not capped by max_common; the union is
          u_src + u_dst - common.
        - nodes[i]: the common neighbours, the one src[i] met most recently first (by the latest
          position in A that leads to it), the first min(common[i], K) of them, then -1.
        - cnt_src[i, k], cnt_dst[i, k]: how many edges of A and of B lead to nodes[i, k]; what
          pair_history(src, nodes[:, k], ...).count gives under the same window.  0 in the padding.

        src[i] == dst[i] is legal: every neighbour is then common.  The endpoints themselves are
        NOT removed from the sets: on a graph built with reverse edges a pair that has interacted
        has dst[i] among src[i]'s neighbours (and the other way round), and dst[i] is a common
        neighbour if it also has a loop.  A node that is negative, past the node table or without
        live edges has no considered edge.  "Strictly before" and "live" as for seen_mask.  The
        exact rule is in include/gnnflow_hip.h (gf_graph_common_neighbors), the window in
        csrc/history_window.hpp, and it is restated in numpy in tests/common_neighbors_ref.py.

        src, dst: int64 [N], ts: float32 [N]; since: None, a float or a float32 tensor [N]; all
        tensors on the graph's device; 0 <= max_common <= 512.  N == 0 returns empty tensors of
        these shapes without a launch; a graph without nodes gives zeros and -1.

        One kernel (csrc/common_neighbors.hip: a row's two windows hashed into a table in LDS,
        integers only, the same inputs give the same bits) on the current stream, memory from
        torch, never synchronises.  Synchronise the streams that calls were launched on before
        add_edges or offload_old_blocks, as for seen_mask.  The cost is the 2 * max_history
        records read per row."""
        N, H, K = check_common_neighbors_args(src, dst, ts, since, max_history, max_common)
        dev = self._check_on_device(src.device)
        with torch.cuda.device(self._device):
            n_src, n_dst, u_src, u_dst, common = (
                torch.empty(N, dtype=torch.int32, device=dev) for _ in range(5))
            nodes = torch.empty((N, K), dtype=torch.int64, device=dev)
            cnt_src = torch.empty((N, K), dtype=torch.int32, device=dev)
            cnt_dst = torch.empty((N, K), dtype=torch.int32, device=dev)
            if N:
                s, d, t = _row_tensors(src, dst, ts)
                lo = self._since_tensor(since, (N,), dev)
                self._launch(self._lib.gf_graph_common_neighbors, s.data_ptr(), d.data_ptr(),
                             t.data_ptr(), _ptr(lo), N, H, K, n_src.data_ptr(), n_dst.data_ptr(),
                             u_src.data_ptr(), u_dst.data_ptr(), common.data_ptr(),
                             *(_ptr(x if K else None) for x in (nodes, cnt_src, cnt_dst)))
        return CommonNeighbors(n_src, n_dst, u_src, u_dst, common, nodes, cnt_src, cnt_dst)

    def temporal_degree(self, nodes: torch.Tensor, ts: torch.Tensor, *,
                        since=None) -> torch.Tensor:
        """int64 of nodes' shape: the number of live edges of nodes[...] whose timestamp is
        strictly below ts[...] and, with `since`, not below since[...] -- common_neighbors'
        window without max_history.  A node that is negative (the -1 padding of
        CommonNeighbors.nodes), past the node table or without live edges gives 0, so padded
        lists need no mask.

        nodes: int64 of any shape, ts: float32 of the same shape; since: None, a float or a
        float32 tensor of that shape; all on the graph's device.  One kernel, a lane per element,
        on the current stream; never synchronises; an empty `nodes` launches nothing."""
        n = check_temporal_degree_args(nodes, ts, since)
        dev = self._check_on_device(nodes.device)
        with torch.cuda.device(self._device):
            out = torch.empty(nodes.shape, dtype=torch.int64, device=dev)
            if n:
                v, t = _row_tensors(nodes, ts)
                lo = self._since_tensor(since, nodes.shape, dev)
                self._launch(self._lib.gf_graph_temporal_degree, v.data_ptr(), t.data_ptr(),
                             _ptr(lo), n, out.data_ptr())
        return out

    def neighbor_cooccurrence(self, src: torch.Tensor, dst: torch.Tensor, ts: torch.Tensor, *,
                              since=None, length: int = 32,
                              include_self: bool = True) -> NeighborCooccurrence:
        """The pair inputs of the sequence-based temporal models (DyGFormer, GraphMixer):
        NeighborCooccurrence(lengths int32 [N, 2]; nodes, eids int64 [N, 2, L]; times float32
        [N, 2, L]; counts int32 [N, 2, L, 2]), L = length.  Side 0 is src[i]'s sequence, side 1
        dst[i]'s.

        The sequence of a node is, with include_self, the node itself and then its considered
        edges, oldest first.  The considered edges are common_neighbors': the node's live edges
        in the store whose timestamp is strictly below ts[i] (float <: a NaN time gives none)
        and, with `since`, not below since[i] -- the lower end is inclusive, a NaN since[i] is no
        lower end -- and of that window only the newest H = length - include_self, so that a
        side never has more than `length` elements.  Both sides are taken at the same time and
        lower end.

        - lengths[i, side]: the filled slots, the self slot included.
        - nodes[i, side]: the node itself (with include_self), then the destinations of its
          considered edges, then -1.
        - eids[i, side], times[i, side]: the edges' ids and timestamps, bits copied; the self slot
          has eid -1 and time ts[i]; the padding has -1 and 0.  ts[i, None, None] - times is
          the models' time delta.
        - counts[i, side, p, 0], counts[i, side, p, 1]: how often nodes[i, side, p] occurs in
          src[i]'s sequence and how often in dst[i]'s -- channel 0 is "in src's sequence" on both
          sides, as DyGFormer's padded node appearances.  0, 0 in the padding.

        The self slot is present whatever the node is (negative, unknown to the graph, without
        edges) and counts as one occurrence of the node.  A negative id, the self slot's or a
        stored destination's, is nobody's neighbour: it is not counted and its own counts are
        0, 0; `lengths` tells it apart from the padding.  src[i] == dst[i] is legal: both sides
        are then equal.  "Strictly before" and "live" as for seen_mask: edges that
        offload_old_blocks took are gone, and on a graph built with reverse edges a node's
        sequence also holds the nodes that pointed at it.  The exact rule is in
        include/gnnflow_hip.h (gf_graph_neighbor_cooccurrence), the window in
        csrc/history_window.hpp, and it is restated in numpy in
        tests/neighbor_cooccurrence_ref.py.

        src, dst: int64 [N], ts: float32 [N]; since: None, a float or a float32 tensor [N]; all
        tensors on the graph's device; include_self a bool; 1 + include_self <= length <= 512.
        N == 0 returns empty tensors of these shapes without a launch; a graph without nodes
        gives the self slots alone.  nn.NeighborCooccurrenceEncoder turns the counts into
        features.

        One kernel (csrc/neighbor_cooccurrence.hip: a row's two sequences hashed into a table
        in LDS, integers only, the same inputs give the same bits) on the current stream, memory
        from torch, never synchronises.  Synchronise the streams that calls were launched on
        before add_edges or offload_old_blocks, as for seen_mask.  The cost is the 2 * H records
        read per row and the 2 * length * 32 bytes written."""
        N, L, self_slot = check_neighbor_cooccurrence_args(src, dst, ts, since, length,
                                                           include_self)
        dev = self._check_on_device(src.device)
        with torch.cuda.device(self._device):
            lengths = torch.empty((N, 2), dtype=torch.int32, device=dev)
            nodes = torch.empty((N, 2, L), dtype=torch.int64, device=dev)
            eids = torch.empty((N, 2, L), dtype=torch.int64, device=dev)
            times = torch.empty((N, 2, L), dtype=torch.float32, device=dev)
            counts = torch.empty((N, 2, L, 2), dtype=torch.int32, device=dev)
            if N:
                s, d, t = _row_tensors(src, dst, ts)
                lo = self._since_tensor(since, (N,), dev)
                self._launch(self._lib.gf_graph_neighbor_cooccurrence, s.data_ptr(),
                             d.data_ptr(), t.data_ptr(), _ptr(lo), N, L, self_slot,
                             lengths.data_ptr(), nodes.data_ptr(), eids.data_ptr(),
                             times.data_ptr(), counts.data_ptr())
        return NeighborCooccurrence(lengths, nodes, eids, times, counts)

    def neighbor_aggregate(self, nodes: torch.Tensor, ts: torch.Tensor, *,
                           node_feats: Optional[torch.Tensor] = None,
                           edge_feats: Optional[torch.Tensor] = None, since=None,
                           max_history: int = 0, reduce: str = "mean") -> NeighborAggregate:
        """The features of what each node met before the row's time, summed or averaged over
        its history window: NeighborAggregate(count int64 [N], node float32 [N, dn] or None,
        edge float32 [N, de] or None).  GraphMixer's node encoder input (models.GraphMixer:
        node_x + the mean of the features of the nodes met) and windowed mean pooling.

        The considered edges of row i are pair_history's: the live edges of nodes[i] in the store
        whose timestamp is strictly below ts[i] (float <: a NaN time gives none) and, with
        `since`, not below since[i] -- the lower end is inclusive, a NaN since[i] is no lower end
        -- and, when max_history > 0, only the newest max_history of that window (the bound comes
        after `since`).  count[i] is their number n.  node[i] reduces node_feats[dst] over their
        destinations and edge[i] reduces edge_feats[eid] over their edge ids, in the store's
        order, oldest first: reduce="sum" is the float32 sum in that order starting from +0.0,
        reduce="mean" that sum divided once by float(n) (a correctly rounded division), zeros
        where n == 0.  An id without a row in its table (negative, or at or past the table's
        number of rows) contributes a zero row and still counts in n, the rule
        Memory.prepare_input uses for unknown ids.  A node that is negative, past the node table
        or without live edges gives count 0 and zero rows.  "Strictly before" and "live" as for
        seen_mask: edges that offload_old_blocks took are gone, and on a graph built with reverse
        edges the window also holds the edges that pointed at the node.  The exact rule is in
        include/gnnflow_hip.h (gf_graph_neighbor_aggregate), the window in
        csrc/history_window.hpp, and it is restated in numpy in tests/neighbor_aggregate_ref.py:
        the result is that sequential loop's, bit for bit, and the same from run to run.

        nodes: int64 [N], ts: float32 [N]; since: None, a float or a float32 tensor [N];
        node_feats, edge_feats: float32 [rows, 1 .. 1024], at least one of them, contiguous (a
        non-contiguous table is a ValueError, not a silent copy of what may be gigabytes); all
        tensors on the graph's device.  The tables are detached: no gradient flows to them, and
        the outputs do not require grad.  The output of a table that is not given is None.
        N == 0 returns empty tensors of these shapes without a launch.

        One kernel (csrc/neighbor_aggregate.hip: a wave per row, the lanes own columns, no
        [N, H, d] intermediate) on the current stream, memory from torch, never synchronises.
        Edges added to the graph are seen by calls made after add_edges returns; add_edges and
        offload_old_blocks move and free segments: synchronise the streams that calls were
        launched on before calling either, as for seen_mask.

        The cost is proportional to the edges considered: a row's window is walked by one wave,
        which reads one table row per considered edge, so a hub with 10^6 earlier edges is 10^6
        row reads for each of its rows.  max_history and since are what bound it."""
        N, dn, de = check_neighbor_aggregate_args(nodes, ts, node_feats, edge_feats, since,
                                                  max_history, reduce)
        dev = self._check_on_device(nodes.device)
        with torch.cuda.device(self._device):
            count = torch.empty(N, dtype=torch.int64, device=dev)
            node = torch.empty((N, dn), dtype=torch.float32, device=dev) if dn else None
            edge = torch.empty((N, de), dtype=torch.float32, device=dev) if de else None
            if N:
                v, t = _row_tensors(nodes, ts)
                lo = self._since_tensor(since, (N,), dev)
                self._launch(self._lib.gf_graph_neighbor_aggregate, v.data_ptr(), t.data_ptr(),
                             _ptr(lo), N, max_history, *_table(node_feats, dn),
                             *_table(edge_feats, de), 1 if reduce == "mean" else 0,
                             count.data_ptr(), _ptr(node), _ptr(edge))
        return NeighborAggregate(count, node, edge)

    def neighbor_sequence(self, nodes: torch.Tensor, ts: torch.Tensor, *, since=None,
                          length: int = 32, edge_feats: Optional[torch.Tensor] = None,
                          node_feats: Optional[torch.Tensor] = None,
                          time_encoder=None) -> NeighborSequence:
        """Each node's newest interactions before the row's time as one padded sequence, and
        optionally the finished tokens of a sequence model: NeighborSequence(lengths int32 [N];
        nodes, eids int64 [N, L]; times, delta_t float32 [N, L]; tokens float32
        [N, L, de + dn + dT] or None), L = length.  The per-node reader of GraphMixer's link
        encoder (models.GraphMixer.forward_tokens) and of DyGFormer- or TCL-style models, where
        neighbor_cooccurrence reads the two ends of a pair.

        The window of row i is pair_history's: the live edges of nodes[i] in the store whose
        timestamp is strictly below ts[i] (float <: a NaN time gives none) and, with `since`, not
        below since[i] -- the lower end is inclusive, a NaN since[i] is no lower end -- and of
        those the newest `length`, oldest first.  lengths[i] = n is their number.

        - For p < n: nodes[i, p], eids[i, p] and times[i, p] are the edge's destination, id and
          timestamp (bits copied), delta_t[i, p] = ts[i] - times[i, p], one float32 subtraction.
        - For p >= n, the padding: -1, -1, 0, 0 -- neighbor_cooccurrence's convention, whose
          side 0 with include_self=False the first four outputs equal element for element.
        - tokens[i, p] = [edge_feats[eid] | node_feats[dst] | cos(w * delta_t[i, p] + b)] for
          p < n.  The table parts are copies of the rows, bit for bit; an id without a row in
          its table (negative, or at or past its number of rows) gives a zero part,
          neighbor_aggregate's rule.  The time part is ops.time_encode's expression evaluated by
          the same code: it equals ops.time_encode(delta_t.reshape(-1), weight, bias) bit for
          bit.  Every element of a padded slot is +0.0, the time part too: what
          masked_fill(padding, 0.0) leaves.  tokens is None when no part is given.

        A node that is negative, past the node table or without live edges gives an all-padding
        row.  "Strictly before" and "live" as for seen_mask: edges that offload_old_blocks took
        are gone, and on a graph built with reverse edges the window also holds the edges that
        pointed at the node.  The exact rule is in include/gnnflow_hip.h
        (gf_graph_neighbor_sequence), the window in csrc/history_window.hpp, and it is restated
        in numpy in tests/neighbor_sequence_ref.py.

        nodes: int64 [N], ts: float32 [N]; since: None, a float or a float32 tensor [N];
        1 <= length <= 512; edge_feats, node_feats: float32 [rows, 1 .. 1024], contiguous (a
        non-contiguous table is a ValueError, not a silent copy of what may be gigabytes; a
        float16 or bfloat16 table is a TypeError); time_encoder: a module that holds `weight`
        [dT, 1] and `bias` [dT] (nn.FixedTimeEncode, nn.TimeEncode) or a (weight, bias) pair,
        float32, 1 <= dT <= 1024; all tensors on the graph's device.  The tables and the
        encoder are read detached: no gradient flows to them or to ts, and the outputs do not
        require grad.  N == 0 returns empty tensors of these shapes without a launch.

        One kernel (csrc/neighbor_sequence.hip: a wave per row, the lanes spread over the
        row's positions and over the flattened (position, column) space of its tokens; the same
        inputs give the same bits) on the current stream, memory from torch, never
        synchronises.  Synchronise the streams that calls were launched on before add_edges or
        offload_old_blocks, as for seen_mask.  The cost is the `length` records and table rows
        read per row and the length * (24 + 4 * width) bytes written."""
        N, L, de, dn, dT = check_neighbor_sequence_args(nodes, ts, since, length, edge_feats,
                                                        node_feats, time_encoder)
        dev = self._check_on_device(nodes.device)
        width = de + dn + dT
        with torch.cuda.device(self._device):
            lengths = torch.empty(N, dtype=torch.int32, device=dev)
            out_nodes = torch.empty((N, L), dtype=torch.int64, device=dev)
            eids = torch.empty((N, L), dtype=torch.int64, device=dev)
            times = torch.empty((N, L), dtype=torch.float32, device=dev)
            delta_t = torch.empty((N, L), dtype=torch.float32, device=dev)
            tokens = torch.empty((N, L, width), dtype=torch.float32,
                                 device=dev) if width else None
            if N:
                v, t = _row_tensors(nodes, ts)
                lo = self._since_tensor(since, (N,), dev)
                w, b = (x.detach().reshape(dT).contiguous()
                        for x in _encoder_tensors(time_encoder)) if dT else (None, None)
                self._launch(self._lib.gf_graph_neighbor_sequence, v.data_ptr(), t.data_ptr(),
                             _ptr(lo), N, L, *_table(edge_feats, de), *_table(node_feats, dn),
                             _ptr(w), _ptr(b), dT, lengths.data_ptr(), out_nodes.data_ptr(),
                             eids.data_ptr(), times.data_ptr(), delta_t.data_ptr(), _ptr(tokens))
        return NeighborSequence(lengths, out_nodes, eids, times, delta_t, tokens)

    def pair_sequence(self, src: torch.Tensor, dst: torch.Tensor, ts: torch.Tensor, *,
                      since=None, length: int = 32, node_feats: Optional[torch.Tensor] = None,
                      edge_feats: Optional[torch.Tensor] = None,
                      time_encoder=None) -> PairSequence:
        """Everything DyGFormer concatenates for a pair, finished, from one launch:
        PairSequence(lengths int32 [N, 2]; nodes, eids int64 [N, 2, L]; times, delta_t float32
        [N, 2, L]; counts int32 [N, 2, L, 2]; node float32 [N, 2, L, dn] or None; edge float32
        [N, 2, L, de] or None; time float32 [N, 2, L, dT] or None), L = length.  Side 0 is
        src[i]'s sequence, side 1 dst[i]'s.  The pair reader with features (models.DyGFormer.
        forward_graph), where neighbor_sequence is the per-node one.

        - lengths, nodes, eids, times and counts are neighbor_cooccurrence(src, dst, ts,
          since=since, length=L, include_self=True)'s, element for element and bit for bit: the
          self slot is always there (position 0, eid -1, time ts[i], counted), the window behind
          it is csrc/history_window.hpp's with the bound L - 1, oldest first, and the padding is
          -1, -1, 0, (0, 0).
        - delta_t[i, side, p] = ts[i] - times[i, side, p], one float32 subtraction on every
          filled slot, the self slot included (ts[i] - ts[i]); the padding holds +0.0.
        - node[i, side, p] = node_feats[nodes[i, side, p]] and edge[i, side, p] =
          edge_feats[eids[i, side, p]] on a filled slot: copies of the rows, bit for bit; an id
          without a row in its table (negative, or at or past its number of rows) gives zeros,
          neighbor_aggregate's rule.  The self slot therefore has the node's own row in `node`
          and a zero row in `edge`.
        - time[i, side, p] = cos(w * delta_t[i, side, p] + b) on a filled slot, ops.time_encode's
          expression evaluated by the same code: it equals ops.time_encode(delta_t.reshape(-1),
          weight, bias) bit for bit there.  The self slot is the encoding of its own delta_t,
          not zero.
        - Every element of a padded slot is +0.0 in all three parts: what masked_fill(padding,
          0.0) leaves.  A part that is not given is None.

        Each part is its own contiguous tensor, because DyGFormer patches and projects each
        channel on its own: part.reshape(N, 2, L // P, P * d) is a view.  src[i] == dst[i] is
        legal.  "Strictly before" and "live" as for seen_mask.  The exact rule is in
        include/gnnflow_hip.h (gf_graph_pair_sequence), and it is restated in numpy in
        tests/pair_sequence_ref.py.

        src, dst: int64 [N], ts: float32 [N]; since: None, a float or a float32 tensor [N];
        2 <= length <= 512; node_feats, edge_feats: float32 [rows, 1 .. 1024], contiguous (a
        non-contiguous table is a ValueError, not a silent copy of what may be gigabytes; a
        float16 or bfloat16 table is a TypeError); time_encoder: a module that holds `weight`
        [dT, 1] and `bias` [dT] (nn.FixedTimeEncode, nn.TimeEncode) or a (weight, bias) pair,
        float32, 1 <= dT <= 1024; all tensors on the graph's device.  The tables and the
        encoder are read detached: no gradient flows to them or to ts, and the outputs do not
        require grad.  N == 0 returns empty tensors of these shapes without a launch; a graph
        without nodes gives the self slots alone.

        One kernel (csrc/pair_sequence.hip: neighbor_cooccurrence's LDS table and phases, then
        the row's threads spread over the flattened (side, position, column) space of each
        part; the same inputs give the same bits) on the current stream, memory from torch,
        never synchronises.  Synchronise the streams that calls were launched on before
        add_edges or offload_old_blocks, as for seen_mask.  The cost is the 2 * (length - 1)
        records and table rows read per row and the 2 * length * (36 + 4 * (dn + de + dT))
        bytes written."""
        N, L, dn, de, dT = check_pair_sequence_args(src, dst, ts, since, length, node_feats,
                                                    edge_feats, time_encoder)
        dev = self._check_on_device(src.device)

        def part(width):
            return torch.empty((N, 2, L, width), dtype=torch.float32,
                               device=dev) if width else None

        with torch.cuda.device(self._device):
            lengths = torch.empty((N, 2), dtype=torch.int32, device=dev)
            nodes = torch.empty((N, 2, L), dtype=torch.int64, device=dev)
            eids = torch.empty((N, 2, L), dtype=torch.int64, device=dev)
            times = torch.empty((N, 2, L), dtype=torch.float32, device=dev)
            delta_t = torch.empty((N, 2, L), dtype=torch.float32, device=dev)
            counts = torch.empty((N, 2, L, 2), dtype=torch.int32, device=dev)
            node, edge, time = part(dn), part(de), part(dT)
            if N:
                s, d, t = _row_tensors(src, dst, ts)
                lo = self._since_tensor(since, (N,), dev)
                w, b = (x.detach().reshape(dT).contiguous()
                        for x in _encoder_tensors(time_encoder)) if dT else (None, None)
                self._launch(self._lib.gf_graph_pair_sequence, s.data_ptr(), d.data_ptr(),
                             t.data_ptr(), _ptr(lo), N, L, *_table(node_feats, dn),
                             *_table(edge_feats, de), _ptr(w), _ptr(b), dT, lengths.data_ptr(),
                             nodes.data_ptr(), eids.data_ptr(), times.data_ptr(),
                             delta_t.data_ptr(), counts.data_ptr(), _ptr(node), _ptr(edge),
                             _ptr(time))
        return PairSequence(lengths, nodes, eids, times, delta_t, counts, node, edge, time)

    def temporal_random_walk(self, src: torch.Tensor, ts: torch.Tensor, length: int,
                             num_walks: int = 1, *, recency: int = 1, max_history: int = 0,
                             seed: int = 0, epoch: int = 0, first_row: int = 0) -> TemporalWalks:
        """W = num_walks backward-in-time random walks of L = length steps from each root:
        TemporalWalks(nodes int64 [B, W, L + 1], eids int64 [B, W, L], times float32 [B, W, L]).

        Walk (i, w) starts at src[i] at time ts[i]; nodes[i, w, 0] = src[i] always.  A step goes
        from the current node v at the current time t over one of the considered edges of v: its
        live edges in the store whose timestamp is strictly below t (float <) and, when
        max_history > 0, only the newest max_history of them.  The step writes the edge's
        destination to nodes[i, w, j + 1], its id to eids[i, w, j] and its timestamp to
        times[i, w, j], which become the next v and t.  A walk ends where v is negative or past
        the node table or has no considered edge; every slot from that step on holds nodes = -1,
        eids = -1, times = 0.  The exact rule, draws included, is in include/gnnflow_hip.h
        (gf_graph_temporal_walks), the window in csrc/history_window.hpp, and it is restated in
        numpy in tests/temporal_walk_ref.py.

        - Time strictly decreases along a walk: no edge is taken twice, an edge at the current
          time (a tie) is never followed, and a NaN time ends the walk at once.
        - recency = 1 draws uniformly from the n considered edges.  recency = p (1 .. 8) takes
          the maximum of p uniform draws, P(index <= k) = ((k + 1) / n) ** p counted from the
          oldest: a power-law preference for recent edges.  Integer arithmetic only, so the
          kernel is checked bit for bit.
        - Draws are Philox words keyed by (seed, the root's global row first_row + i, w, epoch,
          step), not by the root's place in the call: walking rows [a, b) with first_row = a
          gives rows a .. b of walking everything; another seed or epoch gives other walks.  A
          seed tag of their own keeps them independent of DeviceBatchStream's draws.  The p
          draws of a step are keyed seed ^ (tag + a), a < p, so seeds that differ only in their
          low five bits can key the same draws: tell seeds apart above those bits.
        - "Live" and reverse edges as for seen_mask: edges that offload_old_blocks took are gone,
          and on a graph built with reverse edges a walk also follows edges that pointed at its
          node.

        src: int64 [B], ts: float32 [B], on the graph's device; 1 <= length <= 32,
        1 <= num_walks < 2**16, B * num_walks < 2**31, recency in 1 .. 8, max_history >= 0;
        seed, epoch and first_row in [0, 2**64).  B == 0 returns empty tensors of these shapes
        without a launch; a graph without nodes gives walks that all end on step 0.

        One kernel (csrc/temporal_walk.hip, a lane per walk) on the current stream, memory from
        torch, never synchronises.  Synchronise the streams that calls were launched on before
        add_edges or offload_old_blocks, as for seen_mask.  ops.walk_position_counts encodes the
        result for CAWN-style models."""
        B, W, L = check_temporal_walk_args(src, ts, length, num_walks, recency, max_history,
                                           seed, epoch, first_row)
        dev = self._check_on_device(src.device)
        with torch.cuda.device(self._device):
            nodes = torch.empty((B, W, L + 1), dtype=torch.int64, device=dev)
            eids = torch.empty((B, W, L), dtype=torch.int64, device=dev)
            times = torch.empty((B, W, L), dtype=torch.float32, device=dev)
            if B:
                s, t = _row_tensors(src, ts)
                self._launch(self._lib.gf_graph_temporal_walks, s.data_ptr(), t.data_ptr(), B,
                             W, L, int(recency), int(max_history), int(seed), int(epoch),
                             int(first_row), nodes.data_ptr(), eids.data_ptr(), times.data_ptr())
        return TemporalWalks(nodes, eids, times)
