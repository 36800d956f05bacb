"""Message passing on an MFGBlock: the DGL calls the reference's layers
make on a sampled block, on HIP segment kernels (csrc/block_ops.hip) with autograd.

    edge_softmax(block, logits)            dgl.ops.edge_softmax      (layers.py:153)
    block.update_all(fn.copy_src('v','m'), fn.sum('m','h'))          (layers.py:159)
    copy_u / u_mul_e messages, sum / mean reducers                   (dgl.nn.SAGEConv / GATConv)
    block_attention(block, q, k, v)        layers.py:144-159 in one launch (csrc/block_attention.hip)
      ... dropout_p=, dropout_seed=        with the attention dropout of layers.py:155 inside it, from a
                                           stateless Philox mask (no mask tensor, reproducible on the CPU)
    block_gat(block, feat, el, er)         dgl.nn.GATConv's u_add_v -> leaky_relu -> edge_softmax ->
                                           (attn_drop) -> u_mul_e + sum in one launch each way
                                           (csrc/block_gat.hip), the same dropout_p= / dropout_seed=
    time_encode_cat(parts, t, w, b)        torch.cat([*parts, TimeEncode(t)], 1) in one launch
                                           (layers.py:16-42, 118-137; csrc/time_encode.hip)
    edge_score(src, dst, w, b)             out_fc(relu(src + dst)) of EdgePredictor (layers.py:195-197),
                                           every dst block against the one src block, in one launch
                                           (csrc/edge_score.hip)
    dropout_relu_layer_norm(x, w, b)       layer_norm(relu(dropout(x))), the last line of
                                           TemporalAttentionLayer.forward after w_out, in one launch
                                           with the Philox mask of block_attention, redrawn in the
                                           backward (csrc/layer_epilogue.hip)
    gru_cell(gi, gh, hx, residual)         everything torch.nn.GRUCell does behind its two GEMMs, the
                                           residual add of the memory updater and the copy of the
                                           first rows for Memory.update_mem_mail
                                           (memory_updater.py:62-85), one launch each way without a
                                           workspace (csrc/gru_cell.hip)
    link_metrics(pos, neg)                 average_precision_score / roc_auc_score of the reference's
                                           evaluate() (scripts/offline_edge_prediction.py:141-146) and
                                           the MRR, counted on the GPU without a sort, a sync or a copy
                                           to the host (csrc/link_metrics.hip)
    link_loss(pos, neg)                    criterion(pred_pos, ones) + criterion(pred_neg, zeros) of the
                                           reference's training step (BCEWithLogitsLoss), one launch
                                           each way, with a running epoch sum on the device
                                           (csrc/link_loss.hip)
    edge_rank(src, cand, w, b, k, ...)     the edge score of every source against one shared candidate
                                           set, of which the top k and the rank counts of a reference
                                           score are kept and nothing else is stored
                                           (csrc/edge_rank.hip); no autograd
    walk_position_counts(nodes, ref)       the position-count ("anonymous") encoding of the walks
                                           DynamicGraph.temporal_random_walk returns, CAWN's
                                           set-based anonymisation (csrc/walk_positions.hip); integers,
                                           no autograd

block_attention, block_reduce, block_max, block_gat, time_encode_cat, edge_score, link_loss,
gru_cell and dropout_relu_layer_norm also run on bfloat16 (the tensors autocast hands them), by one rule: float32 arithmetic, one rounding on
store.  Every bfloat16 element is widened to float32 where it is loaded (exact), the arithmetic is
the float32 kernels' own in the same order, and each bfloat16 result is rounded once, to nearest
even.  So op(x.bfloat16()) == op(x.bfloat16().float()).to(torch.bfloat16) bit for bit, forward and
backward, and the float32 outputs (attention, scores, parameter gradients) are equal.  The ops
choose by the dtypes they are given and behave the same inside and outside an autocast region.
What may be bfloat16 is what autocast makes bfloat16, the rows a Linear returns: q / k / v, the
source rows of block_reduce and block_max, feat of block_gat.  What autocast leaves float32 stays
float32 only: edge weights (a softmax output), el and er (a float32 sum), and edge_softmax
altogether.  A gradient of a source may meet several edges (an explicit col): it is summed in a
float32 scratch and rounded once, never once per edge.

A block's edges are grouped by destination (the sampler emits them that way); blocks built by
hand with unordered edges are handled through a stable permutation.
"""
import ctypes as C
from typing import NamedTuple, Optional

import torch

from . import _capi
from .dynamic_graph import WALK_MAX_LENGTH


def _stream(device):
    return _capi.current_stream(device)


def _f32(t: torch.Tensor) -> torch.Tensor:
    if t.dtype != torch.float32:
        raise TypeError("block ops compute in float32, got {}".format(t.dtype))
    return t.contiguous()


def _ptr(t):
    return t.data_ptr() if t is not None and t.numel() else None


def _grad_as(grad: torch.Tensor, dtype) -> torch.Tensor:
    """The incoming gradient of an output of `dtype`, contiguous."""
    if grad.dtype != dtype:
        raise TypeError("the gradient of a {} output is {}".format(dtype, grad.dtype))
    return grad.contiguous()


# The autograd Functions of the ops that take bfloat16 call no torch op that autocast would
# recast, and custom_fwd / custom_bwd without cast_inputs keep it that way: the forward sees the
# tensors as they are given, the backward runs under the forward's autocast state wherever
# loss.backward() is called.
_fwd = torch.amp.custom_fwd(device_type="cuda")
_bwd = torch.amp.custom_bwd(device_type="cuda")


class _EdgeSoftmax(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, offsets, num_dst):
        x = _f32(logits)
        E = x.shape[0]
        heads = x.numel() // E if E else 0
        y = torch.empty_like(x)
        if E:
            with torch.cuda.device(x.device):
                _capi.check(_capi.load().gf_block_edge_softmax(
                    offsets.data_ptr(), num_dst, E, heads, x.data_ptr(), y.data_ptr(),
                    x.device.index, _stream(x.device)))
        ctx.save_for_backward(y, offsets)
        ctx.num_dst = num_dst
        return y

    @staticmethod
    def backward(ctx, grad):
        y, offsets = ctx.saved_tensors
        g = _f32(grad)
        E = y.shape[0]
        gx = torch.empty_like(y)
        if E:
            with torch.cuda.device(y.device):
                _capi.check(_capi.load().gf_block_edge_softmax_backward(
                    offsets.data_ptr(), ctx.num_dst, E, y.numel() // E, y.data_ptr(),
                    g.data_ptr(), gx.data_ptr(), y.device.index, _stream(y.device)))
        return gx, None, None


def _scratch(t, col, wanted=True):
    """The float32 buffer a bfloat16 gradient of `t`'s shape is summed in when the block has an
    explicit col; None for float32, for the sampler's layout, or when it is not wanted."""
    if t.dtype != torch.bfloat16 or col is None or not wanted:
        return None
    return torch.empty(t.shape, dtype=torch.float32, device=t.device)


class _BlockReduce(torch.autograd.Function):
    @staticmethod
    @_fwd
    def forward(ctx, src, weight, offsets, col, num_dst, mean, num_edges):
        # col is None for the sampler's layout (source of edge k = row num_dst + k); src fp32 or
        # bf16 (checked by block_reduce), weight fp32; out in src's dtype
        s = src.contiguous()
        num_src = s.shape[0]
        dim = s.numel() // num_src if num_src else 0
        w, heads = None, 1
        if weight is not None:
            w = _f32(weight)
            E = w.shape[0]
            heads = w.numel() // E if E else 1
            if dim % max(heads, 1):
                raise ValueError("feature size {} is not a multiple of the {} edge-weight heads"
                                 .format(dim, heads))
        out = torch.zeros((num_dst,) + tuple(s.shape[1:]), dtype=s.dtype, device=s.device)
        if num_dst and dim and num_edges:
            lib = _capi.load()
            fn = lib.gf_block_reduce_bf16 if s.dtype == torch.bfloat16 else lib.gf_block_reduce
            with torch.cuda.device(s.device):
                _capi.check(fn(
                    offsets.data_ptr(), num_dst, _ptr(col), s.data_ptr(), dim, _ptr(w), heads,
                    1 if mean else 0, out.data_ptr(), s.device.index, _stream(s.device)))
        ctx.save_for_backward(s, w, offsets, col)
        ctx.meta = (num_dst, mean, heads, dim, num_edges)
        return out

    @staticmethod
    @_bwd
    def backward(ctx, grad):
        s, w, offsets, col = ctx.saved_tensors
        num_dst, mean, heads, dim, num_edges = ctx.meta
        g = _grad_as(grad, s.dtype)
        need_src, need_w = ctx.needs_input_grad[0], w is not None and ctx.needs_input_grad[1]
        gs = torch.empty_like(s) if need_src else None
        gw = torch.zeros_like(w) if need_w else None
        if (need_src or need_w) and dim:
            if num_edges == 0 or num_dst == 0:
                if gs is not None:
                    gs.zero_()
            else:
                lib = _capi.load()
                args = (offsets.data_ptr(), num_dst, _ptr(col), s.data_ptr(), dim, _ptr(w),
                        heads, 1 if mean else 0, g.data_ptr(), _ptr(gs), s.shape[0], _ptr(gw),
                        s.device.index, _stream(s.device))
                with torch.cuda.device(s.device):
                    if s.dtype == torch.bfloat16:
                        _capi.check(lib.gf_block_reduce_backward_bf16(
                            *args, _ptr(_scratch(s, col, need_src))))
                    else:
                        _capi.check(lib.gf_block_reduce_backward(*args))
        return gs, gw, None, None, None, None, None


class _BlockMax(torch.autograd.Function):
    @staticmethod
    @_fwd
    def forward(ctx, src, offsets, col, num_dst, num_edges):
        s = src.contiguous()      # fp32 or bf16 (checked by block_max); out in its dtype
        num_src = s.shape[0]
        dim = s.numel() // num_src if num_src else 0
        out = torch.zeros((num_dst,) + tuple(s.shape[1:]), dtype=s.dtype, device=s.device)
        arg = torch.full((num_dst, max(dim, 1)), -1, dtype=torch.int64, device=s.device)
        if num_dst and dim and num_edges:
            lib = _capi.load()
            fn = lib.gf_block_reduce_max_bf16 if s.dtype == torch.bfloat16 \
                else lib.gf_block_reduce_max
            with torch.cuda.device(s.device):
                _capi.check(fn(
                    offsets.data_ptr(), num_dst, _ptr(col), s.data_ptr(), dim, out.data_ptr(),
                    arg.data_ptr(), s.device.index, _stream(s.device)))
        ctx.save_for_backward(arg, col)
        ctx.meta = (num_dst, dim, tuple(s.shape), s.dtype)
        ctx.mark_non_differentiable(arg)
        return out

    @staticmethod
    @_bwd
    def backward(ctx, grad):
        arg, col = ctx.saved_tensors
        num_dst, dim, shape, dtype = ctx.meta
        g = _grad_as(grad, dtype)
        gs = torch.empty(shape, dtype=dtype, device=g.device)
        lib = _capi.load()
        args = (num_dst, _ptr(col), dim, _ptr(g), arg.data_ptr(), gs.data_ptr(), shape[0],
                g.device.index, _stream(g.device))
        with torch.cuda.device(g.device):
            if dtype == torch.bfloat16:
                _capi.check(lib.gf_block_reduce_max_backward_bf16(*args, _ptr(_scratch(gs, col))))
            else:
                _capi.check(lib.gf_block_reduce_max_backward(*args))
        return gs, None, None, None, None


MAX_ATTENTION_WIDTH = 1024      # GF_BLOCK_ATTENTION_MAX_WIDTH: the limit on heads * head_dim


class _BlockAttention(torch.autograd.Function):
    @staticmethod
    @_fwd
    def forward(ctx, q, k, v, offsets, num_dst, slope):
        # q [num_dst, H, D], k / v [E, H, D] contiguous, all fp32 or all bf16, edges grouped by
        # destination; out in their dtype, att fp32
        E, H, D = k.shape
        out = torch.empty((num_dst, H, D), dtype=q.dtype, device=q.device)
        att = torch.empty((E, H), dtype=torch.float32, device=q.device)
        lib = _capi.load()
        fn = lib.gf_block_attention_bf16 if q.dtype == torch.bfloat16 else lib.gf_block_attention
        with torch.cuda.device(q.device):
            _capi.check(fn(
                offsets.data_ptr(), num_dst, E, H, D, q.data_ptr(), k.data_ptr(), v.data_ptr(),
                slope, out.data_ptr(), att.data_ptr(), q.device.index, _stream(q.device)))
        ctx.save_for_backward(q, k, v, att, offsets)
        ctx.slope = slope
        ctx.mark_non_differentiable(att)
        return out, att

    @staticmethod
    @_bwd
    def backward(ctx, grad, _grad_att):
        q, k, v, att, offsets = ctx.saved_tensors
        g = _grad_as(grad, q.dtype)
        E, H, D = k.shape
        need_q, need_k, need_v = ctx.needs_input_grad[:3]
        gq = torch.empty_like(q) if need_q else None
        gk = torch.empty_like(k) if need_k else None
        gv = torch.empty_like(v) if need_v else None
        if need_q or need_k or need_v:
            lib = _capi.load()
            fn = lib.gf_block_attention_bf16_backward if q.dtype == torch.bfloat16 \
                else lib.gf_block_attention_backward
            with torch.cuda.device(q.device):
                _capi.check(fn(
                    offsets.data_ptr(), q.shape[0], E, H, D, q.data_ptr(), k.data_ptr(),
                    v.data_ptr(), att.data_ptr(), ctx.slope, g.data_ptr(), _ptr(gq), _ptr(gk),
                    _ptr(gv), q.device.index, _stream(q.device)))
        return gq, gk, gv, None, None, None


class _BlockAttentionDropout(torch.autograd.Function):
    @staticmethod
    @_fwd
    def forward(ctx, q, k, v, offsets, num_dst, slope, p, seed, want_dropped):
        # as _BlockAttention; att is the pre-dropout softmax (saved), dropped = att * w, both fp32
        E, H, D = k.shape
        out = torch.empty((num_dst, H, D), dtype=q.dtype, device=q.device)
        att = torch.empty((E, H), dtype=torch.float32, device=q.device)
        dropped = torch.empty_like(att) if want_dropped else None
        lib = _capi.load()
        fn = lib.gf_block_attention_dropout_bf16 if q.dtype == torch.bfloat16 \
            else lib.gf_block_attention_dropout
        with torch.cuda.device(q.device):
            _capi.check(fn(
                offsets.data_ptr(), num_dst, E, H, D, q.data_ptr(), k.data_ptr(), v.data_ptr(),
                slope, p, seed, out.data_ptr(), att.data_ptr(), _ptr(dropped), q.device.index,
                _stream(q.device)))
        ctx.save_for_backward(q, k, v, att, offsets)
        ctx.meta = (slope, p, seed)
        if dropped is None:
            return out, None
        ctx.mark_non_differentiable(dropped)
        return out, dropped

    @staticmethod
    @_bwd
    def backward(ctx, grad, _grad_dropped):
        q, k, v, att, offsets = ctx.saved_tensors
        slope, p, seed = ctx.meta
        g = _grad_as(grad, q.dtype)
        E, H, D = k.shape
        need_q, need_k, need_v = ctx.needs_input_grad[:3]
        gq = torch.empty_like(q) if need_q else None
        gk = torch.empty_like(k) if need_k else None
        gv = torch.empty_like(v) if need_v else None
        if need_q or need_k or need_v:
            lib = _capi.load()
            fn = lib.gf_block_attention_dropout_bf16_backward if q.dtype == torch.bfloat16 \
                else lib.gf_block_attention_dropout_backward
            with torch.cuda.device(q.device):
                _capi.check(fn(
                    offsets.data_ptr(), q.shape[0], E, H, D, q.data_ptr(), k.data_ptr(),
                    v.data_ptr(), att.data_ptr(), slope, p, seed, g.data_ptr(), _ptr(gq),
                    _ptr(gk), _ptr(gv), q.device.index, _stream(q.device)))
        return gq, gk, gv, None, None, None, None, None, None


class _NoEdgeAttention(torch.autograd.Function):
    """A block without edges or without destinations: zeros, and zero gradients."""
    @staticmethod
    def forward(ctx, q, k, v):
        ctx.save_for_backward(q, k, v)
        return torch.zeros_like(q)

    @staticmethod
    def backward(ctx, grad):
        return tuple(torch.zeros_like(t) if need else None
                     for t, need in zip(ctx.saved_tensors, ctx.needs_input_grad))


def block_attention(block, q: torch.Tensor, k: torch.Tensor, v: torch.Tensor,
                    negative_slope: float = 0.2, return_attention: bool = False, heads=None,
                    dropout_p: float = 0.0, dropout_seed: Optional[int] = None):
    """The attention of the reference's TransfomerAttentionLayer (layers.py:144-159) with
    per-edge keys and values, in one kernel each way:

        att[e, h] = edge_softmax(leaky_relu(sum_c q[row[e], h, c] * k[e, h, c], negative_slope))
        out[d, h] = sum over the edges e into d of att[e, h] * v[e, h]      (0 without in-edges)

    q: [num_dst_nodes, H, D]; k, v: [num_edges, H, D], all three float32 or all three bfloat16
    (anything else, a mixture included, raises TypeError).  bfloat16 follows the module's rule --
    float32 arithmetic, one rounding on store --: out and the gradients are bfloat16 and equal,
    bit for bit, the float32 op's results on q.float(), k.float(), v.float() rounded to bfloat16;
    the attention that return_attention=True gives stays float32 and is equal to the float32
    op's.  The inputs are 3-D; a 2-D
    [rows, H * D] input is accepted only together with `heads=H`.  H * D is at most
    MAX_ATTENTION_WIDTH.  Returns out [num_dst_nodes, H, D], and with return_attention=True
    also att [num_edges, H] in the caller's edge order (not differentiable).

    dropout_p > 0 drops attention weights after the softmax (the reference's att_dropout,
    layers.py:155) inside the same kernels, from a stateless mask that is never stored and that
    the backward draws again.  With p = float32(dropout_p), 0 <= p < 1, and i the position of an
    edge in the GROUPED order the kernel sees -- the order of block.segments(): the caller's
    order for a sampler block, the stable sort by destination (`perm`) for an unordered one --

        T          = uint32(float64(p) * 2**32)
        keep[i, h] = gf_philox4x32_10_first(dropout_seed, i * H + h, 0) >= T   (gnnflow_rng.h)
        w[i, h]    = float32(1) / (float32(1) - p) if keep[i, h] else 0
        out[d, h]  = sum over the edges i into d of (att[i, h] * w[i, h]) * v[i, h]

    dropout_seed (0 <= seed < 2**64) is required when dropout_p > 0; the same seed gives the
    same mask and the same bits.  return_attention=True then returns the DROPPED attention
    att * w, the weights that multiplied v (caller's edge order, not differentiable).  A dropped
    edge contributes exactly 0 and its v row is not read: a non-finite v on a dropped edge does
    not propagate, unlike 0 * inf in the composed edge_softmax -> dropout -> block_reduce chain.
    dropout_p == 0 is the call without the two arguments, bit for bit."""
    dropout_p = float(dropout_p)
    if not 0.0 <= dropout_p < 1.0:          # NaN fails too
        raise ValueError("dropout_p must be in [0, 1), got {}".format(dropout_p))
    p32 = C.c_float(dropout_p).value        # the fp32 value the kernels see
    if p32 >= 1.0:
        raise ValueError("dropout_p rounds to 1 in float32")
    if dropout_seed is not None:
        dropout_seed = int(dropout_seed)
        if not 0 <= dropout_seed < 2 ** 64:
            raise ValueError("dropout_seed must be in [0, 2**64), got {}".format(dropout_seed))
    elif dropout_p > 0:
        raise ValueError("dropout_p > 0 needs a dropout_seed")
    num_dst, E = block.num_dst_nodes(), block.num_edges()
    dtypes = (q.dtype, k.dtype, v.dtype)
    if dtypes not in ((torch.float32,) * 3, (torch.bfloat16,) * 3):
        raise TypeError("block_attention takes q, k and v all float32 or all bfloat16 (block ops "
                        "compute in float32), got {}, {} and {}".format(*dtypes))
    q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
    if q.shape[0] != num_dst:
        raise ValueError("q must have one row per destination node")
    if k.shape[0] != E or v.shape[0] != E:
        raise ValueError("k and v must have one row per edge")
    shaped = []
    for name, t in (("q", q), ("k", k), ("v", v)):
        if t.dim() == 2 and heads is not None:
            if heads < 1 or t.shape[1] % heads or t.shape[1] == 0:
                raise ValueError("{} has {} columns, not a multiple of heads={}".format(
                    name, t.shape[1], heads))
            t = t.view(t.shape[0], heads, t.shape[1] // heads)
        elif t.dim() != 3:
            raise ValueError("{} must be [rows, H, D] (or [rows, H * D] with heads=), got {}"
                             .format(name, tuple(t.shape)))
        shaped.append(t)
    q, k, v = shaped
    if q.shape[1:] != k.shape[1:] or k.shape[1:] != v.shape[1:]:
        raise ValueError("q, k and v differ in [H, D]: {}, {}, {}".format(
            tuple(q.shape[1:]), tuple(k.shape[1:]), tuple(v.shape[1:])))
    H, D = int(q.shape[1]), int(q.shape[2])
    if heads is not None and heads != H:
        raise ValueError("heads={} but the inputs have {} heads".format(heads, H))
    if H < 1 or D < 1:
        raise ValueError("block_attention needs H >= 1 and D >= 1")
    if H * D > MAX_ATTENTION_WIDTH:
        raise ValueError("H * D = {} exceeds the limit of {}".format(H * D, MAX_ATTENTION_WIDTH))
    if E == 0 or num_dst == 0:
        out = _NoEdgeAttention.apply(q, k, v)      # nothing to launch
        return (out, torch.zeros((E, H), dtype=torch.float32, device=q.device)) \
            if return_attention else out
    offsets, _, perm = block.segments()
    if perm is not None:
        k, v = k[perm], v[perm]
    if p32 > 0:
        out, att = _BlockAttentionDropout.apply(q, k, v, offsets, num_dst, float(negative_slope),
                                                p32, dropout_seed, bool(return_attention))
    else:
        out, att = _BlockAttention.apply(q, k, v, offsets, num_dst, float(negative_slope))
    if not return_attention:
        return out
    if perm is not None:
        att = torch.empty_like(att).index_copy(0, perm, att)
    return out, att


class _BlockGat(torch.autograd.Function):
    @staticmethod
    @_fwd
    def forward(ctx, feat, el, er, offsets, col, num_dst, E, slope, p, seed, want_dropped):
        # feat [num_src, H, D] fp32 or bf16, el [num_src, H], er [num_dst, H] fp32, contiguous;
        # col is None for the sampler's layout.  att is the pre-dropout softmax (saved, with the
        # float32 out, for backward).  bf16: the kernel writes out twice, rounded (returned) and
        # as summed ([num_dst, H, D] float32, saved).
        num_src, H, D = feat.shape
        bf16 = feat.dtype == torch.bfloat16
        out = torch.empty((num_dst, H, D), dtype=feat.dtype, device=feat.device)
        out32 = torch.empty((num_dst, H, D), dtype=torch.float32, device=feat.device) \
            if bf16 else out
        att = torch.empty((E, H), dtype=torch.float32, device=feat.device)
        dropped = torch.empty_like(att) if want_dropped and p > 0 else None
        lib = _capi.load()
        args = (offsets.data_ptr(), num_dst, E, _ptr(col), num_src, H, D, feat.data_ptr(),
                el.data_ptr(), er.data_ptr(), slope, p, seed, out.data_ptr(), att.data_ptr(),
                _ptr(dropped), feat.device.index, _stream(feat.device))
        with torch.cuda.device(feat.device):
            if bf16:
                _capi.check(lib.gf_block_gat_bf16(*args, out32.data_ptr()))
            else:
                _capi.check(lib.gf_block_gat(*args))
        ctx.save_for_backward(feat, el, er, att, out32, offsets, col)
        ctx.meta = (slope, p, seed)
        shown = dropped if p > 0 else att
        if not want_dropped:
            return out, None
        ctx.mark_non_differentiable(shown)
        return out, shown

    @staticmethod
    @_bwd
    def backward(ctx, grad, _grad_att):
        feat, el, er, att, out32, offsets, col = ctx.saved_tensors
        slope, p, seed = ctx.meta
        g = _grad_as(grad, feat.dtype)
        num_src, H, D = feat.shape
        need_feat, need_el, need_er = ctx.needs_input_grad[:3]
        gfeat = torch.empty_like(feat) if need_feat else None
        gel = torch.empty_like(el) if need_el else None
        ger = torch.empty_like(er) if need_er else None
        if need_feat or need_el or need_er:
            lib = _capi.load()
            args = (offsets.data_ptr(), er.shape[0], att.shape[0], _ptr(col), num_src, H, D,
                    feat.data_ptr(), el.data_ptr(), er.data_ptr(), att.data_ptr(),
                    out32.data_ptr(), slope, p, seed, g.data_ptr(), _ptr(gfeat), _ptr(gel),
                    _ptr(ger), feat.device.index, _stream(feat.device))
            with torch.cuda.device(feat.device):
                if feat.dtype == torch.bfloat16:
                    _capi.check(lib.gf_block_gat_backward_bf16(
                        *args, _ptr(_scratch(feat, col, need_feat))))
                else:
                    _capi.check(lib.gf_block_gat_backward(*args))
        return gfeat, gel, ger, None, None, None, None, None, None, None, None


class _NoEdgeGat(torch.autograd.Function):
    """A block without edges or without destinations: zeros, and zero gradients."""
    @staticmethod
    def forward(ctx, feat, el, er):
        ctx.save_for_backward(feat, el, er)
        return torch.zeros((er.shape[0],) + tuple(feat.shape[1:]), dtype=feat.dtype,
                           device=feat.device)

    @staticmethod
    def backward(ctx, grad):
        return tuple(torch.zeros_like(t) if need else None
                     for t, need in zip(ctx.saved_tensors, ctx.needs_input_grad))


def block_gat(block, feat: torch.Tensor, el: torch.Tensor, er: torch.Tensor,
              negative_slope: float = 0.2, return_attention: bool = False,
              dropout_p: float = 0.0, dropout_seed: Optional[int] = None):
    """The message passing of dgl.nn.GATConv in one kernel each way:

        att[e, h] = edge_softmax(leaky_relu(el[col[e], h] + er[row[e], h], negative_slope))
        out[d, h] = sum over the edges e into d of att[e, h] * feat[col[e], h]   (0 without in-edges)

    feat: [num_src_nodes, H, D]; el: [num_src_nodes, H]; er: [num_dst_nodes, H], float32 on one
    GPU; H * D is at most MAX_ATTENTION_WIDTH.  Returns out [num_dst_nodes, H, D], and with
    return_attention=True also att [num_edges, H] in the caller's edge order (not
    differentiable).  Differentiable in feat, el and er; the forward's out is kept for the
    backward, which then reads every feat row once.

    feat may instead be bfloat16 (fc(h) under autocast) with el and er float32 (there a float32
    sum); anything else raises TypeError.  The module's rule -- float32 arithmetic, one rounding
    on store -- applies: out and the gradient of feat are bfloat16 and equal, bit for bit, the
    float32 op's on feat.float() rounded once; the attention and the gradients of el and er are
    float32 and equal to its.  The out kept for the backward is the float32 one, before rounding.

    dropout_p / dropout_seed are those of block_attention, with the same mask: p =
    float32(dropout_p) in [0, 1), i the position of an edge in the grouped order of
    block.segments(), keep[i, h] = gf_philox4x32_10_first(dropout_seed, i * H + h, 0) >=
    uint32(float64(p) * 2**32), and a kept weight scaled by float32(1) / (float32(1) - p).  The
    seed (0 <= seed < 2**64) is required when dropout_p > 0; return_attention=True then returns
    the DROPPED attention att * w.  A dropped edge contributes exactly 0 and its feat row is not
    read, forward or backward.  dropout_p == 0 is the call without the two arguments, bit for bit.

    On a sampler block (segments()[1] is None: source of edge k = node num_dst + k) the backward
    uses no atomics and two runs give the same bits.  On a block with an explicit col a source
    may feed several edges; the gradients of feat and el are then accumulated with atomic adds
    (float32 ones also for a bfloat16 feat: in a float32 scratch, rounded once afterwards):
    correct within the same error bounds, rows no edge reads exact zeros, but NOT bit-identical
    from run to run."""
    dropout_p = float(dropout_p)
    if not 0.0 <= dropout_p < 1.0:          # NaN fails too
        raise ValueError("dropout_p must be in [0, 1), got {}".format(dropout_p))
    p32 = C.c_float(dropout_p).value        # the fp32 value the kernels see
    if p32 >= 1.0:
        raise ValueError("dropout_p rounds to 1 in float32")
    if dropout_seed is not None:
        dropout_seed = int(dropout_seed)
        if not 0 <= dropout_seed < 2 ** 64:
            raise ValueError("dropout_seed must be in [0, 2**64), got {}".format(dropout_seed))
    elif dropout_p > 0:
        raise ValueError("dropout_p > 0 needs a dropout_seed")
    for name, t in (("feat", feat), ("el", el), ("er", er)):
        if not isinstance(t, torch.Tensor):
            raise TypeError("{} must be a tensor, got {}".format(name, type(t).__name__))
    if feat.dtype not in (torch.float32, torch.bfloat16) or el.dtype != torch.float32 or \
            er.dtype != torch.float32:
        raise TypeError("block_gat computes in float32 and takes feat float32 or bfloat16 with "
                        "el and er float32, feat is {}, el is {} and er is {}".format(
                            feat.dtype, el.dtype, er.dtype))
    num_dst, num_src, E = block.num_dst_nodes(), block.num_src_nodes(), block.num_edges()
    if feat.dim() != 3:
        raise ValueError("feat must be [num_src, H, D], got {}".format(tuple(feat.shape)))
    if el.dim() != 2 or er.dim() != 2:
        raise ValueError("el and er must be [rows, H], got {} and {}".format(
            tuple(el.shape), tuple(er.shape)))
    if feat.shape[0] != num_src or el.shape[0] != num_src:
        raise ValueError("feat and el must have one row per source node")
    if er.shape[0] != num_dst:
        raise ValueError("er must have one row per destination node")
    H, D = int(feat.shape[1]), int(feat.shape[2])
    if el.shape[1] != H or er.shape[1] != H:
        raise ValueError("feat, el and er differ in H: {}, {}, {}".format(
            H, el.shape[1], er.shape[1]))
    if H < 1 or D < 1:
        raise ValueError("block_gat needs H >= 1 and D >= 1")
    if H * D > MAX_ATTENTION_WIDTH:
        raise ValueError("H * D = {} exceeds the limit of {}".format(H * D, MAX_ATTENTION_WIDTH))
    if el.device != feat.device or er.device != feat.device:
        raise ValueError("feat is on {}, el on {}, er on {}".format(
            feat.device, el.device, er.device))
    if feat.device.type != "cuda":
        raise ValueError("block_gat runs on the GPU, the inputs are on {}".format(feat.device))
    feat, el, er = feat.contiguous(), el.contiguous(), er.contiguous()
    if E == 0 or num_dst == 0:
        out = _NoEdgeGat.apply(feat, el, er)       # nothing to launch
        return (out, torch.zeros((E, H), dtype=torch.float32, device=feat.device)) \
            if return_attention else out
    offsets, col, perm = block.segments()
    out, att = _BlockGat.apply(feat, el, er, offsets, col, num_dst, E, float(negative_slope),
                               p32, dropout_seed if p32 > 0 else 0, bool(return_attention))
    if not return_attention:
        return out
    if perm is not None:
        att = torch.empty_like(att).index_copy(0, perm, att)
    return out, att


class _TimeEncodeCat(torch.autograd.Function):
    @staticmethod
    @_fwd
    def forward(ctx, out_dtype, t, weight, bias, *parts):
        # t [n], weight / bias [T], parts: contiguous [n, W] with W > 0; all fp32 on one device;
        # out_dtype fp32 or bf16
        n, T = t.shape[0], bias.shape[0]
        widths = [p.shape[1] for p in parts]
        out = torch.empty((n, sum(widths) + T), dtype=out_dtype, device=t.device)
        if n:
            a, b = (list(parts) + [None, None])[:2]
            wa, wb = (widths + [0, 0])[:2]
            lib = _capi.load()
            fn = lib.gf_time_encode_cat_bf16 if out_dtype == torch.bfloat16 \
                else lib.gf_time_encode_cat
            with torch.cuda.device(t.device):
                _capi.check(fn(
                    _ptr(a), wa, _ptr(b), wb, t.data_ptr(), weight.data_ptr(), bias.data_ptr(),
                    n, T, out.data_ptr(), t.device.index, _stream(t.device)))
        ctx.save_for_backward(t, weight, bias)
        ctx.widths = widths
        ctx.out_dtype = out_dtype
        return out

    @staticmethod
    @_bwd
    def backward(ctx, grad):
        t, weight, bias = ctx.saved_tensors
        n, T = t.shape[0], bias.shape[0]
        g = _grad_as(grad, ctx.out_dtype)
        bf16 = ctx.out_dtype == torch.bfloat16
        need_w, need_b = ctx.needs_input_grad[2], ctx.needs_input_grad[3]
        gw = gb = None
        if need_w or need_b:
            # n == 0: zeros, and nothing to launch
            gw = torch.zeros_like(weight) if need_w else None
            gb = torch.zeros_like(bias) if need_b else None
            if n:
                lib = _capi.load()
                rows = C.c_size_t(0)
                _capi.check(lib.gf_time_encode_backward_partial_rows(n, C.byref(rows)))
                partials = torch.empty((rows.value, 2, T), dtype=torch.float32, device=t.device)
                fn = lib.gf_time_encode_backward_bf16 if bf16 else lib.gf_time_encode_backward
                with torch.cuda.device(t.device):
                    _capi.check(fn(
                        t.data_ptr(), weight.data_ptr(), bias.data_ptr(), n, T, g.data_ptr(),
                        g.shape[1], sum(ctx.widths), partials.data_ptr(), rows.value,
                        _ptr(gw), _ptr(gb), t.device.index, _stream(t.device)))
        gparts, off = [], 0
        for k, w in enumerate(ctx.widths):      # column slices of grad: views, no kernel
            gp = g[:, off:off + w] if ctx.needs_input_grad[4 + k] else None
            # the parts are fp32: a bf16 slice is widened once (exact)
            gparts.append(gp.float() if gp is not None and bf16 else gp)
            off += w
        return (None, None, gw, gb) + tuple(gparts)      # no gradient flows to t


def _time_encode_cat(parts, t, weight, bias, out_dtype=None):
    """time_encode_cat: checks every argument, then the kernel."""
    if out_dtype is None:
        out_dtype = torch.float32
    if out_dtype not in (torch.float32, torch.bfloat16):
        raise ValueError("out_dtype must be None, torch.float32 or torch.bfloat16, got {}".format(
            out_dtype))
    parts = tuple(parts)
    if len(parts) > 2:
        raise ValueError("time_encode_cat takes at most two parts, got {}".format(len(parts)))
    for name, x in (("t", t), ("weight", weight), ("bias", bias)) + \
            tuple(("parts[{}]".format(i), p) for i, p in enumerate(parts)):
        if not isinstance(x, torch.Tensor):
            raise TypeError("{} must be a tensor, got {}".format(name, type(x).__name__))
        if x.dtype != torch.float32:
            raise TypeError("time_encode_cat computes in float32, {} is {}".format(name, x.dtype))
    if t.dim() == 2 and t.shape[1] == 1:
        t = t.reshape(-1)
    if t.dim() != 1:
        raise ValueError("t must be [n] or [n, 1], got {}".format(tuple(t.shape)))
    if bias.dim() != 1:
        raise ValueError("bias must be [T], got {}".format(tuple(bias.shape)))
    T = int(bias.shape[0])
    if T == 0:
        raise ValueError("time_encode_cat needs T >= 1")
    if tuple(weight.shape) not in ((T, 1), (T,)):
        raise ValueError("weight must be [T, 1] or [T] with T = {}, got {}".format(
            T, tuple(weight.shape)))
    n = int(t.shape[0])
    for i, p in enumerate(parts):
        if p.dim() != 2:
            raise ValueError("parts[{}] must be [n, W], got {}".format(i, tuple(p.shape)))
        if p.shape[0] != n:
            raise ValueError("parts[{}] has {} rows, t has {}".format(i, p.shape[0], n))
    for name, x in (("weight", weight), ("bias", bias)) + \
            tuple(("parts[{}]".format(i), p) for i, p in enumerate(parts)):
        if x.device != t.device:
            raise ValueError("{} is on {}, t on {}".format(name, x.device, t.device))
    if t.device.type != "cuda":
        raise ValueError("time_encode_cat runs on the GPU, the inputs are on {}".format(t.device))
    # a part without columns adds nothing to the row (and has no address to hand over)
    parts = tuple(p.contiguous() for p in parts if p.shape[1])
    return _TimeEncodeCat.apply(out_dtype, t.detach().contiguous(),
                                weight.reshape(T).contiguous(), bias.contiguous(), *parts)


def time_encode_cat(parts, t: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor,
                    out_dtype=None):
    """torch.cat([*parts, torch.cos(t[:, None] * weight.T + bias)], dim=1) in one kernel: the
    input rows every temporal layer of the reference builds (layers.py:118-137,
    memory_updater.py:62-65).

    parts: a sequence of 0, 1 or 2 float32 tensors [n, W] (row slices such as h[R:] are taken
    as they are; any other non-contiguous part is copied first); t: [n] or [n, 1]; weight:
    [T, 1] or [T] (TimeEncode.w.weight); bias: [T]; all float32 on one GPU.  Returns
    [n, sum(W) + T].  Differentiable in parts, weight and bias; t gets no gradient (the
    reference never asks for one).  The gradients of weight and bias are summed in a fixed
    order: bit-identical from run to run.

    out_dtype: None or torch.float32 (the call without it, bit for bit) or torch.bfloat16; any
    other value raises ValueError.  The inputs stay float32 either way.  bfloat16 follows the
    module's rule -- float32 arithmetic, one rounding on store --: the rows are what the float32
    call returns, converted with .to(torch.bfloat16), written by the kernel itself.  The backward
    then takes a bfloat16 gradient: the gradients of weight and bias are float32 and equal, bit
    for bit, the float32 op's on the widened gradient, and those of the parts are its column
    slices widened to float32."""
    return _time_encode_cat(parts, t, weight, bias, out_dtype)


def time_encode(t: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor,
                out_dtype=None) -> torch.Tensor:
    """cos(t[:, None] * weight.T + bias): time_encode_cat without parts, [n, T]."""
    return _time_encode_cat((), t, weight, bias, out_dtype)


class _EdgeScore(torch.autograd.Function):
    @staticmethod
    @_fwd
    def forward(ctx, src, dst, weight, bias):
        # src [B, D], dst [M, D] contiguous, both fp32 or both bf16; weight [D], bias [1] fp32
        M = dst.shape[0]
        out = torch.empty((M, 1), dtype=torch.float32, device=dst.device)
        if M:
            lib = _capi.load()
            fn = lib.gf_edge_score_bf16 if dst.dtype == torch.bfloat16 else lib.gf_edge_score
            with torch.cuda.device(dst.device):
                _capi.check(fn(
                    src.data_ptr(), dst.data_ptr(), weight.data_ptr(), bias.data_ptr(),
                    src.shape[0], M, dst.shape[1], out.data_ptr(), dst.device.index,
                    _stream(dst.device)))
        ctx.save_for_backward(src, dst, weight)
        return out

    @staticmethod
    @_bwd
    def backward(ctx, grad):
        src, dst, weight = ctx.saved_tensors
        (B, D), M = src.shape, dst.shape[0]
        need_src, need_dst, need_w, need_b = ctx.needs_input_grad
        f32 = dict(dtype=torch.float32, device=dst.device)
        if M == 0:      # zeros, and nothing to launch
            return (torch.zeros_like(src) if need_src else None,
                    torch.zeros_like(dst) if need_dst else None,
                    torch.zeros_like(weight) if need_w else None,
                    torch.zeros(1, **f32) if need_b else None)
        if not (need_src or need_dst or need_w or need_b):
            return None, None, None, None
        g = _f32(grad)
        gs = torch.empty_like(src) if need_src else None
        gd = torch.empty_like(dst) if need_dst else None
        gw = torch.empty_like(weight) if need_w else None
        gb = torch.empty(1, **f32) if need_b else None
        lib = _capi.load()
        partials, rows = None, C.c_size_t(0)
        if need_w or need_b:
            _capi.check(lib.gf_edge_score_backward_partial_rows(B, C.byref(rows)))
            partials = torch.empty((rows.value, D + 1), **f32)
        fn = lib.gf_edge_score_backward_bf16 if dst.dtype == torch.bfloat16 \
            else lib.gf_edge_score_backward
        with torch.cuda.device(dst.device):
            _capi.check(fn(
                src.data_ptr(), dst.data_ptr(), weight.data_ptr(), B, M, D, g.data_ptr(),
                _ptr(partials), rows.value, _ptr(gs), _ptr(gd), _ptr(gw), _ptr(gb),
                dst.device.index, _stream(dst.device)))
        return gs, gd, gw, gb


def edge_score(src: torch.Tensor, dst: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor):
    """out[j, 0] = bias + sum_d weight[d] * relu(src[j mod B, d] + dst[j, d]): the tail of the
    reference's EdgePredictor (layers.py:195-197) for every block of dst rows in one kernel.

    src: [B, D]; dst: [M, D] with M = r * B, block k of B rows paired with src (r = 2: the
    positive and the negative half; r > 2: several negatives per positive, block after block);
    weight: [D] or [1, D] (out_fc.weight); bias: [1]; all float32 on one GPU (row slices such as
    h[B:] are taken as they are; any other non-contiguous input is copied first).  Returns
    [M, 1].  Differentiable in all four; every gradient is summed in a fixed order:
    bit-identical from run to run.

    src and dst may instead both be bfloat16 (the Linear outputs under autocast) with weight and
    bias float32; any other dtype or a mixture raises TypeError.  The module's rule -- float32
    arithmetic, one rounding on store -- applies: the scores and the gradients of weight and bias
    are float32 and equal, bit for bit, the float32 op's on src.float() and dst.float(); the
    gradients of src and dst are bfloat16, its float32 gradients rounded once."""
    for name, x in (("src", src), ("dst", dst), ("weight", weight), ("bias", bias)):
        if not isinstance(x, torch.Tensor):
            raise TypeError("{} must be a tensor, got {}".format(name, type(x).__name__))
    if (src.dtype, dst.dtype) not in ((torch.float32,) * 2, (torch.bfloat16,) * 2):
        raise TypeError("edge_score computes in float32 and takes src and dst both float32 or "
                        "both bfloat16, src is {} and dst is {}".format(src.dtype, dst.dtype))
    for name, x in (("weight", weight), ("bias", bias)):
        if x.dtype != torch.float32:
            raise TypeError("edge_score computes in float32, {} is {}".format(name, x.dtype))
    if src.dim() != 2 or dst.dim() != 2:
        raise ValueError("src and dst must be [B, D] and [M, D], got {} and {}".format(
            tuple(src.shape), tuple(dst.shape)))
    (B, D), M = (int(n) for n in src.shape), int(dst.shape[0])
    if dst.shape[1] != D:
        raise ValueError("src has {} columns, dst has {}".format(D, dst.shape[1]))
    if D == 0:
        raise ValueError("edge_score needs D >= 1")
    if tuple(weight.shape) not in ((D,), (1, D)):
        raise ValueError("weight must be [D] or [1, D] with D = {}, got {}".format(
            D, tuple(weight.shape)))
    if tuple(bias.shape) != (1,):
        raise ValueError("bias must be [1], got {}".format(tuple(bias.shape)))
    if M % B if B else M:
        raise ValueError("dst has {} rows, not a multiple of the {} rows of src".format(M, B))
    for name, x in (("src", src), ("weight", weight), ("bias", bias)):
        if x.device != dst.device:
            raise ValueError("{} is on {}, dst on {}".format(name, x.device, dst.device))
    if dst.device.type != "cuda":
        raise ValueError("edge_score runs on the GPU, the inputs are on {}".format(dst.device))
    return _EdgeScore.apply(src.contiguous(), dst.contiguous(), weight.reshape(D).contiguous(),
                            bias.contiguous())


EDGE_RANK_MAX_K = 64                 # GF_EDGE_RANK_MAX_K: the longest top-k list
EDGE_RANK_CHUNK = 256                # GF_EDGE_RANK_CHUNK: candidates per workgroup pass of the kernel


class EdgeRank(NamedTuple):
    """What edge_rank returns.  values, indices: [B, k] (float32, int64); greater, equal: [B]
    (int64) or None without a reference score."""
    values: torch.Tensor
    indices: torch.Tensor
    greater: Optional[torch.Tensor]
    equal: Optional[torch.Tensor]

    @property
    def rank(self) -> Optional[torch.Tensor]:
        """float64 [B]: 1 + greater + equal / 2, the mean of the optimistic and the pessimistic
        rank (the convention of link_metrics); None without a reference score."""
        if self.greater is None:
            return None
        return 1.0 + self.greater.double() + self.equal.double() / 2


def edge_rank(src: torch.Tensor, cand: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor,
              k: int = 0, ref_score: Optional[torch.Tensor] = None,
              skip: Optional[torch.Tensor] = None,
              exclude: Optional[torch.Tensor] = None) -> EdgeRank:
    """Scores every source against ONE shared candidate set and keeps, per source, the k best
    candidates and the number of candidates that beat or tie a reference score:

        score(i, c) = bias + sum_d weight[d] * relu(src[i, d] + cand[c, d])

    in one streaming kernel (csrc/edge_rank.hip) that stores neither the [B * C, D] rows that
    edge_score(src, cand.repeat_interleave(B, 0)) would need nor the [B, C] scores.  score(i, c)
    is the float32 value edge_score returns for that pair of rows, bit for bit, so a ref_score
    taken from edge_score ties exactly with the same candidate here; the one exception is a NaN
    in src[i, d] + cand[c, d], which makes the score NaN (torch.relu keeps a NaN, edge_score's
    relu turns it into 0).

    src: [B, D]; cand: [C, D]; weight: [D] or [1, D]; bias: [1]; ref_score: [B] or [B, 1] or
    None; all float32 on one GPU.  skip: int64 [B] or None.  exclude: int64 [B, W] with
    W = (C + 63) // 64, or None.  0 <= k <= min(C, EDGE_RANK_MAX_K), D >= 1, 1 <= C < 2**31.  Inputs are detached: there is no autograd.  Row slices are taken as
    they are; any other non-contiguous input is copied.

    Returns EdgeRank(values, indices, greater, equal):
      values, indices [B, k]  the k best candidates of each source, score descending, then
          candidate index ascending among equal scores.  A NaN score sorts below -inf (by
          ascending index among NaNs) and is returned as NaN.  A row with fewer than k candidates
          left (k == C with a valid skip, or exclusions) ends in (-inf, -1).  [B, 0] when k == 0.
      greater, equal [B]  the candidates with score > / == ref_score[i]; a NaN score is neither,
          and a NaN ref_score gives two zeros.  None without ref_score.  .rank is
          1 + greater + equal / 2.
    Candidate skip[i] is left out of row i's counts and list (the "filtered" setting: the true
    destination); a value outside [0, C) excludes nothing.  skip works without ref_score too.
    Candidate c is left out of row i in exactly the same way when bit c % 64 of
    exclude[i, c // 64] is set: a per-source SET of candidates, such as the nodes the source has
    already interacted with (DynamicGraph.seen_mask returns this layout).  skip and exclude may
    both be given; bits at positions >= C are ignored; a row with every candidate excluded gets a
    list of (-inf, -1) and, with ref_score, zero counts.

    Runs on the current stream and never synchronises; selection under a total order and
    integer counts: the same inputs give the same bits.

    A candidate set too large for one call is cut into shards cand[a:b]: the counts of the
    shards add, and the lists (indices + a) are concatenated and go through one
    torch.topk(values, k) -- after which equal scores are no longer in index order across
    shards, unless the shards' lists are merged by (value, index) instead.  A shard cand[a:b]
    with a % 64 == 0 takes exclude[:, a // 64:(b + 63) // 64]."""
    named = (("src", src), ("cand", cand), ("weight", weight), ("bias", bias))
    if ref_score is not None:
        named += (("ref_score", ref_score),)
    ints = tuple((name, x) for name, x in (("skip", skip), ("exclude", exclude)) if x is not None)
    for name, x in named + ints:
        if not isinstance(x, torch.Tensor):
            raise TypeError("{} must be a tensor, got {}".format(name, type(x).__name__))
    for name, x in named:
        if x.dtype != torch.float32:
            raise TypeError("edge_rank computes in float32, {} is {}".format(name, x.dtype))
    for name, x in ints:
        if x.dtype != torch.int64:
            raise TypeError("{} must be int64, got {}".format(name, x.dtype))
    if isinstance(k, bool) or not isinstance(k, int):
        raise TypeError("k must be an int, got {}".format(type(k).__name__))
    if src.dim() != 2 or cand.dim() != 2:
        raise ValueError("src and cand must be [B, D] and [C, D], got {} and {}".format(
            tuple(src.shape), tuple(cand.shape)))
    (B, D), Cn = (int(n) for n in src.shape), int(cand.shape[0])
    if cand.shape[1] != D:
        raise ValueError("src has {} columns, cand has {}".format(D, cand.shape[1]))
    if D == 0:
        raise ValueError("edge_rank needs D >= 1")
    if Cn == 0:
        raise ValueError("edge_rank needs at least one candidate")
    if Cn >= 2 ** 31:
        raise ValueError("edge_rank takes fewer than 2**31 candidates per call, got {}".format(Cn))
    if tuple(weight.shape) not in ((D,), (1, D)):
        raise ValueError("weight must be [D] or [1, D] with D = {}, got {}".format(
            D, tuple(weight.shape)))
    if tuple(bias.shape) != (1,):
        raise ValueError("bias must be [1], got {}".format(tuple(bias.shape)))
    if k < 0 or k > min(Cn, EDGE_RANK_MAX_K):
        raise ValueError("k must be in [0, min(C, {})] with C = {}, got {}".format(
            EDGE_RANK_MAX_K, Cn, k))
    if ref_score is not None and tuple(ref_score.shape) not in ((B,), (B, 1)):
        raise ValueError("ref_score must be [B] or [B, 1] with B = {}, got {}".format(
            B, tuple(ref_score.shape)))
    if skip is not None and tuple(skip.shape) != (B,):
        raise ValueError("skip must be [B] with B = {}, got {}".format(B, tuple(skip.shape)))
    if exclude is not None and tuple(exclude.shape) != (B, (Cn + 63) // 64):
        raise ValueError("exclude must be [B, (C + 63) // 64] = [{}, {}], got {}".format(
            B, (Cn + 63) // 64, tuple(exclude.shape)))
    for name, x in named[1:] + ints:
        if x.device != src.device:
            raise ValueError("{} is on {}, src on {}".format(name, x.device, src.device))
    if src.device.type != "cuda":
        raise ValueError("edge_rank runs on the GPU, the inputs are on {}".format(src.device))
    dev = src.device
    s, c = src.detach().contiguous(), cand.detach().contiguous()
    w, b = weight.detach().reshape(D).contiguous(), bias.detach().contiguous()
    ref = None if ref_score is None else ref_score.detach().reshape(B).contiguous()
    sk = None if skip is None else skip.detach().contiguous()
    ex = None if exclude is None else exclude.detach().contiguous()
    values = torch.empty((B, k), dtype=torch.float32, device=dev)
    indices = torch.empty((B, k), dtype=torch.int64, device=dev)
    greater = equal = None
    if ref is not None:
        greater = torch.empty(B, dtype=torch.int64, device=dev)
        equal = torch.empty(B, dtype=torch.int64, device=dev)
    if B and (k or ref is not None):
        lib = _capi.load()
        nbytes = C.c_size_t(0)
        _capi.check(lib.gf_edge_rank_scratch(B, Cn, k, C.byref(nbytes)))
        scratch = torch.empty((nbytes.value + 7) // 8, dtype=torch.int64, device=dev)
        with torch.cuda.device(dev):
            _capi.check(lib.gf_edge_rank_masked(
                s.data_ptr(), c.data_ptr(), w.data_ptr(), b.data_ptr(), B, Cn, D, k, _ptr(ref),
                _ptr(sk), _ptr(ex), scratch.data_ptr(), scratch.numel() * 8, _ptr(values),
                _ptr(indices), _ptr(greater), _ptr(equal), dev.index, _stream(dev)))
    return EdgeRank(values, indices, greater, equal)


LAYER_EPILOGUE_MAX_WIDTH = 1024      # GF_LAYER_EPILOGUE_MAX_WIDTH: the limit on D


class _DropoutReluLayerNorm(torch.autograd.Function):
    @staticmethod
    @_fwd
    def forward(ctx, x, weight, bias, eps, p32, seed):
        # x [R, D] contiguous, fp32 or bf16; weight, bias [D] fp32 contiguous; out fp32
        R, D = x.shape
        f32 = dict(dtype=torch.float32, device=x.device)
        out = torch.empty((R, D), **f32)
        mean, rstd = torch.empty(R, **f32), torch.empty(R, **f32)
        if R:
            lib = _capi.load()
            fn = lib.gf_layer_epilogue_bf16 if x.dtype == torch.bfloat16 else lib.gf_layer_epilogue
            with torch.cuda.device(x.device):
                _capi.check(fn(
                    x.data_ptr(), weight.data_ptr(), bias.data_ptr(), R, D, eps, p32, seed,
                    out.data_ptr(), mean.data_ptr(), rstd.data_ptr(), x.device.index,
                    _stream(x.device)))
        ctx.save_for_backward(x, weight, mean, rstd)      # neither out nor a mask
        ctx.p32, ctx.seed = p32, seed
        return out

    @staticmethod
    @_bwd
    def backward(ctx, grad):
        x, weight, mean, rstd = ctx.saved_tensors
        R, D = x.shape
        need_x, need_w, need_b = ctx.needs_input_grad[:3]
        if R == 0:      # zeros, and nothing to launch
            return (torch.zeros_like(x) if need_x else None,
                    torch.zeros_like(weight) if need_w else None,
                    torch.zeros_like(weight) if need_b else None, None, None, None)
        if not (need_x or need_w or need_b):
            return None, None, None, None, None, None
        g = _grad_as(grad, torch.float32)
        gx = torch.empty_like(x) if need_x else None
        gw = torch.empty_like(weight) if need_w else None
        gb = torch.empty_like(weight) if need_b else None
        lib = _capi.load()
        partials, rows = None, C.c_size_t(0)
        if need_w or need_b:
            _capi.check(lib.gf_layer_epilogue_backward_partial_rows(R, C.byref(rows)))
            partials = torch.empty((rows.value, 2 * D), dtype=torch.float32, device=x.device)
        fn = lib.gf_layer_epilogue_backward_bf16 if x.dtype == torch.bfloat16 \
            else lib.gf_layer_epilogue_backward
        with torch.cuda.device(x.device):
            _capi.check(fn(
                x.data_ptr(), weight.data_ptr(), mean.data_ptr(), rstd.data_ptr(), R, D, ctx.p32,
                ctx.seed, g.data_ptr(), _ptr(partials), rows.value, _ptr(gx), _ptr(gw), _ptr(gb),
                x.device.index, _stream(x.device)))
        return gx, gw, gb, None, None, None


def dropout_relu_layer_norm(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor,
                            eps: float = 1e-5, dropout_p: float = 0.0, dropout_seed: int = 0):
    """layer_norm(relu(dropout(x)), (D,), weight, bias, eps) over the rows of x [R, D]: the last
    line of the reference's TemporalAttentionLayer after w_out, in one kernel each way
    (csrc/layer_epilogue.hip).  Returns float32 [R, D].

    x: [R, D], float32 or bfloat16 (what w_out returns under autocast), D <=
    LAYER_EPILOGUE_MAX_WIDTH; weight, bias: float32 [D]; all on one GPU (a non-contiguous x is
    copied first).  Any other dtype raises TypeError.  With p = float32(dropout_p), 0 <= p < 1:

        T          = uint32(float64(p) * 2**32)
        keep[r, d] = gf_philox4x32_10_first(dropout_seed, r * D + d, 0) >= T      (gnnflow_rng.h)
        y          = relu(keep ? x * fl32(1 / (1 - p)) : 0)
        out        = (y - mean) * rstd * weight + bias      mean, var over the row, rstd = 1 / sqrt(var + eps)

    dropout_p == 0 keeps everything and ignores dropout_seed (0 <= seed < 2**64).  The mask is not
    stored: the backward draws it again from the seed, and saves x, weight and the rows' mean and
    rstd, neither the output nor a mask.  tests/attention_dropout_ref.py restates the generator in
    numpy.  Differentiable in x, weight and bias; a gradient that is not asked for is None and is
    not computed, and the gradients of weight and bias are summed in a fixed order: bit-identical
    from run to run.

    The module's rule for bfloat16 applies -- float32 arithmetic, one rounding on store --: the
    output and the gradients of weight and bias equal, bit for bit, the float32 op's on
    x.float(); the gradient of x is bfloat16, its float32 gradient rounded once."""
    for name, t in (("x", x), ("weight", weight), ("bias", bias)):
        if not isinstance(t, torch.Tensor):
            raise TypeError("{} must be a tensor, got {}".format(name, type(t).__name__))
    if x.dtype not in (torch.float32, torch.bfloat16):
        raise TypeError("dropout_relu_layer_norm computes in float32 and takes x float32 or "
                        "bfloat16, x is {}".format(x.dtype))
    for name, t in (("weight", weight), ("bias", bias)):
        if t.dtype != torch.float32:
            raise TypeError("dropout_relu_layer_norm computes in float32, {} is {}".format(
                name, t.dtype))
    if x.dim() != 2:
        raise ValueError("x must be [R, D], got {}".format(tuple(x.shape)))
    D = int(x.shape[1])
    if D == 0:
        raise ValueError("dropout_relu_layer_norm needs D >= 1")
    if D > LAYER_EPILOGUE_MAX_WIDTH:
        raise ValueError("D = {} exceeds LAYER_EPILOGUE_MAX_WIDTH ({})".format(
            D, LAYER_EPILOGUE_MAX_WIDTH))
    for name, t in (("weight", weight), ("bias", bias)):
        if tuple(t.shape) != (D,):
            raise ValueError("{} must be [D] with D = {}, got {}".format(name, D, tuple(t.shape)))
    eps = float(eps)
    if not eps > 0.0 or not C.c_float(eps).value > 0.0:      # NaN fails too
        raise ValueError("eps must be > 0 in float32, got {}".format(eps))
    dropout_p = float(dropout_p)
    if not 0.0 <= dropout_p < 1.0:          # NaN fails too
        raise ValueError("dropout_p must be in [0, 1), got {}".format(dropout_p))
    p32 = C.c_float(dropout_p).value        # the fp32 value the kernels see
    if not p32 < 1.0:
        raise ValueError("dropout_p rounds to 1 in float32")
    dropout_seed = int(dropout_seed)
    if not 0 <= dropout_seed < 2 ** 64:
        raise ValueError("dropout_seed must be in [0, 2**64), got {}".format(dropout_seed))
    for name, t in (("weight", weight), ("bias", bias)):
        if t.device != x.device:
            raise ValueError("{} is on {}, x on {}".format(name, t.device, x.device))
    if x.device.type != "cuda":
        raise ValueError("dropout_relu_layer_norm runs on the GPU, the inputs are on {}".format(
            x.device))
    return _DropoutReluLayerNorm.apply(x.contiguous(), weight.contiguous(), bias.contiguous(),
                                       eps, p32, dropout_seed if p32 > 0 else 0)


class _GruCell(torch.autograd.Function):
    @staticmethod
    @_fwd
    def forward(ctx, gi, gh, hx, residual, num_last):
        # gi, gh [N, 3H] contiguous, both fp32 or both bf16; hx [N, H] fp32; residual [N, H] fp32
        # or bf16 or None
        N, H = hx.shape
        f32 = dict(dtype=torch.float32, device=hx.device)
        out, last = torch.empty((N, H), **f32), torch.empty((num_last, H), **f32)
        if N:
            lib = _capi.load()
            fn = lib.gf_gru_cell_bf16 if gi.dtype == torch.bfloat16 else lib.gf_gru_cell
            with torch.cuda.device(hx.device):
                _capi.check(fn(
                    gi.data_ptr(), gh.data_ptr(), hx.data_ptr(), _ptr(residual),
                    int(residual is not None and residual.dtype == torch.bfloat16), N, H,
                    num_last, out.data_ptr(), _ptr(last), hx.device.index, _stream(hx.device)))
        ctx.save_for_backward(gi, gh, hx)      # neither the gates nor a workspace
        ctx.residual_dtype = None if residual is None else residual.dtype
        ctx.mark_non_differentiable(last)
        return out, last

    @staticmethod
    @_bwd
    def backward(ctx, grad, _grad_last):
        gi, gh, hx = ctx.saved_tensors
        N, H = hx.shape
        need_gi, need_gh, need_hx, need_res = ctx.needs_input_grad[:4]
        need_res = need_res and ctx.residual_dtype is not None
        if N == 0:      # zeros, and nothing to launch
            return (torch.zeros_like(gi) if need_gi else None,
                    torch.zeros_like(gh) if need_gh else None,
                    torch.zeros_like(hx) if need_hx else None,
                    torch.zeros_like(hx, dtype=ctx.residual_dtype) if need_res else None, None)
        if not (need_gi or need_gh or need_hx or need_res):
            return None, None, None, None, None
        g = _grad_as(grad, torch.float32)
        dgi = torch.empty_like(gi) if need_gi else None
        dgh = torch.empty_like(gh) if need_gh else None
        dhx = torch.empty_like(hx) if need_hx else None
        if need_gi or need_gh or need_hx:
            lib = _capi.load()
            fn = lib.gf_gru_cell_backward_bf16 if gi.dtype == torch.bfloat16 \
                else lib.gf_gru_cell_backward
            with torch.cuda.device(hx.device):
                _capi.check(fn(
                    gi.data_ptr(), gh.data_ptr(), hx.data_ptr(), N, H, g.data_ptr(), _ptr(dgi),
                    _ptr(dgh), _ptr(dhx), hx.device.index, _stream(hx.device)))
        # the residual's gradient is the incoming one: no kernel
        return dgi, dgh, dhx, (g.to(ctx.residual_dtype) if need_res else None), None


def gru_cell(gi: torch.Tensor, gh: torch.Tensor, hx: torch.Tensor,
             residual: Optional[torch.Tensor] = None, num_last: int = 0):
    """What torch.nn.GRUCell does behind its two GEMMs, with the memory updater's residual add and
    its copy of the first rows, in one kernel each way (csrc/gru_cell.hip).

    gi = F.linear(x, weight_ih, bias_ih) and gh = F.linear(hx, weight_hh, bias_hh): [N, 3H], gate
    chunks in torch's order r, z, n; hx: [N, H]; residual: [N, H] or None; 0 <= num_last <= N:

        r = sigmoid(gi_r + gh_r)      z = sigmoid(gi_z + gh_z)      n = tanh(gi_n + r * gh_n)
        u = (1 - z) * n + z * hx
        h_out = u + residual  (u without one)          last = u[:num_last]

    Returns (h_out [N, H], last [num_last, H]), both float32.  `last` is a buffer of its own,
    never includes the residual and is not differentiable: what Memory.update_mem_mail stores.
    Differentiable in gi, gh, hx and residual.  The forward writes no workspace: gi, gh and hx are
    saved and the gates recomputed by the same expressions in the backward.  A gradient that is
    not asked for is None and is not computed; the residual's gradient is the incoming gradient
    itself.  Nothing is summed, so every result is bit-identical from run to run.

    gi and gh are both float32 or both bfloat16 (what the Linears return under autocast), hx is
    float32 always (Memory's state is never rounded), residual float32 or bfloat16 independently;
    any other dtype raises TypeError.  The module's rule -- float32 arithmetic, one rounding on
    store -- applies: h_out, last and the gradient of hx equal, bit for bit, the float32 op's on
    gi.float() and gh.float(); the gradients of gi and gh are bfloat16, its float32 gradients
    rounded once.  All on one GPU; row slices such as mem[:N] are taken as they are, any other
    non-contiguous input is copied first."""
    for name, x in (("gi", gi), ("gh", gh), ("hx", hx)):
        if not isinstance(x, torch.Tensor):
            raise TypeError("{} must be a tensor, got {}".format(name, type(x).__name__))
    if residual is not None and not isinstance(residual, torch.Tensor):
        raise TypeError("residual must be a tensor or None, got {}".format(
            type(residual).__name__))
    if isinstance(num_last, bool) or not isinstance(num_last, int):
        raise TypeError("num_last must be an int, got {}".format(type(num_last).__name__))
    if (gi.dtype, gh.dtype) not in ((torch.float32,) * 2, (torch.bfloat16,) * 2):
        raise TypeError("gru_cell computes in float32 and takes gi and gh both float32 or both "
                        "bfloat16, gi is {} and gh is {}".format(gi.dtype, gh.dtype))
    if hx.dtype != torch.float32:
        raise TypeError("gru_cell computes in float32, hx is {}".format(hx.dtype))
    if residual is not None and residual.dtype not in (torch.float32, torch.bfloat16):
        raise TypeError("gru_cell takes a float32 or bfloat16 residual, residual is {}".format(
            residual.dtype))
    if hx.dim() != 2:
        raise ValueError("hx must be [N, H], got {}".format(tuple(hx.shape)))
    N, H = (int(n) for n in hx.shape)
    if H == 0:
        raise ValueError("gru_cell needs H >= 1")
    for name, x in (("gi", gi), ("gh", gh)):
        if tuple(x.shape) != (N, 3 * H):
            raise ValueError("{} must be [N, 3H] = [{}, {}], got {}".format(
                name, N, 3 * H, tuple(x.shape)))
    if residual is not None and tuple(residual.shape) != (N, H):
        raise ValueError("residual must be [N, H] = [{}, {}], got {}".format(
            N, H, tuple(residual.shape)))
    if not 0 <= num_last <= N:
        raise ValueError("num_last must be in [0, {}], got {}".format(N, num_last))
    for name, x in (("gi", gi), ("gh", gh), ("residual", residual)):
        if x is not None and x.device != hx.device:
            raise ValueError("{} is on {}, hx on {}".format(name, x.device, hx.device))
    if hx.device.type != "cuda":
        raise ValueError("gru_cell runs on the GPU, the inputs are on {}".format(hx.device))
    return _GruCell.apply(gi.contiguous(), gh.contiguous(), hx.contiguous(),
                          None if residual is None else residual.contiguous(), num_last)


LINK_METRICS_MAX_SCORES = 65536      # GF_LINK_METRICS_MAX_SCORES: the limit on P + N
LINK_METRICS_TILE = 2048             # GF_LINK_METRICS_TILE: scores per LDS tile of the kernel
_LINK_METRICS_PARTIAL_WORDS = 4      # GF_LINK_METRICS_PARTIAL_WORDS


def link_metrics(pos: torch.Tensor, neg: torch.Tensor,
                 accumulator: Optional[torch.Tensor] = None) -> torch.Tensor:
    """[AP, AUC, MRR] of one batch as a float64 tensor [3] on the GPU: sklearn's
    average_precision_score and roc_auc_score of torch.cat([pos, neg]) against the labels
    [1] * P + [0] * N, as the reference's evaluate() computes them per batch, and the mean
    reciprocal rank of each positive among its own negatives.

    pos: [P] or [P, 1], the scores of the true edges; neg: [N] or [N, 1], those of the negative
    ones, as EdgePredictor returns them; float32 on one GPU, P >= 1, N >= 1 and
    P + N <= LINK_METRICS_MAX_SCORES.  Both are detached; a non-contiguous input is copied.
    MRR needs N = r * P with positive i's negatives at neg[k * P + i] (the block layout of
    edge_score); its rank is 1 + #greater + #equal / 2, the mean of the optimistic and the
    pessimistic rank.  When N is not a multiple of P it is NaN.

    accumulator: a float64 [8] tensor on the same GPU, the running sums of a validation pass
    (sum_ap, sum_auc, sum_mrr, batches, mrr_batches, nonfinite, 2 reserved), updated on the
    device; metrics.LinkMetrics wraps it.  A NaN or an infinity among the scores (scikit-learn
    raises) gives three NaNs and adds 1 to `nonfinite` alone.

    Runs on the current stream and never synchronises.  Ties are counted, not broken, and the
    sums run in a fixed order: the same inputs give the same bits.

    The scores are ranked as given.  sigmoid is increasing, so ranking logits is ranking their
    exact sigmoids; float32 torch.sigmoid saturates (to 1.0 from about 17 on, to 0 below about
    -104) and rounds neighbouring logits to one value, so sigmoid(logits) has ties that the logits
    do not have, and its metrics can differ from those of the logits.  Pass what you want ranked."""
    for name, x in (("pos", pos), ("neg", neg)):
        if not isinstance(x, torch.Tensor):
            raise TypeError("{} must be a tensor, got {}".format(name, type(x).__name__))
        if x.dtype != torch.float32:
            raise TypeError("link_metrics ranks float32 scores, {} is {}".format(name, x.dtype))
        if not (x.dim() == 1 or (x.dim() == 2 and x.shape[1] == 1)):
            raise ValueError("{} must be [n] or [n, 1], got {}".format(name, tuple(x.shape)))
    P, N = int(pos.shape[0]), int(neg.shape[0])
    if P == 0 or N == 0:
        raise ValueError("link_metrics needs at least one positive and one negative score, got "
                         "{} and {}".format(P, N))
    if P + N > LINK_METRICS_MAX_SCORES:
        raise ValueError("link_metrics takes at most {} scores per call, got {} + {}".format(
            LINK_METRICS_MAX_SCORES, P, N))
    if neg.device != pos.device:
        raise ValueError("neg is on {}, pos on {}".format(neg.device, pos.device))
    if pos.device.type != "cuda":
        raise ValueError("link_metrics runs on the GPU, the inputs are on {}".format(pos.device))
    acc = accumulator
    if acc is not None:
        if not isinstance(acc, torch.Tensor):
            raise TypeError("accumulator must be a tensor, got {}".format(type(acc).__name__))
        if acc.dtype != torch.float64:
            raise TypeError("accumulator must be float64, got {}".format(acc.dtype))
        if tuple(acc.shape) != (8,) or not acc.is_contiguous():
            raise ValueError("accumulator must be a contiguous [8] tensor, got {}".format(
                tuple(acc.shape)))
        if acc.device != pos.device:
            raise ValueError("accumulator is on {}, pos on {}".format(acc.device, pos.device))
    p = pos.detach().reshape(P).contiguous()
    n = neg.detach().reshape(N).contiguous()
    lib = _capi.load()
    rows = C.c_size_t(0)
    _capi.check(lib.gf_link_metrics_partial_rows(P, C.byref(rows)))
    f64 = dict(dtype=torch.float64, device=p.device)
    partials = torch.empty((rows.value, _LINK_METRICS_PARTIAL_WORDS), **f64)
    out = torch.empty(3, **f64)
    with torch.cuda.device(p.device):
        _capi.check(lib.gf_link_metrics(
            p.data_ptr(), n.data_ptr(), P, N, partials.data_ptr(), rows.value, out.data_ptr(),
            _ptr(acc), p.device.index, _stream(p.device)))
    return out


WALK_MAX_REF_ENTRIES = 4096          # GF_WALK_MAX_REF_ENTRIES: Wr * (Lr + 1), one row's set in LDS


def check_walk_position_counts_args(nodes, ref=None):
    """Arguments of walk_position_counts, checked before anything is launched or allocated.
    Needs no device.  Returns (B, W, L + 1, Wr, Lr + 1)."""
    for name, x in (("nodes", nodes), ("ref", ref)):
        if x is None and name == "ref":
            continue
        if not isinstance(x, torch.Tensor):
            raise TypeError("{} must be a tensor, got {}".format(name, type(x).__name__))
        if x.dtype != torch.int64:
            raise TypeError("{} must be torch.int64, got {}".format(name, x.dtype))
        if x.dim() != 3:
            raise ValueError("{} must be [rows, walks, length + 1], got shape {}".format(
                name, tuple(x.shape)))
        if not 1 <= int(x.shape[2]) <= WALK_MAX_LENGTH + 1:
            raise ValueError("{} must hold walks of 0 to {} steps (1 to {} nodes), got {} nodes"
                             .format(name, WALK_MAX_LENGTH, WALK_MAX_LENGTH + 1, int(x.shape[2])))
    B, W, L1 = (int(n) for n in nodes.shape)
    Br, Wr, Lr1 = (B, W, L1) if ref is None else (int(n) for n in ref.shape)
    if Br != B:
        raise ValueError("nodes has {} rows, ref has {}".format(B, Br))
    if Wr * Lr1 > WALK_MAX_REF_ENTRIES:
        raise ValueError("walk_position_counts counts in at most {} entries per row, got "
                         "{} x {}".format(WALK_MAX_REF_ENTRIES, Wr, Lr1))
    if B >= 2 ** 31:
        raise ValueError("walk_position_counts takes fewer than 2**31 rows, got {}".format(B))
    if W * L1 * Lr1 >= 2 ** 31:
        raise ValueError("walk_position_counts writes fewer than 2**31 counts per row, got "
                         "{} x {} x {}".format(W, L1, Lr1))
    if ref is not None and ref.device != nodes.device:
        raise ValueError("ref is on {}, nodes on {}".format(ref.device, nodes.device))
    return B, W, L1, Wr, Lr1


def walk_position_counts(nodes: torch.Tensor, ref: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The position-count ("anonymous") encoding of temporal walks, CAWN's set-based
    anonymisation: an int32 tensor [B, W, L + 1, Lr + 1] with

        out[i, w, j, p] = #{w' < Wr : ref[i, w', p] == nodes[i, w, j]}   if nodes[i, w, j] >= 0
                          0                                              otherwise

    nodes: int64 [B, W, L + 1], the walks to encode (TemporalWalks.nodes); ref: int64
    [B, Wr, Lr + 1], the walks to count in, nodes itself when None.  With ref=None a node is
    encoded by how often it stands at each position of its own root's walks; for a link (u, v) a
    second call with the partner's walks as ref gives the counts relative to the other side.
    Negative entries (the slots of ended walks) encode to zeros and are never counted.  L and Lr
    are at most 32 and Wr * (Lr + 1) at most WALK_MAX_REF_ENTRIES; B == 0 or W == 0 returns an
    empty tensor without a launch.  The outputs are integers and carry no autograd.

    One kernel (csrc/walk_positions.hip) on the current stream, never synchronises: a workgroup
    per row holds ref[i] in LDS and compares every entry of nodes[i] with every entry of it,
    W (L + 1) * Wr (Lr + 1) compares per row."""
    B, W, L1, Wr, Lr1 = check_walk_position_counts_args(nodes, ref)
    dev = nodes.device
    if dev.type != "cuda":
        raise ValueError("walk_position_counts runs on the GPU, the inputs are on {}".format(dev))
    n = nodes.detach().contiguous()
    r = n if ref is None else ref.detach().contiguous()
    with torch.cuda.device(dev):
        out = torch.empty((B, W, L1, Lr1), dtype=torch.int32, device=dev)
        if B and W:
            _capi.check(_capi.load().gf_walk_position_counts(
                n.data_ptr(), _ptr(r), B, W, L1, Wr, Lr1, out.data_ptr(), dev.index,
                _stream(dev)))
    return out


LINK_LOSS_TILE = 1024                # GF_LINK_LOSS_TILE: logits per workgroup pass of the kernel
LINK_LOSS_SINGLE_TILES = 8           # GF_LINK_LOSS_SINGLE_TILES: up to here the forward is one launch
LINK_LOSS_MAX_PARTIAL_ROWS = 256     # GF_LINK_LOSS_MAX_PARTIAL_ROWS: half of them for each side
LINK_LOSS_ACC_FIELDS = 5             # GF_LINK_LOSS_ACC_FIELDS


class _LinkLoss(torch.autograd.Function):
    @staticmethod
    @_fwd
    def forward(ctx, pos, neg, acc):
        # pos [P], neg [N] contiguous, both fp32 or both bf16; acc None or float64 [5]
        P, N = pos.shape[0], neg.shape[0]
        lib = _capi.load()
        rows = C.c_size_t(0)
        _capi.check(lib.gf_link_loss_partial_rows(P, N, C.byref(rows)))
        partials = torch.empty(rows.value, dtype=torch.float64, device=pos.device) \
            if rows.value else None
        out = torch.empty((), dtype=torch.float32, device=pos.device)
        fn = lib.gf_link_loss_bf16 if pos.dtype == torch.bfloat16 else lib.gf_link_loss
        with torch.cuda.device(pos.device):
            _capi.check(fn(pos.data_ptr(), neg.data_ptr(), P, N, _ptr(partials), rows.value,
                           out.data_ptr(), _ptr(acc), pos.device.index, _stream(pos.device)))
        ctx.save_for_backward(pos, neg)
        return out

    @staticmethod
    @_bwd
    def backward(ctx, grad):
        pos, neg = ctx.saved_tensors
        need_pos, need_neg, _ = ctx.needs_input_grad
        if not (need_pos or need_neg):
            return None, None, None
        g = _grad_as(grad, torch.float32)
        gp = torch.empty_like(pos) if need_pos else None
        gn = torch.empty_like(neg) if need_neg else None
        lib = _capi.load()
        fn = lib.gf_link_loss_backward_bf16 if pos.dtype == torch.bfloat16 \
            else lib.gf_link_loss_backward
        with torch.cuda.device(pos.device):
            _capi.check(fn(pos.data_ptr(), neg.data_ptr(), pos.shape[0], neg.shape[0],
                           g.data_ptr(), _ptr(gp), _ptr(gn), pos.device.index,
                           _stream(pos.device)))
        return gp, gn, None


def link_loss(pos: torch.Tensor, neg: torch.Tensor,
              accumulator: Optional[torch.Tensor] = None) -> torch.Tensor:
    """mean(softplus(-pos)) + mean(softplus(neg)) as a float32 scalar tensor (shape []) on the
    GPU: the reference's training loss, criterion(pred_pos, ones) + criterion(pred_neg, zeros)
    with BCEWithLogitsLoss, in one launch (two beyond LINK_LOSS_SINGLE_TILES tiles of
    LINK_LOSS_TILE logits in all) and one more for the backward.

    pos: [P] or [P, 1], the logits of the true edges; neg: [N] or [N, 1], those of the negative
    ones, as EdgePredictor returns them; N need not be a multiple of P.  Both float32 or both
    bfloat16 on one GPU, P >= 1, N >= 1; any other dtype or a mixture raises TypeError.  Row
    slices of one buffer (out[:B], out[B:] of edge_score) are taken as they are; a non-contiguous
    input is copied.  Differentiable in pos and neg; only the logits are saved.

    Every term is float32 arithmetic, the sums are float64 in a fixed order and the loss is
    rounded to float32 once: the same inputs give the same bits.  bfloat16 logits follow the
    module's rule: the loss is float32 and equals link_loss(pos.float(), neg.float()) bit for
    bit, the gradients are bfloat16, the float32 gradients rounded once.

    accumulator: a float64 contiguous [LINK_LOSS_ACC_FIELDS] = [5] tensor on the same GPU, the
    running sums of an epoch (sum_loss, sum_loss_times_P, batches, nonfinite, sum_P), updated on
    the device in the forward from the float32 loss; nn.LinkLoss wraps it.  A NaN logit gives a
    NaN loss, infinities follow the formulas; a loss that is not finite adds 1 to `nonfinite`
    alone.

    Runs on the current stream and never synchronises."""
    for name, x in (("pos", pos), ("neg", neg)):
        if not isinstance(x, torch.Tensor):
            raise TypeError("{} must be a tensor, got {}".format(name, type(x).__name__))
    if (pos.dtype, neg.dtype) not in ((torch.float32,) * 2, (torch.bfloat16,) * 2):
        raise TypeError("link_loss computes in float32 and takes pos and neg both float32 or both "
                        "bfloat16, pos is {} and neg is {}".format(pos.dtype, neg.dtype))
    for name, x in (("pos", pos), ("neg", neg)):
        if not (x.dim() == 1 or (x.dim() == 2 and x.shape[1] == 1)):
            raise ValueError("{} must be [n] or [n, 1], got {}".format(name, tuple(x.shape)))
    P, N = int(pos.shape[0]), int(neg.shape[0])
    if P == 0 or N == 0:
        raise ValueError("link_loss needs at least one positive and one negative logit, got "
                         "{} and {}".format(P, N))
    if P >= 1 << 31 or N >= 1 << 31:
        raise ValueError("link_loss takes fewer than 2^31 logits on a side, got {} and {}".format(
            P, N))
    acc = accumulator
    if acc is not None:
        if not isinstance(acc, torch.Tensor):
            raise TypeError("accumulator must be a tensor, got {}".format(type(acc).__name__))
        if acc.dtype != torch.float64:
            raise TypeError("accumulator must be float64, got {}".format(acc.dtype))
        if tuple(acc.shape) != (LINK_LOSS_ACC_FIELDS,) or not acc.is_contiguous():
            raise ValueError("accumulator must be a contiguous [{}] tensor, got {}".format(
                LINK_LOSS_ACC_FIELDS, tuple(acc.shape)))
    if neg.device != pos.device:
        raise ValueError("neg is on {}, pos on {}".format(neg.device, pos.device))
    if acc is not None and acc.device != pos.device:
        raise ValueError("accumulator is on {}, pos on {}".format(acc.device, pos.device))
    if pos.device.type != "cuda":
        raise ValueError("link_loss runs on the GPU, the inputs are on {}".format(pos.device))
    return _LinkLoss.apply(pos.reshape(P).contiguous(), neg.reshape(N).contiguous(),
                           None if acc is None else acc.detach())


def _src_dtype(op, src):
    if not isinstance(src, torch.Tensor):
        raise TypeError("src must be a tensor, got {}".format(type(src).__name__))
    if src.dtype not in (torch.float32, torch.bfloat16):
        raise TypeError("{} computes in float32 and takes src float32 or bfloat16, src is {}"
                        .format(op, src.dtype))


def block_max(block, src: torch.Tensor) -> torch.Tensor:
    """out[d] = element-wise max over the edges into d of src[source(k)] (0 without in-edges):
    update_all(copy_src, max).  src float32 or bfloat16 (anything else raises TypeError); out and
    the gradient of src have its dtype.  A maximum is one of the inputs, so the bfloat16 op
    returns exactly what the float32 op returns on src.float(), and routes the gradient to the
    same edge (the lowest on ties)."""
    _src_dtype("block_max", src)
    if src.shape[0] != block.num_src_nodes():
        raise ValueError("src must have one row per source node")
    offsets, col, _ = block.segments()
    return _BlockMax.apply(src, offsets, col, block.num_dst_nodes(), block.num_edges())


def edge_softmax(block, logits: torch.Tensor) -> torch.Tensor:
    """Softmax of `logits[num_edges, ...]` over the edges that share a destination node
    (dgl.ops.edge_softmax with the default norm_by='dst')."""
    if logits.shape[0] != block.num_edges():
        raise ValueError("logits must have one row per edge")
    offsets, _, perm = block.segments()
    if perm is None:
        return _EdgeSoftmax.apply(logits, offsets, block.num_dst_nodes())
    y = _EdgeSoftmax.apply(logits[perm], offsets, block.num_dst_nodes())
    return torch.empty_like(y).index_copy(0, perm, y)


def block_reduce(block, src: torch.Tensor, edge_weight=None, mean: bool = False) -> torch.Tensor:
    """out[d] = sum (mean) over the edges k into d of edge_weight[k] * src[source(k)].
    src: [num_src_nodes, ...]; edge_weight: None or [num_edges, heads(, 1)], each head
    scaling `feature_size / heads` consecutive values.

    src is float32 or bfloat16, edge_weight float32 (under autocast a softmax output); anything
    else raises TypeError.  With a bfloat16 src the module's rule applies -- float32 arithmetic,
    one rounding on store --: out and the gradient of src are bfloat16 and equal, bit for bit,
    the float32 op's on src.float() rounded once (on a block with an explicit col, where a source
    may feed several edges, that gradient is summed in float32 and rounded once at the end); the
    gradient of edge_weight is float32 and equal to its."""
    _src_dtype("block_reduce", src)
    if edge_weight is not None:
        if not isinstance(edge_weight, torch.Tensor):
            raise TypeError("edge_weight must be a tensor or None, got {}".format(
                type(edge_weight).__name__))
        if edge_weight.dtype != torch.float32:
            raise TypeError("block_reduce computes in float32 and takes edge_weight float32 "
                            "(src float32 or bfloat16), src is {} and edge_weight is {}".format(
                                src.dtype, edge_weight.dtype))
    if src.shape[0] != block.num_src_nodes():
        raise ValueError("src must have one row per source node")
    offsets, col, perm = block.segments()
    if edge_weight is not None and perm is not None:
        edge_weight = edge_weight[perm]
    return _BlockReduce.apply(src, edge_weight, offsets, col, block.num_dst_nodes(), mean,
                              block.num_edges())
