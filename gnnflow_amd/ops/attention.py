"""block_attention (csrc/block_attention.hip) and block_gat (csrc/block_gat.hip): the fused
attention of a sampled block, with the Philox attention dropout inside the kernels."""
from typing import Optional

import torch

from ._common import (_bwd, _check_on_gpu, _check_tensors, _dropout_args, _fwd, _grad_as,
                      _grads_like, _launch, _ptr, _scratch)

MAX_ATTENTION_WIDTH = 1024      # GF_BLOCK_ATTENTION_MAX_WIDTH: the limit on heads * head_dim


class _BlockAttention(torch.autograd.Function):
    @staticmethod
    @_fwd
    def forward(ctx, q, k, v, offsets, num_dst, slope, p, seed, want_dropped):
        # q [num_dst, H, D], k / v [E, H, D] contiguous, all fp32 or all bf16, edges grouped by
        # destination; out in their dtype.  att is the pre-dropout softmax (saved), dropped =
        # att * w, both fp32.  The dropout kernels are entry points of their own
        # (block_attention.hip says why); p == 0 calls the plain ones, without p and seed.
        E, H, D = k.shape
        out = torch.empty((num_dst, H, D), dtype=q.dtype, device=q.device)
        att = torch.empty((E, H), dtype=torch.float32, device=q.device)
        dropped = torch.empty_like(att) if want_dropped and p > 0 else None
        args = (offsets.data_ptr(), num_dst, E, H, D, q.data_ptr(), k.data_ptr(), v.data_ptr(),
                slope)
        if p > 0:
            _launch(q.device, "gf_block_attention_dropout", "gf_block_attention_dropout_bf16",
                    q.dtype, args + (p, seed, out.data_ptr(), att.data_ptr(), _ptr(dropped)))
        else:
            _launch(q.device, "gf_block_attention", "gf_block_attention_bf16", q.dtype,
                    args + (out.data_ptr(), att.data_ptr()))
        ctx.save_for_backward(q, k, v, att, offsets)
        ctx.meta = (slope, p, seed)
        shown = dropped if p > 0 else att
        if not want_dropped:
            return out, None
        ctx.mark_non_differentiable(shown)
        return out, shown

    @staticmethod
    @_bwd
    def backward(ctx, grad, _grad_att):
        q, k, v, att, offsets = ctx.saved_tensors
        slope, p, seed = ctx.meta
        g = _grad_as(grad, q.dtype)
        E, H, D = k.shape
        needs = ctx.needs_input_grad[:3]
        gq, gk, gv = _grads_like((q, k, v), needs)
        if any(needs):
            args = (offsets.data_ptr(), q.shape[0], E, H, D, q.data_ptr(), k.data_ptr(),
                    v.data_ptr(), att.data_ptr(), slope)
            grads = (g.data_ptr(), _ptr(gq), _ptr(gk), _ptr(gv))
            if p > 0:
                _launch(q.device, "gf_block_attention_dropout_backward",
                        "gf_block_attention_dropout_bf16_backward", q.dtype,
                        args + (p, seed) + grads)
            else:
                _launch(q.device, "gf_block_attention_backward",
                        "gf_block_attention_bf16_backward", q.dtype, args + grads)
        return gq, gk, gv, None, None, None, None, None, None


class _NoEdgeAttention(torch.autograd.Function):
    """A block without edges or without destinations: zeros, and zero gradients."""
    @staticmethod
    def forward(ctx, q, k, v):
        ctx.save_for_backward(q, k, v)
        return torch.zeros_like(q)

    @staticmethod
    def backward(ctx, grad):
        return _grads_like(ctx.saved_tensors, ctx.needs_input_grad, zero=True)


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
    p32, seed = _dropout_args(dropout_p, dropout_seed, seed_required=True)
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
    # unlike block_gat, block_attention checks neither that q, k, v are tensors nor their devices
    if E == 0 or num_dst == 0:
        out = _NoEdgeAttention.apply(q, k, v)      # nothing to launch
        return (out, torch.zeros((E, H), dtype=torch.float32, device=q.device)) \
            if return_attention else out
    offsets, _, perm = block.segments()
    if perm is not None:
        k, v = k[perm], v[perm]
    out, att = _BlockAttention.apply(q, k, v, offsets, num_dst, float(negative_slope), p32, seed,
                                     bool(return_attention))
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
        _launch(feat.device, "gf_block_gat", "gf_block_gat_bf16", feat.dtype,
                (offsets.data_ptr(), num_dst, E, _ptr(col), num_src, H, D, feat.data_ptr(),
                 el.data_ptr(), er.data_ptr(), slope, p, seed, out.data_ptr(), att.data_ptr(),
                 _ptr(dropped)),
                bf16_tail=(out32.data_ptr(),))
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
        needs = ctx.needs_input_grad[:3]
        gfeat, gel, ger = _grads_like((feat, el, er), needs)
        if any(needs):
            _launch(feat.device, "gf_block_gat_backward", "gf_block_gat_backward_bf16",
                    feat.dtype,
                    (offsets.data_ptr(), er.shape[0], att.shape[0], _ptr(col), num_src, H, D,
                     feat.data_ptr(), el.data_ptr(), er.data_ptr(), att.data_ptr(),
                     out32.data_ptr(), slope, p, seed, g.data_ptr(), _ptr(gfeat), _ptr(gel),
                     _ptr(ger)),
                    bf16_tail=(_ptr(_scratch(feat, col, needs[0])),))
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
        return _grads_like(ctx.saved_tensors, ctx.needs_input_grad, zero=True)


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
    p32, seed = _dropout_args(dropout_p, dropout_seed, seed_required=True)
    _check_tensors(("feat", feat), ("el", el), ("er", er))
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
    # not _check_same_device: this message names all three devices at once
    if el.device != feat.device or er.device != feat.device:
        raise ValueError("feat is on {}, el on {}, er on {}".format(
            feat.device, el.device, er.device))
    _check_on_gpu("block_gat", feat.device)
    feat, el, er = feat.contiguous(), el.contiguous(), er.contiguous()
    if E == 0 or num_dst == 0:
        out = _NoEdgeGat.apply(feat, el, er)       # nothing to launch
        return (out, torch.zeros((E, H), dtype=torch.float32, device=feat.device)) \
            if return_attention else out
    offsets, col, perm = block.segments()
    out, att = _BlockGat.apply(feat, el, er, offsets, col, num_dst, E, float(negative_slope),
                               p32, seed, bool(return_attention))
    if not return_attention:
        return out
    if perm is not None:
        att = torch.empty_like(att).index_copy(0, perm, att)
    return out, att
