"""edge_softmax, block_reduce and block_max: the segment kernels of csrc/block_ops.hip."""
import torch

from ._common import _bwd, _check_tensors, _f32, _fwd, _grad_as, _launch, _ptr, _scratch


class _EdgeSoftmax(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, offsets, num_dst):
        x = _f32(logits)
        E = x.shape[0]
        heads = x.numel() // E if E else 0
        y = torch.empty_like(x)
        if E:
            _launch(x.device, "gf_block_edge_softmax", None, None,
                    (offsets.data_ptr(), num_dst, E, heads, x.data_ptr(), y.data_ptr()))
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
            _launch(y.device, "gf_block_edge_softmax_backward", None, None,
                    (offsets.data_ptr(), ctx.num_dst, E, y.numel() // E, y.data_ptr(),
                     g.data_ptr(), gx.data_ptr()))
        return gx, None, None


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
            _launch(s.device, "gf_block_reduce", "gf_block_reduce_bf16", s.dtype,
                    (offsets.data_ptr(), num_dst, _ptr(col), s.data_ptr(), dim, _ptr(w), heads,
                     1 if mean else 0, out.data_ptr()))
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
                _launch(s.device, "gf_block_reduce_backward", "gf_block_reduce_backward_bf16",
                        s.dtype,
                        (offsets.data_ptr(), num_dst, _ptr(col), s.data_ptr(), dim, _ptr(w),
                         heads, 1 if mean else 0, g.data_ptr(), _ptr(gs), s.shape[0], _ptr(gw)),
                        bf16_tail=(_ptr(_scratch(s, col, need_src)),))
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
            _launch(s.device, "gf_block_reduce_max", "gf_block_reduce_max_bf16", s.dtype,
                    (offsets.data_ptr(), num_dst, _ptr(col), s.data_ptr(), dim, out.data_ptr(),
                     arg.data_ptr()))
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
        _launch(g.device, "gf_block_reduce_max_backward", "gf_block_reduce_max_backward_bf16",
                dtype,
                (num_dst, _ptr(col), dim, _ptr(g), arg.data_ptr(), gs.data_ptr(), shape[0]),
                bf16_tail=(_ptr(_scratch(gs, col)),))
        return gs, None, None, None, None


def _src_dtype(op, src):
    _check_tensors(("src", src))
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
        # not _check_tensors: this one may be None, and its message says so
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
