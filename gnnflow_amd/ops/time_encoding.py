"""time_encode and time_encode_cat: the fused time encoding of csrc/time_encode.hip."""
import torch

from .. import _capi
from ._common import (_bwd, _check_on_gpu, _check_same_device, _check_tensors, _fwd, _grad_as,
                      _grads_like, _launch, _partial_rows, _ptr)


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
            _launch(t.device, "gf_time_encode_cat", "gf_time_encode_cat_bf16", out_dtype,
                    (_ptr(a), wa, _ptr(b), wb, t.data_ptr(), weight.data_ptr(), bias.data_ptr(),
                     n, T, out.data_ptr()))
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
        needs = ctx.needs_input_grad[2:4]
        gw = gb = None
        if any(needs):
            # n == 0: zeros, and nothing to launch
            gw, gb = _grads_like((weight, bias), needs, zero=True)
            if n:
                rows = _partial_rows(_capi.load().gf_time_encode_backward_partial_rows, n)
                partials = torch.empty((rows, 2, T), dtype=torch.float32, device=t.device)
                _launch(t.device, "gf_time_encode_backward", "gf_time_encode_backward_bf16",
                        ctx.out_dtype,
                        (t.data_ptr(), weight.data_ptr(), bias.data_ptr(), n, T, g.data_ptr(),
                         g.shape[1], sum(ctx.widths), partials.data_ptr(), rows, _ptr(gw),
                         _ptr(gb)))
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
    named_parts = tuple(("parts[{}]".format(i), p) for i, p in enumerate(parts))
    for name, x in (("t", t), ("weight", weight), ("bias", bias)) + named_parts:
        _check_tensors((name, x))      # type and dtype of one argument before the next one's
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
    _check_same_device("t", t, ("weight", weight), ("bias", bias), *named_parts)
    _check_on_gpu("time_encode_cat", t.device)
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
