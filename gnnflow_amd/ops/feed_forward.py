"""feed_forward (csrc/feed_forward.hip): the Linear -> GELU -> dropout -> Linear of DyGFormer's
encoder block and GraphMixer's channel MLP as one kernel each way, without the hidden tensor."""
import ctypes as C
from typing import Optional

import torch

from .. import _capi
from ._common import (_check_on_gpu, _check_same_device, _check_tensors, _dropout_args, _grad_as,
                      _grads_like, _launch, _partial_rows, _ptr)

FEED_FORWARD_MAX_WIDTH = 256         # GF_FEED_FORWARD_MAX_WIDTH, C


class _FeedForward(torch.autograd.Function):
    """Saved: the five inputs and nothing of size M * Hd; u, g and the mask are recomputed in the
    backward, which is launched only for the gradients needs_input_grad asks for."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, p32, seed):
        Hd, Cn = w1.shape
        M = x.numel() // Cn
        y = torch.empty_like(x)
        if M:
            _launch(x.device, "gf_feed_forward", None, None,
                    (x.data_ptr(), w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr(), M,
                     Cn, Hd, C.c_float(p32), C.c_uint64(seed), y.data_ptr()))
        ctx.save_for_backward(x, w1, b1, w2, b2)
        ctx.args = (M, p32, seed)
        return y

    @staticmethod
    def backward(ctx, grad):
        needs = ctx.needs_input_grad[:5]
        if not any(needs):
            return (None,) * 7
        x, w1, b1, w2, b2 = ctx.saved_tensors
        M, p32, seed = ctx.args
        Hd, Cn = w1.shape
        if M == 0:      # zeros, and nothing to launch
            return _grads_like((x, w1, b1, w2, b2), needs, zero=True) + (None, None)
        grads = _grads_like((x, w1, b1, w2, b2), needs)
        g = _grad_as(grad, torch.float32)
        rows, partials = 0, None
        if any(needs[1:]):
            rows = _partial_rows(_capi.load().gf_feed_forward_backward_partial_rows, M, Cn, Hd)
            partials = torch.empty((rows, 2 * Hd * Cn + Hd + Cn), dtype=torch.float32,
                                   device=x.device)
        _launch(x.device, "gf_feed_forward_backward", None, None,
                (x.data_ptr(), w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), M, Cn, Hd,
                 C.c_float(p32), C.c_uint64(seed), g.data_ptr(), _ptr(partials), rows) +
                tuple(_ptr(t) for t in grads))
        return grads + (None, None)


def _fused_route(flag):
    """A model's fused_feed_forward flag as (route, compute_dtype): False, True (float32) or
    "bfloat16"; anything else is refused."""
    if isinstance(flag, (bool, int)) and flag in (False, True):
        return bool(flag), torch.float32
    if isinstance(flag, str) and flag == "bfloat16":
        return flag, torch.bfloat16
    raise ValueError('fused_feed_forward must be False, True or "bfloat16", got {!r}'.format(flag))


def _workspace(device, Cn, Hd, backward):
    """The buffer a bfloat16 pass packs bf(w1) and bf(w2) into; it lives for that pass alone."""
    size = _partial_rows(_capi.load().gf_feed_forward_bf16_workspace, Cn, Hd, int(backward))
    return torch.empty(size, dtype=torch.uint8, device=device)


class _FeedForwardBf16(torch.autograd.Function):
    """_FeedForward on the bfloat16 matrix instruction (csrc/feed_forward_bf16.hip): float32
    tensors in and out, the same things saved.  Each pass packs the rounded weights into a
    workspace of its own, freed with the pass: at most 2 (forward) or 3 (backward) arrays of
    2 * round64(Hd) * round64(C) bytes, and nothing held between the two."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, p32, seed):
        Hd, Cn = w1.shape
        M = x.numel() // Cn
        y = torch.empty_like(x)
        if M:
            ws = _workspace(x.device, Cn, Hd, False)
            _launch(x.device, "gf_feed_forward_bf16", None, None,
                    (x.data_ptr(), w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr(), M,
                     Cn, Hd, C.c_float(p32), C.c_uint64(seed), ws.data_ptr(), ws.numel(),
                     y.data_ptr()))
        ctx.save_for_backward(x, w1, b1, w2, b2)
        ctx.args = (M, p32, seed)
        return y

    @staticmethod
    def backward(ctx, grad):
        needs = ctx.needs_input_grad[:5]
        if not any(needs):
            return (None,) * 7
        x, w1, b1, w2, b2 = ctx.saved_tensors
        M, p32, seed = ctx.args
        Hd, Cn = w1.shape
        if M == 0:      # zeros, and nothing to launch
            return _grads_like((x, w1, b1, w2, b2), needs, zero=True) + (None, None)
        grads = _grads_like((x, w1, b1, w2, b2), needs)
        g = _grad_as(grad, torch.float32)
        rows, partials = 0, None
        if any(needs[1:]):
            rows = _partial_rows(_capi.load().gf_feed_forward_bf16_backward_partial_rows, M, Cn,
                                 Hd)
            partials = torch.empty((rows, 2 * Hd * Cn + Hd + Cn), dtype=torch.float32,
                                   device=x.device)
        ws = _workspace(x.device, Cn, Hd, True)
        _launch(x.device, "gf_feed_forward_bf16_backward", None, None,
                (x.data_ptr(), w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), M, Cn, Hd,
                 C.c_float(p32), C.c_uint64(seed), g.data_ptr(), ws.data_ptr(), ws.numel(),
                 _ptr(partials), rows) + tuple(_ptr(t) for t in grads))
        return grads + (None, None)


def feed_forward(x: torch.Tensor, w1: torch.Tensor, b1: torch.Tensor, w2: torch.Tensor,
                 b2: torch.Tensor, dropout_p: float = 0.0,
                 dropout_seed: Optional[int] = None,
                 compute_dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """F.linear(dropout(F.gelu(F.linear(x, w1, b1))), w2, b2) with the hidden activation never
    stored.  With M the product of x's leading dimensions, m < M, j < Hd, c < C:

        u[m, j] = sum_c x[m, c] w1[j, c] + b1[j]
        g[m, j] = 0.5 u (1 + erf(u / sqrt 2))                         torch's default GELU
        w[m, j] = 1 / (1 - p) if gf_philox4x32_10_first(seed, m * Hd + j, 0) >= T else 0
        y[m, c] = sum_j (g w)[m, j] w2[c, j] + b2[c]

    x: float32 [..., C], contiguous; w1 [Hd, C], b1 [Hd], w2 [C, Hd], b2 [C]: the tensors of two
    nn.Linear as they are, float32 and contiguous, everything on one GPU.  p = float32(dropout_p),
    T = uint32(float64(p) * 2**32) (block_attention's T and scale); p == 0 gives w = 1 and is the
    call without the two arguments, bit for bit; dropout_p > 0 needs a dropout_seed in [0, 2**64).
    A dropped element is an exact 0 that is multiplied like any other.  Returns float32 of x's
    shape.

    1 <= C <= 256 (the output accumulators: 16 quads), Hd >= 1 with M * Hd < 2**63 (the hidden
    width is only ever walked in chunks).  float32 only, inside an autocast region too: any other
    dtype raises TypeError.

    Gradients go to x, w1, b1, w2 and b2, each only where it is required; with frozen weights the
    weight pass is not launched.  The forward saves its inputs and nothing of size M * Hd: the
    backward recomputes u from x, draws the mask again and uses g'(u) = 0.5 (1 + erf(u / sqrt 2))
    + u exp(-u^2 / 2) / sqrt(2 pi).  The weight gradients are summed in a fixed order through a
    workspace of at most 256 partial rows and 64 MiB; every output element has one writer,
    nothing is atomic, and the bits are the same on every run.  Runs on the current stream
    (csrc/feed_forward.hip: both GEMMs of each pass on the float32 matrix instructions) and
    never synchronises; no rows, no launch.

    compute_dtype=torch.bfloat16 runs both products of every pass on the bfloat16 matrix
    instruction (csrc/feed_forward_bf16.hip).  The tensors stay float32 in memory, in and out;
    only the matrix operands are rounded, bf(v) = v.to(bfloat16), and every sum is float32:

        u  = b1 + sum_c bf(x) bf(w1)                    float32, never rounded
        h  = bf(gelu(u) w)                              w as above: same counter, T and scale
        y  = b2 + sum_j h bf(w2)
        dh = sum_c bf(dy) bf(w2)        du = bf(dh w gelu'(u))
        dx = sum_j du bf(w1)    dw1 = sum_m du bf(x)    dw2 = sum_m bf(dy) h
        db1 = colsum du         db2 = colsum bf(dy)     (summed after rounding)

    Everything else above holds as it stands: the limits, what is saved, the order and
    determinism of the sums, p == 0.  Each pass first packs bf(w1) and bf(w2) into a workspace it
    frees again (2 or 3 arrays of 2 * round64(Hd) * round64(C) bytes).  The keyword means the
    same inside an autocast region and outside it.  Any other compute_dtype raises ValueError."""
    if compute_dtype not in (torch.float32, torch.bfloat16):
        raise ValueError("compute_dtype must be torch.float32 or torch.bfloat16, got {}".format(
            compute_dtype))
    named = (("x", x), ("w1", w1), ("b1", b1), ("w2", w2), ("b2", b2))
    _check_tensors(*named)
    for name, t in named:
        if t.dtype != torch.float32 and compute_dtype == torch.bfloat16:
            raise TypeError("feed_forward takes float32 tensors whatever its compute_dtype, {} is "
                            "{}".format(name, t.dtype))
        if t.dtype != torch.float32:
            raise TypeError("feed_forward computes in float32, {} is {}".format(name, t.dtype))
    if x.dim() < 1:
        raise ValueError("x must be [..., C], got a scalar")
    if w1.dim() != 2 or w1.shape[1] != x.shape[-1]:
        raise ValueError("w1 must be [Hd, C] with C = {}, the last dimension of x, got {}".format(
            x.shape[-1], tuple(w1.shape)))
    Hd, Cn = (int(n) for n in w1.shape)
    if not 1 <= Cn <= FEED_FORWARD_MAX_WIDTH:
        raise ValueError("x has {} columns, feed_forward takes 1 to {}".format(
            Cn, FEED_FORWARD_MAX_WIDTH))
    if Hd < 1:
        raise ValueError("w1 has no rows: the hidden width must be >= 1")
    for name, t, shape in (("b1", b1, (Hd,)), ("w2", w2, (Cn, Hd)), ("b2", b2, (Cn,))):
        if tuple(t.shape) != shape:
            raise ValueError("{} must be {}, got {}".format(name, list(shape), tuple(t.shape)))
    if (x.numel() // Cn) * Hd >= 2 ** 63:
        raise ValueError("feed_forward takes fewer than 2**63 hidden elements per call")
    p32, seed = _dropout_args(dropout_p, dropout_seed, seed_required=True)
    for name, t in named:
        if not t.is_contiguous():
            raise ValueError("{} must be contiguous: it is read in place, not copied".format(name))
    _check_same_device("x", x, *named[1:])
    _check_on_gpu("feed_forward", x.device)
    function = _FeedForwardBf16 if compute_dtype == torch.bfloat16 else _FeedForward
    return function.apply(x, w1, b1, w2, b2, p32, seed)
