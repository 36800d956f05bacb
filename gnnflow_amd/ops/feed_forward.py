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


def feed_forward(x: torch.Tensor, w1: torch.Tensor, b1: torch.Tensor, w2: torch.Tensor,
                 b2: torch.Tensor, dropout_p: float = 0.0,
                 dropout_seed: Optional[int] = None) -> torch.Tensor:
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
    never synchronises; no rows, no launch."""
    named = (("x", x), ("w1", w1), ("b1", b1), ("w2", w2), ("b2", b2))
    _check_tensors(*named)
    for name, t in named:
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
    return _FeedForward.apply(x, w1, b1, w2, b2, p32, seed)
