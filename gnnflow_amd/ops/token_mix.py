"""token_mix (csrc/token_mix.hip): the token-mixing half of GraphMixer's MixerBlock, LayerNorm ->
Linear over the tokens -> GELU -> dropout -> Linear -> dropout -> residual, as one kernel each way
without a transposed copy or a hidden tensor."""
import ctypes as C
import math
from typing import Optional

import torch

from .. import _capi
from ._common import (_check_on_gpu, _check_same_device, _check_tensors, _dropout_args, _grad_as,
                      _grads_like, _launch, _partial_rows, _ptr)

TOKEN_MIX_MAX_TOKENS = 64            # GF_TOKEN_MIX_MAX_TOKENS, K and Kh
TOKEN_MIX_MAX_WIDTH = 256            # GF_TOKEN_MIX_MAX_WIDTH, C


class _TokenMix(torch.autograd.Function):
    """Saved: the seven inputs and mean, rstd [N, K]; nothing of size N * K * C or N * Kh * C.  z,
    u, h and both masks are recomputed in the backward, which is launched only for the gradients
    needs_input_grad asks for."""

    @staticmethod
    def forward(ctx, x, gamma, beta, w1, b1, w2, b2, eps, p32, seed):
        N, K, Cn = x.shape
        Kh = w1.shape[0]
        y = torch.empty_like(x)
        mean = torch.empty((N, K), dtype=torch.float32, device=x.device)
        rstd = torch.empty_like(mean)
        if N:
            _launch(x.device, "gf_token_mix", None, None,
                    (x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), w1.data_ptr(), b1.data_ptr(),
                     w2.data_ptr(), b2.data_ptr(), N, K, Kh, Cn, C.c_float(eps), C.c_float(p32),
                     C.c_uint64(seed), y.data_ptr(), mean.data_ptr(), rstd.data_ptr()))
        ctx.save_for_backward(x, gamma, beta, w1, b1, w2, b2, mean, rstd)
        ctx.args = (p32, seed)
        return y

    @staticmethod
    def backward(ctx, grad):
        needs = ctx.needs_input_grad[:7]
        if not any(needs):
            return (None,) * 10
        inputs, (mean, rstd) = ctx.saved_tensors[:7], ctx.saved_tensors[7:]
        x, gamma, beta, w1, b1, w2, _ = inputs
        p32, seed = ctx.args
        N, K, Cn = x.shape
        Kh = w1.shape[0]
        if N == 0:      # zeros, and nothing to launch
            return _grads_like(inputs, needs, zero=True) + (None, None, None)
        grads = _grads_like(inputs, needs)
        g = _grad_as(grad, torch.float32)
        rows, partials = 0, None
        if any(needs[1:]):
            rows = _partial_rows(_capi.load().gf_token_mix_backward_partial_rows, N, K, Kh, Cn)
            partials = torch.empty((rows, 2 * K * Kh + K + Kh + 2 * Cn), dtype=torch.float32,
                                   device=x.device)
        _launch(x.device, "gf_token_mix_backward", None, None,
                (x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), w1.data_ptr(), b1.data_ptr(),
                 w2.data_ptr(), mean.data_ptr(), rstd.data_ptr(), N, K, Kh, Cn, C.c_float(p32),
                 C.c_uint64(seed), g.data_ptr(), _ptr(partials), rows) +
                tuple(_ptr(t) for t in grads))
        return grads + (None, None, None)


def token_mix(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, w1: torch.Tensor,
              b1: torch.Tensor, w2: torch.Tensor, b2: torch.Tensor, eps: float = 1e-5,
              dropout_p: float = 0.0, dropout_seed: Optional[int] = None) -> torch.Tensor:
    """x + drop(F.linear(drop(F.gelu(F.linear(F.layer_norm(x, [C], gamma, beta, eps).transpose(1,
    2), w1, b1))), w2, b2)).transpose(1, 2), the first line of MixerBlock.forward, with neither
    transpose made and nothing of x's size stored besides the result.  With n < N, k < K, j < Kh,
    c < C:

        mean[n,k], var[n,k]  over c of x[n,k,:]  (biased)      rstd = 1 / sqrt(var + eps)
        xh[n,k,c] = (x - mean) rstd                            z = xh gamma[c] + beta[c]
        u[n,j,c]  = b1[j] + sum_k w1[j,k] z[n,k,c]
        h[n,j,c]  = 0.5 u (1 + erf(u / sqrt 2)) m1[n,j,c]
        t[n,k,c]  = b2[k] + sum_j w2[k,j] h[n,j,c]
        y[n,k,c]  = x[n,k,c] + t[n,k,c] m2[n,k,c]
        m1 = 1 / (1 - p) if gf_philox4x32_10_first(seed, (n C + c) Kh + j, 0) >= T else 0
        m2 = 1 / (1 - p) if gf_philox4x32_10_first(seed, (n C + c) K  + k, 1) >= T else 0

    x: float32 [N, K, C]; gamma, beta [C] (the LayerNorm's); w1 [Kh, K], b1 [Kh], w2 [K, Kh], b2
    [K]: the two nn.Linear of the token MLP as they are; all float32, contiguous, on one GPU.  p =
    float32(dropout_p), T = uint32(float64(p) * 2**32) (block_attention's T and scale), the same p
    for both masks; p == 0 gives m1 = m2 = 1 and is the call without the two arguments, bit for
    bit; dropout_p > 0 needs a dropout_seed in [0, 2**64).  Returns float32 [N, K, C].

    1 <= K, Kh <= 64 (a weight is one LDS tile), 1 <= C <= 256, N C max(K, Kh) < 2**63, eps > 0.
    float32 only, inside an autocast region too: any other dtype raises TypeError.

    Gradients go to all seven tensors, each only where it is required.  The forward saves its
    inputs and mean, rstd [N, K]; the backward recomputes z, u and h, draws both masks again, and
    with dt = dy m2, dh = w2^T dt, du = dh m1 g'(u), dz = w1^T du, a = dz gamma gives dx = dy +
    rstd (a - mean_c a - xh mean_c(a xh)) and the six parameter gradients, summed in a fixed order
    through at most 512 partial rows (one per workgroup) and a reduction launch: one writer per
    element, nothing atomic, the same bits on every run.  With every parameter frozen neither the
    partial rows nor the reduction are made.  Runs on the current stream (csrc/token_mix.hip: all
    six products on the float32 matrix instructions) and never synchronises; no rows, no
    launch."""
    named = (("x", x), ("gamma", gamma), ("beta", beta), ("w1", w1), ("b1", b1), ("w2", w2),
             ("b2", b2))
    _check_tensors(*named)
    for name, t in named:
        if t.dtype != torch.float32:
            raise TypeError("token_mix computes in float32, {} is {}".format(name, t.dtype))
    if x.dim() != 3:
        raise ValueError("x must be [N, K, C], got {}".format(tuple(x.shape)))
    N, K, Cn = (int(n) for n in x.shape)
    if w1.dim() != 2 or w1.shape[1] != K:
        raise ValueError("w1 must be [Kh, K] with K = {}, the tokens of x, got {}".format(
            K, tuple(w1.shape)))
    Kh = int(w1.shape[0])
    for what, n in (("tokens", K), ("hidden units", Kh)):
        if not 1 <= n <= TOKEN_MIX_MAX_TOKENS:
            raise ValueError("{} {}, token_mix takes 1 to {}".format(n, what, TOKEN_MIX_MAX_TOKENS))
    if not 1 <= Cn <= TOKEN_MIX_MAX_WIDTH:
        raise ValueError("x has {} columns, token_mix takes 1 to {}".format(
            Cn, TOKEN_MIX_MAX_WIDTH))
    for name, t, shape in (("gamma", gamma, (Cn,)), ("beta", beta, (Cn,)), ("b1", b1, (Kh,)),
                           ("w2", w2, (K, Kh)), ("b2", b2, (K,))):
        if tuple(t.shape) != shape:
            raise ValueError("{} must be {}, got {}".format(name, list(shape), tuple(t.shape)))
    if N * Cn * max(K, Kh) >= 2 ** 63:
        raise ValueError("token_mix takes fewer than 2**63 elements per call")
    eps = float(eps)
    if not (eps > 0.0 and math.isfinite(eps)):
        raise ValueError("eps must be positive and finite, got {}".format(eps))
    p32, seed = _dropout_args(dropout_p, dropout_seed, seed_required=True)
    for name, t in named:
        if not t.is_contiguous():
            raise ValueError("{} must be contiguous: it is read in place, not copied".format(name))
    _check_same_device("x", x, *named[1:])
    _check_on_gpu("token_mix", x.device)
    return _TokenMix.apply(x, gamma, beta, w1, b1, w2, b2, eps, p32, seed)
