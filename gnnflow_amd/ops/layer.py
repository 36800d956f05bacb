"""dropout_relu_layer_norm (csrc/layer_epilogue.hip) and gru_cell (csrc/gru_cell.hip): the
element-wise tails of the temporal attention layer and of the memory updater."""
import ctypes as C
from typing import Optional

import torch

from .. import _capi
from ._common import (_bwd, _check_on_gpu, _check_same_device, _check_tensors, _dropout_args,
                      _fwd, _grad_as, _grads_like, _launch, _partial_rows, _ptr)

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
            _launch(x.device, "gf_layer_epilogue", "gf_layer_epilogue_bf16", x.dtype,
                    (x.data_ptr(), weight.data_ptr(), bias.data_ptr(), R, D, eps, p32, seed,
                     out.data_ptr(), mean.data_ptr(), rstd.data_ptr()))
        ctx.save_for_backward(x, weight, mean, rstd)      # neither out nor a mask
        ctx.p32, ctx.seed = p32, seed
        return out

    @staticmethod
    @_bwd
    def backward(ctx, grad):
        x, weight, mean, rstd = ctx.saved_tensors
        R, D = x.shape
        needs = ctx.needs_input_grad[:3]
        if R == 0:      # zeros, and nothing to launch
            return _grads_like((x, weight, weight), needs, zero=True) + (None, None, None)
        if not any(needs):
            return None, None, None, None, None, None
        g = _grad_as(grad, torch.float32)
        gx, gw, gb = _grads_like((x, weight, weight), needs)
        partials, rows = None, 0
        if needs[1] or needs[2]:
            rows = _partial_rows(_capi.load().gf_layer_epilogue_backward_partial_rows, R)
            partials = torch.empty((rows, 2 * D), dtype=torch.float32, device=x.device)
        _launch(x.device, "gf_layer_epilogue_backward", "gf_layer_epilogue_backward_bf16",
                x.dtype,
                (x.data_ptr(), weight.data_ptr(), mean.data_ptr(), rstd.data_ptr(), R, D, ctx.p32,
                 ctx.seed, g.data_ptr(), _ptr(partials), rows, _ptr(gx), _ptr(gw), _ptr(gb)))
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
    _check_tensors(("x", x), ("weight", weight), ("bias", bias))
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
    p32, seed = _dropout_args(dropout_p, dropout_seed, seed_required=False)
    _check_same_device("x", x, ("weight", weight), ("bias", bias))
    _check_on_gpu("dropout_relu_layer_norm", x.device)
    return _DropoutReluLayerNorm.apply(x.contiguous(), weight.contiguous(), bias.contiguous(),
                                       eps, p32, seed)


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
            _launch(hx.device, "gf_gru_cell", "gf_gru_cell_bf16", gi.dtype,
                    (gi.data_ptr(), gh.data_ptr(), hx.data_ptr(), _ptr(residual),
                     int(residual is not None and residual.dtype == torch.bfloat16), N, H,
                     num_last, out.data_ptr(), _ptr(last)))
        ctx.save_for_backward(gi, gh, hx)      # neither the gates nor a workspace
        ctx.residual_dtype = None if residual is None else residual.dtype
        ctx.mark_non_differentiable(last)
        return out, last

    @staticmethod
    @_bwd
    def backward(ctx, grad, _grad_last):
        gi, gh, hx = ctx.saved_tensors
        N, H = hx.shape
        needs = ctx.needs_input_grad[:3]
        need_res = ctx.needs_input_grad[3] and ctx.residual_dtype is not None
        if N == 0:      # zeros, and nothing to launch
            return _grads_like((gi, gh, hx), needs, zero=True) + \
                (torch.zeros_like(hx, dtype=ctx.residual_dtype) if need_res else None, None)
        if not (any(needs) or need_res):
            return None, None, None, None, None
        g = _grad_as(grad, torch.float32)
        dgi, dgh, dhx = _grads_like((gi, gh, hx), needs)
        if any(needs):
            _launch(hx.device, "gf_gru_cell_backward", "gf_gru_cell_backward_bf16", gi.dtype,
                    (gi.data_ptr(), gh.data_ptr(), hx.data_ptr(), N, H, g.data_ptr(), _ptr(dgi),
                     _ptr(dgh), _ptr(dhx)))
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
    _check_tensors(("gi", gi), ("gh", gh), ("hx", hx))
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
    _check_same_device("hx", hx, ("gi", gi), ("gh", gh), ("residual", residual))
    _check_on_gpu("gru_cell", hx.device)
    return _GruCell.apply(gi.contiguous(), gh.contiguous(), hx.contiguous(),
                          None if residual is None else residual.contiguous(), num_last)
