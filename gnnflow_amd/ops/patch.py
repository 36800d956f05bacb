"""patch_project and patch_project_time (csrc/patch_project.hip): DyGFormer's patching and channel
projection straight from the planes a sequence reader returns, without the channel tensor."""
from typing import Optional

import torch

from .. import _capi
from ._common import (_check_on_gpu, _check_same_device, _check_tensors, _grad_as, _launch,
                      _partial_rows, _ptr)

PATCH_MAX_LENGTH = 512               # GF_PATCH_MAX_LENGTH
PATCH_MAX_WIDTH = 1024               # GF_PATCH_MAX_WIDTH, d
PATCH_MAX_PATCH_WIDTH = 4096         # GF_PATCH_MAX_PATCH_WIDTH, P * d
PATCH_MAX_CHANNELS = 128             # GF_PATCH_MAX_CHANNELS
PATCH_MAX_PARTIAL_ROWS = 256         # GF_PATCH_MAX_PARTIAL_ROWS


def _source_args(ids, table, delta_t, time_weight, time_bias, lengths):
    """the seven source arguments of gf_patch_project, one form given and the other null"""
    if ids is not None:
        return (ids.data_ptr(), table.data_ptr(), table.shape[0], None, None, None, _ptr(lengths))
    return (None, None, 0, delta_t.data_ptr(), time_weight.data_ptr(), time_bias.data_ptr(),
            _ptr(lengths))


class _PatchProject(torch.autograd.Function):
    """Either (ids, table) or (delta_t, time_weight, time_bias) is given, the rest None; only
    weight and bias get a gradient, and x is gathered again in the backward, not saved."""

    @staticmethod
    def forward(ctx, weight, bias, ids, table, delta_t, time_weight, time_bias, lengths, dims):
        R, L, P, d, lead = dims
        Cn = weight.shape[0]
        plane = ids if ids is not None else delta_t
        out = torch.empty(lead + (L // P, Cn), dtype=torch.float32, device=plane.device)
        if R:
            _launch(plane.device, "gf_patch_project", None, None,
                    _source_args(ids, table, delta_t, time_weight, time_bias, lengths) +
                    (R, L, P, d, weight.data_ptr(), bias.data_ptr(), Cn, out.data_ptr()))
        ctx.save_for_backward(ids, table, delta_t, time_weight, time_bias, lengths)
        ctx.dims = dims
        ctx.shapes = (tuple(weight.shape), plane.device)
        return out

    @staticmethod
    def backward(ctx, grad):
        need_w, need_b = ctx.needs_input_grad[:2]
        R, L, P, d, _ = ctx.dims
        (Cn, K), dev = ctx.shapes
        rest = (None,) * 7
        if not (need_w or need_b):
            return (None, None) + rest
        f32 = dict(dtype=torch.float32, device=dev)
        if R == 0:      # zeros, and nothing to launch
            return (torch.zeros((Cn, K), **f32) if need_w else None,
                    torch.zeros(Cn, **f32) if need_b else None) + rest
        g = _grad_as(grad, torch.float32)
        gw = torch.empty((Cn, K), **f32) if need_w else None
        gb = torch.empty(Cn, **f32) if need_b else None
        rows = _partial_rows(_capi.load().gf_patch_project_backward_partial_rows,
                             R * (L // P), Cn, K)
        partials = torch.empty((rows, Cn * (K + 1)), **f32)
        _launch(dev, "gf_patch_project_backward", None, None,
                _source_args(*ctx.saved_tensors) +
                (R, L, P, d, Cn, g.data_ptr(), partials.data_ptr(), rows, _ptr(gw), _ptr(gb)))
        return (gw, gb) + rest


def _check_patch(op, plane_name, plane, plane_dtype, lengths, d, weight, bias, patch_size):
    """What the two forms check in the same words, after their own source tensors.  Returns
    (R, L, P, lead)."""
    if plane.dtype != plane_dtype:
        raise TypeError("{} must be {}, got {}".format(plane_name, plane_dtype, plane.dtype))
    if lengths is not None and lengths.dtype != torch.int32:
        raise TypeError("lengths must be int32, got {}".format(lengths.dtype))
    for name, x in (("weight", weight), ("bias", bias)):
        if x.dtype != torch.float32:
            raise TypeError("{} computes in float32, {} is {}".format(op, name, x.dtype))
    if isinstance(patch_size, bool) or not isinstance(patch_size, int):
        raise TypeError("patch_size must be an int, got {}".format(type(patch_size).__name__))
    if plane.dim() < 1:
        raise ValueError("{} must be [*lead, L], got a scalar".format(plane_name))
    lead, L, P = tuple(int(n) for n in plane.shape[:-1]), int(plane.shape[-1]), patch_size
    if lengths is not None and tuple(lengths.shape) != lead:
        raise ValueError("lengths must be {}, the leading dimensions of {}, got {}".format(
            list(lead), plane_name, tuple(lengths.shape)))
    if not 1 <= d <= PATCH_MAX_WIDTH:
        raise ValueError("the rows have {} columns, {} takes 1 to {}".format(
            d, op, PATCH_MAX_WIDTH))
    if not 1 <= L <= PATCH_MAX_LENGTH:
        raise ValueError("{} has {} slots, {} takes 1 to {}".format(
            plane_name, L, op, PATCH_MAX_LENGTH))
    if P < 1 or L % P:
        raise ValueError("the {} slots are not a multiple of patch_size {}".format(L, P))
    if P * d > PATCH_MAX_PATCH_WIDTH:
        raise ValueError("a patch has patch_size * d = {} columns, {} takes up to {}".format(
            P * d, op, PATCH_MAX_PATCH_WIDTH))
    if weight.dim() != 2 or weight.shape[1] != P * d:
        raise ValueError("weight must be [C, patch_size * d] = [C, {}], got {}".format(
            P * d, tuple(weight.shape)))
    Cn = int(weight.shape[0])
    if not 1 <= Cn <= PATCH_MAX_CHANNELS:
        raise ValueError("weight has {} rows, {} takes 1 to {}".format(
            Cn, op, PATCH_MAX_CHANNELS))
    if tuple(bias.shape) != (Cn,):
        raise ValueError("bias must be [{}], got {}".format(Cn, tuple(bias.shape)))
    R = 1
    for n in lead:
        R *= n
    if R * (L // P) >= 2 ** 31:
        raise ValueError("{} takes fewer than 2**31 patches per call, got {}".format(
            op, R * (L // P)))
    return R, L, P, lead


def patch_project(ids: torch.Tensor, lengths: Optional[torch.Tensor], table: torch.Tensor,
                  weight: torch.Tensor, bias: torch.Tensor, patch_size: int) -> torch.Tensor:
    """F.linear(x.reshape(*lead, L // P, P * d), weight, bias) for the rows

        x[r, l, :] = table[ids[r, l], :]   if l < lengths[r] and 0 <= ids[r, l] < rows, else 0

    with x never stored: the rows are gathered into LDS and multiplied there, on the float32
    matrix instructions (csrc/patch_project.hip).  This is DynamicGraph.pair_sequence's rule for
    its node and edge parts followed by DyGFormer's proj: an id without a row (the self slot's
    eid of -1, the padding) is a zero row, and a patch wholly past lengths gives exactly bias.

    ids: int64 [*lead, L] (pair_sequence(...).nodes or .eids, [N, 2, L]); lengths: int32 [*lead]
    or None for "every slot filled"; table: float32 [rows, d], contiguous (a non-contiguous table
    is an error, not a copy); weight: float32 [C, P * d], an nn.Linear's; bias: float32 [C];
    patch_size: P.  1 <= d <= 1024, 1 <= L <= 512 with L % P == 0, P * d <= 4096, 1 <= C <= 128,
    fewer than 2**31 patches, everything on one GPU.  float32 only, inside an autocast region too:
    any other dtype raises TypeError.  Returns float32 [*lead, L // P, C].

    Gradients go to weight and bias only (the tables get none, as with the readers); the backward
    gathers x again from ids, sums in a fixed order through a workspace of at most 256 partial
    rows and 64 MiB, and is bit-identical from run to run.  Runs on the current stream and never
    synchronises; no rows, no launch."""
    _check_tensors(("ids", ids), ("table", table), ("weight", weight), ("bias", bias))
    if lengths is not None:
        _check_tensors(("lengths", lengths))
    if table.dtype != torch.float32:
        raise TypeError("patch_project computes in float32, table is {}".format(table.dtype))
    if table.dim() != 2:
        raise ValueError("table must be [rows, d], got {}".format(tuple(table.shape)))
    R, L, P, lead = _check_patch("patch_project", "ids", ids, torch.int64, lengths,
                                 int(table.shape[1]), weight, bias, patch_size)
    if not table.is_contiguous():
        raise ValueError("table must be contiguous: rows are read in place, not copied")
    _check_same_device("ids", ids, ("lengths", lengths), ("table", table), ("weight", weight),
                       ("bias", bias))
    _check_on_gpu("patch_project", ids.device)
    return _PatchProject.apply(
        weight.contiguous(), bias.contiguous(), ids.detach().contiguous(), table.detach(), None,
        None, None, None if lengths is None else lengths.detach().contiguous(),
        (R, L, P, int(table.shape[1]), lead))


def patch_project_time(delta_t: torch.Tensor, lengths: Optional[torch.Tensor],
                       time_weight: torch.Tensor, time_bias: torch.Tensor, weight: torch.Tensor,
                       bias: torch.Tensor, patch_size: int) -> torch.Tensor:
    """patch_project for the time channel: the rows are

        x[r, l, :] = cos(time_weight * delta_t[r, l] + time_bias)   if l < lengths[r], else 0

    evaluated where patch_project gathers, by the expression of ops.time_encode (a row holds that
    op's bits).  delta_t: float32 [*lead, L]; time_weight: float32 [dT, 1] or [dT] and time_bias:
    float32 [dT], a time encoder's (what nn.FixedTimeEncode holds); d = dT; the rest as in
    patch_project.  The time encoder gets no gradient: a trained one stays on the torch route."""
    _check_tensors(("delta_t", delta_t), ("time_weight", time_weight), ("time_bias", time_bias),
                   ("weight", weight), ("bias", bias))
    if lengths is not None:
        _check_tensors(("lengths", lengths))
    for name, x in (("time_weight", time_weight), ("time_bias", time_bias)):
        if x.dtype != torch.float32:
            raise TypeError("patch_project_time computes in float32, {} is {}".format(
                name, x.dtype))
    if time_bias.dim() != 1:
        raise ValueError("time_bias must be [dT], got {}".format(tuple(time_bias.shape)))
    dT = int(time_bias.shape[0])
    if tuple(time_weight.shape) not in ((dT,), (dT, 1)):
        raise ValueError("time_weight must be [dT] or [dT, 1] with dT = {}, got {}".format(
            dT, tuple(time_weight.shape)))
    R, L, P, lead = _check_patch("patch_project_time", "delta_t", delta_t, torch.float32, lengths,
                                 dT, weight, bias, patch_size)
    _check_same_device("delta_t", delta_t, ("lengths", lengths), ("time_weight", time_weight),
                       ("time_bias", time_bias), ("weight", weight), ("bias", bias))
    _check_on_gpu("patch_project_time", delta_t.device)
    return _PatchProject.apply(
        weight.contiguous(), bias.contiguous(), None, None, delta_t.detach().contiguous(),
        time_weight.detach().reshape(dT).contiguous(), time_bias.detach().contiguous(),
        None if lengths is None else lengths.detach().contiguous(), (R, L, P, dT, lead))
