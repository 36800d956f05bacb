"""What the op modules share: the one path to a native launch, the pointer and gradient helpers
of the autograd Functions, and the one copy of every argument check that more than one op makes
in the same words."""
import ctypes as C

import torch

from .. import _capi


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


def _grads_like(tensors, needs, zero=False):
    """A gradient buffer for each tensor that needs one, None for the others: uninitialised for a
    kernel to fill, zeros when nothing is launched."""
    make = torch.zeros_like if zero else torch.empty_like
    return tuple(make(t) if need else None for t, need in zip(tensors, needs))


# The autograd Functions of the ops that take bfloat16 call no torch op that autocast would
# recast, and custom_fwd / custom_bwd without cast_inputs keep it that way: the forward sees the
# tensors as they are given, the backward runs under the forward's autocast state wherever
# loss.backward() is called.
_fwd = torch.amp.custom_fwd(device_type="cuda")
_bwd = torch.amp.custom_bwd(device_type="cuda")


def _scratch(t, col, wanted=True):
    """The float32 buffer a bfloat16 gradient of `t`'s shape is summed in when the block has an
    explicit col; None for float32, for the sampler's layout, or when it is not wanted."""
    if t.dtype != torch.bfloat16 or col is None or not wanted:
        return None
    return torch.empty(t.shape, dtype=torch.float32, device=t.device)


def _launch(device, name, bf16_name, dtype, args, bf16_tail=()):
    """Every native launch of the package: entry point `bf16_name` for a bfloat16 `dtype`, `name`
    otherwise (a float32-only op passes None, None), called on `device` with `args`, the device
    index and torch's current stream.  The two names are spelled out because the suffix is not
    regular (gf_block_attention_bf16_backward, gf_block_reduce_backward_bf16).  `bf16_tail` is
    what a bfloat16 entry point alone takes after the stream: the float32 scratch of three
    backwards, the float32 out of gf_block_gat_bf16.  The library is looked up through
    _capi.load() and the entry point by attribute, per call."""
    lib = _capi.load()
    with torch.cuda.device(device):
        if dtype == torch.bfloat16:
            rc = getattr(lib, bf16_name)(*args, device.index, _stream(device), *bf16_tail)
        else:
            rc = getattr(lib, name)(*args, device.index, _stream(device))
        _capi.check(rc)


def _partial_rows(fn, *counts):
    """The size the library derives from `counts` through `fn`, one of its *_partial_rows entry
    points (or gf_edge_rank_scratch, in bytes): what the caller then allocates."""
    rows = C.c_size_t(0)
    _capi.check(fn(*counts, C.byref(rows)))
    return rows.value


# ---- argument checks shared word for word; each op still lists, in its own order, what it checks

def _check_tensors(*named):
    for name, t in named:
        if not isinstance(t, torch.Tensor):
            raise TypeError("{} must be a tensor, got {}".format(name, type(t).__name__))


def _check_same_device(anchor_name, anchor, *named):
    """Every named tensor (None: an optional one that was not given) is where `anchor` is."""
    for name, t in named:
        if t is not None and t.device != anchor.device:
            raise ValueError("{} is on {}, {} on {}".format(name, t.device, anchor_name,
                                                            anchor.device))


def _check_on_gpu(op, device):
    if device.type != "cuda":
        raise ValueError("{} runs on the GPU, the inputs are on {}".format(op, device))


def _check_accumulator(acc, fields):
    """Type, dtype and shape of the float64 running sums of link_metrics and link_loss.  Its
    device is checked by each op, at the place in its own order."""
    if not isinstance(acc, torch.Tensor):
        raise TypeError("accumulator must be a tensor, got {}".format(type(acc).__name__))
    if acc.dtype != torch.float64:
        raise TypeError("accumulator must be float64, got {}".format(acc.dtype))
    if tuple(acc.shape) != (fields,) or not acc.is_contiguous():
        raise ValueError("accumulator must be a contiguous [{}] tensor, got {}".format(
            fields, tuple(acc.shape)))


def _dropout_args(dropout_p, dropout_seed, seed_required):
    """(p32, seed) of a Philox dropout: p32 the float32 value the kernels see, seed 0 when
    nothing is dropped.  seed_required: None is a seed not given, an error when dropout_p > 0
    (block_attention, block_gat); otherwise the op's signature defaults it
    (dropout_relu_layer_norm)."""
    dropout_p = float(dropout_p)
    if not 0.0 <= dropout_p < 1.0:          # NaN fails too
        raise ValueError("dropout_p must be in [0, 1), got {}".format(dropout_p))
    p32 = C.c_float(dropout_p).value        # the fp32 value the kernels see
    if p32 >= 1.0:
        raise ValueError("dropout_p rounds to 1 in float32")
    if dropout_seed is not None or not seed_required:
        dropout_seed = int(dropout_seed)
        if not 0 <= dropout_seed < 2 ** 64:
            raise ValueError("dropout_seed must be in [0, 2**64), got {}".format(dropout_seed))
    elif dropout_p > 0:
        raise ValueError("dropout_p > 0 needs a dropout_seed")
    return p32, dropout_seed if p32 > 0 else 0
