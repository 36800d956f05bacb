"""sequence_attention (csrc/sequence_attention.hip): the self-attention of DyGFormer's encoder
block between in_proj and out_proj, from the packed in_proj rows, without the [S, S] weights."""
import ctypes as C
from typing import Optional

import torch

from ._common import _check_on_gpu, _check_tensors, _dropout_args, _grad_as, _launch

SEQ_ATTENTION_MAX_LENGTH = 128       # GF_SEQ_ATTENTION_MAX_LENGTH, S
SEQ_ATTENTION_MAX_HEAD_DIM = 128     # GF_SEQ_ATTENTION_MAX_HEAD_DIM, dh
SEQ_ATTENTION_MAX_WIDTH = 1024       # GF_SEQ_ATTENTION_MAX_WIDTH, H * dh


class _SequenceAttention(torch.autograd.Function):
    """qkv alone gets a gradient.  Saved: qkv and the rows' log-sum-exp [n, H, S]; the weights and
    the mask are recomputed in the backward."""

    @staticmethod
    def forward(ctx, qkv, num_heads, p32, seed):
        n, S, width = qkv.shape
        dh = width // (3 * num_heads)
        out = torch.empty((n, S, num_heads * dh), dtype=torch.float32, device=qkv.device)
        lse = torch.empty((n, num_heads, S), dtype=torch.float32, device=qkv.device)
        if n:
            _launch(qkv.device, "gf_sequence_attention", None, None,
                    (qkv.data_ptr(), n, S, num_heads, dh, C.c_float(p32), C.c_uint64(seed),
                     out.data_ptr(), lse.data_ptr()))
        ctx.save_for_backward(qkv, lse)
        ctx.args = (num_heads, dh, p32, seed)
        return out

    @staticmethod
    def backward(ctx, grad):
        if not ctx.needs_input_grad[0]:
            return None, None, None, None
        qkv, lse = ctx.saved_tensors
        num_heads, dh, p32, seed = ctx.args
        n, S, _ = qkv.shape
        gqkv = torch.empty_like(qkv)
        if n:
            g = _grad_as(grad, torch.float32)
            _launch(qkv.device, "gf_sequence_attention_backward", None, None,
                    (qkv.data_ptr(), lse.data_ptr(), n, S, num_heads, dh, C.c_float(p32),
                     C.c_uint64(seed), g.data_ptr(), gqkv.data_ptr()))
        return gqkv, None, None, None


def sequence_attention(qkv: torch.Tensor, num_heads: int, dropout_p: float = 0.0,
                       dropout_seed: Optional[int] = None) -> torch.Tensor:
    """Unmasked multi-head self-attention over the rows F.linear(x, in_proj_weight, in_proj_bias)
    of an nn.MultiheadAttention, taken as they are (no split, no transpose, no copy):

        s[r,h,i,j]   = (sum_c q[r,i,h,c] k[r,j,h,c]) / sqrt(dh)
        a[r,h,i,:]   = softmax_j(s[r,h,i,:])
        out[r,i,h,:] = sum_j (a[r,h,i,j] w[r,h,i,j]) v[r,j,h,:]

    qkv: float32 [n, S, 3 * H * dh], contiguous, the last dimension [q | k | v], each [H, dh];
    num_heads: H.  Returns float32 [n, S, H * dh], the heads concatenated: what out_proj reads.
    With p = float32(dropout_p) > 0, T = uint32(float64(p) * 2**32):

        keep[r,h,i,j] = gf_philox4x32_10_first(seed, ((r H + h) S + i) S + j, 0) >= T
        w             = 1 / (1 - p) if keep else 0                    (block_attention's T and scale)

    The mask is never stored; the backward draws it again.  A dropped weight is an exact 0 that is
    multiplied with its v row like any other weight (the row is not skipped): it contributes
    exactly 0 for finite v, and a non-finite v[r,j,h,:] reaches every query of its (row, head)
    whether j was dropped or not, as in torch's dense product.  dropout_p == 0 is the call without
    the two arguments, bit for bit; dropout_p > 0 needs a dropout_seed in [0, 2**64).

    1 <= S <= 128, 1 <= dh <= 128, H >= 1, H * dh <= 1024, n * H < 2**31.  float32 only, inside an
    autocast region too: any other dtype raises TypeError.  The gradient goes to qkv, one packed
    [n, S, 3 * H * dh] tensor; the forward saves qkv and a float32 [n, H, S] log-sum-exp, never an
    [S, S] tensor; the backward writes every element once, without atomics, and is bit-identical
    from run to run.  One launch each way (csrc/sequence_attention.hip: one workgroup per (row,
    head), both products on the float32 matrix instructions), on the current stream, never
    synchronising; no rows, no launch."""
    _check_tensors(("qkv", qkv))
    if qkv.dtype != torch.float32:
        raise TypeError("sequence_attention computes in float32, qkv is {}".format(qkv.dtype))
    if isinstance(num_heads, bool) or not isinstance(num_heads, int):
        raise TypeError("num_heads must be an int, got {}".format(type(num_heads).__name__))
    if qkv.dim() != 3:
        raise ValueError("qkv must be [n, S, 3 * H * dh], got {}".format(tuple(qkv.shape)))
    if num_heads < 1:
        raise ValueError("num_heads must be >= 1, got {}".format(num_heads))
    n, S, width = (int(x) for x in qkv.shape)
    if not 1 <= S <= SEQ_ATTENTION_MAX_LENGTH:
        raise ValueError("qkv has {} tokens a row, sequence_attention takes 1 to {}".format(
            S, SEQ_ATTENTION_MAX_LENGTH))
    if width == 0 or width % (3 * num_heads):
        raise ValueError("the last dimension of qkv must be 3 * num_heads * head_dim, {} is no "
                         "multiple of 3 * {}".format(width, num_heads))
    dh = width // (3 * num_heads)
    if dh > SEQ_ATTENTION_MAX_HEAD_DIM:
        raise ValueError("a head has {} columns, sequence_attention takes 1 to {}".format(
            dh, SEQ_ATTENTION_MAX_HEAD_DIM))
    if num_heads * dh > SEQ_ATTENTION_MAX_WIDTH:
        raise ValueError("num_heads * head_dim = {}, sequence_attention takes up to {}".format(
            num_heads * dh, SEQ_ATTENTION_MAX_WIDTH))
    if n * num_heads >= 2 ** 31:
        raise ValueError("sequence_attention takes fewer than 2**31 (row, head) pairs per call, "
                         "got {}".format(n * num_heads))
    p32, seed = _dropout_args(dropout_p, dropout_seed, seed_required=True)
    if not qkv.is_contiguous():
        raise ValueError("qkv must be contiguous: the rows are read in place, not copied")
    _check_on_gpu("sequence_attention", qkv.device)
    return _SequenceAttention.apply(qkv, num_heads, p32, seed)
