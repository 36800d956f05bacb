"""ops.sequence_attention's argument checks and DyGFormer(fused_attention=True)'s constructor
refusals: all raised in Python before any launch, so they are tested without a GPU."""
import pytest
import torch

from gnnflow_amd import ops
from gnnflow_amd.models import DyGFormer


def qkv(S=4, H=2, dh=3, n=2, dtype=torch.float32):
    return torch.zeros(n, S, 3 * H * dh, dtype=dtype)


CHECKS = [
    ("not a tensor", lambda: ops.sequence_attention([1.0], 2), TypeError, "must be a tensor"),
    ("dtype", lambda: ops.sequence_attention(qkv(dtype=torch.bfloat16), 2), TypeError,
     "computes in float32"),
    ("heads type", lambda: ops.sequence_attention(qkv(), 2.0), TypeError, "num_heads must be an"),
    ("rank", lambda: ops.sequence_attention(qkv()[0], 2), ValueError, "must be [n, S, 3 * H * dh]"),
    ("heads", lambda: ops.sequence_attention(qkv(), 0), ValueError, "num_heads must be >= 1"),
    ("last dimension", lambda: ops.sequence_attention(torch.zeros(2, 4, 20), 2), ValueError,
     "3 * num_heads * head_dim"),
    ("S = 0", lambda: ops.sequence_attention(qkv(S=0), 2), ValueError, "0 tokens"),
    ("S = 129", lambda: ops.sequence_attention(qkv(S=129), 2), ValueError, "129 tokens"),
    ("dh = 129", lambda: ops.sequence_attention(qkv(H=1, dh=129), 1), ValueError, "129 columns"),
    ("H dh", lambda: ops.sequence_attention(qkv(H=9, dh=128), 9), ValueError, "= 1152"),
    ("p = 1", lambda: ops.sequence_attention(qkv(), 2, 1.0, 1), ValueError, "[0, 1)"),
    ("p < 0", lambda: ops.sequence_attention(qkv(), 2, -0.1, 1), ValueError, "[0, 1)"),
    ("no seed", lambda: ops.sequence_attention(qkv(), 2, 0.5), ValueError, "needs a dropout_seed"),
    ("not contiguous", lambda: ops.sequence_attention(qkv(S=8)[:, ::2], 2), ValueError,
     "must be contiguous"),
    ("cpu", lambda: ops.sequence_attention(qkv(), 2), ValueError, "runs on the GPU"),
    ("model: sequence", lambda: DyGFormer(4, 4, max_length=130, patch_size=2, fused_attention=True),
     ValueError, "2 * max_length / patch_size = 130"),
    ("model: head", lambda: DyGFormer(4, 4, channel_dim=65, num_heads=2, fused_attention=True),
     ValueError, "dim / num_heads = 130"),
]


@pytest.mark.parametrize("call,error,fragment", [c[1:] for c in CHECKS], ids=[c[0] for c in CHECKS])
def test_refused_before_any_launch(call, error, fragment):
    with pytest.raises(error) as info:
        call()
    assert fragment in str(info.value)

