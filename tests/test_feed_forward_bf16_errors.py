"""What compute_dtype= and fused_feed_forward="bfloat16" refuse: all raised in Python before any
launch, so they are tested without a GPU."""
import pytest
import torch

from gnnflow_amd import ops
from gnnflow_amd.models import DyGFormer, GraphMixer
from gnnflow_amd.models.dygformer import EncoderBlock
from gnnflow_amd.models.graphmixer import MixerBlock
from tests.test_feed_forward_errors import args, swap

BF16 = torch.bfloat16
CHECKS = [
    ("float16", lambda: ops.feed_forward(*args(), compute_dtype=torch.float16), ValueError,
     "torch.float32 or torch.bfloat16"),
    ("a string", lambda: ops.feed_forward(*args(), compute_dtype="bfloat16"), ValueError,
     "torch.float32 or torch.bfloat16"),
    ("x dtype", lambda: ops.feed_forward(*swap(0, lambda t: t.bfloat16()), compute_dtype=BF16),
     TypeError, "float32 tensors whatever its compute_dtype, x is torch.bfloat16"),
    ("w1 dtype", lambda: ops.feed_forward(*swap(1, lambda t: t.bfloat16()), compute_dtype=BF16),
     TypeError, "w1 is torch.bfloat16"),
    ("cpu", lambda: ops.feed_forward(*args(), compute_dtype=BF16), ValueError, "runs on the GPU"),
    ("EncoderBlock flag", lambda: EncoderBlock(20, 2, 0.1, fused_feed_forward="float16"),
     ValueError, "False, True or \"bfloat16\""),
    ("DyGFormer flag", lambda: DyGFormer(4, 4, fused_feed_forward=torch.bfloat16), ValueError,
     "False, True or \"bfloat16\""),
    ("MixerBlock flag", lambda: MixerBlock(8, 20, 0.5, 4.0, 0.1, fused_feed_forward=2), ValueError,
     "False, True or \"bfloat16\""),
    ("GraphMixer flag", lambda: GraphMixer(4, 4, fused_feed_forward="bf16"), ValueError,
     "False, True or \"bfloat16\""),
    ("DyGFormer width", lambda: DyGFormer(4, 4, channel_dim=65, fused_feed_forward="bfloat16"),
     ValueError, "4 channels of channel_dim 65"),
    ("GraphMixer width", lambda: GraphMixer(4, 4, dim_embed=257, fused_feed_forward="bfloat16"),
     ValueError, "up to 256, got 257"),
]


@pytest.mark.parametrize("call,error,fragment", [c[1:] for c in CHECKS], ids=[c[0] for c in CHECKS])
def test_refused_before_any_launch(call, error, fragment):
    with pytest.raises(error) as info:
        call()
    assert fragment in str(info.value)
