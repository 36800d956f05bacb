"""ops.feed_forward's argument checks and the constructors' refusals of fused_feed_forward=True:
all raised in Python before any launch, so they are tested without a GPU."""
import pytest
import torch

from gnnflow_amd import ops
from gnnflow_amd.models import DyGFormer, GraphMixer


def args(C=3, Hd=4, lead=(2,), dtype=torch.float32):
    return [torch.zeros(*shape, dtype=dtype) for shape in
            (lead + (C,), (Hd, C), (Hd,), (C, Hd), (C,))]


def swap(i, t, **kw):
    a = args(**kw)
    a[i] = t(a[i]) if callable(t) else t
    return a


CHECKS = [
    ("not a tensor", lambda: ops.feed_forward(*swap(0, [1.0])), TypeError, "x must be a tensor"),
    ("x dtype", lambda: ops.feed_forward(*swap(0, lambda t: t.bfloat16())), TypeError,
     "computes in float32, x is"),
    ("w2 dtype", lambda: ops.feed_forward(*swap(3, lambda t: t.double())), TypeError,
     "computes in float32, w2 is"),
    ("scalar", lambda: ops.feed_forward(*swap(0, torch.zeros(()))), ValueError, "got a scalar"),
    ("w1 shape", lambda: ops.feed_forward(*swap(1, torch.zeros(4, 5))), ValueError,
     "w1 must be [Hd, C]"),
    ("b1 shape", lambda: ops.feed_forward(*swap(2, torch.zeros(5))), ValueError, "b1 must be [4]"),
    ("w2 shape", lambda: ops.feed_forward(*swap(3, torch.zeros(4, 3))), ValueError,
     "w2 must be [3, 4]"),
    ("b2 shape", lambda: ops.feed_forward(*swap(4, torch.zeros(3, 1))), ValueError,
     "b2 must be [3]"),
    ("Hd = 0", lambda: ops.feed_forward(*args(Hd=0)), ValueError, "hidden width must be >= 1"),
    ("C = 0", lambda: ops.feed_forward(*args(C=0)), ValueError, "0 columns"),
    ("C = 257", lambda: ops.feed_forward(*args(C=257)), ValueError, "257 columns"),
    ("x not contiguous", lambda: ops.feed_forward(*swap(0, lambda t: t[::2], lead=(4,))),
     ValueError, "x must be contiguous"),
    ("w2 not contiguous", lambda: ops.feed_forward(*swap(3, torch.zeros(4, 3).t())), ValueError,
     "w2 must be contiguous"),
    ("p = 1", lambda: ops.feed_forward(*args(), 1.0, 1), ValueError, "[0, 1)"),
    ("p < 0", lambda: ops.feed_forward(*args(), -0.1, 1), ValueError, "[0, 1)"),
    ("no seed", lambda: ops.feed_forward(*args(), 0.5), ValueError, "needs a dropout_seed"),
    ("cpu", lambda: ops.feed_forward(*args()), ValueError, "runs on the GPU"),
    ("DyGFormer", lambda: DyGFormer(4, 4, channel_dim=65, fused_feed_forward=True), ValueError,
     "4 channels of channel_dim 65"),
    ("GraphMixer", lambda: GraphMixer(4, 4, dim_embed=257, fused_feed_forward=True), ValueError,
     "up to 256, got 257"),
]


@pytest.mark.parametrize("call,error,fragment", [c[1:] for c in CHECKS], ids=[c[0] for c in CHECKS])
def test_refused_before_any_launch(call, error, fragment):
    with pytest.raises(error) as info:
        call()
    assert fragment in str(info.value)
