"""ops.token_mix's argument checks and the constructors' refusals of fused_token_mix=True: all
raised in Python before any launch, so they are tested without a GPU."""
import pytest
import torch

from gnnflow_amd import ops
from gnnflow_amd.models import GraphMixer
from gnnflow_amd.models.graphmixer import MixerBlock


def args(N=2, K=3, Kh=4, C=5, dtype=torch.float32):
    return [torch.zeros(*shape, dtype=dtype) for shape in
            ((N, K, C), (C,), (C,), (Kh, K), (Kh,), (K, Kh), (K,))]


def swap(i, t, **kw):
    a = args(**kw)
    a[i] = t(a[i]) if callable(t) else t
    return a


def on_meta(a):      # the only other device a machine without a GPU has
    return [a[0].to("meta")] + a[1:]


CHECKS = [
    ("not a tensor", lambda: ops.token_mix(*swap(1, [1.0])), TypeError, "gamma must be a tensor"),
    ("x dtype", lambda: ops.token_mix(*swap(0, lambda t: t.bfloat16())), TypeError,
     "computes in float32, x is"),
    ("w2 dtype", lambda: ops.token_mix(*swap(5, lambda t: t.double())), TypeError,
     "computes in float32, w2 is"),
    ("x shape", lambda: ops.token_mix(*swap(0, torch.zeros(3, 5))), ValueError,
     "x must be [N, K, C]"),
    ("w1 shape", lambda: ops.token_mix(*swap(3, torch.zeros(4, 2))), ValueError,
     "w1 must be [Kh, K]"),
    ("gamma shape", lambda: ops.token_mix(*swap(1, torch.zeros(4))), ValueError,
     "gamma must be [5]"),
    ("beta shape", lambda: ops.token_mix(*swap(2, torch.zeros(5, 1))), ValueError,
     "beta must be [5]"),
    ("b1 shape", lambda: ops.token_mix(*swap(4, torch.zeros(3))), ValueError, "b1 must be [4]"),
    ("w2 shape", lambda: ops.token_mix(*swap(5, torch.zeros(4, 3))), ValueError,
     "w2 must be [3, 4]"),
    ("b2 shape", lambda: ops.token_mix(*swap(6, torch.zeros(4))), ValueError, "b2 must be [3]"),
    ("K = 0", lambda: ops.token_mix(*args(K=0)), ValueError, "0 tokens"),
    ("K = 65", lambda: ops.token_mix(*args(K=65)), ValueError, "65 tokens"),
    ("Kh = 0", lambda: ops.token_mix(*args(Kh=0)), ValueError, "0 hidden units"),
    ("Kh = 65", lambda: ops.token_mix(*args(Kh=65)), ValueError, "65 hidden units"),
    ("C = 0", lambda: ops.token_mix(*args(C=0)), ValueError, "0 columns"),
    ("C = 257", lambda: ops.token_mix(*args(C=257)), ValueError, "257 columns"),
    ("2^63 elements", lambda: ops.token_mix(*swap(0, torch.zeros(1, 1, 256).expand(
        2 ** 49, 1, 256), K=1, Kh=64, C=256)), ValueError, "fewer than 2**63 elements"),
    ("eps", lambda: ops.token_mix(*args(), 0.0), ValueError, "eps must be positive"),
    ("x not contiguous", lambda: ops.token_mix(*swap(0, lambda t: t[::2], N=4)), ValueError,
     "x must be contiguous"),
    ("w2 not contiguous", lambda: ops.token_mix(*swap(5, torch.zeros(4, 3).t())), ValueError,
     "w2 must be contiguous"),
    ("p = 1", lambda: ops.token_mix(*args(), 1e-5, 1.0, 1), ValueError, "[0, 1)"),
    ("p < 0", lambda: ops.token_mix(*args(), 1e-5, -0.1, 1), ValueError, "[0, 1)"),
    ("no seed", lambda: ops.token_mix(*args(), 1e-5, 0.5), ValueError, "needs a dropout_seed"),
    ("seed range", lambda: ops.token_mix(*args(), 1e-5, 0.5, 2 ** 64), ValueError,
     "[0, 2**64)"),
    ("mixed devices", lambda: ops.token_mix(*on_meta(args())), ValueError, "gamma is on cpu"),
    ("cpu", lambda: ops.token_mix(*args()), ValueError, "runs on the GPU"),
]

REFUSALS = [
    ("tokens", lambda: MixerBlock(65, 16, 0.5, 4.0, 0.1, fused_token_mix=True),
     "up to 64 tokens and hidden units, got 65 and 32"),
    ("hidden", lambda: MixerBlock(40, 16, 2.0, 4.0, 0.1, fused_token_mix=True),
     "up to 64 tokens and hidden units, got 40 and 80"),
    ("width", lambda: MixerBlock(32, 257, 0.5, 4.0, 0.1, fused_token_mix=True),
     "width of up to 256, got 257"),
    ("GraphMixer", lambda: GraphMixer(4, 4, num_tokens=65, fused_token_mix=True),
     "up to 64 tokens"),
]


@pytest.mark.parametrize("call,error,fragment", [c[1:] for c in CHECKS], ids=[c[0] for c in CHECKS])
def test_refused_before_any_launch(call, error, fragment):
    with pytest.raises(error) as info:
        call()
    assert fragment in str(info.value)


@pytest.mark.parametrize("make,fragment", [c[1:] for c in REFUSALS], ids=[c[0] for c in REFUSALS])
def test_constructors_refuse_what_the_op_would(make, fragment):
    with pytest.raises(ValueError) as info:
        make()
    assert fragment in str(info.value)
    assert MixerBlock(65, 257, 2.0, 4.0, 0.1) is not None      # the default route has no limits
