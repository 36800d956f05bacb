"""ops.feed_forward (csrc/feed_forward.hip) against its definition in float64 on the CPU, the
output and all five gradients written out, with the mask of tests/attention_dropout_ref.py; its
exact properties bit for bit; and EncoderBlock / GraphMixer(fused_feed_forward=True) against the
default route.

The tolerance is test_gpu_sequence_attention.py's rule: the same expression in plain float32 torch
on the GPU (F.linear, F.gelu, the same mask, F.linear, autograd) is held against the float64
reference, and the kernel may err 4 times as much, with a floor of 16 * 2^-24 * max|ref| per
tensor.  Worst (kernel error) / (allowed error) seen on an MI355X over the thirteen cases: y 0.24,
dx 0.22, dw1 0.12, db1 0.12, dw2 0.11, db2 0.10; 0.04 on a model's output, 0.09 on a parameter's
gradient.
"""
import copy
import functools
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import attention_dropout_ref as R

pytestmark = pytest.mark.gpu

SEED = R.SEED                      # above 2^32
TWO_ROWS = (257, 5, 7)             # 5 row tiles: the smallest M with two partial rows
SHAPES = [(1, 1, 1), (3, 5, 7), (16, 16, 16), (17, 20, 33), (64, 64, 64), (65, 68, 65),
          (130, 100, 400), (70, 200, 800), (33, 256, 96), TWO_ROWS]
DROPPED = [(17, 20, 33), (65, 68, 65), (70, 200, 800)]
LEAD = {130: (10, 13), 70: (2, 35)}          # x's leading shape where it is not [M]
CASES = [s + (0.0,) for s in SHAPES] + [s + (0.5,) for s in DROPPED]
NAMES = ("y", "dx", "dw1", "db1", "dw2", "db2")


def weights(M, Hd, p, seed):
    """w [M, Hd] float64 of the op's definition"""
    if p == 0:
        return np.ones((M, Hd))
    u = R.philox_first(seed, np.arange(M * Hd, dtype=np.uint64), 0)
    return ((u >= np.uint32(R.threshold(p))) * float(R.scale(p))).reshape(M, Hd)


def reference(x, w1, b1, w2, b2, dy, w):
    """y and the five gradients, float64, from [M, C] rows"""
    u = x @ w1.T + b1
    cdf = 0.5 * (1 + torch.erf(u / math.sqrt(2)))
    h = u * cdf * w
    dh = dy @ w2
    du = dh * w * (cdf + u * torch.exp(-u * u / 2) / math.sqrt(2 * math.pi))
    return h @ w2.T + b2, du @ w1, du.T @ x, du.sum(0), dy.T @ h, dy.sum(0)


def torch32(x, w1, b1, w2, b2, dy, w):
    leaves = [t.clone().requires_grad_() for t in (x, w1, b1, w2, b2)]
    y = F.linear(F.gelu(F.linear(leaves[0], leaves[1], leaves[2])) * w, leaves[3], leaves[4])
    y.backward(dy)
    return [y.detach()] + [t.grad for t in leaves]


def allowed(yardstick, ref):
    """4 max(max|torch32 - ref|, 16 * 2^-24 * max|ref|)"""
    ref = ref.double().cpu().numpy()
    err = np.abs(yardstick.double().cpu().numpy().reshape(ref.shape) - ref).max()
    return 4 * max(err, 16 * 2.0 ** -24 * np.abs(ref).max())


def ratio(got, yardstick, ref):
    ref = ref.double().cpu()
    return float((got.double().cpu().reshape(ref.shape) - ref).abs().max()) / allowed(yardstick, ref)


@functools.lru_cache(maxsize=None)
def case(M, C, Hd, p):
    """inputs on the GPU (x and dy in x's leading shape), the float64 reference and the float32
    yardstick of a case; computed once"""
    g = torch.Generator().manual_seed(1000 * M + Hd)
    x, dy = torch.randn(M, C, generator=g), torch.randn(M, C, generator=g)
    w1, b1 = torch.randn(Hd, C, generator=g) / C ** 0.5, torch.randn(Hd, generator=g) / 2
    w2, b2 = torch.randn(C, Hd, generator=g) / Hd ** 0.5, torch.randn(C, generator=g) / 2
    w = torch.from_numpy(weights(M, Hd, p, SEED))
    ref = reference(*(t.double() for t in (x, w1, b1, w2, b2, dy)), w)
    x, w1, b1, w2, b2, dy = (t.cuda() for t in (x, w1, b1, w2, b2, dy))
    yard = torch32(x, w1, b1, w2, b2, dy, w.float().cuda())
    lead = LEAD.get(M, (M,)) + (C,)
    return (x.reshape(lead), w1, b1, w2, b2), dy.reshape(lead), ref, yard


def run(inputs, dy, *dropout, frozen=()):
    """[y, dx, dw1, db1, dw2, db2]; the inputs whose index is in `frozen` ask for no gradient"""
    from gnnflow_amd import ops
    leaves = [t.detach().requires_grad_(i not in frozen) for i, t in enumerate(inputs)]
    y = ops.feed_forward(*leaves, *dropout)
    y.backward(dy)
    return [y.detach()] + [t.grad for t in leaves]


@pytest.mark.parametrize("M,C,Hd,p", CASES)
def test_forward_and_gradients_against_float64(M, C, Hd, p):
    inputs, dy, ref, yard = case(M, C, Hd, p)
    got = run(inputs, dy, p, SEED) if p else run(inputs, dy)
    ratios = [ratio(g, y, r) for g, y, r in zip(got, yard, ref)]
    print("feed_forward {} p={}: error / allowed ".format((M, C, Hd), p) +
          " ".join("{} {:.3f}".format(n, r) for n, r in zip(NAMES, ratios)))
    assert got[0].shape == inputs[0].shape and max(ratios) <= 1


def test_the_weight_pass_sums_two_partial_rows():
    from gnnflow_amd import _capi
    from gnnflow_amd.ops._common import _partial_rows
    M, C, Hd = TWO_ROWS
    rows = _capi.load().gf_feed_forward_backward_partial_rows
    assert _partial_rows(rows, M, C, Hd) >= 2 and _partial_rows(rows, M - 1, C, Hd) == 1


@pytest.mark.parametrize("M,C,Hd", DROPPED)
def test_exact_properties(M, C, Hd):
    from gnnflow_amd import ops
    inputs, dy, _, _ = case(M, C, Hd, 0.5)
    plain, zero = run(inputs, dy), run(inputs, dy, 0.0, SEED)
    assert all(torch.equal(a, b) for a, b in zip(plain, zero))
    first, again, other = (run(inputs, dy, 0.5, s) for s in (SEED, SEED, SEED + 1))
    assert all(torch.equal(a, b) for a, b in zip(first, again))
    assert not torch.equal(first[0], other[0])
    x, params = inputs[0].reshape(M, C), inputs[1:]
    rows = torch.cat([x, x.flip(0), x])                     # rows are independent
    whole = ops.feed_forward(rows, *params)
    assert torch.equal(whole[M:2 * M + 1], ops.feed_forward(rows[M:2 * M + 1].clone(), *params))
    assert torch.equal(whole[:M], plain[0].reshape(M, C))
    bufs = [torch.empty(x.numel() + 4, device=x.device) for _ in range(2)]      # 4 bytes off
    off, goff = (b[1:1 + x.numel()].view(t.shape).copy_(t) for b, t in zip(bufs, (inputs[0], dy)))
    assert inputs[0].data_ptr() % 16 == 0 and off.data_ptr() % 16 == 4
    assert all(torch.equal(a, b) for a, b in zip(run((off,) + params, goff, 0.5, SEED), first))
    frozen = ops.feed_forward(*inputs, 0.5, SEED)           # no gradient asked for: no backward
    assert not frozen.requires_grad and frozen.grad_fn is None and torch.equal(frozen, first[0])
    only_x = run(inputs, dy, 0.5, SEED, frozen=(1, 2, 3, 4))
    assert all(g is None for g in only_x[2:]) and torch.equal(only_x[1], first[1])


def test_no_rows_launch_nothing():
    inputs = [t.detach().requires_grad_() for t in case(3, 5, 7, 0.0)[0]]
    x = torch.zeros(0, 2, 5, device="cuda", requires_grad=True)
    from gnnflow_amd import ops
    y = ops.feed_forward(x, *inputs[1:], 0.5, 3)
    y.sum().backward()
    assert y.shape == x.shape and x.grad.shape == x.shape
    assert all(not t.grad.any() for t in inputs[1:])


# ---- the models -----------------------------------------------------------------------------------

def encoder_block(fused):
    from gnnflow_amd.models.dygformer import EncoderBlock
    return EncoderBlock(20, 2, 0.1, fused_feed_forward=fused), (3, 8, 20), lambda m, x: m(x)


def graph_mixer(fused):
    from gnnflow_amd.models import GraphMixer
    model = GraphMixer(0, 3, dim_time=5, dim_embed=20, num_tokens=8, fused_feed_forward=fused)
    return model, (6, 8, 8), lambda m, x: m.forward_tokens(x, return_embed=True)


@pytest.mark.parametrize("make", [encoder_block, graph_mixer])
def test_model_matches_the_default_route(make):
    torch.manual_seed(5)
    plain, shape, call = make(False)
    fused = make(True)[0]
    assert list(fused.state_dict()) == list(plain.state_dict())
    fused.load_state_dict(plain.state_dict())
    exact = copy.deepcopy(plain).double()
    x = torch.randn(shape, generator=torch.Generator().manual_seed(11))
    outs = []
    for m, xs in ((fused.cuda(), x.cuda()), (plain.cuda(), x.cuda()), (exact, x.double())):
        m.eval()
        outs.append(call(m, xs))
        outs[-1].square().sum().backward()
    r = ratio(outs[0].detach(), outs[1].detach(), outs[2].detach())
    worst = max(ratio(f.grad, p.grad, e.grad) for p, f, e in
                zip(plain.parameters(), fused.parameters(), exact.parameters())
                if p.grad is not None)
    print("{}: error / allowed output {:.3f}, worst gradient {:.3f}".format(make.__name__, r, worst))
    assert r <= 1 and worst <= 1
