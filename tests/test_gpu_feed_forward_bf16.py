"""ops.feed_forward(..., compute_dtype=torch.bfloat16) (csrc/feed_forward_bf16.hip) against the
exact float64 definition of test_gpu_feed_forward.py -- no internal rounding in the reference --
on inputs whose x, dy, w1 and w2 are bfloat16-representable, so that rounding the inputs is exact;
its exact properties bit for bit; and EncoderBlock / GraphMixer(fused_feed_forward="bfloat16")
outside and inside a bfloat16 autocast region.

The tolerance is the project's rule moved to this precision: the same expression in torch on
bfloat16 tensors on the GPU (F.linear, F.gelu, the same mask, F.linear, autograd: what autocast
runs) is held against the float64 reference, and the kernel may err 4 times as much, with a floor
of 2^-9 * max|ref| per tensor.  Worst (kernel error) / (allowed error) seen on an MI355X over the
twelve cases: y 0.22, dx 0.22, dw1 0.20, db1 0.27, dw2 0.19, db2 0.00 (db2 sums exact inputs);
on a model's output 0.09 outside autocast and 0.23 inside, on a parameter's gradient (printed,
not asserted beyond finite) 0.25 and 0.46.
"""
import copy
import functools

import pytest
import torch
import torch.nn.functional as F

from tests.test_gpu_feed_forward import (LEAD, NAMES, SEED, TWO_ROWS, encoder_block, graph_mixer,
                                         reference, run, weights)

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
SHAPES = [(1, 1, 1), (3, 5, 7), (16, 32, 32), (17, 31, 33), (65, 68, 65), (130, 100, 400),
          (70, 200, 800), (33, 256, 96), TWO_ROWS]
DROPPED = [(17, 31, 33), (65, 68, 65), (70, 200, 800)]
CASES = [s + (0.0,) for s in SHAPES] + [s + (0.5,) for s in DROPPED]


def torch_bf16(x, w1, b1, w2, b2, dy, w):
    leaves = [t.to(BF16).requires_grad_() for t in (x, w1, b1, w2, b2)]
    y = F.linear(F.gelu(F.linear(leaves[0], leaves[1], leaves[2])) * w.to(BF16), leaves[3],
                 leaves[4])
    y.backward(dy.to(BF16))
    return [y.detach()] + [t.grad for t in leaves]


def ratio(got, yardstick, ref):
    """max|got - ref| / (4 max(max|yardstick - ref|, 2^-9 max|ref|))"""
    ref = ref.detach().double().cpu()
    err = (yardstick.detach().double().cpu().reshape(ref.shape) - ref).abs().max()
    allowed = 4 * max(float(err), 2.0 ** -9 * float(ref.abs().max()))
    return float((got.detach().double().cpu().reshape(ref.shape) - ref).abs().max()) / allowed


@functools.lru_cache(maxsize=None)
def case(M, C, Hd, p):
    """inputs on the GPU (x and dy in x's leading shape), the float64 reference and the bfloat16
    yardstick of a case; computed once"""
    g = torch.Generator().manual_seed(1000 * M + Hd)
    exact = lambda t: t.to(BF16).float()
    x, dy = exact(torch.randn(M, C, generator=g)), exact(torch.randn(M, C, generator=g))
    w1, b1 = exact(torch.randn(Hd, C, generator=g) / C ** 0.5), torch.randn(Hd, generator=g) / 2
    w2, b2 = exact(torch.randn(C, Hd, generator=g) / Hd ** 0.5), torch.randn(C, generator=g) / 2
    w = torch.from_numpy(weights(M, Hd, p, SEED))
    ref = reference(*(t.double() for t in (x, w1, b1, w2, b2, dy)), w)
    x, w1, b1, w2, b2, dy = (t.cuda() for t in (x, w1, b1, w2, b2, dy))
    yard = torch_bf16(x, w1, b1, w2, b2, dy, w.float().cuda())
    lead = LEAD.get(M, (M,)) + (C,)
    return (x.reshape(lead), w1, b1, w2, b2), dy.reshape(lead), ref, yard


@pytest.mark.parametrize("M,C,Hd,p", CASES)
def test_forward_and_gradients_against_float64(M, C, Hd, p):
    inputs, dy, ref, yard = case(M, C, Hd, p)
    got = run(inputs, dy, p, SEED if p else None, BF16)
    ratios = [ratio(g, y, r) for g, y, r in zip(got, yard, ref)]
    print("feed_forward bf16 {} p={}: error / allowed ".format((M, C, Hd), p) +
          " ".join("{} {:.3f}".format(n, r) for n, r in zip(NAMES, ratios)))
    assert got[0].shape == inputs[0].shape and got[0].dtype == torch.float32
    assert max(ratios) <= 1


def test_the_weight_pass_sums_two_partial_rows():
    from gnnflow_amd import _capi
    from gnnflow_amd.ops._common import _partial_rows
    M, C, Hd = TWO_ROWS
    rows = _capi.load().gf_feed_forward_bf16_backward_partial_rows
    assert _partial_rows(rows, M, C, Hd) == 2 and _partial_rows(rows, M - 1, C, Hd) == 1


@pytest.mark.parametrize("M,C,Hd", DROPPED)
def test_exact_properties(M, C, Hd):
    from gnnflow_amd import ops
    inputs, dy, _, _ = case(M, C, Hd, 0.5)
    plain, zero = run(inputs, dy, 0.0, None, BF16), run(inputs, dy, 0.0, SEED, BF16)
    assert all(torch.equal(a, b) for a, b in zip(plain, zero))
    first, again, other = (run(inputs, dy, 0.5, s, BF16) for s in (SEED, SEED, SEED + 1))
    assert all(torch.equal(a, b) for a, b in zip(first, again))
    assert not torch.equal(first[0], other[0])
    x, params = inputs[0].reshape(M, C), inputs[1:]
    rows = torch.cat([x, x.flip(0), x])                     # rows are independent
    whole = ops.feed_forward(rows, *params, compute_dtype=BF16)
    assert torch.equal(whole[M:2 * M + 1],
                       ops.feed_forward(rows[M:2 * M + 1].clone(), *params, compute_dtype=BF16))
    assert torch.equal(whole[:M], plain[0].reshape(M, C))
    bufs = [torch.empty(x.numel() + 4, device=x.device) for _ in range(2)]      # 4 bytes off
    off, goff = (b[1:1 + x.numel()].view(t.shape).copy_(t) for b, t in zip(bufs, (inputs[0], dy)))
    assert inputs[0].data_ptr() % 16 == 0 and off.data_ptr() % 16 == 4
    assert all(torch.equal(a, b)
               for a, b in zip(run((off,) + params, goff, 0.5, SEED, BF16), first))
    only_x = run(inputs, dy, 0.5, SEED, BF16, frozen=(1, 2, 3, 4))
    assert all(g is None for g in only_x[2:]) and torch.equal(only_x[1], first[1])
    none = run((torch.zeros(0, 2, C, device="cuda"),) + params, torch.zeros(0, 2, C, device="cuda"),
               0.5, SEED, BF16)                             # no rows: nothing launched
    assert none[0].shape == none[1].shape == (0, 2, C) and all(not g.any() for g in none[2:])


@pytest.mark.parametrize("autocast", [False, True])
@pytest.mark.parametrize("make", [encoder_block, graph_mixer])
def test_model_under_the_bfloat16_rule(make, autocast):
    torch.manual_seed(5)
    plain, shape, call = make(False)
    fused = make("bfloat16")[0]
    assert list(fused.state_dict()) == list(plain.state_dict())
    fused.load_state_dict(plain.state_dict())
    exact = copy.deepcopy(plain).double()
    x = torch.randn(shape, generator=torch.Generator().manual_seed(11))
    outs = []
    for m, xs, cast in ((fused.cuda(), x.cuda(), autocast), (plain.cuda(), x.cuda(), True),
                        (exact, x.double(), False)):
        m.eval()
        with torch.autocast("cuda", dtype=BF16, enabled=cast):
            outs.append(call(m, xs))
        outs[-1].double().square().sum().backward()
    r = ratio(*outs)
    grads = [ratio(f.grad, p.grad, e.grad) for p, f, e in
             zip(plain.parameters(), fused.parameters(), exact.parameters()) if e.grad is not None]
    print("{} autocast={}: error / allowed output {:.3f}, worst gradient {:.3f}".format(
        make.__name__, autocast, r, max(grads)))
    assert r <= 1
    assert all(p.grad is not None and torch.isfinite(p.grad).all()
               for p, e in zip(fused.parameters(), exact.parameters()) if e.grad is not None)
