"""ops.token_mix (csrc/token_mix.hip) against its definition in float64 on the CPU, the output and
all seven gradients written out, with the masks of tests/attention_dropout_ref.py; its exact
properties bit for bit; and MixerBlock / GraphMixer(fused_token_mix=True) against the default route.

The tolerance is test_gpu_feed_forward.py's rule: the same expression in plain float32 torch on the
GPU (F.layer_norm, transposes, F.linear, F.gelu, the same masks, autograd) is held against the
float64 reference, and the kernel may err 4 times as much, with a floor of 16 * 2^-24 * max|ref|
per tensor.  Worst (kernel error) / (allowed error) seen on an MI355X over the fourteen cases:
y 0.07, dx 0.09, dgamma 0.11, dbeta 0.07, dw1 0.18, db1 0.09, dw2 0.12, db2 0.03; 0.04 on a model's
output, 0.09 on a parameter's gradient.
"""
import copy
import functools
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import attention_dropout_ref as R
from tests.test_gpu_feed_forward import allowed

pytestmark = pytest.mark.gpu

SEED = R.SEED                      # above 2^32
SECOND_ROW = (2, 4, 3, 6)          # the smallest N at which one workgroup walks a second row
TWO_ROWS = (5, 4, 3, 6)            # the smallest N with two partial rows
SHAPES = [(1, 1, 1, 1), (2, 3, 2, 5), (3, 16, 16, 16), (2, 17, 9, 20), (3, 32, 16, 100),
          (2, 20, 10, 172), (2, 33, 17, 65), (2, 64, 64, 64), (1, 64, 32, 256), SECOND_ROW,
          TWO_ROWS]
DROPPED = [(2, 17, 9, 20), (3, 32, 16, 100), (2, 33, 17, 65)]
CASES = [s + (0.0,) for s in SHAPES] + [s + (0.5,) for s in DROPPED]
NAMES = ("y", "dx", "dgamma", "dbeta", "dw1", "db1", "dw2", "db2")
EPS = 1e-5


def ratio(got, yardstick, ref):
    """error / allowed; an exact result is 0 where nothing is allowed either (dgamma at C = 1)"""
    ref = ref.double().cpu()
    err = float((got.double().cpu().reshape(ref.shape) - ref).abs().max())
    return err / allowed(yardstick, ref) if err else 0.0


def masks(N, K, Kh, C, p, seed):
    """m1 [N, Kh, C] and m2 [N, K, C], float64, of the op's definition"""
    def draw(T, call):
        if p == 0:
            return np.ones((N, T, C))
        nc = np.arange(N, dtype=np.uint64)[:, None, None] * np.uint64(C) + \
            np.arange(C, dtype=np.uint64)[None, None, :]
        u = R.philox_first(seed, nc * np.uint64(T) + np.arange(T, dtype=np.uint64)[None, :, None],
                           call)
        return (u >= np.uint32(R.threshold(p))) * float(R.scale(p))
    return torch.from_numpy(draw(Kh, 0)), torch.from_numpy(draw(K, 1))


def reference(x, gamma, beta, w1, b1, w2, b2, dy, m1, m2):
    """y and the seven gradients, float64"""
    mean = x.mean(2, keepdim=True)
    rstd = 1 / torch.sqrt(((x - mean) ** 2).mean(2, keepdim=True) + EPS)
    xh = (x - mean) * rstd
    z = xh * gamma + beta
    u = torch.einsum("jk,nkc->njc", w1, z) + b1[None, :, None]
    cdf = 0.5 * (1 + torch.erf(u / math.sqrt(2)))
    h = u * cdf * m1
    y = x + (torch.einsum("kj,njc->nkc", w2, h) + b2[None, :, None]) * m2
    dt = dy * m2
    dh = torch.einsum("kj,nkc->njc", w2, dt)
    du = dh * m1 * (cdf + u * torch.exp(-u * u / 2) / math.sqrt(2 * math.pi))
    dz = torch.einsum("jk,njc->nkc", w1, du)
    a = dz * gamma
    dx = dy + rstd * (a - a.mean(2, keepdim=True) - xh * (a * xh).mean(2, keepdim=True))
    return (y, dx, (dz * xh).sum((0, 1)), dz.sum((0, 1)), torch.einsum("njc,nkc->jk", du, z),
            du.sum((0, 2)), torch.einsum("nkc,njc->kj", dt, h), dt.sum((0, 2)))


def torch32(inputs, dy, m1, m2):
    x, gamma, beta, w1, b1, w2, b2 = leaves = [t.clone().requires_grad_() for t in inputs]
    z = F.layer_norm(x, x.shape[2:], gamma, beta, EPS).transpose(1, 2)
    h = F.gelu(F.linear(z, w1, b1)) * m1.transpose(1, 2)
    y = x + (F.linear(h, w2, b2) * m2.transpose(1, 2)).transpose(1, 2)
    y.backward(dy)
    return [y.detach()] + [t.grad for t in leaves]


@functools.lru_cache(maxsize=None)
def case(N, K, Kh, C, p):
    """inputs and dy on the GPU, the float64 reference and the float32 yardstick; computed once"""
    g = torch.Generator().manual_seed(1000 * N + 10 * K + C)
    x, dy = torch.randn(N, K, C, generator=g), torch.randn(N, K, C, generator=g)
    gamma, beta = 1 + torch.randn(C, generator=g) / 4, torch.randn(C, generator=g) / 2
    w1, b1 = torch.randn(Kh, K, generator=g) / K ** 0.5, torch.randn(Kh, generator=g) / 2
    w2, b2 = torch.randn(K, Kh, generator=g) / Kh ** 0.5, torch.randn(K, generator=g) / 2
    m1, m2 = masks(N, K, Kh, C, p, SEED)
    inputs = (x, gamma, beta, w1, b1, w2, b2)
    ref = reference(*(t.double() for t in inputs + (dy,)), m1, m2)
    inputs, dy = tuple(t.cuda() for t in inputs), dy.cuda()
    return inputs, dy, ref, torch32(inputs, dy, m1.float().cuda(), m2.float().cuda())


def run(inputs, dy, *dropout, frozen=()):
    """[y, dx, dgamma, dbeta, dw1, db1, dw2, db2]; inputs whose index is in `frozen` ask for none"""
    from gnnflow_amd import ops
    leaves = [t.detach().requires_grad_(i not in frozen) for i, t in enumerate(inputs)]
    y = ops.token_mix(*leaves, EPS, *dropout)
    y.backward(dy)
    return [y.detach()] + [t.grad for t in leaves]


@pytest.mark.parametrize("N,K,Kh,C,p", CASES)
def test_forward_and_gradients_against_float64(N, K, Kh, C, p):
    inputs, dy, ref, yard = case(N, K, Kh, C, p)
    got = run(inputs, dy, p, SEED) if p else run(inputs, dy)
    ratios = [ratio(g, y, r) for g, y, r in zip(got, yard, ref)]
    print("token_mix {} p={}: error / allowed ".format((N, K, Kh, C), p) +
          " ".join("{} {:.3f}".format(n, r) for n, r in zip(NAMES, ratios)))
    assert got[0].shape == inputs[0].shape and all(r <= 1 for r in ratios)


def test_the_cases_walk_a_second_row_and_sum_two_partial_rows():
    from gnnflow_amd import _capi
    from gnnflow_amd.ops._common import _partial_rows
    rows = _capi.load().gf_token_mix_backward_partial_rows
    assert _partial_rows(rows, 1, *SECOND_ROW[1:]) == 1      # one workgroup, and N = 2 has one too
    assert _partial_rows(rows, *SECOND_ROW) == 1 and SECOND_ROW[0] == 2
    assert _partial_rows(rows, *TWO_ROWS) == 2
    assert _partial_rows(rows, TWO_ROWS[0] - 1, *TWO_ROWS[1:]) == 1


@pytest.mark.parametrize("N,K,Kh,C", DROPPED)
def test_exact_properties(N, K, Kh, C):
    from gnnflow_amd import ops
    inputs, dy, _, _ = case(N, K, Kh, C, 0.5)
    plain, zero = run(inputs, dy), run(inputs, dy, 0.0, SEED)
    assert all(torch.equal(a, b) for a, b in zip(plain, zero))
    first, again, other = (run(inputs, dy, 0.5, s) for s in (SEED, SEED, SEED + 1))
    assert all(torch.equal(a, b) for a, b in zip(first, again))
    assert not torch.equal(first[0], other[0])
    x, params = inputs[0], inputs[1:]
    whole = ops.token_mix(torch.cat([x, x.flip(0)]), *params, EPS, 0.5, SEED)    # rows are independent
    assert torch.equal(whole[:N], first[0])
    bufs = [torch.empty(x.numel() + 4, device=x.device) for _ in range(2)]       # 4 bytes off
    off, goff = (b[1:1 + x.numel()].view(t.shape).copy_(t) for b, t in zip(bufs, (x, dy)))
    assert x.data_ptr() % 16 == 0 and off.data_ptr() % 16 == 4
    assert all(torch.equal(a, b) for a, b in zip(run((off,) + params, goff, 0.5, SEED), first))
    frozen = ops.token_mix(*inputs, EPS, 0.5, SEED)          # no gradient asked for: no backward
    assert not frozen.requires_grad and frozen.grad_fn is None and torch.equal(frozen, first[0])
    only_x = run(inputs, dy, 0.5, SEED, frozen=range(1, 7))
    assert all(g is None for g in only_x[2:]) and torch.equal(only_x[1], first[1])


def test_no_rows_launch_nothing():
    inputs = [t.detach().requires_grad_() for t in case(2, 3, 2, 5, 0.0)[0]]
    x = torch.zeros(0, 3, 5, device="cuda", requires_grad=True)
    from gnnflow_amd import ops
    y = ops.token_mix(x, *inputs[1:], EPS, 0.5, 3)
    y.sum().backward()
    assert y.shape == x.shape and x.grad.shape == x.shape
    assert all(t.grad.shape == t.shape and not t.grad.any() for t in inputs[1:])


# ---- the models -----------------------------------------------------------------------------------

def mixer_block(**flags):
    from gnnflow_amd.models.graphmixer import MixerBlock
    return MixerBlock(8, 20, 0.5, 4.0, 0.1, **flags), (3, 8, 20), lambda m, x: m(x)


def graph_mixer(**flags):
    from gnnflow_amd.models import GraphMixer
    model = GraphMixer(0, 3, dim_time=5, dim_embed=20, num_tokens=8, **flags)
    return model, (6, 8, 8), lambda m, x: m.forward_tokens(x, return_embed=True)


@pytest.mark.parametrize("both", [False, True], ids=["token_mix", "both_flags"])
@pytest.mark.parametrize("make", [mixer_block, graph_mixer])
def test_model_matches_the_default_route(make, both):
    torch.manual_seed(5)
    plain, shape, call = make()
    fused = make(fused_token_mix=True, fused_feed_forward=both)[0]
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
