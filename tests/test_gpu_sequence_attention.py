"""ops.sequence_attention (csrc/sequence_attention.hip) against its definition in numpy float64,
forward and dqkv, with the mask of tests/attention_dropout_ref.py; its exact properties bit for
bit; and DyGFormer(fused_attention=True) against the default route.

The tolerance is measured, not chosen: the same expression in plain float32 torch (matmul,
softmax, the same mask, matmul, autograd) is held against the float64 reference, and the kernel
may err 4 times as much -- both are float32 evaluations of one formula that differ in summation
order and exp; a lost tail column, a wrong scale or a wrongly indexed mask errs five orders above
that -- with a floor of 16 * 2^-24 * max|ref| so that a lucky torch run cannot make the test
unpassable.  Worst (kernel error) / (allowed error) seen on an MI355X: out 0.20, dqkv 0.18 over
the twelve cases; 0.05 on the model's scores, 0.27 on a parameter's gradient.
"""
import copy
import functools

import numpy as np
import pytest
import torch

from tests import attention_dropout_ref as R

pytestmark = pytest.mark.gpu

SEED = R.SEED                      # above 2^32
SHAPES = [(1, 1, 1, 1), (2, 2, 1, 3), (3, 16, 2, 4), (2, 17, 1, 5), (5, 7, 8, 16), (3, 33, 3, 20),
          (2, 64, 2, 100), (1, 65, 1, 64), (1, 128, 1, 128)]
DROPPED = [(2, 17, 1, 5), (2, 64, 2, 100), (1, 65, 1, 64)]
CASES = [s + (0.0,) for s in SHAPES] + [s + (0.5,) for s in DROPPED]


def weights(n, S, H, p, seed):
    """w [n, H, S, S] float64 of the op's definition"""
    if p == 0:
        return np.ones((n, H, S, S))
    u = R.philox_first(seed, np.arange(n * H * S * S, dtype=np.uint64), 0)
    keep = u >= np.uint32(R.threshold(p))
    return (keep * float(R.scale(p))).reshape(n, H, S, S)


def split(x, H):
    """[n, S, 3 H dh] -> q, k, v [n, H, S, dh]"""
    n, S, width = x.shape
    x = x.reshape(n, S, 3, H, width // (3 * H))
    return (x[:, :, t].swapaxes(1, 2) for t in range(3))


def reference(qkv, H, dout, w):
    q, k, v = split(qkv.astype(np.float64), H)
    n, _, S, dh = q.shape
    s = q @ k.swapaxes(2, 3) / np.sqrt(dh)
    a = np.exp(s - s.max(-1, keepdims=True))
    a /= a.sum(-1, keepdims=True)
    out = ((a * w) @ v).swapaxes(1, 2).reshape(n, S, H * dh)
    g = dout.astype(np.float64).reshape(n, S, H, dh).swapaxes(1, 2)
    dv = (a * w).swapaxes(2, 3) @ g
    da = (g @ v.swapaxes(2, 3)) * w
    ds = a * (da - (a * da).sum(-1, keepdims=True))
    dq, dk = ds @ k / np.sqrt(dh), ds.swapaxes(2, 3) @ q / np.sqrt(dh)
    dqkv = np.stack([t.swapaxes(1, 2) for t in (dq, dk, dv)], axis=2).reshape(qkv.shape)
    return out, dqkv


def torch32(qkv, H, dout, w):
    x = qkv.clone().requires_grad_()
    q, k, v = split(x, H)
    a = torch.softmax(q @ k.transpose(2, 3) / q.shape[3] ** 0.5, dim=-1)
    out = ((a * w) @ v).transpose(1, 2).reshape(dout.shape)
    out.backward(dout)
    return out.detach(), x.grad


def allowed(yardstick, ref):
    """4 max(max|torch32 - ref|, 16 * 2^-24 * max|ref|)"""
    ref = np.asarray(ref, dtype=np.float64)
    err = np.abs(yardstick.double().cpu().numpy() - ref).max()
    return 4 * max(err, 16 * 2.0 ** -24 * np.abs(ref).max())


def ratio(got, yardstick, ref):
    return np.abs(got.double().cpu().numpy() - ref).max() / allowed(yardstick, ref)


@functools.lru_cache(maxsize=None)
def case(n, S, H, dh, p):
    """inputs, the float64 reference and the float32 yardstick of a case; computed once"""
    rng = np.random.RandomState(1000 * S + dh)
    qkv = rng.standard_normal((n, S, 3 * H * dh)).astype(np.float32)
    dout = rng.standard_normal((n, S, H * dh)).astype(np.float32)
    w = weights(n, S, H, p, SEED)
    dev = torch.device("cuda", 0)
    t_qkv, t_dout = torch.from_numpy(qkv).to(dev), torch.from_numpy(dout).to(dev)
    yard = torch32(t_qkv, H, t_dout, torch.from_numpy(w.astype(np.float32)).to(dev))
    return t_qkv, t_dout, reference(qkv, H, dout, w), yard


def run(qkv, H, dout, *dropout):
    from gnnflow_amd import ops
    x = qkv.clone().requires_grad_()
    out = ops.sequence_attention(x, H, *dropout)
    out.backward(dout)
    return out.detach(), x.grad


@pytest.mark.parametrize("n,S,H,dh,p", CASES)
def test_forward_and_gradient_against_float64(n, S, H, dh, p):
    qkv, dout, ref, yard = case(n, S, H, dh, p)
    got = run(qkv, H, dout, p, SEED) if p else run(qkv, H, dout)
    ratios = [ratio(g, y, r) for g, y, r in zip(got, yard, ref)]
    print("sequence_attention {} p={}: error / allowed out {:.3f} dqkv {:.3f}".format(
        (n, S, H, dh), p, *ratios))
    assert ratios[0] <= 1 and ratios[1] <= 1


@pytest.mark.parametrize("n,S,H,dh", DROPPED)
def test_exact_properties(n, S, H, dh):
    from gnnflow_amd import ops
    qkv, dout, _, _ = case(n, S, H, dh, 0.5)
    plain, zero = run(qkv, H, dout), run(qkv, H, dout, 0.0, SEED)
    assert all(torch.equal(a, b) for a, b in zip(plain, zero))
    first, again, other = (run(qkv, H, dout, 0.5, s) for s in (SEED, SEED, SEED + 1))
    assert all(torch.equal(a, b) for a, b in zip(first, again))
    assert not torch.equal(first[0], other[0])
    rows = torch.cat([qkv, qkv.flip(0), qkv])              # rows are independent
    whole = ops.sequence_attention(rows, H)
    assert torch.equal(whole[n:2 * n + 1], ops.sequence_attention(rows[n:2 * n + 1].clone(), H))
    assert torch.equal(whole[:n], plain[0])
    frozen = ops.sequence_attention(qkv, H, 0.5, SEED)     # no gradient asked for: no backward
    assert not frozen.requires_grad and frozen.grad_fn is None
    assert torch.equal(frozen, first[0])


def test_alignment_does_not_change_the_bits():
    n, S, H, dh = 2, 64, 2, 100
    qkv, dout, _, _ = case(n, S, H, dh, 0.5)
    buf = torch.empty(qkv.numel() + 4, device=qkv.device)
    gbuf = torch.empty(dout.numel() + 4, device=qkv.device)
    off = buf[1:1 + qkv.numel()].view(qkv.shape).copy_(qkv)
    goff = gbuf[1:1 + dout.numel()].view(dout.shape).copy_(dout)
    assert qkv.data_ptr() % 16 == 0 and off.data_ptr() % 16 == 4 and off.is_contiguous()
    from gnnflow_amd import ops
    x = off.requires_grad_()
    out = ops.sequence_attention(x, H, 0.5, SEED)
    out.backward(goff)
    aligned = run(qkv, H, dout, 0.5, SEED)
    assert torch.equal(out.detach(), aligned[0]) and torch.equal(x.grad, aligned[1])


def test_no_rows_launch_nothing():
    from gnnflow_amd import ops
    x = torch.zeros(0, 5, 24, device="cuda", requires_grad=True)
    out = ops.sequence_attention(x, 2, 0.5, 3)
    out.sum().backward()
    assert out.shape == (0, 5, 8) and x.grad.shape == x.shape


# ---- the model ------------------------------------------------------------------------------------

def models(P, dropout):
    from gnnflow_amd.models import DyGFormer
    torch.manual_seed(5)
    kw = dict(dim_time=8, channel_dim=6, patch_size=P, num_heads=2, dropout=dropout, max_length=8,
              dim_embed=8)
    plain = DyGFormer(5, 3, **kw).cuda()
    fused = DyGFormer(5, 3, fused_attention=True, **kw).cuda()
    assert list(fused.state_dict()) == list(plain.state_dict())
    fused.load_state_dict(plain.state_dict())
    return plain, fused, copy.deepcopy(plain).double()


def parts(dtype=torch.float32, N=6, L=8):
    g = torch.Generator().manual_seed(11)
    lengths = torch.randint(1, L + 1, (N, 2), generator=g)
    pad = (torch.arange(L) >= lengths.unsqueeze(2)).unsqueeze(3)
    xs = [torch.randn(N, 2, L, d, generator=g).masked_fill(pad, 0.0).to("cuda", dtype)
          for d in (5, 3, 8)]
    counts = torch.randint(0, L, (N, 2, L, 2), generator=g).cuda()
    return xs + [counts, lengths.cuda()]


@pytest.mark.parametrize("P", [1, 4])
def test_model_eval_and_gradients_match_the_default_route(P):
    plain, fused, exact = models(P, 0.0)
    for m in (plain, fused, exact):
        m.eval()
    with torch.no_grad():
        ref = exact.forward_parts(*parts(torch.float64)).cpu().numpy()
        r = ratio(fused.forward_parts(*parts()), plain.forward_parts(*parts()), ref)
    print("DyGFormer P={} eval: error / allowed {:.3f}".format(P, r))
    assert r <= 1
    for m, dtype in ((plain, torch.float32), (fused, torch.float32), (exact, torch.float64)):
        m.train()                                           # dropout = 0: the routes still agree
        m.forward_parts(*parts(dtype)).square().sum().backward()
    worst = max(ratio(f.grad, p.grad, e.grad.cpu().numpy()) for p, f, e in
                zip(plain.parameters(), fused.parameters(), exact.parameters())
                if p.grad is not None)
    print("DyGFormer P={} training: worst gradient error / allowed {:.3f}".format(P, worst))
    assert worst <= 1


def test_model_trains_with_dropout_inside_the_kernel():
    _, fused, _ = models(1, 0.1)
    fused.train()
    scores = []
    for _ in range(2):
        torch.manual_seed(3)
        fused.zero_grad()
        scores.append(fused.forward_parts(*parts()))
    scores[1].sum().backward()
    assert torch.isfinite(scores[0]).all() and torch.equal(scores[0], scores[1])
    assert all(p.grad is not None and torch.isfinite(p.grad).all()
               for p in fused.parameters() if p.requires_grad)
