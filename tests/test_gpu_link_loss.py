"""ops.link_loss on the GPU, float32, against tests/link_loss_ref.py (float64; the bounds and
their derivations are there) and against torch's own float32 expression.

The shapes cover one element a side, the wave and 256 edges, the reference's 600 + 5400, the
pair 3 tiles + 1 a side (the last size the one-launch kernel takes), 4 tiles + 1 a side (two
launches) and a side of more tiles than it has partial rows (a workgroup walks two tiles)."""
import functools
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import link_loss_ref as R

pytestmark = pytest.mark.gpu


def shapes():
    from gnnflow_amd import ops
    T, rows = ops.LINK_LOSS_TILE, ops.LINK_LOSS_MAX_PARTIAL_ROWS // 2
    return [(1, 1), (255, 257), (256, 256), (257, 1), (1, 513), (600, 5400),
            (3 * T + 1, 3 * T + 1), (4 * T + 1, 4 * T + 1), (rows * T + 3, 5), (7, rows * T + T + 1)]


SHAPE_IDS = list(range(10))


@functools.lru_cache(maxsize=None)
def case(k, upstream=1.0):
    """(pos, neg, reference) of shape number k, computed once."""
    P, N = shapes()[k]
    pos, neg = R.make_logits(P, N, seed=100 + k)
    return pos, neg, R.reference(pos, neg, upstream)


def run(pos, neg, upstream=1.0, acc=None, need=(True, True)):
    from gnnflow_amd import ops
    x = torch.from_numpy(pos).cuda().requires_grad_(need[0])
    y = torch.from_numpy(neg).cuda().requires_grad_(need[1])
    loss = ops.link_loss(x, y, acc)
    (upstream * loss).backward()
    return loss.detach(), x.grad, y.grad


def torch_f32(pos, neg):
    x, y = torch.from_numpy(pos).cuda(), torch.from_numpy(neg).cuda()
    return F.binary_cross_entropy_with_logits(x, torch.ones_like(x)) + \
        F.binary_cross_entropy_with_logits(y, torch.zeros_like(y))


def test_shapes_cover_both_forward_paths_and_the_row_cap():
    from gnnflow_amd import ops
    T, S = ops.LINK_LOSS_TILE, ops.LINK_LOSS_SINGLE_TILES
    tiles = [math.ceil(P / T) + math.ceil(N / T) for P, N in shapes()]
    assert len(shapes()) == len(SHAPE_IDS)
    assert S in tiles and S + 2 in tiles and min(tiles) == 2
    assert max(max(P, N) for P, N in shapes()) > T * ops.LINK_LOSS_MAX_PARTIAL_ROWS // 2


@pytest.mark.parametrize("k", SHAPE_IDS)
def test_loss_against_the_float64_reference_and_torch(k):
    pos, neg, ref = case(k)
    loss, _, _ = run(pos, neg)
    assert loss.dtype == torch.float32 and loss.shape == () and loss.is_cuda
    got = float(loss)
    print("\n[link_loss] P, N = {}: loss {:.9g}, |loss - ref| / ref = {:.3g} (bound {:.3g})".format(
        shapes()[k], got, abs(got - ref["loss"]) / ref["loss"], R.LOSS_RTOL))
    assert abs(got - ref["loss"]) <= R.LOSS_RTOL * ref["loss"]
    torch.testing.assert_close(loss, torch_f32(pos, neg))


@pytest.mark.parametrize("upstream", [1.0, 3.0])
@pytest.mark.parametrize("k", SHAPE_IDS)
def test_gradients_against_the_float64_reference(k, upstream):
    pos, neg, ref = case(k, upstream)
    assert max(np.abs(pos).max(), np.abs(neg).max()) <= 80
    _, gp, gn = run(pos, neg, upstream)
    assert gp.dtype == torch.float32 and gp.shape == pos.shape and gn.shape == neg.shape
    for got, want in ((gp, ref["grad_pos"]), (gn, ref["grad_neg"])):
        got = got.cpu().numpy().astype(np.float64)
        err = np.abs(got - want) / (R.GRAD_RTOL * np.abs(want) + R.GRAD_ATOL)
        print("\n[link_loss] P, N = {} x{}: worst gradient error / bound = {:.3g}".format(
            shapes()[k], upstream, err.max()))
        assert (err <= 1).all()


def test_large_logits():
    """At +-100 and +-1e4 the loss is |x|-dominated and within the forward bound; the gradients
    are finite, of the right sign, and within 1e-37 of the reference."""
    big = np.array([100.0, -100.0, 1e4, -1e4], dtype=np.float32)
    pos = np.concatenate([big, R.make_logits(300, 1, seed=7)[0]])
    neg = np.concatenate([R.make_logits(1, 500, seed=8)[1], big])
    ref = R.reference(pos, neg)
    loss, gp, gn = run(pos, neg)
    assert abs(float(loss) - ref["loss"]) <= R.LOSS_RTOL * ref["loss"]
    assert ref["loss"] > 1e4 / len(pos)
    gp, gn = gp.cpu().numpy(), gn.cpu().numpy()
    assert np.isfinite(gp).all() and np.isfinite(gn).all()
    assert (gp <= 0).all() and (gn >= 0).all()
    np.testing.assert_allclose(gp[:4], ref["grad_pos"][:4], rtol=R.GRAD_RTOL, atol=1e-37)
    np.testing.assert_allclose(gn[-4:], ref["grad_neg"][-4:], rtol=R.GRAD_RTOL, atol=1e-37)
    # the saturated ends: -1 / P for a confidently wrong positive, 1 / N for such a negative
    assert gp[1] == np.float32(-1.0) / np.float32(len(pos)) and gp[3] == gp[1]
    assert gn[-4] == np.float32(1.0) / np.float32(len(neg)) and gn[-2] == gn[-4]


def test_infinite_logits_follow_the_formulas():
    from gnnflow_amd import ops
    inf = float("inf")
    pos = torch.tensor([inf, 1.0], device="cuda")
    neg = torch.tensor([-inf, -1.0, 0.5], device="cuda")
    ref = R.reference(pos.cpu().numpy(), neg.cpu().numpy())
    assert abs(float(ops.link_loss(pos, neg)) - ref["loss"]) <= R.LOSS_RTOL * ref["loss"]
    assert float(ops.link_loss(-pos, neg)) == inf
    assert float(ops.link_loss(pos, -neg)) == inf


def test_only_the_gradient_asked_for():
    pos, neg, ref = case(1)
    _, gp, gn = run(pos, neg, need=(True, False))
    _, hp, hn = run(pos, neg, need=(False, True))
    _, fp, fn = run(pos, neg)
    assert gn is None and hp is None
    assert torch.equal(gp, fp) and torch.equal(hn, fn)


@pytest.mark.parametrize("k", [5, 7])
def test_two_calls_give_the_same_bits(k):
    pos, neg, _ = case(k)
    a, b = run(pos, neg, 3.0), run(pos, neg, 3.0)
    assert all(torch.equal(u, v) for u, v in zip(a, b))


def test_row_slices_and_columns_are_taken_as_they_are():
    from gnnflow_amd import ops
    B = 300
    pos, neg = R.make_logits(B, 2 * B, seed=21)
    buf = torch.from_numpy(np.concatenate([pos, neg])).cuda().reshape(3 * B, 1).requires_grad_()
    p, n = buf[:B], buf[B:]
    assert n.data_ptr() == buf.data_ptr() + 4 * B
    loss = ops.link_loss(p, n)
    loss.backward()
    want, gp, gn = run(pos, neg)
    assert torch.equal(loss.detach(), want)
    assert buf.grad.shape == (3 * B, 1) and torch.equal(buf.grad.reshape(-1), torch.cat([gp, gn]))
    # a strided view is copied, not misread
    wide = torch.from_numpy(np.stack([neg, -neg], 1)).cuda()
    assert torch.equal(ops.link_loss(torch.from_numpy(pos).cuda(), wide[:, 0]), want)


def test_accumulator_over_batches_and_the_nan_rule():
    from gnnflow_amd import ops
    acc = torch.zeros(ops.LINK_LOSS_ACC_FIELDS, dtype=torch.float64, device="cuda")
    mine, theirs = R.Accumulator(), R.Accumulator()
    for k, (P, N) in enumerate(((5, 11), (600, 5400), (4 * ops.LINK_LOSS_TILE + 1, 4100))):
        pos, neg = R.make_logits(P, N, seed=40 + k)
        loss, _, _ = run(pos, neg, acc=acc)      # the backward adds nothing
        mine.add(pos, neg, loss=float(loss))
        theirs.add(pos, neg)
    state = acc.cpu().numpy()
    # the kernel adds its own float32 loss, in float64, batch after batch: the same adds
    assert np.array_equal(state, mine.state)
    np.testing.assert_allclose(state, theirs.state, rtol=R.LOSS_RTOL, atol=0)
    assert state[2] == 3 and state[3] == 0 and state[4] == 5 + 600 + 4 * ops.LINK_LOSS_TILE + 1
    for P, N in ((7, 9), (4 * ops.LINK_LOSS_TILE + 1, 4100)):      # either forward path
        pos, neg = R.make_logits(P, N, seed=50)
        neg[N // 2] = np.nan
        before = acc.clone()
        loss, gp, gn = run(pos, neg, acc=acc)
        assert math.isnan(float(loss))
        after = acc.cpu().numpy()
        assert after[3] == before[3].item() + 1
        assert np.array_equal(np.delete(after, 3).view(np.uint64),
                              np.delete(before.cpu().numpy(), 3).view(np.uint64))
        assert torch.isfinite(gp).all() and int(torch.isnan(gn).sum()) == 1
    # an infinite loss is left out the same way
    ops.link_loss(torch.full((3,), -float("inf"), device="cuda"), torch.zeros(2, device="cuda"), acc)
    assert acc[3].item() == 3 and acc[2].item() == 3


def test_no_accumulator_writes_nothing_else():
    """accumulator=None: the call returns the same loss and leaves an accumulator used before
    and after it alone."""
    from gnnflow_amd import ops
    pos, neg, _ = case(5)
    acc = torch.zeros(ops.LINK_LOSS_ACC_FIELDS, dtype=torch.float64, device="cuda")
    first, _, _ = run(pos, neg, acc=acc)
    kept = acc.clone()
    second, _, _ = run(pos, neg)
    assert torch.equal(first, second) and torch.equal(acc, kept)
    assert acc[2].item() == 1 and acc[0].item() == float(first)


def test_under_no_grad_and_on_the_current_stream():
    from gnnflow_amd import ops
    pos, neg, _ = case(5)
    x, y = torch.from_numpy(pos).cuda().requires_grad_(), torch.from_numpy(neg).cuda()
    want = ops.link_loss(x, y).detach()
    with torch.no_grad():
        assert not ops.link_loss(x, y).requires_grad
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got = ops.link_loss(x, y)
        got.backward()
    side.synchronize()
    assert torch.equal(got.detach(), want) and torch.isfinite(x.grad).all()
