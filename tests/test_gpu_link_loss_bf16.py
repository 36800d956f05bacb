"""ops.link_loss on bfloat16 logits: float32 arithmetic, one rounding on store.  The loss equals
the float32 op's on the widened logits bit for bit, the gradients are that op's float32
gradients rounded once to bfloat16, and the op runs under autocast as it is given its inputs."""
import numpy as np
import pytest
import torch

from tests import link_loss_ref as R
from tests.test_gpu_link_loss import SHAPE_IDS, shapes

pytestmark = pytest.mark.gpu


def both(k, upstream):
    from gnnflow_amd import ops
    P, N = shapes()[k]
    pos, neg = R.make_logits(P, N, seed=200 + k)
    out = []
    for dtype in (torch.bfloat16, torch.float32):
        x = torch.from_numpy(pos).cuda().bfloat16().to(dtype).requires_grad_()
        y = torch.from_numpy(neg).cuda().bfloat16().to(dtype).requires_grad_()
        loss = ops.link_loss(x, y)
        (upstream * loss).backward()
        out.append((loss.detach(), x.grad, y.grad))
    return out


@pytest.mark.parametrize("upstream", [1.0, 3.0])
@pytest.mark.parametrize("k", SHAPE_IDS)
def test_bf16_is_the_float32_op_rounded_once(k, upstream):
    (lb, gpb, gnb), (lf, gpf, gnf) = both(k, upstream)
    assert lb.dtype == torch.float32 and lb.shape == ()
    assert gpb.dtype == torch.bfloat16 and gnb.dtype == torch.bfloat16
    assert torch.equal(lb, lf)
    assert torch.equal(gpb, gpf.to(torch.bfloat16)) and torch.equal(gnb, gnf.to(torch.bfloat16))


def test_bf16_gradients_against_the_reference_rounding():
    """Against link_loss_ref.bf16_gradients: equal, or one bfloat16 ulp apart where the kernel's
    float32 gradient and the reference's straddle a rounding boundary.  The two are within
    8 * 2**-24 relative and bfloat16 boundaries 2**-8 apart, so fewer than 1 in 1000 elements can
    straddle one; 1 in 100 is allowed."""
    from gnnflow_amd import ops
    pos, neg = R.make_logits(600, 5400, seed=31)
    pos, neg = R.round_bf16(pos), R.round_bf16(neg)
    x = torch.from_numpy(pos).cuda().bfloat16().requires_grad_()
    y = torch.from_numpy(neg).cuda().bfloat16().requires_grad_()
    ops.link_loss(x, y).backward()
    for got, want in zip((x.grad, y.grad), R.bf16_gradients(pos, neg)):
        got = got.float().cpu().numpy()
        steps = np.abs((got.view(np.uint32) >> 16).astype(np.int64) -
                       (want.view(np.uint32) >> 16).astype(np.int64))
        assert steps.max() <= 1 and (steps == 0).mean() > 0.99


def test_nan_and_accumulator_on_bf16():
    from gnnflow_amd import ops
    acc = torch.zeros(ops.LINK_LOSS_ACC_FIELDS, dtype=torch.float64, device="cuda")
    x = torch.tensor([0.5, -2.0, 3.0], device="cuda").bfloat16()
    y = torch.tensor([1.5, float("nan")], device="cuda").bfloat16()
    assert torch.isnan(ops.link_loss(x, y, acc))
    loss = ops.link_loss(x, y[:1], acc)
    assert acc.tolist() == [float(loss), 3 * float(loss), 1.0, 1.0, 3.0]


def test_under_autocast_without_a_cast_by_the_caller():
    from gnnflow_amd import ops
    torch.manual_seed(0)
    lin = torch.nn.Linear(16, 1).cuda()
    h = torch.randn(900, 16, device="cuda")
    with torch.autocast("cuda", dtype=torch.bfloat16):
        out = lin(h)
        assert out.dtype == torch.bfloat16
        loss = ops.link_loss(out[:300], out[300:])
        assert loss.dtype == torch.float32
    loss.backward()
    assert lin.weight.grad is not None and torch.isfinite(lin.weight.grad).all()
    want = ops.link_loss(out[:300].detach().float(), out[300:].detach().float())
    assert torch.equal(loss.detach(), want)
    # float32 logits inside the region are taken as float32
    with torch.autocast("cuda", dtype=torch.bfloat16):
        assert torch.equal(ops.link_loss(out[:300].detach().float(), out[300:].detach().float()), want)
