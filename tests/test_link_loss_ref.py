"""CPU checks of tests/link_loss_ref.py, the restatement ops.link_loss is tested against: torch's
own float64 expression and its autograd gradients, the closed forms at the fixed logits, the
accumulator's NaN rule, and the constants the header, the kernel and ops.py share."""
import math
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import link_loss_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(1, 1), (3, 7), (9, 9), (600, 5400)]


def torch_f64(pos, neg, upstream=1.0):
    x = torch.from_numpy(pos.astype(np.float64)).requires_grad_()
    y = torch.from_numpy(neg.astype(np.float64)).requires_grad_()
    loss = F.binary_cross_entropy_with_logits(x, torch.ones_like(x)) + \
        F.binary_cross_entropy_with_logits(y, torch.zeros_like(y))
    (upstream * loss).backward()
    return float(loss.detach()), x.grad.numpy(), y.grad.numpy()


@pytest.mark.parametrize("P,N", CASES)
@pytest.mark.parametrize("upstream", [1.0, 3.0])
def test_reference_is_torchs_float64_expression(P, N, upstream):
    """rtol 1e-12 on the loss and on the gradients.  torch's backward writes the positive
    gradient as (sigmoid(x) - 1) / P, whose subtraction loses up to 2**-53 absolutely (all of
    the result at x = 80): that error of torch's, upstream * 2 * 2**-53 / n, is the atol."""
    pos, neg = R.make_logits(P, N, seed=1000 + P + N)
    ref = R.reference(pos, neg, upstream)
    loss, gp, gn = torch_f64(pos, neg, upstream)
    assert abs(ref["loss"] - loss) <= 1e-12 * abs(loss)
    np.testing.assert_allclose(ref["grad_pos"], gp, rtol=1e-12, atol=upstream * 2.0 ** -52 / P)
    np.testing.assert_allclose(ref["grad_neg"], gn, rtol=1e-12, atol=upstream * 2.0 ** -52 / N)


def test_closed_forms_at_the_fixed_logits():
    x = np.array(R.FIXED, dtype=np.float32)
    lp, ln = R.terms(x, x)
    want_pos = {0.0: math.log(2.0), 20.0: math.log1p(math.exp(-20.0)),
                -20.0: 20.0 + math.log1p(math.exp(-20.0)), 80.0: math.exp(-80.0),
                -80.0: 80.0}
    for v, lpv, lnv in zip(x.tolist(), lp, ln):
        if v in want_pos:
            assert lpv == pytest.approx(want_pos[v], rel=1e-15)
            assert lnv == pytest.approx(want_pos[-v], rel=1e-15)      # l_neg(y) = l_pos(-y)
    # +-1e-8: log 2 -+ x / 2 to first order
    assert lp[1] == pytest.approx(math.log(2.0) - float(x[1]) / 2, rel=1e-15)
    assert ln[1] == pytest.approx(math.log(2.0) + float(x[1]) / 2, rel=1e-15)
    r = R.reference(x, x)
    assert (r["grad_pos"] < 0).all() and (r["grad_neg"] > 0).all()
    # the positive gradient at 80 is -exp(-80) / P, not the 0 that s(x) - 1 would give
    assert r["grad_pos"][5] == pytest.approx(-math.exp(-80.0) / len(x), rel=1e-15)
    np.testing.assert_allclose(r["grad_neg"] - r["grad_pos"], 1.0 / len(x), rtol=1e-14)


def test_infinities_follow_the_formulas_and_nan_stays():
    one = np.ones(1, dtype=np.float32)
    inf = np.float32(np.inf)
    assert R.reference(one * inf, one * -inf)["loss"] == 0.0
    assert R.reference(one * -inf, one)["loss"] == math.inf
    assert R.reference(one, one * inf)["loss"] == math.inf
    assert math.isnan(R.reference(one * np.float32(np.nan), one)["loss"])
    assert math.isnan(R.reference(one, one * np.float32(np.nan))["loss"])


def test_accumulator_sums_and_nan_rule():
    acc = R.Accumulator()
    losses, Ps = [], (5, 600, 33)
    for k, P in enumerate(Ps):
        pos, neg = R.make_logits(P, 2 * P + 1, seed=k)
        losses.append(acc.add(pos, neg))
    assert acc.state[0] == sum(losses) and acc.state[2] == 3 and acc.state[4] == sum(Ps)
    assert acc.state[1] == losses[0] * 5 + losses[1] * 600 + losses[2] * 33
    assert all(l == float(np.float32(l)) for l in losses)      # the float32 loss is what is added
    before = acc.state.copy()
    pos, neg = R.make_logits(7, 9, seed=9)
    neg[3] = np.nan
    assert math.isnan(acc.add(pos, neg))
    assert acc.state[3] == 1
    assert np.array_equal(np.delete(acc.state, 3), np.delete(before, 3))
    pos[2] = -np.inf      # l_pos(-inf) = inf: the NaN case too
    neg[3] = 0
    assert acc.add(pos, neg) == math.inf and acc.state[3] == 2
    out = acc.compute()
    assert out["batches"] == 3 and out["nonfinite"] == 2
    assert out["mean_loss"] == sum(losses) / 3
    assert out["edge_weighted_loss"] == acc.state[1] / sum(Ps)
    assert math.isnan(R.Accumulator().compute()["mean_loss"])


def test_round_bf16_is_torchs():
    x = np.concatenate([R.make_logits(600, 600, seed=4)[0] * 1e-3,
                        np.array([1.00390625, 1.01171875, -1.00390625, 0.0, 3.3e-39],
                                 dtype=np.float32)])      # two ties, a zero, a denormal
    want = torch.from_numpy(x).to(torch.bfloat16).float().numpy()
    assert np.array_equal(R.round_bf16(x).view(np.uint32), want.view(np.uint32))
    gp, gn = R.bf16_gradients(*R.make_logits(9, 9, seed=5))
    assert gp.dtype == np.float32 and (gp.view(np.uint32) & 0xFFFF == 0).all() and (gn > 0).all()


def test_constants_agree():
    """The header's macros, the kernel's constants behind them (a static_assert in capi.hip ties
    the two) and the copies in ops.py."""
    from gnnflow_amd import ops
    text = open(os.path.join(ROOT, "include", "gnnflow_hip.h")).read()
    macro = {k: int(v) for k, v in re.findall(r"#define (GF_LINK_LOSS_[A-Z_]+) (\d+)", text)}
    assert macro == {"GF_LINK_LOSS_TILE": ops.LINK_LOSS_TILE,
                     "GF_LINK_LOSS_SINGLE_TILES": ops.LINK_LOSS_SINGLE_TILES,
                     "GF_LINK_LOSS_MAX_PARTIAL_ROWS": ops.LINK_LOSS_MAX_PARTIAL_ROWS,
                     "GF_LINK_LOSS_ACC_FIELDS": ops.LINK_LOSS_ACC_FIELDS}
    assert ops.LINK_LOSS_ACC_FIELDS == len(R.ACC_FIELDS)
    assert ops.LINK_LOSS_TILE % 64 == 0 and ops.LINK_LOSS_TILE <= 1024
