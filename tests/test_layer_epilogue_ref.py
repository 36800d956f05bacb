"""CPU checks of tests/layer_epilogue_ref.py, the yardstick of the GPU tests of
ops.dropout_relu_layer_norm: its float64 formulas against torch's layer_norm and autograd in
float64, its bfloat16 rounding against torch's, its mask statistics for the seeds the GPU tests
use, and its a priori bounds against an fp32 emulation of the kernels' arithmetic (which they must
hold) and against the one-pass variance E[y^2] - mean^2 (which they must reject)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from gnnflow_amd import ops
from tests import layer_epilogue_ref as LE
from tests.attention_dropout_ref import scale

SMALL = [c for c in LE.CASES if c[0] * c[1] <= 1025 * 100]


@pytest.mark.parametrize("p", LE.PS)
@pytest.mark.parametrize("case", SMALL, ids=LE.case_id)
def test_reference_is_torch_in_float64(case, p):
    c = LE.make_inputs(case)
    r = LE.reference(c, p=p)
    R, D = case
    x = torch.from_numpy(c["x"]).double().requires_grad_(True)
    w = torch.from_numpy(c["weight"]).double().requires_grad_(True)
    b = torch.from_numpy(c["bias"]).double().requires_grad_(True)
    keep = torch.from_numpy(LE.keep_mask(R, D, p, LE.SEED)).double()
    out = F.layer_norm(F.relu(x * keep * float(scale(p))), (D,), w, b, float(np.float32(LE.EPS)))
    out.backward(torch.from_numpy(c["gout"]).double())
    # rtol, with an absolute term of the same 1e-12 on the size of what is subtracted to give the
    # value: a gradient that is 0 in exact arithmetic (D = 1) is rounding noise in torch
    g64 = c["gout"].astype(np.float64) * c["weight"].astype(np.float64)
    size = dict(out=np.abs(r.out).max(), gx=r.rstd.max() * np.abs(g64).max() * float(scale(p)),
                ggamma=(np.abs(c["gout"]) * (r.y + r.mean[:, None]) * r.rstd[:, None]).sum(0).max(),
                gbeta=np.abs(c["gout"]).sum(0).max())
    for name, got, want in (("out", r.out, out), ("gx", r.gx, x.grad),
                            ("ggamma", r.ggamma, w.grad), ("gbeta", r.gbeta, b.grad)):
        np.testing.assert_allclose(got, want.detach().numpy(), rtol=1e-12,
                                   atol=1e-12 * size[name], err_msg=name)
    y = F.relu(x * keep * float(scale(p))).detach()
    np.testing.assert_allclose(r.mean, y.mean(1).numpy(), rtol=1e-12, atol=1e-300)
    np.testing.assert_allclose(
        r.rstd, (y.var(1, unbiased=False) + float(np.float32(LE.EPS))).rsqrt().numpy(),
        rtol=1e-12)


def test_round_bf16_is_torchs():
    rng = np.random.RandomState(5)
    a = np.concatenate([
        rng.standard_normal(4096).astype(np.float32) * np.float32(3),
        np.array([0.0, -0.0, 1.0, 1.00390625, 1.01171875, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8,
                  3.3895313892515355e38, 1e-40, -1e-40], np.float32)])
    want = torch.from_numpy(a).bfloat16().float().numpy()
    assert np.array_equal(LE.round_bf16(a).view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("p", LE.PS)
@pytest.mark.parametrize("case", SMALL, ids=LE.case_id)
def test_fp32_arithmetic_holds_the_bounds(case, p):
    c = LE.make_inputs(case)
    ratios = LE.reference(c, p=p).ratios(**LE.emulate_fp32(c, p=p))
    assert set(ratios) == {"out", "mean", "rstd", "gx", "ggamma", "gbeta"}
    assert max(ratios.values()) <= 1.0, ratios


def test_special_rows_hold_the_bounds_and_the_one_pass_variance_does_not():
    """Two passes over the deviations hold every bound on the rows that break a careless kernel.
    E[y^2] - mean^2 does not: on the row of large, nearly equal entries its rstd is off by far
    more than the bound.  On the row with one 1e4 entry among 1e-3 entries the two formulas are
    NOT told apart in fp32 (the variance, 9.9e5, is of the size of E[y^2] itself, so nothing
    cancels; measured one-pass error / bound of rstd there is below 1): that row is kept as a
    case the kernels must pass, the nearly-equal row is the one that rejects the formula."""
    c = LE.special_case()
    r = LE.reference(c)
    assert max(r.ratios(**LE.emulate_fp32(c)).values()) <= 1.0
    bad = LE.emulate_fp32(c, one_pass_variance=True)
    with np.errstate(invalid="ignore"):
        err = np.abs(bad["rstd"].astype(np.float64) - r.rstd) / r.b_rstd
    print("\n[one-pass rstd error / bound per row]", err)
    assert err[2] <= 1.0          # the 1e4 row does not tell the formulas apart
    assert not err[4] <= 1.0      # far off, or NaN from a negative variance
    assert r.ratios(rstd=bad["rstd"])["rstd"] > 1.0


def test_constant_row_has_the_exact_mean():
    c = LE.special_case()
    e = LE.emulate_fp32(c)
    assert e["mean"][0] == np.float32(1.5) and np.array_equal(e["out"][0], c["bias"])
    assert np.array_equal(e["out"][1], c["bias"]) and not e["gx"][1].any()      # y = 0
    assert not e["gx"][3, ::3].any()                                            # x = 0, kept


def test_mask_statistics_of_the_seeds_used():
    """The kept share over 257 x 100 elements lies within 5 binomial standard deviations of 0.8,
    and the first rows of the mask are the prefix-independent counters r * D + d."""
    n = 257 * 100
    for seed in (LE.SEED, 977):
        keep = LE.keep_mask(257, 100, 0.2, seed)
        assert abs(keep.mean() - 0.8) <= 5 * np.sqrt(0.2 * 0.8 / n)
        assert np.array_equal(LE.keep_mask(5, 100, 0.2, seed), keep[:5])
    assert LE.keep_mask(3, 7, 0.0, 1).all()


def test_all_dropped_seed():
    seed = LE.find_all_dropped_seed(3, 0.9)
    assert seed == LE.ALL_DROPPED_SEED
    assert (~LE.keep_mask(4, 3, 0.9, seed)).all(axis=1).any()


def test_width_constant_matches_the_op():
    assert LE.MAX_WIDTH == ops.LAYER_EPILOGUE_MAX_WIDTH
