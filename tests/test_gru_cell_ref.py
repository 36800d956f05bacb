"""tests/gru_cell_ref.py is torch.nn.GRUCell: the float64 statement of the forward and of every
gradient against the cell in float64 on the CPU, forward and through autograd, with gi and gh
built from random x, h and the cell's parameters.  Both sides are float64 evaluations of the same
expressions that differ in association only, a handful of roundings of 2^-53 each on values of
order one: rtol 1e-12 (against the largest value of each tensor) leaves three decimal orders.
Also the case list, the saturation inputs, the float32 restatement and the bfloat16 rounding."""
import numpy as np
import pytest
import torch

from tests import gru_cell_ref as GR

RTOL = 1e-12


def _close(got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == np.float64
    return np.abs(got - want).max() <= RTOL * max(np.abs(want).max(), 1.0)


@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("N,K,H", [(1, 1, 1), (5, 3, 4), (33, 17, 7), (40, 24, 100)])
def test_reference_is_torchs_gru_cell(N, K, H, bias):
    F = torch.nn.functional
    torch.manual_seed(N + 10 * K + 100 * H)
    cell = torch.nn.GRUCell(K, H, bias=bias).double()
    x = torch.randn(N, K, dtype=torch.float64)
    h = torch.randn(N, H, dtype=torch.float64, requires_grad=True)
    g = torch.randn(N, H, dtype=torch.float64)
    gi = F.linear(x, cell.weight_ih, cell.bias_ih).detach()
    gh = F.linear(h.detach(), cell.weight_hh, cell.bias_hh).detach()
    ref = GR.Reference(gi.numpy(), gh.numpy(), h.detach().numpy(), g.numpy(),
                       input_dtype=np.float64)
    # the cell itself, forward and through autograd: with d_gi, d_gh and d_hx of the reference,
    # d h = d_hx + d_gh W_hh, d W_ih = d_gi^T x, d W_hh = d_gh^T h, d b = the column sums
    out = cell(x, h)
    out.backward(g)
    assert _close(ref.u, out.detach().numpy())
    assert _close(ref.d_hx + ref.d_gh @ cell.weight_hh.detach().numpy(), h.grad.numpy())
    assert _close(ref.d_gi.T @ x.numpy(), cell.weight_ih.grad.numpy())
    assert _close(ref.d_gh.T @ h.detach().numpy(), cell.weight_hh.grad.numpy())
    if bias:
        assert _close(ref.d_gi.sum(0), cell.bias_ih.grad.numpy())
        assert _close(ref.d_gh.sum(0), cell.bias_hh.grad.numpy())
    # and tensor by tensor: the gates' formula on gi, gh and h as leaves, through autograd
    gi_t, gh_t = gi.clone().requires_grad_(True), gh.clone().requires_grad_(True)
    h_t = h.detach().clone().requires_grad_(True)
    r = torch.sigmoid(gi_t[:, :H] + gh_t[:, :H])
    z = torch.sigmoid(gi_t[:, H:2 * H] + gh_t[:, H:2 * H])
    n = torch.tanh(gi_t[:, 2 * H:] + r * gh_t[:, 2 * H:])
    u = (1 - z) * n + z * h_t
    assert _close(u.detach().numpy(), out.detach().numpy())      # the formula is the cell
    u.backward(g)
    assert _close(ref.u, u.detach().numpy())
    assert _close(ref.d_gi, gi_t.grad.numpy())
    assert _close(ref.d_gh, gh_t.grad.numpy())
    assert _close(ref.d_hx, h_t.grad.numpy())


def test_case_list():
    assert GR.CASES == [(1, 1, 1), (3, 3, 0), (5, 4, 5), (64, 7, 64), (65, 100, 17),
                        (257, 8, 64), (130, 172, 43)]
    assert all(0 <= R <= N for N, _, R in GR.CASES)
    assert len({GR.case_id(c) for c in GR.CASES}) == len(GR.CASES)
    c = GR.make_inputs((5, 4, 5))
    assert c["gi"].shape == c["gh"].shape == (5, 12) and c["hx"].shape == (5, 4)
    assert all(c[k].dtype == np.float32 for k in ("gi", "gh", "hx", "residual", "g"))
    again = GR.make_inputs((5, 4, 5))
    assert all(np.array_equal(c[k], again[k]) for k in ("gi", "gh", "hx", "residual", "g"))


def test_residual_and_last():
    c = GR.make_inputs((65, 100, 17))
    with_res, without = GR.reference(c), GR.reference(c, with_residual=False)
    assert np.array_equal(without.h_out, without.u) and np.array_equal(with_res.u, without.u)
    assert np.array_equal(with_res.h_out, without.u + c["residual"].astype(np.float64))
    assert with_res.last.shape == (17, 100) and np.array_equal(with_res.last, without.u[:17])
    assert np.array_equal(with_res.d_residual, c["g"].astype(np.float64))
    for k in ("d_gi", "d_gh", "d_hx"):      # the residual changes no other gradient
        assert np.array_equal(with_res.tensors()[k], without.tensors()[k])


def test_saturated_inputs_cover_the_extremes_and_stay_finite():
    case = (65, 100, 17)
    c = GR.make_saturated(case)
    H = case[1]
    pre_r = c["gi"][:, :H] + c["gh"][:, :H]
    pre_z = c["gi"][:, H:2 * H] + c["gh"][:, H:2 * H]
    for pre in (pre_r, pre_z, c["gi"][:, 2 * H:][:, ::2], c["gh"][:, 2 * H:][:, 1::2]):
        assert {float(v) for v in np.unique(pre)} == {float(np.float32(v)) for v in GR.EXTREMES}
    ref = GR.reference(c)
    for t in ref.tensors().values():
        assert np.isfinite(t).all()
    got = GR.emulate_fp32(c)
    for k, t in got.items():
        assert np.isfinite(t).all(), k


@pytest.mark.parametrize("case", GR.CASES, ids=GR.case_id)
def test_fp32_restatement_obeys_the_rule_against_itself(case):
    """The float32 restatement is within a few float32 roundings of the reference, and the rule's
    ratio of an evaluation against itself is at most 1/2."""
    c = GR.make_inputs(case)
    ref, got = GR.reference(c).tensors(), GR.emulate_fp32(c)
    for k in ref:
        assert GR.max_error(got[k], ref[k]) <= 64 * GR.FLOOR * max(np.abs(ref[k]).max(), 1.0) \
            if ref[k].size else True
        assert GR.ratio(got[k], got[k], ref[k]) <= 0.5


def test_round_bf16_is_torchs():
    rng = np.random.RandomState(5)
    a = np.concatenate([rng.standard_normal(4096).astype(np.float32) * 10,
                        np.array([0.0, -0.0, 1.0, 1.00390625, 1.01171875, 3.3895314e38],
                                 np.float32)])
    want = torch.from_numpy(a).to(torch.bfloat16).float().numpy()
    assert np.array_equal(GR.round_bf16(a).view(np.uint32), want.view(np.uint32))
