"""CPU checks of tests/edge_score_ref.py: the float64 reference against torch autograd in
float64, an fp32 numpy evaluation of the same formula inside the bounds (and bit-equal where the
reference asks for equality), the exact mask, the case list's coverage and the cases'
reproducibility from their seeds."""
import numpy as np
import pytest

from tests import edge_score_ref as ES

ALL = ES.CASES + [ES.TALL]


def _torch64(c):
    import torch
    import torch.nn.functional as F
    t = {k: torch.from_numpy(v.astype(np.float64)).requires_grad_(True)
         for k, v in c.items() if k != "g"}
    B, M = c["src"].shape[0], c["dst"].shape[0]
    outs = [F.linear(F.relu(t["src"] + t["dst"][k * B:(k + 1) * B]), t["w"][None, :], t["bias"])
            for k in range(M // B)]
    out = torch.cat(outs)
    out.backward(torch.from_numpy(c["g"].astype(np.float64)).reshape(M, 1))
    return out.detach().numpy(), {k: v.grad.numpy() for k, v in t.items()}


@pytest.mark.parametrize("case", ES.CASES, ids=ES.case_id)
def test_reference_equals_torch_autograd_in_float64(case):
    c = ES.make_inputs(case)
    r = ES.reference(c)
    out, grads = _torch64(c)
    tol = dict(rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(r.out, out, **tol)
    np.testing.assert_allclose(r.gsrc, grads["src"], **tol)
    np.testing.assert_allclose(r.gdst, grads["dst"], **tol)
    np.testing.assert_allclose(r.gw, grads["w"], **tol)
    np.testing.assert_allclose(r.gbias, grads["bias"], **tol)


@pytest.mark.parametrize("case", ALL, ids=ES.case_id)
def test_fp32_evaluation_sits_inside_the_bounds(case):
    c = ES.make_inputs(case)
    r = ES.reference(c)
    out, gsrc, gdst, gw, gbias = ES.emulate_fp32(c)
    assert np.array_equal(r.mask32, r.mask), "the fp32 mask is not the exact mask"
    if r.mask.size >= 64:      # on, off, and off through an exact zero all occur
        x0 = c["src"][np.arange(r.M) % r.B] + c["dst"] == 0
        assert r.mask.any() and (~r.mask & ~x0).any() and x0.any()
    assert r.exact_equal(gsrc=gsrc, gdst=gdst)
    ratios = r.ratios(out=out, gw=gw, gbias=gbias)
    print("\n[error/bound] {}: {}".format(ES.case_id(case), ratios))
    assert max(ratios.values()) <= 1.0, ratios
    # the restatement is the float64 gradient rounded once (gdst) and r - 1 times more (gsrc)
    assert ES.error_ratio(r.gdst32, r.gdst, ES.U * np.abs(r.gdst)) <= 1.0
    assert ES.error_ratio(r.gsrc32, r.gsrc,
                          ES.gamma(r.r) * np.abs(r.gdst).reshape(r.r, r.B, r.D).sum(0)) <= 1.0


def test_a_wrong_result_is_outside_the_bounds():
    c = ES.make_inputs((17, 100, 2))
    r = ES.reference(c)
    out, gsrc, gdst, gw, gbias = ES.emulate_fp32(c)
    assert r.ratios(out=out * np.float32(1 + 2e-5))["out"] > 1.0
    assert r.ratios(gw=np.roll(gw, 1))["gw"] > 1.0
    assert r.ratios(gbias=gbias + np.float32(1e-3))["gbias"] > 1.0
    assert not r.exact_equal(gdst=np.nextafter(gdst, np.float32(np.inf)))
    assert not r.exact_equal(gsrc=gsrc[::-1])
    assert not r.exact_equal(gsrc=gsrc.astype(np.float64))


def test_every_product_stays_a_normal_fp32():
    tiny = np.finfo(np.float32).tiny
    for case in ALL:
        c = ES.make_inputs(case)
        for v in c.values():
            assert v.dtype == np.float32 and (np.abs(v) >= 2.0 ** -3).all() and (np.abs(v) <= 4).all()
        B, M = c["src"].shape[0], c["dst"].shape[0]
        x = c["src"][np.arange(M) % B] + c["dst"]
        nz = np.abs(x[x != 0])
        assert nz.size == 0 or nz.min() * 2.0 ** -3 * 2.0 ** -3 >= tiny


def test_cases_cover_every_axis_value_and_are_reproducible():
    assert {c[0] for c in ES.CASES} == {1, 3, 15, 16, 17, 63, 64, 65, 600}
    assert {c[1] for c in ES.CASES} == {1, 3, 4, 100, 128, 172, 257}
    assert {c[2] for c in ES.CASES} == {1, 2, 3}
    assert ES.TALL == (70001, 8, 1)
    assert len(set(ES.CASES)) == len(ES.CASES)
    for case in (ES.CASES[3], ES.CASES[15]):
        a, b = ES.make_inputs(case), ES.make_inputs(case)
        assert all(np.array_equal(a[k], b[k]) for k in a)
        other = ES.make_inputs(case, seed=5)
        assert not np.array_equal(a["dst"], other["dst"])
        assert all(np.array_equal(other[k], ES.make_inputs(case, seed=5)[k]) for k in other)
