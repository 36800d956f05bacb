"""ops.time_encode_cat (csrc/time_encode.hip) against the float64 reference of
tests/time_encode_ref.py, within its a priori fp32 bounds, forward and backward: row counts
around a wave and far beyond a workgroup's rows, widths on the 16-byte and on the scalar path,
aligned and misaligned row pitch, the sampler's dt, large arguments, t = 0 and negative t,
row-slice and non-contiguous parts, both weight shapes, every gradient subset, n = 0,
determinism, the torch expression on the device and the error paths.  Each test prints its
largest error-to-bound ratio (run with -s)."""
import itertools

import numpy as np
import pytest

from tests import time_encode_ref as TE

pytestmark = pytest.mark.gpu


class _Margin:
    def __init__(self):
        self.worst = 0.0

    def check(self, what, ref, **got):
        for name, r in ref.ratios(**got).items():
            self.worst = max(self.worst, r)
            assert r <= 1.0, "{} {}: error / bound = {:.3g}".format(what, name, r)


@pytest.fixture
def margin(request):
    m = _Margin()
    yield m
    print("\n[error/bound] {}: {:.3g}".format(request.node.name, m.worst))


def _np(t):
    return t.detach().cpu().numpy()


def _dev(a, grad=False):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda().requires_grad_(grad)


_REFS = {}


def _ref(case):
    """(inputs, float64 reference) of a shared case: computed once, never modified."""
    if case not in _REFS:
        c = TE.make_inputs(case)
        _REFS[case] = (c, TE.reference(c))
    return _REFS[case]


def run(c, need_parts=True, need_w=True, need_bias=True, weight_2d=True, parts=None):
    """Forward + backward of the op -> (out, gw, gbias, [gparts]) as numpy (None: no grad)."""
    from gnnflow_amd import ops
    T = len(c["w"])
    parts = [_dev(p, need_parts) for p in c["parts"]] if parts is None else parts
    w = _dev(c["w"].reshape(T, 1) if weight_2d else c["w"], need_w)
    bias = _dev(c["bias"], need_bias)
    out = ops.time_encode_cat(parts, _dev(c["t"]), w, bias)
    assert tuple(out.shape) == c["gout"].shape
    if out.requires_grad:
        out.backward(_dev(c["gout"]))
    assert (w.grad is not None) == need_w and (bias.grad is not None) == need_bias
    assert w.grad is None or w.grad.shape == w.shape
    return (_np(out), None if w.grad is None else _np(w.grad).ravel(),
            None if bias.grad is None else _np(bias.grad),
            [None if p.grad is None else _np(p.grad) for p in parts])


@pytest.mark.parametrize("case", TE.CASES, ids=TE.case_id)
def test_forward_and_backward_within_the_bounds(case, margin):
    c, r = _ref(case)
    out, gw, gbias, gparts = run(c)
    assert r.copied_equal(out), "copied columns are not bit-equal"
    margin.check(TE.case_id(case), r, out=out, gw=gw, gbias=gbias)
    for got, want in zip(gparts, r.gparts):
        assert np.array_equal(got.astype(np.float64), want)


@pytest.mark.parametrize("case", [TE.CASES[3], TE.CASES[7]], ids=TE.case_id)
def test_weight_as_a_vector(case, margin):
    c, r = _ref(case)
    out, gw, gbias, _ = run(c, weight_2d=False)
    assert r.copied_equal(out)
    margin.check("weight [T]", r, out=out, gw=gw, gbias=gbias)
    assert np.array_equal(out, run(c, weight_2d=True)[0])


def test_t_as_a_column_and_time_encode_alone(margin):
    import torch
    from gnnflow_amd import ops
    c, r = _ref(TE.CASES[8])      # no parts
    t, w, bias = _dev(c["t"]), _dev(c["w"]), _dev(c["bias"])
    out = ops.time_encode(t.reshape(-1, 1), w, bias)
    margin.check("time_encode", r, out=_np(out))
    assert torch.equal(out, ops.time_encode_cat((), t, w.reshape(-1, 1), bias))


@pytest.mark.parametrize("case", [TE.CASES[4], TE.CASES[5]], ids=TE.case_id)
def test_row_slice_and_non_contiguous_parts(case, margin):
    """parts[0] = h[R:] of a taller tensor (the layer's source rows, taken as it is); parts[1]
    a column slice of a wider one (copied first).  Gradients reach the tensors behind them."""
    import torch
    c, r = _ref(case)
    n, R = len(c["t"]), 37
    wa, wb = c["parts"][0].shape[1], c["parts"][1].shape[1]
    h = torch.cat([torch.full((R, wa), 7.0), torch.from_numpy(c["parts"][0])]).cuda()
    h.requires_grad_(True)
    wide = torch.cat([torch.full((n, 2), 7.0), torch.from_numpy(c["parts"][1]),
                      torch.full((n, 1), 7.0)], 1).cuda().requires_grad_(True)
    a, b = h[R:], wide[:, 2:2 + wb]
    assert a.is_contiguous() and not b.is_contiguous()
    out, gw, gbias, _ = run(c, parts=[a, b])
    assert r.copied_equal(out)
    margin.check("views", r, out=out, gw=gw, gbias=gbias)
    gh, gwide = _np(h.grad), _np(wide.grad)
    assert not gh[:R].any() and np.array_equal(gh[R:].astype(np.float64), r.gparts[0])
    assert not gwide[:, :2].any() and not gwide[:, 2 + wb:].any()
    assert np.array_equal(gwide[:, 2:2 + wb].astype(np.float64), r.gparts[1])


def test_misaligned_base_pointer_takes_the_scalar_path(margin):
    """Widths that allow 16-byte accesses, behind an address that does not."""
    import torch
    c, r = _ref(TE.CASES[2])
    n, width = c["parts"][0].shape
    flat = torch.zeros(n * width + 1, device="cuda")
    part = flat[1:].view(n, width)
    part.copy_(torch.from_numpy(c["parts"][0]))
    assert part.is_contiguous() and part.data_ptr() % 16 == 4
    out, gw, gbias, _ = run(c, parts=[part.requires_grad_(True)])
    assert r.copied_equal(out)
    margin.check("misaligned", r, out=out, gw=gw, gbias=gbias)


@pytest.mark.parametrize("need", list(itertools.product([False, True], repeat=3)),
                         ids=lambda n: "".join("PWB"[i] if x else "-" for i, x in enumerate(n)))
def test_every_requires_grad_subset(need, margin):
    """An unrequested gradient is None; the requested ones do not depend on the others."""
    c, r = _ref(TE.CASES[5])
    need_parts, need_w, need_bias = need
    out, gw, gbias, gparts = run(c, need_parts, need_w, need_bias)
    assert r.copied_equal(out)
    margin.check(str(need), r, out=out, gw=gw, gbias=gbias)
    assert (gw is not None) == need_w and (gbias is not None) == need_bias
    for got, want in zip(gparts, r.gparts):
        assert (got is not None) == need_parts
        assert got is None or np.array_equal(got.astype(np.float64), want)
    full = run(c)
    assert gw is None or np.array_equal(gw, full[1])
    assert gbias is None or np.array_equal(gbias, full[2])


@pytest.mark.parametrize("widths", [(), (3,), (100, 16)], ids=str)
def test_no_rows(widths, monkeypatch):
    """n == 0: [0, W], zero gradients, and no native launch either way."""
    import torch
    from gnnflow_amd import _capi, ops
    T = 20
    parts = [torch.zeros((0, w), device="cuda", requires_grad=True) for w in widths]
    w = torch.ones((T, 1), device="cuda", requires_grad=True)
    bias = torch.ones(T, device="cuda", requires_grad=True)

    def no_native(*a, **k):
        raise AssertionError("native library touched")
    monkeypatch.setattr(_capi, "load", no_native)
    out = ops.time_encode_cat(parts, torch.zeros(0, device="cuda"), w, bias)
    assert tuple(out.shape) == (0, sum(widths) + T)
    out.sum().backward()
    assert w.grad.shape == (T, 1) and not w.grad.any() and not bias.grad.any()
    for p in parts:
        assert p.grad.shape == p.shape


def test_c_entry_points_with_no_rows_and_the_partials_query():
    import ctypes as C
    from gnnflow_amd import _capi
    lib = _capi.load()
    rows = C.c_size_t(99)
    for n, want in ((0, 0), (1, 1), (16, 1), (17, 2), (70001, 1024), (1 << 40, 1024)):
        _capi.check(lib.gf_time_encode_backward_partial_rows(n, C.byref(rows)))
        assert rows.value == want
    _capi.check(lib.gf_time_encode_cat(None, 0, None, 0, None, None, None, 0, 4, None, 0, None))
    _capi.check(lib.gf_time_encode_backward(None, None, None, 0, 4, None, 4, 0, None, 0, None,
                                            None, 0, None))


@pytest.mark.parametrize("case", [TE.CASES[4], TE.CASES[10], TE.CASES[11]], ids=TE.case_id)
def test_two_runs_are_bit_identical(case):
    c, _ = _ref(case)
    first, second = run(c), run(c)
    assert np.array_equal(first[0], second[0])
    assert np.array_equal(first[1], second[1]) and np.array_equal(first[2], second[2])


@pytest.mark.parametrize("case", [TE.CASES[1], TE.CASES[4], TE.CASES[5], TE.CASES[6]],
                         ids=TE.case_id)
def test_equals_the_torch_expression_on_the_device(case, margin):
    """torch.cat + TimeEncode's torch expression in fp32 on the device obeys the same bounds
    (its argument is one fused or two separate roundings, its cos and sin at most as far off,
    its sums some order of fp32 adds), so the two differ by at most the sum of both sides'
    bounds = twice the bound."""
    import torch
    import torch.nn.functional as F
    c, r = _ref(case)
    out, gw, gbias, gparts = run(c)
    parts = [_dev(p, True) for p in c["parts"]]
    w, bias = _dev(c["w"].reshape(-1, 1), True), _dev(c["bias"], True)
    want = torch.cat(parts + [torch.cos(F.linear(_dev(c["t"])[:, None], w, bias))], 1)
    want.backward(_dev(c["gout"]))
    off = r.offset
    assert np.array_equal(out[:, :off], _np(want)[:, :off])
    for name, got, ref, bound in (("enc", out[:, off:], _np(want)[:, off:], r.b_enc),
                                  ("gw", gw, _np(w.grad).ravel(), r.b_gw),
                                  ("gbias", gbias, _np(bias.grad), r.b_gbias)):
        ratio = TE.error_ratio(got, ref, 2 * bound)
        margin.worst = max(margin.worst, ratio)
        assert ratio <= 1.0, "{}: difference / (2 x bound) = {:.3g}".format(name, ratio)
    for got, p in zip(gparts, parts):
        assert np.array_equal(got, _np(p.grad))


def test_time_encode_module_takes_the_op_on_the_device(monkeypatch):
    import torch
    from gnnflow_amd import nn as gnn
    from gnnflow_amd import ops
    calls = []
    real = ops.time_encode
    monkeypatch.setattr(ops, "time_encode", lambda *a, **k: calls.append(1) or real(*a, **k))
    te = gnn.TimeEncode(20)
    dt = torch.tensor([0.0, 1.5, 300.0])
    on_cpu = te(dt)
    assert not calls
    te = te.cuda()
    got = te(dt.cuda())
    assert len(calls) == 1 and tuple(got.shape) == (3, 20)
    r = TE.Reference([], dt.numpy(), _np(te.w.weight), _np(te.w.bias), np.zeros((3, 20)))
    assert r.ratios(out=_np(got))["enc"] <= 1.0 and r.ratios(out=_np(on_cpu))["enc"] <= 1.0
    got.sum().backward()
    assert te.w.weight.grad.shape == (20, 1) and te.w.bias.grad.shape == (20,)


def test_error_paths():
    import ctypes as C
    import torch
    from gnnflow_amd import _capi, ops
    n, T = 6, 4
    t, w, b = (torch.zeros(n, device="cuda"), torch.ones(T, 1, device="cuda"),
               torch.zeros(T, device="cuda"))
    part = torch.zeros(n, 3, device="cuda")
    with pytest.raises(ValueError, match="at most two parts"):
        ops.time_encode_cat((part, part, part), t, w, b)
    with pytest.raises(TypeError, match="float32"):
        ops.time_encode_cat((part.half(),), t, w, b)
    with pytest.raises(ValueError, match="rows"):
        ops.time_encode_cat((part[1:],), t, w, b)
    with pytest.raises(ValueError, match="T >= 1"):
        ops.time_encode_cat((part,), t, w[:0], b[:0])
    with pytest.raises(ValueError, match="is on"):
        ops.time_encode_cat((part.cpu(),), t, w, b)
    # the C entry points: null t / w / bias / out, T == 0, a pitch the columns do not fit, a
    # partials buffer smaller than the query asks for -- rejected before any launch
    lib = _capi.load()
    out = torch.empty(n, 3 + T, device="cuda")

    def p(x):
        return C.c_void_p(x.data_ptr())
    good = [p(part), 3, None, 0, p(t), p(w), p(b), n, T, p(out), 0, None]
    for i in (4, 5, 6, 9):
        args = list(good)
        args[i] = None
        assert lib.gf_time_encode_cat(*args) == _capi.GF_ERR_INVALID_ARGUMENT
        assert b"null" in lib.gf_last_error()
    args = list(good)
    args[8] = 0
    assert lib.gf_time_encode_cat(*args) == _capi.GF_ERR_INVALID_ARGUMENT
    args = list(good)
    args[0] = None                                     # width 3 without an address
    assert lib.gf_time_encode_cat(*args) == _capi.GF_ERR_INVALID_ARGUMENT
    partials = torch.empty(1, 2, T, device="cuda")
    gw, gb = torch.empty(T, device="cuda"), torch.empty(T, device="cuda")
    good = [p(t), p(w), p(b), n, T, p(out), 3 + T, 3, p(partials), 1, p(gw), p(gb), 0, None]
    for i, value in ((0, None), (1, None), (2, None), (5, None), (4, 0), (7, 4), (8, None),
                     (9, 0)):
        args = list(good)
        args[i] = value
        assert lib.gf_time_encode_backward(*args) == _capi.GF_ERR_INVALID_ARGUMENT, i
    with pytest.raises(ValueError):
        _capi.check(lib.gf_time_encode_backward_partial_rows(n, None))
    torch.cuda.synchronize()
