"""ops.edge_score (csrc/edge_score.hip) against the float64 reference of tests/edge_score_ref.py:
out, gw and gbias within its a priori fp32 bounds, gsrc and gdst bit-equal to its fp32
restatement.  Row counts around a lane group, a wave and the backward's row groups, widths on the
16-byte and the scalar path and beyond one pass of the lanes, one to three dst blocks, a tall
case at the cap of the partial rows, both weight shapes, a misaligned base pointer, row-slice
and non-contiguous inputs, every gradient subset, M = 0, the C entry points, determinism, the
torch expression on the device and the error paths.  Each test prints its largest
error-to-bound ratio (run with -s)."""
import itertools

import numpy as np
import pytest

from tests import edge_score_ref as ES

pytestmark = pytest.mark.gpu


class _Margin:
    def __init__(self):
        self.worst = 0.0

    def check(self, what, ref, scale=1.0, **got):
        for name, r in ref.ratios(scale=scale, **got).items():
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
        c = ES.make_inputs(case)
        _REFS[case] = (c, ES.reference(c))
    return _REFS[case]


def run(c, need=(True, True, True, True), weight_2d=False, src=None, dst=None):
    """Forward + backward of the op -> (out, gsrc, gdst, gw, gbias) as numpy (None: no grad)."""
    from gnnflow_amd import ops
    D, M = len(c["w"]), len(c["g"])
    src = _dev(c["src"], need[0]) if src is None else src
    dst = _dev(c["dst"], need[1]) if dst is None else dst
    w = _dev(c["w"].reshape(1, D) if weight_2d else c["w"], need[2])
    bias = _dev(c["bias"], need[3])
    out = ops.edge_score(src, dst, w, bias)
    assert tuple(out.shape) == (M, 1) and out.requires_grad == any(need)
    if out.requires_grad:
        out.backward(_dev(c["g"].reshape(M, 1)))
    leaves = (src, dst, w, bias)
    for t, n in zip(leaves, need):
        if t.is_leaf:
            assert (t.grad is not None) == n
            assert t.grad is None or t.grad.shape == t.shape
    return (_np(out),) + tuple(None if (not t.is_leaf or t.grad is None) else _np(t.grad)
                               for t in leaves)


def _check(what, r, res, margin, scale=1.0):
    out, gsrc, gdst, gw, gbias = res
    margin.check(what, r, scale=scale, out=out, gw=gw, gbias=gbias)
    assert r.exact_equal(gsrc=gsrc), what + ": gsrc is not bit-equal"
    assert r.exact_equal(gdst=gdst), what + ": gdst is not bit-equal"


@pytest.mark.parametrize("case", ES.CASES + [ES.TALL], ids=ES.case_id)
def test_forward_and_backward(case, margin):
    c, r = _ref(case)
    _check(ES.case_id(case), r, run(c), margin)


@pytest.mark.parametrize("case", [(17, 172, 3), (65, 3, 1)], ids=ES.case_id)
def test_weight_as_a_row(case, margin):
    c, r = _ref(case)
    res = run(c, weight_2d=True)
    assert res[3].shape == (1, case[1])
    _check("weight [1, D]", r, res, margin)
    for a, b in zip(res, run(c)):
        assert np.array_equal(a.ravel(), b.ravel())


@pytest.mark.parametrize("case", [(64, 4, 3), (15, 100, 2), (16, 128, 1)], ids=ES.case_id)
def test_misaligned_base_pointers_take_the_scalar_path(case, margin):
    """D % 4 == 0 behind addresses that do not allow 16-byte loads: each of src, dst and weight
    in turn.  The columns stay on their lanes, so even out is bit-equal to the aligned run."""
    import torch
    c, r = _ref(case)
    aligned = run(c)

    def shifted(a):
        flat = torch.zeros(a.size + 1, device="cuda")
        t = flat[1:].view(*a.shape)
        t.copy_(torch.from_numpy(a))
        assert t.is_contiguous() and t.data_ptr() % 16 == 4
        return t.requires_grad_(True)

    from gnnflow_amd import ops
    for which in ("src", "dst", "w"):
        t = {k: (shifted(c[k]) if k == which else _dev(c[k], True)) for k in ("src", "dst", "w")}
        bias = _dev(c["bias"], True)
        out = ops.edge_score(t["src"], t["dst"], t["w"], bias)
        out.backward(_dev(c["g"].reshape(-1, 1)))
        res = (_np(out), _np(t["src"].grad), _np(t["dst"].grad), _np(t["w"].grad), _np(bias.grad))
        _check("misaligned " + which, r, res, margin)
        for a, b in zip(res, aligned):
            assert np.array_equal(a, b), which


@pytest.mark.parametrize("case", [(17, 100, 1), (63, 257, 2)], ids=ES.case_id)
def test_row_slice_and_non_contiguous_inputs(case, margin):
    """src = h[:B] and dst = h[B:] of one taller tensor (the predictor's rows, taken as they
    are), then dst a column slice of a wider tensor (copied first).  Gradients reach the tensors
    behind them."""
    import torch
    c, r = _ref(case)
    B, D, _ = case
    h = torch.from_numpy(np.concatenate([c["src"], c["dst"]])).cuda().requires_grad_(True)
    src, dst = h[:B], h[B:]
    assert src.is_contiguous() and dst.is_contiguous() and dst.data_ptr() != h.data_ptr()
    res = run(c, src=src, dst=dst)
    gh = _np(h.grad)
    _check("row slices", r, (res[0], gh[:B], gh[B:], res[3], res[4]), margin)
    wide = torch.cat([torch.full((len(c["dst"]), 2), 7.0), torch.from_numpy(c["dst"]),
                      torch.full((len(c["dst"]), 1), 7.0)], 1).cuda().requires_grad_(True)
    dst = wide[:, 2:2 + D]
    assert not dst.is_contiguous()
    res = run(c, dst=dst)
    gwide = _np(wide.grad)
    assert not gwide[:, :2].any() and not gwide[:, 2 + D:].any()
    _check("column slice", r, (res[0], res[1], np.ascontiguousarray(gwide[:, 2:2 + D]), res[3],
                               res[4]), margin)


@pytest.mark.parametrize("need", list(itertools.product([False, True], repeat=4)),
                         ids=lambda n: "".join("SDWB"[i] if x else "-" for i, x in enumerate(n)))
def test_every_requires_grad_subset(need, margin):
    """An unrequested gradient is None; the requested ones are bit-equal to the full run."""
    c, r = _ref((17, 172, 3))
    res = run(c, need)
    full = run(c)
    assert np.array_equal(res[0], full[0])
    margin.check(str(need), r, out=res[0], gw=res[3], gbias=res[4])
    for got, want, n in zip(res[1:], full[1:], need):
        assert (got is not None) == n
        assert got is None or np.array_equal(got, want)
    assert r.exact_equal(gsrc=res[1], gdst=res[2])


@pytest.mark.parametrize("B", [0, 5])
def test_no_dst_rows(B, monkeypatch):
    """M == 0: [0, 1], zero gradients, and no native call either way."""
    import torch
    from gnnflow_amd import _capi, ops
    D = 12
    src = torch.ones((B, D), device="cuda", requires_grad=True)
    dst = torch.ones((0, D), device="cuda", requires_grad=True)
    w = torch.ones((1, D), device="cuda", requires_grad=True)
    bias = torch.ones(1, device="cuda", requires_grad=True)

    def no_native(*a, **k):
        raise AssertionError("native library touched")
    monkeypatch.setattr(_capi, "load", no_native)
    out = ops.edge_score(src, dst, w, bias)
    assert tuple(out.shape) == (0, 1)
    out.sum().backward()
    for t in (src, dst, w, bias):
        assert t.grad.shape == t.shape and not t.grad.any()


def test_c_entry_points_with_no_rows_and_the_partials_query():
    import ctypes as C
    from gnnflow_amd import _capi
    lib = _capi.load()
    rows = C.c_size_t(99)
    for n, want in ((0, 0), (1, 1), (8, 1), (9, 2), (8192, 1024), (8193, 1024), (70001, 1024),
                    (1 << 40, 1024)):
        _capi.check(lib.gf_edge_score_backward_partial_rows(n, C.byref(rows)))
        assert rows.value == want, n
    for B in (0, 3):
        _capi.check(lib.gf_edge_score(None, None, None, None, B, 0, 4, None, 0, None))
        _capi.check(lib.gf_edge_score_backward(None, None, None, B, 0, 4, None, None, 0, None,
                                               None, None, None, 0, None))


def test_backward_without_gw_and_gbias_needs_no_partials(margin):
    """The C entry point with null d_grad_w, d_grad_bias AND a null partials buffer: gsrc and
    gdst only.  And with only d_grad_bias: nothing else is written."""
    import ctypes as C
    import torch
    from gnnflow_amd import _capi
    case = (65, 128, 3)
    c, r = _ref(case)
    B, D, _ = case
    M = len(c["g"])
    lib = _capi.load()

    def p(x):
        return C.c_void_p(x.data_ptr())
    src, dst, w, g = _dev(c["src"]), _dev(c["dst"]), _dev(c["w"]), _dev(c["g"])
    gsrc, gdst = torch.full((B, D), 7.0, device="cuda"), torch.full((M, D), 7.0, device="cuda")
    _capi.check(lib.gf_edge_score_backward(p(src), p(dst), p(w), B, M, D, p(g), None, 0, p(gsrc),
                                           p(gdst), None, None, 0, None))
    assert r.exact_equal(gsrc=_np(gsrc), gdst=_np(gdst))
    rows = C.c_size_t(0)
    _capi.check(lib.gf_edge_score_backward_partial_rows(B, C.byref(rows)))
    partials = torch.empty((rows.value, D + 1), device="cuda")
    gbias = torch.full((1,), 7.0, device="cuda")
    _capi.check(lib.gf_edge_score_backward(p(src), p(dst), p(w), B, M, D, p(g), p(partials),
                                           rows.value, None, None, None, p(gbias), 0, None))
    margin.check("gbias alone", r, gbias=_np(gbias))


@pytest.mark.parametrize("case", [(600, 172, 2), (63, 257, 2), ES.TALL], ids=ES.case_id)
def test_two_runs_are_bit_identical(case):
    c, _ = _ref(case)
    for a, b in zip(run(c), run(c)):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("case", [(3, 3, 3), (16, 128, 1), (600, 100, 2), (600, 257, 3)],
                         ids=ES.case_id)
def test_equals_the_torch_expression_on_the_device(case, margin):
    """relu(src + dst block) @ w.T + bias per block in fp32 on the device obeys the same bounds
    (its add and its mask are the kernel's, its sums some order of fp32 adds and multiplies,
    fused or not), so the two differ by at most the sum of both sides' bounds = twice the
    bound; gdst is one rounding of g w m on either side and gsrc at most r of the blocks' sum."""
    import torch
    import torch.nn.functional as F
    c, r = _ref(case)
    B = case[0]
    got = run(c)
    src, dst = _dev(c["src"], True), _dev(c["dst"], True)
    w, bias = _dev(c["w"].reshape(1, -1), True), _dev(c["bias"], True)
    want = torch.cat([F.linear(F.relu(src + dst[k * B:(k + 1) * B]), w, bias)
                      for k in range(case[2])])
    want.backward(_dev(c["g"].reshape(-1, 1)))
    for name, a, b, bound in (("out", got[0], _np(want), r.b_out),
                              ("gw", got[3], _np(w.grad).ravel(), r.b_gw),
                              ("gbias", got[4], _np(bias.grad), r.b_gbias)):
        ratio = ES.error_ratio(a, b, 2 * bound)
        margin.worst = max(margin.worst, ratio)
        assert ratio <= 1.0, "{}: difference / (2 x bound) = {:.3g}".format(name, ratio)
    # gdst is one rounding of g w m on either side, gsrc at most r roundings of the blocks' sum
    blocks = np.abs(r.gdst).reshape(r.r, r.B, r.D).sum(0)
    for name, a, b, bound in (("gdst", got[2], _np(dst.grad), ES.U * np.abs(r.gdst)),
                              ("gsrc", got[1], _np(src.grad), ES.gamma(r.r) * blocks)):
        ratio = ES.error_ratio(a, b, 2 * bound)
        margin.worst = max(margin.worst, ratio)
        assert ratio <= 1.0, "{}: difference / (2 x bound) = {:.3g}".format(name, ratio)


def test_error_paths():
    import ctypes as C
    import torch
    from gnnflow_amd import _capi, ops
    B, M, D = 3, 6, 4
    src, dst = torch.zeros(B, D, device="cuda"), torch.zeros(M, D, device="cuda")
    w, b = torch.ones(1, D, device="cuda"), torch.zeros(1, device="cuda")
    with pytest.raises(TypeError, match="float32"):
        ops.edge_score(src.half(), dst, w, b)
    with pytest.raises(TypeError, match="float32"):
        ops.edge_score(src, dst, w.double(), b)
    with pytest.raises(TypeError, match="tensor"):
        ops.edge_score(src, dst, w, 0.0)
    with pytest.raises(ValueError, match="multiple"):
        ops.edge_score(src, dst[:5], w, b)
    with pytest.raises(ValueError, match="multiple"):
        ops.edge_score(src[:0], dst, w, b)                 # B = 0 with M > 0
    with pytest.raises(ValueError, match="columns"):
        ops.edge_score(src, dst[:, :3], w, b)
    with pytest.raises(ValueError, match="D >= 1"):
        ops.edge_score(src[:, :0], dst[:, :0], w[:, :0], b)
    with pytest.raises(ValueError, match="weight"):
        ops.edge_score(src, dst, w[:, :3], b)
    with pytest.raises(ValueError, match="bias"):
        ops.edge_score(src, dst, w, torch.zeros(2, device="cuda"))
    with pytest.raises(ValueError, match=r"\[B, D\]"):
        ops.edge_score(src[0], dst, w, b)
    with pytest.raises(ValueError, match="is on"):
        ops.edge_score(src.cpu(), dst, w, b)
    with pytest.raises(ValueError, match="is on"):
        ops.edge_score(src, dst, w, b.cpu())
    with pytest.raises(ValueError, match="on the GPU"):
        ops.edge_score(src.cpu(), dst.cpu(), w.cpu(), b.cpu())
    # the C entry points: null pointers, D == 0, M % B != 0, B == 0, a partials buffer that is
    # missing or smaller than the query asks for -- rejected before any launch
    lib = _capi.load()
    out, g = torch.empty(M, device="cuda"), torch.ones(M, device="cuda")

    def p(x):
        return C.c_void_p(x.data_ptr())
    good = [p(src), p(dst), p(w), p(b), B, M, D, p(out), 0, None]
    _capi.check(lib.gf_edge_score(*good))
    for i, value in ((0, None), (1, None), (2, None), (3, None), (7, None), (6, 0), (5, 7),
                     (4, 0), (4, 4)):
        args = list(good)
        args[i] = value
        assert lib.gf_edge_score(*args) == _capi.GF_ERR_INVALID_ARGUMENT, i
        assert (b"null" in lib.gf_last_error()) == (value is None)
    partials = torch.empty(1, D + 1, device="cuda")
    gs, gd = torch.empty(B, D, device="cuda"), torch.empty(M, D, device="cuda")
    gw, gb = torch.empty(D, device="cuda"), torch.empty(1, device="cuda")
    good = [p(src), p(dst), p(w), B, M, D, p(g), p(partials), 1, p(gs), p(gd), p(gw), p(gb), 0,
            None]
    _capi.check(lib.gf_edge_score_backward(*good))
    for i, value in ((0, None), (1, None), (2, None), (6, None), (5, 0), (4, 7), (3, 0), (3, 4),
                     (7, None), (8, 0)):
        args = list(good)
        args[i] = value
        assert lib.gf_edge_score_backward(*args) == _capi.GF_ERR_INVALID_ARGUMENT, i
    with pytest.raises(ValueError):
        _capi.check(lib.gf_edge_score_backward_partial_rows(B, None))
    torch.cuda.synchronize()
