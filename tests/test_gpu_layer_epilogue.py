"""ops.dropout_relu_layer_norm (csrc/layer_epilogue.hip) against the float64 reference of
tests/layer_epilogue_ref.py: out, mean, rstd, grad_x, grad_gamma and grad_beta within its a priori
fp32 bounds.  Widths on both load paths, around a wave's 64 lanes and up to the maximum, row counts
around a workgroup and the cap of the partial rows, p = 0 and 0.2, no rows, the rows that break a
careless kernel, the mask itself, misaligned base pointers, row-slice and non-contiguous inputs,
every gradient subset, determinism, the torch expression on the device and the bfloat16 contract.
Each test prints its largest error-to-bound ratio (run with -s)."""
import itertools

import numpy as np
import pytest

from tests import layer_epilogue_ref as LE

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
    return None if t is None else t.detach().float().cpu().numpy()


def _dev(a, grad=False):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda().requires_grad_(grad)


_REFS = {}


def _ref(case, p=0.0, seed=LE.SEED):
    """(inputs, float64 reference) of a shared case: computed once, never modified."""
    key = (case, p, seed)
    if key not in _REFS:
        c = LE.make_inputs(case)
        _REFS[key] = (c, LE.reference(c, p=p, seed=seed))
    return _REFS[key]


def run(c, p=0.0, seed=LE.SEED, need=(True, True, True), x=None, weight=None, bias=None,
        gout=None, eps=LE.EPS):
    """Forward + backward of the op -> dict(out, gx, ggamma, gbeta) of torch tensors (None: no
    gradient)."""
    import torch
    from gnnflow_amd import ops
    x = _dev(c["x"], need[0]) if x is None else x
    w = _dev(c["weight"], need[1]) if weight is None else weight
    b = _dev(c["bias"], need[2]) if bias is None else bias
    out = ops.dropout_relu_layer_norm(x, w, b, eps=eps, dropout_p=p, dropout_seed=seed)
    assert out.dtype == torch.float32 and out.shape == x.shape
    assert out.requires_grad == any(t.requires_grad for t in (x, w, b))
    if out.requires_grad:
        out.backward(_dev(c["gout"]) if gout is None else gout)
    grads = [t.grad if t.is_leaf else None for t in (x, w, b)]
    for t, g in zip((x, w, b), grads):
        assert g is None or (g.shape == t.shape and g.dtype == t.dtype)
    return dict(out=out.detach(), gx=grads[0], ggamma=grads[1], gbeta=grads[2])


def stats(c, p=0.0, seed=LE.SEED, eps=LE.EPS):
    """(out, mean, rstd) of the C entry point itself: the op returns out alone."""
    import torch
    from gnnflow_amd import _capi
    x, w, b = _dev(c["x"]), _dev(c["weight"]), _dev(c["bias"])
    R, D = x.shape
    out = torch.empty_like(x)
    mean, rstd = torch.empty(R, device="cuda"), torch.empty(R, device="cuda")
    _capi.check(_capi.load().gf_layer_epilogue(
        x.data_ptr(), w.data_ptr(), b.data_ptr(), R, D, eps, p, seed, out.data_ptr(),
        mean.data_ptr(), rstd.data_ptr(), 0, _capi.current_stream(x.device)))
    torch.cuda.synchronize()
    return out, mean, rstd


def _check(what, c, r, margin, p=0.0, seed=LE.SEED):
    res = run(c, p, seed)
    out, mean, rstd = stats(c, p, seed)
    assert bits_equal(out, res["out"]), what + ": the op and the entry point differ"
    margin.check(what, r, mean=_np(mean), rstd=_np(rstd), **{k: _np(v) for k, v in res.items()})
    return res


def bits_equal(a, b):
    import torch
    if a is None or b is None:
        return a is None and b is None
    return a.dtype == b.dtype and a.shape == b.shape and \
        torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def all_bits_equal(a, b):
    return all(bits_equal(a[k], b[k]) for k in a)


@pytest.mark.parametrize("p", LE.PS)
@pytest.mark.parametrize("case", LE.CASES, ids=LE.case_id)
def test_forward_and_backward(case, p, margin):
    c, r = _ref(case, p)
    _check(LE.case_id(case), c, r, margin, p)


def test_no_rows():
    import torch
    c = LE.make_inputs((0, 100))
    for p in LE.PS:
        res = run(c, p)
        assert res["out"].shape == (0, 100) and res["gx"].shape == (0, 100)
        assert res["ggamma"].shape == (100,) and not res["ggamma"].any()
        assert res["gbeta"].shape == (100,) and not res["gbeta"].any()
    # the entry point zeroes the parameter gradients it is given
    from gnnflow_amd import _capi
    gg, gb = torch.ones(100, device="cuda"), torch.ones(100, device="cuda")
    _capi.check(_capi.load().gf_layer_epilogue_backward(
        None, None, None, None, 0, 100, 0.0, 0, None, None, 0, None, gg.data_ptr(),
        gb.data_ptr(), 0, _capi.current_stream(gg.device)))
    torch.cuda.synchronize()
    assert not gg.any() and not gb.any()


def test_rows_that_break_a_careless_kernel(margin):
    """A constant row (variance 0: out is beta exactly), an all-negative row (y = 0), one 1e4
    entry among 1e-3 entries, zeros among positive entries (relu's gradient at 0 is 0) and large,
    nearly equal entries (where E[y^2] - mean^2 misses the bound of rstd by three orders of
    magnitude, tests/test_layer_epilogue_ref.py)."""
    c = LE.special_case()
    r = LE.reference(c)
    res = {k: _np(v) for k, v in _check("special rows", c, r, margin).items()}
    assert np.array_equal(res["out"][0], c["bias"]) and np.array_equal(res["out"][1], c["bias"])
    assert np.isfinite(res["gx"]).all() and np.isfinite(res["ggamma"]).all()
    assert not res["gx"][1].any() and not res["gx"][3, ::3].any()
    assert res["gx"][3, 1::3].all() and res["gx"][3, 2::3].all()


def test_fully_dropped_row(margin):
    R, D, p = 4, 3, 0.9
    seed = LE.ALL_DROPPED_SEED
    dropped = (~LE.keep_mask(R, D, p, seed)).all(axis=1)
    assert dropped.any()
    c = LE.make_inputs((R, D))
    c["x"] = np.abs(c["x"])
    r = LE.reference(c, p=p, seed=seed)
    res = {k: _np(v) for k, v in _check("all dropped", c, r, margin, p, seed).items()}
    assert np.array_equal(res["out"][dropped], np.broadcast_to(c["bias"], (dropped.sum(), D)))
    assert not res["gx"][dropped].any()


@pytest.mark.parametrize("seed", [LE.SEED, 977])
def test_the_mask_is_the_references(seed):
    """gamma = 1, beta = 0 and positive x at p = 0.2: grad_x is 0 exactly where the reference
    drops, the forward of the same call drops the same elements (a dropped element has the row's
    smallest output, that of y = 0), and the kept share is within 5 binomial standard deviations
    of 0.8 (for the reference's mask: tests/test_layer_epilogue_ref.py)."""
    R, D, p = 257, 100, 0.2
    c = LE.make_inputs((R, D))
    c["x"] = np.abs(c["x"])
    c["weight"], c["bias"] = np.ones(D, np.float32), np.zeros(D, np.float32)
    keep = LE.keep_mask(R, D, p, seed)
    res = {k: _np(v) for k, v in run(c, p, seed).items()}
    assert np.array_equal(res["gx"] != 0, keep)
    some = ~keep.all(axis=1)
    assert some.sum() > 200
    assert np.array_equal((res["out"] > res["out"].min(axis=1, keepdims=True))[some], keep[some])
    assert abs((res["gx"] != 0).mean() - 0.8) <= 5 * np.sqrt(0.2 * 0.8 / (R * D))


def _shifted(a):
    """A contiguous copy of `a` one element past a 16-byte boundary."""
    import torch
    flat = torch.zeros(a.size + 1, device="cuda")
    t = flat[1:].view(*a.shape)
    t.copy_(torch.from_numpy(a))
    assert t.is_contiguous() and t.data_ptr() % 16 == 4
    return t


@pytest.mark.parametrize("p", LE.PS)
@pytest.mark.parametrize("case", [(5, 100), (257, 100), (5, 1024)], ids=LE.case_id)
def test_misaligned_base_pointers_take_the_scalar_path(case, p):
    """D % 4 == 0 behind addresses that do not allow 16-byte loads: each of x, gamma, beta and
    grad_out in turn.  The columns stay on their lanes, so every result is bit-equal to the
    aligned run's."""
    c, _ = _ref(case, p)
    aligned = run(c, p)
    for which in ("x", "weight", "bias", "gout"):
        kw = {which: _shifted(c[which])}
        if which != "gout":
            kw[which].requires_grad_(True)
        assert all_bits_equal(aligned, run(c, p, **kw)), which


@pytest.mark.parametrize("p", LE.PS)
def test_row_slice_and_non_contiguous_x(p):
    import torch
    R, D = 257, 100
    c, _ = _ref((R, D), p)
    want = run(c, p)
    big = torch.zeros((R + 2, D), device="cuda")
    big[1:R + 1] = torch.from_numpy(c["x"]).cuda()
    rows = big[1:R + 1].detach().requires_grad_(True)
    wide = torch.zeros((R, D + 3), device="cuda")
    wide[:, 1:D + 1] = torch.from_numpy(c["x"]).cuda()
    cols = wide[:, 1:D + 1].detach().requires_grad_(True)
    assert rows.is_contiguous() and not cols.is_contiguous()
    for name, x in (("row slice", rows), ("column slice", cols),
                    ("transposed", _dev(c["x"].T.copy()).t().requires_grad_(True))):
        got = run(c, p, x=x)
        assert all_bits_equal(want, got), name


class _Spy:
    """The native library with the arguments of every call recorded."""

    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)

        def call(*args):
            self.calls.append((name, args))
            return fn(*args)
        return call


@pytest.mark.parametrize("p", LE.PS)
def test_every_requires_grad_subset(p, monkeypatch):
    from gnnflow_amd import _capi
    c, _ = _ref((257, 100), p)
    full = run(c, p)
    lib = _capi.load()
    for need in itertools.product((False, True), repeat=3):
        spy = _Spy(lib)
        monkeypatch.setattr(_capi, "load", lambda: spy)
        got = run(c, p, need=need)
        monkeypatch.setattr(_capi, "load", lambda: lib)
        assert bits_equal(got["out"], full["out"])
        for k, n in zip(("gx", "ggamma", "gbeta"), need):
            assert (got[k] is not None) == n, (need, k)
            assert got[k] is None or bits_equal(got[k], full[k]), (need, k)
        names = [n for n, _ in spy.calls]
        back = [a for n, a in spy.calls if n == "gf_layer_epilogue_backward"]
        assert len(back) == (1 if any(need) else 0)
        if any(need) and not (need[1] or need[2]):      # no partials: not asked for, not passed
            assert "gf_layer_epilogue_backward_partial_rows" not in names
            assert back[0][9] is None and back[0][10] == 0
            assert back[0][12] is None and back[0][13] is None
        if any(need):
            assert (back[0][11] is None) == (not need[0])


def test_two_runs_give_the_same_bits():
    c, _ = _ref((1025, 100), 0.2)
    a, b = run(c, 0.2), run(c, 0.2)
    assert all_bits_equal(a, b)
    assert not all_bits_equal(a, run(c, 0.2, seed=977))


@pytest.mark.parametrize("p", LE.PS)
@pytest.mark.parametrize("case", [(5, 3), (257, 100), (5, 172), (5, 1024)], ids=LE.case_id)
def test_against_torch_on_the_device(case, p, margin):
    """F.layer_norm(F.relu(x * keep * scale)) with the reference's mask uploaded: torch's fp32
    kernels are held to the same a priori bounds, so the two sides differ by at most their sum."""
    import torch
    import torch.nn.functional as F
    from tests.attention_dropout_ref import scale
    c, r = _ref(case, p)
    R, D = case
    x, w, b = (_dev(c[k], True) for k in ("x", "weight", "bias"))
    keep = _dev(r.keep.astype(np.float32))
    out = F.layer_norm(F.relu(x * keep * float(scale(p))), (D,), w, b, LE.EPS)
    out.backward(_dev(c["gout"]))
    ours = run(c, p)
    theirs = dict(out=out, gx=x.grad, ggamma=w.grad, gbeta=b.grad)
    for k, bound in (("out", r.b_out), ("gx", r.b_gx), ("ggamma", r.b_ggamma),
                     ("gbeta", r.b_gbeta)):
        ratio = LE.error_ratio(_np(ours[k]), _np(theirs[k]).astype(np.float64), 2 * bound)
        margin.worst = max(margin.worst, ratio)
        assert ratio <= 1.0, (k, ratio)


@pytest.mark.parametrize("p", LE.PS)
@pytest.mark.parametrize("case", [(R, D) for D in (3, 100, 172) for R in (5, 257)],
                         ids=LE.case_id)
def test_bfloat16_contract(case, p, margin):
    """With xb = x.bfloat16(): op(xb) equals op(xb.float()) bit for bit in out and the parameter
    gradients, grad_x is the float32 run's rounded once, and a bfloat16 grad_out is the run on
    its widened copy.  The float32 run on the widened rows is within the reference's bounds."""
    import torch
    c = dict(LE.make_inputs(case))
    xb = torch.from_numpy(c["x"]).cuda().bfloat16()
    c["x"] = xb.float().cpu().numpy()
    wide = run(c, p)
    margin.check("widened", LE.reference(c, p=p), **{k: _np(v) for k, v in wide.items()})
    got = run(c, p, x=xb.clone().requires_grad_(True))
    assert got["gx"].dtype == torch.bfloat16
    for k in ("out", "ggamma", "gbeta"):
        assert bits_equal(got[k], wide[k]), k
    assert bits_equal(got["gx"], wide["gx"].to(torch.bfloat16))
    assert np.array_equal(_np(got["gx"]), LE.round_bf16(_np(wide["gx"])))
    gb = _dev(c["gout"]).bfloat16()
    low = run(c, p, x=xb.clone().requires_grad_(True), gout=gb)
    ref = run(c, p, x=xb.clone().requires_grad_(True), gout=gb.float())
    assert all_bits_equal(low, ref)
    # misaligned bfloat16 rows (8-byte loads need D % 4 == 0 and an 8-byte boundary)
    flat = torch.zeros(xb.numel() + 1, device="cuda", dtype=torch.bfloat16)
    flat[1:] = xb.reshape(-1)
    odd = flat[1:].view(*xb.shape).requires_grad_(True)
    assert odd.data_ptr() % 8 == 2
    assert all_bits_equal(got, run(c, p, x=odd))
