"""ops.gru_cell (csrc/gru_cell.hip) against the float64 reference of tests/gru_cell_ref.py.

Tolerance (gru_cell_ref.py): every tensor T of h_out, last, d_gi, d_gh, d_hx must satisfy
e_op <= 2 e_torch + 2^-23 max |T_64|, where T_torch is the same formula written with
torch.sigmoid / torch.tanh in float32 on the same device and differentiated by autograd.  Exact
facts are bit equalities: last == u[:R], h_out == u + residual as one float32 add, the residual's
gradient == g, two runs agree, and the paths (16-byte, scalar behind a misaligned pointer) agree.
Each test prints its largest e_op / bound (run with -s)."""
import itertools

import numpy as np
import pytest

from tests import gru_cell_ref as GR

pytestmark = pytest.mark.gpu

class _Margin:
    def __init__(self):
        self.worst = 0.0

    def check(self, what, got, torch_side, ref):
        for name, want in ref.tensors().items():
            r = GR.ratio(got[name], torch_side[name], want)
            self.worst = max(self.worst, r)
            assert r <= 1.0, "{} {}: e_op / bound = {:.3g} (e_op {:.3g}, e_torch {:.3g})".format(
                what, name, r, GR.max_error(got[name], want),
                GR.max_error(torch_side[name], want))


@pytest.fixture
def margin(request):
    m = _Margin()
    yield m
    print("\n[e_op/bound] {}: {:.3g}".format(request.node.name, m.worst))


def _np(t):
    import torch
    t = t.detach().cpu()
    return (t.float() if t.dtype == torch.bfloat16 else t).numpy()


def _dev(a, grad=False):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda().requires_grad_(grad)


_CACHE = {}


def _case(case, saturated=False, with_residual=True):
    """(inputs, float64 reference, the torch formula's tensors on the device) of a shared case:
    computed once, never modified."""
    key = (case, saturated, with_residual)
    if key not in _CACHE:
        c = GR.make_saturated(case) if saturated else GR.make_inputs(case)
        _CACHE[key] = (c, GR.reference(c, with_residual), torch_formula(c, with_residual))
    return _CACHE[key]


def torch_formula(c, with_residual=True):
    """The op's formula in float32 torch ops on the device, differentiated by autograd."""
    import torch
    H, R = c["hx"].shape[1], c["R"]
    gi, gh, hx = _dev(c["gi"], True), _dev(c["gh"], True), _dev(c["hx"], True)
    r = torch.sigmoid(gi[:, :H] + gh[:, :H])
    z = torch.sigmoid(gi[:, H:2 * H] + gh[:, H:2 * H])
    n = torch.tanh(gi[:, 2 * H:] + r * gh[:, 2 * H:])
    u = (1 - z) * n + z * hx
    out = u + _dev(c["residual"]) if with_residual else u
    out.backward(_dev(c["g"]))
    return dict(h_out=_np(out), last=_np(u[:R]), d_gi=_np(gi.grad), d_gh=_np(gh.grad),
                d_hx=_np(hx.grad))


def run(c, with_residual=True, need=(True, True, True, True), tensors=None):
    """Forward + backward of the op -> dict of numpy arrays (None: no gradient), and
    d_residual."""
    from gnnflow_amd import ops
    t = dict(tensors or {})
    for k, n in zip(("gi", "gh", "hx", "residual"), need):
        if k not in t:
            t[k] = _dev(c[k], n)
    residual = t["residual"] if with_residual else None
    out, last = ops.gru_cell(t["gi"], t["gh"], t["hx"], residual, num_last=c["R"])
    N, H = c["hx"].shape
    assert tuple(out.shape) == (N, H) and tuple(last.shape) == (c["R"], H)
    assert not last.requires_grad
    used = need if with_residual else need[:3]
    assert out.requires_grad == any(used)
    if out.requires_grad:
        out.backward(_dev(c["g"]))
    res = dict(h_out=_np(out), last=_np(last))
    for name, k in (("d_gi", "gi"), ("d_gh", "gh"), ("d_hx", "hx"), ("d_residual", "residual")):
        leaf = t[k]
        res[name] = None if (not leaf.is_leaf or leaf.grad is None) else _np(leaf.grad)
    return res


@pytest.mark.parametrize("with_residual", [False, True], ids=["plain", "residual"])
@pytest.mark.parametrize("case", GR.CASES, ids=GR.case_id)
def test_forward_and_backward(case, with_residual, margin):
    c, ref, tor = _case(case, with_residual=with_residual)
    got = run(c, with_residual)
    margin.check(GR.case_id(case), got, tor, ref)


@pytest.mark.parametrize("with_residual", [False, True], ids=["plain", "residual"])
@pytest.mark.parametrize("case", [(65, 100, 17), (64, 7, 64)], ids=GR.case_id)
def test_saturated_pre_activations(case, with_residual, margin):
    """Pre-activations of +-100, 0 and +-1e-4: no NaN or Inf anywhere, and the rule holds."""
    c, ref, tor = _case(case, saturated=True, with_residual=with_residual)
    got = run(c, with_residual)
    for k, v in got.items():
        assert v is None or np.isfinite(v).all(), k
    margin.check("saturated", got, tor, ref)


@pytest.mark.parametrize("case", GR.CASES, ids=GR.case_id)
def test_exact_facts(case):
    c, _, _ = _case(case)
    plain, res = run(c, False), run(c, True)
    R = c["R"]
    u = plain["h_out"]
    assert np.array_equal(plain["last"], u[:R]) and np.array_equal(res["last"], u[:R])
    want = u + c["residual"]
    assert want.dtype == np.float32 and np.array_equal(res["h_out"], want)
    assert np.array_equal(res["d_residual"], c["g"])
    assert plain["d_residual"] is None
    for k in ("d_gi", "d_gh", "d_hx"):      # the residual changes no other gradient
        assert np.array_equal(plain[k], res[k])
    again = run(c, True)
    for k in res:
        assert np.array_equal(res[k], again[k]), k


def test_bfloat16_residual_is_widened():
    import torch
    c, _, _ = _case((65, 100, 17))
    rb = _dev(c["residual"]).to(torch.bfloat16).requires_grad_(True)
    got = run(c, True, tensors=dict(residual=rb))
    want = run(c, False)["h_out"] + _np(rb.float())
    assert np.array_equal(got["h_out"], want)
    assert rb.grad.dtype == torch.bfloat16
    assert torch.equal(rb.grad, _dev(c["g"]).to(torch.bfloat16))


@pytest.mark.parametrize("case", [(5, 4, 5), (65, 100, 17), (257, 8, 64)], ids=GR.case_id)
def test_misaligned_base_pointers_take_the_scalar_path(case):
    """H % 4 == 0 behind addresses that do not allow 16-byte accesses: each of gi, gh, hx and
    residual in turn.  Every element is the same expression on either path: bit-equal."""
    import torch
    c, _, _ = _case(case)
    aligned = run(c)

    def shifted(a):
        flat = torch.zeros(a.size + 1, device="cuda")
        t = flat[1:].view(*a.shape)
        t.copy_(torch.from_numpy(a))
        assert t.is_contiguous() and t.data_ptr() % 16 == 4
        return t.requires_grad_(True)

    for which in ("gi", "gh", "hx", "residual"):
        got = run(c, tensors={which: shifted(c[which])})
        for k in aligned:
            assert np.array_equal(got[k], aligned[k]), (which, k)


def test_row_slice_and_non_contiguous_inputs(margin):
    """gi a column slice of a wider tensor (copied first) and hx = mem[:N] a row slice of a
    taller one (taken as it is): the gradients reach the tensors behind them."""
    import torch
    case = (65, 100, 17)
    c, ref, tor = _case(case)
    N, H, _ = case
    full = run(c)
    wide = torch.cat([torch.full((N, 2), 7.0), torch.from_numpy(c["gi"]),
                      torch.full((N, 1), 7.0)], 1).cuda().requires_grad_(True)
    mem = torch.cat([torch.from_numpy(c["hx"]), torch.full((9, H), 7.0)]).cuda() \
        .requires_grad_(True)
    gi, hx = wide[:, 2:2 + 3 * H], mem[:N]
    assert not gi.is_contiguous() and hx.is_contiguous() and hx.data_ptr() == mem.data_ptr()
    got = run(c, tensors=dict(gi=gi, hx=hx))
    gwide, gmem = _np(wide.grad), _np(mem.grad)
    assert not gwide[:, :2].any() and not gwide[:, 2 + 3 * H:].any() and not gmem[N:].any()
    got.update(d_gi=np.ascontiguousarray(gwide[:, 2:2 + 3 * H]), d_hx=gmem[:N])
    margin.check("slices", got, tor, ref)
    for k in full:
        assert np.array_equal(got[k], full[k]), k


@pytest.mark.parametrize("need", list(itertools.product([False, True], repeat=4)),
                         ids=lambda n: "".join("IHXR"[i] if x else "-" for i, x in enumerate(n)))
def test_every_requires_grad_subset(need):
    """An unrequested gradient is None; the requested ones are bit-equal to the full run."""
    c, _, _ = _case((65, 100, 17))
    got, full = run(c, need=need), run(c)
    assert np.array_equal(got["h_out"], full["h_out"])
    assert np.array_equal(got["last"], full["last"])
    for k, n in zip(("d_gi", "d_gh", "d_hx", "d_residual"), need):
        assert (got[k] is not None) == n, k
        assert got[k] is None or np.array_equal(got[k], full[k]), k


@pytest.mark.parametrize("with_residual", [False, True])
def test_no_rows(with_residual, monkeypatch):
    """N == 0: empty tensors, zero gradients, and no native call either way."""
    import torch
    from gnnflow_amd import _capi, ops
    H = 12
    gi = torch.ones((0, 3 * H), device="cuda", requires_grad=True)
    gh = torch.ones((0, 3 * H), device="cuda", requires_grad=True)
    hx = torch.ones((0, H), device="cuda", requires_grad=True)
    res = torch.ones((0, H), device="cuda", requires_grad=True) if with_residual else None

    def no_native(*a, **k):
        raise AssertionError("native library touched")
    monkeypatch.setattr(_capi, "load", no_native)
    out, last = ops.gru_cell(gi, gh, hx, res, num_last=0)
    assert tuple(out.shape) == (0, H) and tuple(last.shape) == (0, H)
    out.sum().backward()
    for t in (gi, gh, hx) + ((res,) if with_residual else ()):
        assert t.grad.shape == t.shape and not t.grad.any()


def test_c_entry_points():
    """The C entry points directly: d_hx alone, nothing else written; their error returns."""
    import ctypes as C
    import torch
    from gnnflow_amd import _capi
    case = (65, 100, 17)
    c, _, _ = _case(case)
    N, H, R = case
    lib = _capi.load()

    def p(x):
        return C.c_void_p(x.data_ptr())
    gi, gh, hx, g, res = (_dev(c[k]) for k in ("gi", "gh", "hx", "g", "residual"))
    out, last = torch.full((N, H), 7.0, device="cuda"), torch.full((R, H), 7.0, device="cuda")
    good = [p(gi), p(gh), p(hx), p(res), 0, N, H, R, p(out), p(last), 0, None]
    _capi.check(lib.gf_gru_cell(*good))
    full = run(c)
    assert np.array_equal(_np(out), full["h_out"]) and np.array_equal(_np(last), full["last"])
    for i, value in ((0, None), (1, None), (2, None), (8, None), (9, None), (6, 0), (7, N + 1),
                     (4, 2)):
        args = list(good)
        args[i] = value
        assert lib.gf_gru_cell(*args) == _capi.GF_ERR_INVALID_ARGUMENT, i
        assert (b"null" in lib.gf_last_error()) == (value is None)
    dgi = torch.full((N, 3 * H), 7.0, device="cuda")
    dgh, dhx = torch.full((N, 3 * H), 7.0, device="cuda"), torch.full((N, H), 7.0, device="cuda")
    _capi.check(lib.gf_gru_cell_backward(p(gi), p(gh), p(hx), N, H, p(g), None, None, p(dhx), 0,
                                         None))
    assert np.array_equal(_np(dhx), full["d_hx"])
    assert (_np(dgi) == 7.0).all() and (_np(dgh) == 7.0).all()
    good = [p(gi), p(gh), p(hx), N, H, p(g), p(dgi), p(dgh), p(dhx), 0, None]
    _capi.check(lib.gf_gru_cell_backward(*good))
    assert np.array_equal(_np(dgi), full["d_gi"]) and np.array_equal(_np(dgh), full["d_gh"])
    for i, value in ((0, None), (1, None), (2, None), (5, None), (4, 0)):
        args = list(good)
        args[i] = value
        assert lib.gf_gru_cell_backward(*args) == _capi.GF_ERR_INVALID_ARGUMENT, i
    for n in (0,):      # no rows: success without a launch, whatever the pointers
        _capi.check(lib.gf_gru_cell(None, None, None, None, 0, n, H, 0, None, None, 0, None))
        _capi.check(lib.gf_gru_cell_backward(None, None, None, n, H, None, None, None, None, 0,
                                             None))
    torch.cuda.synchronize()
