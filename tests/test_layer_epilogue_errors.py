"""Error paths of ops.dropout_relu_layer_norm and of the gf_layer_epilogue* entry points that need
no device: the op refuses bad dtypes, shapes, widths, probabilities and CPU tensors before the
native library is touched, and the C entry points refuse bad arguments before any pointer is
looked at or anything is launched."""
import ctypes as C
import math

import pytest
import torch

from gnnflow_amd import _capi, ops

BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
PTR = 4096      # never dereferenced: every call below fails (or has nothing to do) before a launch


def _op(x=F32, w=F32, b=F32, R=4, D=6, wd=None, bd=None, **kw):
    return ops.dropout_relu_layer_norm(
        torch.zeros(R, D, dtype=x), torch.ones(D if wd is None else wd, dtype=w),
        torch.zeros(D if bd is None else bd, dtype=b), **kw)


@pytest.fixture
def no_native_call(monkeypatch):
    def load():
        raise AssertionError("the native library was touched")
    monkeypatch.setattr(_capi, "load", load)


def test_refuses_other_dtypes(no_native_call):
    for x in (F16, torch.float64):
        with pytest.raises(TypeError, match="float16|float64"):
            _op(x=x)
    for kw in (dict(w=BF16), dict(b=BF16), dict(w=F16)):
        with pytest.raises(TypeError, match="float32"):
            _op(x=BF16, **kw)
    with pytest.raises(TypeError, match="tensor"):
        ops.dropout_relu_layer_norm([[1.0]], torch.ones(1), torch.zeros(1))


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_valid_dtypes_get_as_far_as_the_device_check(no_native_call, dtype):
    with pytest.raises(ValueError, match="runs on the GPU"):
        _op(x=dtype)
    with pytest.raises(ValueError, match="runs on the GPU"):
        _op(x=dtype, dropout_p=0.5, dropout_seed=2 ** 64 - 1)


def test_shapes_and_widths(no_native_call):
    with pytest.raises(ValueError, match=r"\[R, D\]"):
        ops.dropout_relu_layer_norm(torch.zeros(6), torch.ones(6), torch.zeros(6))
    with pytest.raises(ValueError, match=r"\[R, D\]"):
        ops.dropout_relu_layer_norm(torch.zeros(2, 3, 6), torch.ones(6), torch.zeros(6))
    with pytest.raises(ValueError, match="weight"):
        _op(wd=5)
    with pytest.raises(ValueError, match="bias"):
        _op(bd=7)
    with pytest.raises(ValueError, match="D >= 1"):
        _op(D=0)
    assert ops.LAYER_EPILOGUE_MAX_WIDTH == 1024
    with pytest.raises(ValueError, match="LAYER_EPILOGUE_MAX_WIDTH"):
        _op(D=1025)


@pytest.mark.parametrize("p", [1.0, -0.1, 1.5, math.nan, 1.0 - 2.0 ** -30])
def test_dropout_p_outside_the_unit_interval(no_native_call, p):
    with pytest.raises(ValueError, match="dropout_p"):
        _op(dropout_p=p, dropout_seed=1)


def test_seed_and_eps(no_native_call):
    for seed in (-1, 2 ** 64):
        with pytest.raises(ValueError, match="dropout_seed"):
            _op(dropout_p=0.5, dropout_seed=seed)
    for eps in (0.0, -1e-5, math.nan, 1e-60):
        with pytest.raises(ValueError, match="eps"):
            _op(eps=eps)


# ---- the C entry points ----------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    return _capi.load()


def _fwd(lib, bf16=False, x=PTR, gamma=PTR, beta=PTR, R=4, D=8, eps=1e-5, p=0.0, out=PTR,
         mean=PTR, rstd=PTR):
    fn = lib.gf_layer_epilogue_bf16 if bf16 else lib.gf_layer_epilogue
    return fn(x, gamma, beta, R, D, eps, p, 7, out, mean, rstd, 0, None)


def _bwd(lib, bf16=False, x=PTR, gamma=PTR, mean=PTR, rstd=PTR, R=4, D=8, p=0.0, go=PTR,
         partials=PTR, rows=1024, gx=PTR, gg=PTR, gb=PTR):
    fn = lib.gf_layer_epilogue_backward_bf16 if bf16 else lib.gf_layer_epilogue_backward
    return fn(x, gamma, mean, rstd, R, D, p, 7, go, partials, rows, gx, gg, gb, 0, None)


@pytest.mark.parametrize("bf16", [False, True])
def test_c_scalar_checks(lib, bf16):
    bad = _capi.GF_ERR_INVALID_ARGUMENT
    for call in (_fwd, _bwd):
        for D, word in ((0, b"dim must be >= 1"), (1025, b"GF_LAYER_EPILOGUE_MAX_WIDTH")):
            assert call(lib, bf16, D=D) == bad
            assert word in lib.gf_last_error() and b"layer_epilogue" in lib.gf_last_error()
        for p in (1.0, -0.1, math.nan):
            assert call(lib, bf16, p=p) == bad, p
            assert b"dropout" in lib.gf_last_error()
        # ... before any pointer is looked at, and also when there are no rows
        assert call(lib, bf16, D=1025, R=0, x=None) == bad
        assert call(lib, bf16, p=1.0, R=0, x=None) == bad
    for eps in (0.0, -1.0, math.nan):
        assert _fwd(lib, bf16, eps=eps) == bad, eps
        assert b"eps" in lib.gf_last_error()


@pytest.mark.parametrize("bf16", [False, True])
def test_c_null_pointers(lib, bf16):
    bad = _capi.GF_ERR_INVALID_ARGUMENT
    for name in ("x", "gamma", "beta", "out", "mean", "rstd"):
        assert _fwd(lib, bf16, **{name: None}) == bad, name
        assert b"null" in lib.gf_last_error()
    for name in ("x", "gamma", "mean", "rstd", "go"):
        assert _bwd(lib, bf16, **{name: None}) == bad, name
        assert b"null" in lib.gf_last_error()


@pytest.mark.parametrize("bf16", [False, True])
def test_c_partials_buffer(lib, bf16):
    bad = _capi.GF_ERR_INVALID_ARGUMENT
    rows = C.c_size_t(0)
    _capi.check(lib.gf_layer_epilogue_backward_partial_rows(100, C.byref(rows)))
    assert rows.value > 1
    for kw in (dict(rows=rows.value - 1), dict(partials=None), dict(rows=rows.value - 1, gg=None),
               dict(rows=0, gb=None)):
        assert _bwd(lib, bf16, R=100, **kw) == bad, kw
        assert b"gf_layer_epilogue_backward_partial_rows" in lib.gf_last_error()


@pytest.mark.parametrize("bf16", [False, True])
def test_c_nothing_to_do_is_a_success_without_a_launch(lib, bf16):
    """No rows (the pointers may be NULL), and a backward that is asked for no gradient."""
    assert _fwd(lib, bf16, R=0, x=None, gamma=None, beta=None, out=None, mean=None,
                rstd=None) == _capi.GF_OK
    assert _bwd(lib, bf16, R=0, x=None, gamma=None, mean=None, rstd=None, go=None, partials=None,
                rows=0, gx=None, gg=None, gb=None) == _capi.GF_OK
    assert _bwd(lib, bf16, partials=None, rows=0, gx=None, gg=None, gb=None) == _capi.GF_OK


def test_partial_rows_entry(lib):
    rows, got = C.c_size_t(99), []
    for R in (0, 1, 1024, 1025, 10 ** 6):
        assert lib.gf_layer_epilogue_backward_partial_rows(R, C.byref(rows)) == _capi.GF_OK
        got.append(rows.value)
    assert got[0] == 0 and got[1] == 1 and got[-1] == 1024
    assert all(r <= 1024 for r in got) and got == sorted(got)
    assert lib.gf_layer_epilogue_backward_partial_rows(5, None) == _capi.GF_ERR_INVALID_ARGUMENT
    assert b"null output" in lib.gf_last_error()
