"""Error paths of ops.gru_cell and of the gf_gru_cell* entry points that need no device: the op
refuses bad types, dtypes, shapes, row counts and CPU tensors before the native library is
touched, the C entry points refuse bad arguments before any pointer is looked at or anything is
launched, and GRUMemoryUpdater carries the `fused_gru` switch, off by default."""
import pytest
import torch

from gnnflow_amd import _capi, nn as gnn, ops

BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
PTR = 4096      # never dereferenced: every call below fails (or has nothing to do) before a launch


def _op(gi=F32, gh=F32, hx=F32, res=None, N=4, H=6, gi_shape=None, gh_shape=None, res_shape=None,
        **kw):
    residual = None if res is None else torch.zeros(res_shape or (N, H), dtype=res)
    return ops.gru_cell(torch.zeros(gi_shape or (N, 3 * H), dtype=gi),
                        torch.zeros(gh_shape or (N, 3 * H), dtype=gh),
                        torch.zeros(N, H, dtype=hx), residual, **kw)


@pytest.fixture
def no_native_call(monkeypatch):
    def load():
        raise AssertionError("the native library was touched")
    monkeypatch.setattr(_capi, "load", load)


def test_refuses_what_is_no_tensor(no_native_call):
    z = torch.zeros(2, 3)
    with pytest.raises(TypeError, match="gi must be a tensor"):
        ops.gru_cell([[0.0] * 3], z, torch.zeros(2, 1))
    with pytest.raises(TypeError, match="gh must be a tensor"):
        ops.gru_cell(z, None, torch.zeros(2, 1))
    with pytest.raises(TypeError, match="hx must be a tensor"):
        ops.gru_cell(z, z, 0.0)
    with pytest.raises(TypeError, match="residual must be a tensor or None"):
        ops.gru_cell(z, z, torch.zeros(2, 1), residual=1.0)
    for bad in (1.0, True, None):
        with pytest.raises(TypeError, match="num_last must be an int"):
            ops.gru_cell(z, z, torch.zeros(2, 1), num_last=bad)


def test_refuses_other_dtypes(no_native_call):
    for kw in (dict(gi=F16, gh=F16), dict(gi=torch.float64, gh=torch.float64)):
        with pytest.raises(TypeError, match="float16|float64"):
            _op(**kw)
    for kw in (dict(gi=BF16), dict(gh=BF16)):      # mixed gates
        with pytest.raises(TypeError, match="both float32 or both bfloat16"):
            _op(**kw)
    for hx in (BF16, F16, torch.float64):
        with pytest.raises(TypeError, match="hx is"):
            _op(gi=BF16, gh=BF16, hx=hx)
    for res in (F16, torch.float64, torch.int32):
        with pytest.raises(TypeError, match="residual is"):
            _op(res=res)


@pytest.mark.parametrize("gates", [F32, BF16])
@pytest.mark.parametrize("res", [None, F32, BF16])
def test_valid_dtypes_get_as_far_as_the_device_check(no_native_call, gates, res):
    with pytest.raises(ValueError, match="runs on the GPU"):
        _op(gi=gates, gh=gates, res=res, num_last=4)


def test_shapes_and_row_counts(no_native_call):
    with pytest.raises(ValueError, match=r"hx must be \[N, H\]"):
        ops.gru_cell(torch.zeros(4, 18), torch.zeros(4, 18), torch.zeros(24))
    with pytest.raises(ValueError, match=r"hx must be \[N, H\]"):
        ops.gru_cell(torch.zeros(4, 18), torch.zeros(4, 18), torch.zeros(2, 2, 6))
    with pytest.raises(ValueError, match="H >= 1"):
        _op(H=0)
    for shape in ((4, 17), (4, 6), (3, 18), (72,), (4, 3, 6)):
        with pytest.raises(ValueError, match=r"gi must be \[N, 3H\]"):
            _op(gi_shape=shape)
        with pytest.raises(ValueError, match=r"gh must be \[N, 3H\]"):
            _op(gh_shape=shape)
    for shape in ((4, 5), (3, 6), (4, 18), (24,)):
        with pytest.raises(ValueError, match=r"residual must be \[N, H\]"):
            _op(res=F32, res_shape=shape)
    for bad in (-1, 5):
        with pytest.raises(ValueError, match="num_last"):
            _op(num_last=bad)
    with pytest.raises(ValueError, match="num_last"):
        _op(N=0, num_last=1)


def test_one_device(no_native_call):
    meta = torch.zeros(4, 18, device="meta")
    with pytest.raises(ValueError, match="gi is on"):
        ops.gru_cell(meta, torch.zeros(4, 18), torch.zeros(4, 6))
    with pytest.raises(ValueError, match="gh is on"):
        ops.gru_cell(torch.zeros(4, 18), meta, torch.zeros(4, 6))
    with pytest.raises(ValueError, match="residual is on"):
        ops.gru_cell(torch.zeros(4, 18), torch.zeros(4, 18), torch.zeros(4, 6),
                     residual=torch.zeros(4, 6, device="meta"))


def test_memory_updater_carries_the_switch():
    assert gnn.FUSED_GRU_DEFAULT is False
    m = gnn.GRUMemoryUpdater(dim_node=0, dim_edge=3, dim_time=4, dim_embed=5, dim_memory=5)
    assert m.fused_gru is False
    assert isinstance(m.updater, torch.nn.GRUCell)
    assert not any("fused" in k for k in m.state_dict())
    m.fused_gru = True      # an attribute, not a parameter or a buffer
    assert not any("fused" in k for k in m.state_dict())


# ---- the C entry points ----------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    return _capi.load()


def _fwd(lib, bf16=False, gi=PTR, gh=PTR, hx=PTR, res=PTR, res_bf16=0, N=4, H=8, R=2, out=PTR,
         last=PTR):
    fn = lib.gf_gru_cell_bf16 if bf16 else lib.gf_gru_cell
    return fn(gi, gh, hx, res, res_bf16, N, H, R, out, last, 0, None)


def _bwd(lib, bf16=False, gi=PTR, gh=PTR, hx=PTR, N=4, H=8, go=PTR, dgi=PTR, dgh=PTR, dhx=PTR):
    fn = lib.gf_gru_cell_backward_bf16 if bf16 else lib.gf_gru_cell_backward
    return fn(gi, gh, hx, N, H, go, dgi, dgh, dhx, 0, None)


@pytest.mark.parametrize("bf16", [False, True])
def test_c_scalar_checks(lib, bf16):
    bad = _capi.GF_ERR_INVALID_ARGUMENT
    for call in (_fwd, _bwd):
        assert call(lib, bf16, H=0) == bad
        assert b"hidden must be >= 1" in lib.gf_last_error() and b"gru_cell" in lib.gf_last_error()
        assert call(lib, bf16, H=1 << 30) == bad
        assert call(lib, bf16, N=1 << 31) == bad
        assert b"rows" in lib.gf_last_error()
        assert call(lib, bf16, N=1 << 30, H=1 << 8) == bad
        assert b"elements" in lib.gf_last_error()
        assert call(lib, bf16, H=0, N=0, gi=None) == bad      # also when there are no rows
    assert _fwd(lib, bf16, R=5) == bad
    assert b"num_last" in lib.gf_last_error()
    assert _fwd(lib, bf16, N=0, R=1) == bad
    for flag in (2, -1):
        assert _fwd(lib, bf16, res_bf16=flag) == bad
        assert b"residual_bf16" in lib.gf_last_error()


@pytest.mark.parametrize("bf16", [False, True])
def test_c_null_pointers(lib, bf16):
    bad = _capi.GF_ERR_INVALID_ARGUMENT
    for name in ("gi", "gh", "hx", "out", "last"):
        assert _fwd(lib, bf16, **{name: None}) == bad, name
        assert b"null" in lib.gf_last_error()
    for name in ("gi", "gh", "hx", "go"):
        assert _bwd(lib, bf16, **{name: None}) == bad, name
        assert b"null" in lib.gf_last_error()


@pytest.mark.parametrize("bf16", [False, True])
def test_c_nothing_to_do_is_a_success_without_a_launch(lib, bf16):
    """No rows (the pointers may be NULL), and a backward that is asked for no gradient."""
    assert _fwd(lib, bf16, N=0, R=0, gi=None, gh=None, hx=None, res=None, out=None,
                last=None) == _capi.GF_OK
    assert _bwd(lib, bf16, N=0, gi=None, gh=None, hx=None, go=None, dgi=None, dgh=None,
                dhx=None) == _capi.GF_OK
    assert _bwd(lib, bf16, dgi=None, dgh=None, dhx=None) == _capi.GF_OK
