"""What ops.link_metrics and gf_link_metrics refuse.  The C-level checks need no GPU: every call
below fails an argument check, and the checks all come before anything touches the device.  The
Python-level checks run on the GPU, where the tensors live."""
import ctypes as C

import pytest


@pytest.fixture(scope="module")
def lib():
    from gnnflow_amd import _build, _capi
    _build.build()
    return _capi.load()


class _Buffers:
    """Host memory standing in for the device buffers: a refused call never reads them."""

    def __init__(self):
        self.pos = (C.c_float * 4)()
        self.neg = (C.c_float * 4)()
        self.partials = (C.c_double * 16)()
        self.out = (C.c_double * 3)()

    def call(self, lib, P=2, N=2, rows=1, **null):
        arg = {k: None if k in null else C.cast(getattr(self, k), C.c_void_p)
               for k in ("pos", "neg", "partials", "out")}
        return lib.gf_link_metrics(arg["pos"], arg["neg"], P, N, arg["partials"], rows, arg["out"],
                                   None, 0, None)


@pytest.mark.parametrize("null", ["pos", "neg", "out", "partials"])
def test_c_entry_rejects_null_pointers(lib, null):
    from gnnflow_amd import _capi
    assert _Buffers().call(lib, **{null: True}) == _capi.GF_ERR_INVALID_ARGUMENT
    msg = lib.gf_last_error()
    assert b"link_metrics" in msg and (b"null" in msg or b"partials" in msg)


@pytest.mark.parametrize("P,N,word", [
    (0, 2, b"at least one"), (2, 0, b"at least one"), (0, 0, b"at least one"),
    (65536, 1, b"more than 65536"), (1, 65536, b"more than 65536"),
    (32768, 32769, b"more than 65536"), (2 ** 40, 2 ** 40, b"more than 65536"),
    (2 ** 64 - 1, 2, b"more than 65536"),
])
def test_c_entry_rejects_empty_sides_and_too_many_scores(lib, P, N, word):
    from gnnflow_amd import _capi
    assert _Buffers().call(lib, P=P, N=N, rows=256) == _capi.GF_ERR_INVALID_ARGUMENT
    assert word in lib.gf_last_error()


def test_c_entry_rejects_a_short_partials_buffer(lib):
    from gnnflow_amd import _capi
    rows = C.c_size_t(0)
    assert lib.gf_link_metrics_partial_rows(257, C.byref(rows)) == _capi.GF_OK
    assert rows.value == 2
    assert _Buffers().call(lib, P=257, N=2, rows=1) == _capi.GF_ERR_INVALID_ARGUMENT
    assert b"gf_link_metrics_partial_rows" in lib.gf_last_error()


def test_partial_rows_entry(lib):
    from gnnflow_amd import _capi
    rows = C.c_size_t(99)
    for P, want in ((1, 1), (256, 1), (257, 2), (65535, 256), (65536, 256)):
        assert lib.gf_link_metrics_partial_rows(P, C.byref(rows)) == _capi.GF_OK
        assert rows.value == want
    assert lib.gf_link_metrics_partial_rows(5, None) == _capi.GF_ERR_INVALID_ARGUMENT
    assert b"null output" in lib.gf_last_error()
    assert lib.gf_link_metrics_partial_rows(65537, C.byref(rows)) == _capi.GF_ERR_INVALID_ARGUMENT
    assert b"more than 65536" in lib.gf_last_error()


# ---- the Python layer, on the GPU -------------------------------------------------------------
@pytest.fixture
def good():
    import torch
    return torch.zeros(4, device="cuda"), torch.ones(8, device="cuda")


@pytest.mark.gpu
def test_python_rejects_wrong_types_and_dtypes(good):
    import torch
    from gnnflow_amd import ops
    pos, neg = good
    with pytest.raises(TypeError, match="pos must be a tensor"):
        ops.link_metrics([0.1, 0.2], neg)
    with pytest.raises(TypeError, match="neg must be a tensor"):
        ops.link_metrics(pos, neg.cpu().numpy())
    with pytest.raises(TypeError, match="float32"):
        ops.link_metrics(pos.double(), neg)
    with pytest.raises(TypeError, match="float32"):
        ops.link_metrics(pos, neg.half())
    with pytest.raises(TypeError, match="accumulator must be a tensor"):
        ops.link_metrics(pos, neg, accumulator=[0.0] * 8)
    with pytest.raises(TypeError, match="accumulator must be float64"):
        ops.link_metrics(pos, neg, accumulator=torch.zeros(8, device="cuda"))


@pytest.mark.gpu
def test_python_rejects_wrong_shapes_devices_and_sizes(good):
    import torch
    from gnnflow_amd import ops
    pos, neg = good
    f64 = dict(dtype=torch.float64, device="cuda")
    with pytest.raises(ValueError, match=r"pos must be \[n\] or \[n, 1\]"):
        ops.link_metrics(pos.reshape(2, 2), neg)
    with pytest.raises(ValueError, match=r"neg must be \[n\] or \[n, 1\]"):
        ops.link_metrics(pos, neg.reshape(1, 8))
    with pytest.raises(ValueError, match=r"pos must be \[n\] or \[n, 1\]"):
        ops.link_metrics(torch.zeros((), device="cuda"), neg)
    with pytest.raises(ValueError, match="at least one positive and one negative"):
        ops.link_metrics(pos[:0], neg)
    with pytest.raises(ValueError, match="at least one positive and one negative"):
        ops.link_metrics(pos, neg[:0].reshape(0, 1))
    with pytest.raises(ValueError, match="at most 65536 scores"):
        ops.link_metrics(torch.zeros(32768, device="cuda"), torch.zeros(32769, device="cuda"))
    with pytest.raises(ValueError, match="runs on the GPU"):
        ops.link_metrics(pos.cpu(), neg.cpu())
    with pytest.raises(ValueError, match="neg is on cpu"):
        ops.link_metrics(pos, neg.cpu())
    with pytest.raises(ValueError, match=r"contiguous \[8\]"):
        ops.link_metrics(pos, neg, accumulator=torch.zeros(6, **f64))
    with pytest.raises(ValueError, match=r"contiguous \[8\]"):
        ops.link_metrics(pos, neg, accumulator=torch.zeros(16, **f64)[::2])
    with pytest.raises(ValueError, match="accumulator is on cpu"):
        ops.link_metrics(pos, neg, accumulator=torch.zeros(8, dtype=torch.float64))
    with pytest.raises(ValueError, match="accumulates on the GPU"):
        import gnnflow_amd
        gnnflow_amd.LinkMetrics("cpu")
    # and the limit itself is accepted
    out = ops.link_metrics(torch.zeros(32768, device="cuda"), torch.zeros(32768, device="cuda"))
    ap, auc, mrr = out.tolist()
    assert ap == 0.5 and auc == 0.5 and abs(mrr - 1 / 1.5) <= (32768 + 2) * 2.0 ** -53
