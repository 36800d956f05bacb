"""What ops.link_loss and gf_link_loss refuse, without a GPU: every call below fails an argument
check, and the checks all come before anything touches the device or the native library.  Also
nn.LinkLoss on CPU tensors, which takes the torch expression."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F


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
        self.out = (C.c_float * 1)()
        self.grad_out = (C.c_float * 1)()
        self.grad_pos = (C.c_float * 4)()
        self.grad_neg = (C.c_float * 4)()

    def _args(self, names, null):
        return {k: None if k in null else C.cast(getattr(self, k), C.c_void_p) for k in names}

    def forward(self, lib, bf16=False, P=2, N=2, rows=16, **null):
        a = self._args(("pos", "neg", "partials", "out"), null)
        fn = lib.gf_link_loss_bf16 if bf16 else lib.gf_link_loss
        return fn(a["pos"], a["neg"], P, N, a["partials"], rows, a["out"], None, 0, None)

    def backward(self, lib, bf16=False, P=2, N=2, **null):
        a = self._args(("pos", "neg", "grad_out", "grad_pos", "grad_neg"), null)
        fn = lib.gf_link_loss_backward_bf16 if bf16 else lib.gf_link_loss_backward
        return fn(a["pos"], a["neg"], P, N, a["grad_out"], a["grad_pos"], a["grad_neg"], 0, None)


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("null", ["pos", "neg", "out"])
def test_c_forward_rejects_null_pointers(lib, bf16, null):
    from gnnflow_amd import _capi
    assert _Buffers().forward(lib, bf16, **{null: True}) == _capi.GF_ERR_INVALID_ARGUMENT
    msg = lib.gf_last_error()
    assert b"link_loss" in msg and b"null" in msg


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("null", ["pos", "neg", "grad_out"])
def test_c_backward_rejects_null_pointers(lib, bf16, null):
    from gnnflow_amd import _capi
    assert _Buffers().backward(lib, bf16, **{null: True}) == _capi.GF_ERR_INVALID_ARGUMENT
    msg = lib.gf_last_error()
    assert b"link_loss backward" in msg and b"null" in msg


@pytest.mark.parametrize("bf16", [False, True])
def test_c_backward_without_a_gradient_to_write_is_a_success_without_a_launch(lib, bf16):
    from gnnflow_amd import _capi
    assert _Buffers().backward(lib, bf16, grad_pos=True, grad_neg=True) == _capi.GF_OK


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("P,N,word", [
    (0, 2, b"at least one"), (2, 0, b"at least one"), (0, 0, b"at least one"),
    (2 ** 31, 1, b"more than 2^31 - 1"), (1, 2 ** 31, b"more than 2^31 - 1"),
    (2 ** 64 - 1, 2, b"more than 2^31 - 1"),
])
def test_c_entries_reject_empty_and_oversized_sides(lib, bf16, P, N, word):
    from gnnflow_amd import _capi
    b = _Buffers()
    rows = C.c_size_t(0)
    for rc in (b.forward(lib, bf16, P=P, N=N), b.backward(lib, bf16, P=P, N=N),
               lib.gf_link_loss_partial_rows(P, N, C.byref(rows))):
        assert rc == _capi.GF_ERR_INVALID_ARGUMENT
        assert word in lib.gf_last_error()


@pytest.mark.parametrize("bf16", [False, True])
def test_c_forward_rejects_a_missing_or_short_partials_buffer(lib, bf16):
    from gnnflow_amd import _capi, ops
    T = ops.LINK_LOSS_TILE
    P = N = (ops.LINK_LOSS_SINGLE_TILES // 2) * T + 1      # one tile past the one-launch sizes
    rows = C.c_size_t(0)
    assert lib.gf_link_loss_partial_rows(P, N, C.byref(rows)) == _capi.GF_OK
    assert rows.value == ops.LINK_LOSS_SINGLE_TILES + 2
    for kw in (dict(rows=rows.value - 1), dict(rows=rows.value, partials=True)):
        assert _Buffers().forward(lib, bf16, P=P, N=N, **kw) == _capi.GF_ERR_INVALID_ARGUMENT
        assert b"gf_link_loss_partial_rows" in lib.gf_last_error()


def test_partial_rows_entry(lib):
    from gnnflow_amd import _capi, ops
    T, S, M = ops.LINK_LOSS_TILE, ops.LINK_LOSS_SINGLE_TILES, ops.LINK_LOSS_MAX_PARTIAL_ROWS
    rows = C.c_size_t(99)
    for P, N, want in ((1, 1, 0), (600, 5400, 0), (T, (S - 1) * T, 0), (T + 1, (S - 1) * T, S + 1),
                       (1, S * T, S + 1), (3 * T + 1, 3 * T + 1, 0), (4 * T + 1, 4 * T + 1, 10),
                       (T * (M // 2) + 1, 5, M // 2 + 1), (2 ** 31 - 1, 2 ** 31 - 1, M)):
        assert lib.gf_link_loss_partial_rows(P, N, C.byref(rows)) == _capi.GF_OK
        assert rows.value == want, (P, N)
    assert lib.gf_link_loss_partial_rows(5, 5, None) == _capi.GF_ERR_INVALID_ARGUMENT
    assert b"null output" in lib.gf_last_error()


# ---- the Python layer, with CPU tensors -------------------------------------------------------
def test_python_rejects_wrong_types_and_dtypes():
    from gnnflow_amd import ops
    pos, neg = torch.zeros(4), torch.ones(8)
    with pytest.raises(TypeError, match="pos must be a tensor"):
        ops.link_loss([0.1, 0.2], neg)
    with pytest.raises(TypeError, match="neg must be a tensor"):
        ops.link_loss(pos, neg.numpy())
    for a, b in ((pos.double(), neg.double()), (pos.half(), neg.half()), (pos, neg.bfloat16()),
                 (pos.bfloat16(), neg), (pos, neg.double()), (pos.long(), neg.long())):
        with pytest.raises(TypeError, match="both float32 or both bfloat16"):
            ops.link_loss(a, b)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_python_rejects_wrong_shapes_and_devices(dtype):
    from gnnflow_amd import ops
    pos, neg = torch.zeros(4, dtype=dtype), torch.ones(8, dtype=dtype)
    with pytest.raises(ValueError, match=r"pos must be \[n\] or \[n, 1\]"):
        ops.link_loss(pos.reshape(2, 2), neg)
    with pytest.raises(ValueError, match=r"neg must be \[n\] or \[n, 1\]"):
        ops.link_loss(pos, neg.reshape(1, 8))
    with pytest.raises(ValueError, match=r"pos must be \[n\] or \[n, 1\]"):
        ops.link_loss(torch.zeros((), dtype=dtype), neg)
    with pytest.raises(ValueError, match="at least one"):
        ops.link_loss(pos[:0], neg)
    with pytest.raises(ValueError, match="at least one"):
        ops.link_loss(pos, neg[:0].reshape(0, 1))
    with pytest.raises(ValueError, match="neg is on"):
        ops.link_loss(pos, neg.to("meta"))
    with pytest.raises(ValueError, match="runs on the GPU"):
        ops.link_loss(pos, neg)
    with pytest.raises(ValueError, match="runs on the GPU"):
        ops.link_loss(pos.reshape(4, 1), neg.reshape(8, 1))


def test_python_rejects_a_wrong_accumulator():
    from gnnflow_amd import ops
    pos, neg = torch.zeros(4), torch.ones(8)
    F5 = ops.LINK_LOSS_ACC_FIELDS
    assert F5 == 5
    with pytest.raises(TypeError, match="accumulator must be a tensor"):
        ops.link_loss(pos, neg, accumulator=[0.0] * F5)
    with pytest.raises(TypeError, match="accumulator must be float64"):
        ops.link_loss(pos, neg, accumulator=torch.zeros(F5))
    for bad in (torch.zeros(4, dtype=torch.float64), torch.zeros(8, dtype=torch.float64),
                torch.zeros(1, F5, dtype=torch.float64),
                torch.zeros(2 * F5, dtype=torch.float64)[::2]):
        with pytest.raises(ValueError, match=r"accumulator must be a contiguous \[5\]"):
            ops.link_loss(pos, neg, accumulator=bad)
    with pytest.raises(ValueError, match="accumulator is on"):
        ops.link_loss(pos, neg, accumulator=torch.zeros(F5, dtype=torch.float64, device="meta"))
    # a good accumulator: the device check of the logits is what is left
    acc = torch.zeros(F5, dtype=torch.float64)
    with pytest.raises(ValueError, match="runs on the GPU"):
        ops.link_loss(pos, neg, accumulator=acc)
    assert not acc.any()


def test_module_takes_the_torch_expression_on_the_cpu():
    import gnnflow_amd
    from gnnflow_amd import metrics, nn
    assert gnnflow_amd.LinkLoss is nn.LinkLoss and metrics.LinkLoss is nn.LinkLoss
    g = torch.Generator().manual_seed(3)
    pos = (3 * torch.randn(33, 1, generator=g)).requires_grad_()
    neg = (3 * torch.randn(99, 1, generator=g)).requires_grad_()
    crit = nn.LinkLoss()
    loss = crit(pos, neg)
    want = F.binary_cross_entropy_with_logits(pos, torch.ones_like(pos)) + \
        F.binary_cross_entropy_with_logits(neg, torch.zeros_like(neg))
    assert loss.dtype == torch.float32 and loss.shape == () and torch.equal(loss, want)
    gp, gn = torch.autograd.grad(loss, (pos, neg))
    wp, wn = torch.autograd.grad(want, (pos, neg))
    assert torch.equal(gp, wp) and torch.equal(gn, wn)
    # not accumulated, and nothing in the state
    assert crit.state is None and crit.state_dict() == {}
    out = crit.compute()
    assert out["batches"] == 0 and out["nonfinite"] == 0 and out["mean_loss"] != out["mean_loss"]
    crit.reset()
    assert torch.equal(crit(pos.double(), neg.double()),
                       F.binary_cross_entropy_with_logits(pos.double(), torch.ones_like(pos).double()) +
                       F.binary_cross_entropy_with_logits(neg.double(), torch.zeros_like(neg).double()))
