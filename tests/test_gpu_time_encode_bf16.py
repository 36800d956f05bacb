"""ops.time_encode_cat with out_dtype=torch.bfloat16 (the uint16_t kernels of csrc/time_encode.hip)
against the float32 op, bit for bit:

    forward    rows == float32 rows .to(torch.bfloat16)           (raw 16-bit patterns)
    backward   gw, gb == the float32 op's on grad.float()          (torch.equal)
               part gradients == the widened column slices of grad

The float32 op is checked against float64 in tests/test_gpu_time_encode.py; no tolerance here."""
import itertools

import numpy as np
import pytest

from tests import time_encode_ref as TE

pytestmark = pytest.mark.gpu

NS = (1, 3, 257)
WIDTHS = ((), (5,), (8,), (8, 3), (172, 100))
TS = (1, 4, 100)
CASES = [(n, T, w, "unit") for n, w, T in itertools.product(NS, WIDTHS, TS)]


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def same_bits(got, want):
    import torch
    assert got.dtype == torch.bfloat16 and want.dtype == torch.bfloat16
    assert got.shape == want.shape
    ng, nw = got.isnan(), want.isnan()
    return torch.equal(ng, nw) and \
        torch.equal(got.contiguous().view(torch.int16)[~ng], want.contiguous().view(torch.int16)[~nw])


def run(c, out_dtype, parts=None):
    """Forward + backward -> (out, gw, gb, part gradients); the gradient is gout rounded to
    bfloat16 on the bfloat16 side and that value widened on the float32 side."""
    import torch
    from gnnflow_amd import ops
    parts = [_dev(p).requires_grad_(True) for p in c["parts"]] if parts is None else parts
    w, bias = _dev(c["w"]).requires_grad_(True), _dev(c["bias"]).requires_grad_(True)
    out = ops.time_encode_cat(parts, _dev(c["t"]), w, bias, out_dtype=out_dtype)
    g = _dev(c["gout"]).to(torch.bfloat16)
    out.backward(g if out.dtype == torch.bfloat16 else g.float())
    return out.detach(), w.grad, bias.grad, [p.grad for p in parts], g


@pytest.mark.parametrize("case", CASES, ids=TE.case_id)
def test_forward_and_backward_equal_the_float32_op(case):
    """Odd and even row widths (odd-width bfloat16 rows start on 2-byte boundaries), the scalar
    and the 4-column path (every width and T a multiple of 4), T <= 32 and T > 32."""
    import torch
    c = TE.make_inputs(case)
    out, gw, gb, gparts, g = run(c, torch.bfloat16)
    out32, gw32, gb32, gparts32, _ = run(c, torch.float32)
    n, T, widths, _ = case
    assert out.dtype == torch.bfloat16 and out.shape == (n, sum(widths) + T)
    assert same_bits(out, out32.to(torch.bfloat16))
    assert gw.dtype == gb.dtype == torch.float32
    assert torch.equal(gw, gw32) and torch.equal(gb, gb32)
    off = 0
    for gp, gp32, width in zip(gparts, gparts32, widths):
        assert gp.dtype == torch.float32
        assert torch.equal(gp, g[:, off:off + width].float()) and torch.equal(gp, gp32)
        off += width
    # the same from run to run
    again = run(c, torch.bfloat16)
    assert same_bits(again[0], out) and torch.equal(again[1], gw) and torch.equal(again[2], gb)


def test_time_encode_without_parts_takes_the_keyword():
    import torch
    from gnnflow_amd import ops
    c = TE.make_inputs((257, 100, (), "large"))
    t, w, bias = (_dev(c[n]) for n in ("t", "w", "bias"))
    out = ops.time_encode(t, w, bias, out_dtype=torch.bfloat16)
    assert same_bits(out, ops.time_encode(t, w, bias).to(torch.bfloat16))


@pytest.mark.parametrize("widths,T", [((8, 4), 4), ((5, 3), 3)], ids=["vector", "scalar"])
def test_row_slice_parts(widths, T):
    """h[R:] of a wider allocation: a part whose first row is not the allocation's."""
    import torch
    R, n = 3, 65
    c = TE.make_inputs((n, T, widths, "unit"))
    rng = np.random.RandomState(5)
    hs = [_dev(rng.randn(R + n, width).astype(np.float32)) for width in widths]
    outs = []
    for dtype in (torch.bfloat16, torch.float32):
        parts = [h[R:].detach().requires_grad_(True) for h in hs]
        outs.append(run(c, dtype, parts))
    assert same_bits(outs[0][0], outs[1][0].to(torch.bfloat16))
    assert same_bits(outs[0][0][:, :widths[0]], hs[0][R:].to(torch.bfloat16))
    assert torch.equal(outs[0][1], outs[1][1]) and torch.equal(outs[0][2], outs[1][2])


def test_conversion_through_the_copied_columns():
    """Crafted float32 values through the pass-through columns, on the scalar path (5 columns)
    and on the 4-column path (8 columns): the output must be x.to(torch.bfloat16)."""
    import torch
    from gnnflow_amd import ops
    bits = np.array([
        0x3F808000,      # 1 + 2^-8: a tie, rounds down to the even 0x3F80
        0x3F818000,      # a tie, rounds up to the even 0x3F82
        0xBF808000, 0xBF818000,      # the same, negative
        0x3F808001,      # just above a tie: up
        0x3F817FFF,      # just below a tie: down
        0x7F7FFFFF,      # the largest finite float32: rounds to +inf
        0xFF7FFFFF,      # -> -inf
        0x7F7F0000,      # the largest bfloat16: stays
        0x7F7F7FFF,      # below the tie above it: stays finite
        0x7F7F8000,      # that tie: to the even side, which is inf
        0x00000001, 0x00007FFF, 0x00008000, 0x00008001, 0x00018000, 0x007FFFFF,   # denormals
        0x80000001, 0x80008001,
        0x00800000,      # the smallest normal
        0x00000000, 0x80000000,      # +-0
        0x7F800000, 0xFF800000,      # +-inf
        0x7FC00000, 0xFFC00000, 0x7F800001, 0x7FFFFFFF, 0x7FC12345,      # NaNs
    ], dtype=np.uint32)
    for width in (5, 8):
        n = -(-len(bits) // width)
        x = np.zeros(n * width, np.uint32)
        x[:len(bits)] = bits
        part = _dev(x.view(np.float32).reshape(n, width))
        T = 4
        out = ops.time_encode_cat((part,), torch.zeros(n, device="cuda"),
                                  torch.ones(T, device="cuda"), torch.zeros(T, device="cuda"),
                                  out_dtype=torch.bfloat16)
        want = part.to(torch.bfloat16)
        assert same_bits(out[:, :width], want)
        assert int(out[:, :width].isnan().sum()) == 5
        assert same_bits(out[:, width:], torch.ones((n, T), device="cuda", dtype=torch.bfloat16))


@pytest.mark.parametrize("case", [(257, 100, (172, 100), "unit"), (3, 1, (5,), "unit")],
                         ids=TE.case_id)
def test_float32_is_todays_call(case):
    """out_dtype=None and torch.float32 are the call without the keyword, bit for bit."""
    import torch
    from gnnflow_amd import ops
    c = TE.make_inputs(case)
    base = None
    for kw in ({}, dict(out_dtype=None), dict(out_dtype=torch.float32)):
        parts = [_dev(p).requires_grad_(True) for p in c["parts"]]
        w, bias = _dev(c["w"]).requires_grad_(True), _dev(c["bias"]).requires_grad_(True)
        out = ops.time_encode_cat(parts, _dev(c["t"]), w, bias, **kw)
        assert out.dtype == torch.float32
        out.backward(_dev(c["gout"]))
        res = [out.detach(), w.grad, bias.grad] + [p.grad for p in parts]
        if base is None:
            base = res
        assert all(torch.equal(a, b) for a, b in zip(res, base))


def test_other_out_dtypes_raise():
    import torch
    from gnnflow_amd import ops
    t = torch.zeros(3, device="cuda")
    for bad in (torch.float16, torch.float64, torch.int32):
        with pytest.raises(ValueError, match="out_dtype"):
            ops.time_encode_cat((), t, torch.ones(4, device="cuda"), torch.zeros(4, device="cuda"),
                                out_dtype=bad)
