"""ops.edge_score on bfloat16 src and dst rows (the uint16_t kernels of csrc/edge_score.hip)
against the float32 op on the widened rows, bit for bit: the float32 scores and the float32
gradients of weight and bias with torch.equal, the bfloat16 gradients of src and dst against the
float32 op's rounded once, on the raw 16-bit patterns.  The float32 op is checked against float64
in tests/test_gpu_edge_score.py; no tolerance here."""
import itertools

import numpy as np
import pytest

from tests import edge_score_ref as ES

pytestmark = pytest.mark.gpu

# B around the forward's 16-row workgroup and the backward's groups, r = 2 and 3, D on the
# scalar path (1, 3) and on the 4-column path (100, 128; 2 passes of the 16 lanes)
CASES = [(B, D, r) for B, r, D in itertools.product((1, 7, 600), (2, 3), (1, 3, 100, 128))]


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


def inputs(case):
    """The case's src and dst rounded to bfloat16; weight, bias and the gradient float32."""
    import torch
    c = ES.make_inputs(case)
    return dict(src=_dev(c["src"]).to(torch.bfloat16), dst=_dev(c["dst"]).to(torch.bfloat16),
                w=_dev(c["w"]), bias=_dev(c["bias"]), g=_dev(c["g"]).reshape(-1, 1))


def run(x, need=(True,) * 4, wide=False, src=None, dst=None):
    """-> (out, gsrc, gdst, gw, gbias), None where no gradient was asked for."""
    import torch
    from gnnflow_amd import ops
    cast = (lambda t: t.float()) if wide else (lambda t: t.clone())
    src = cast(x["src"]).requires_grad_(need[0]) if src is None else src
    dst = cast(x["dst"]).requires_grad_(need[1]) if dst is None else dst
    w, bias = x["w"].clone().requires_grad_(need[2]), x["bias"].clone().requires_grad_(need[3])
    out = ops.edge_score(src, dst, w, bias)
    assert out.dtype == torch.float32 and out.shape == (dst.shape[0], 1)
    if any(need):
        out.backward(x["g"])
    return (out.detach(), src.grad if src.is_leaf else None, dst.grad if dst.is_leaf else None,
            w.grad, bias.grad)


def compare(got, want):
    import torch
    assert torch.equal(got[0], want[0])
    for g, w32 in zip(got[1:3], want[1:3]):
        assert (g is None) == (w32 is None)
        assert g is None or same_bits(g, w32.to(torch.bfloat16))
    for g, w32 in zip(got[3:], want[3:]):
        assert (g is None) == (w32 is None)
        assert g is None or (g.dtype == torch.float32 and torch.equal(g, w32))


@pytest.mark.parametrize("case", CASES, ids=ES.case_id)
def test_forward_and_backward_equal_the_float32_op(case):
    x = inputs(case)
    compare(run(x), run(x, wide=True))


@pytest.mark.parametrize("case", [(7, 100, 2), (7, 3, 3), (600, 128, 2)], ids=ES.case_id)
def test_row_slices_of_one_tensor(case):
    """src = h[:B], dst = h[B:] of one bfloat16 tensor, as EdgePredictor hands them over; with
    B * D odd the dst rows start on a 2-byte boundary."""
    import torch
    B, D, r = case
    x = inputs(case)
    h = torch.cat([x["src"], x["dst"]]).requires_grad_(True)
    got = run(x, src=h[:B], dst=h[B:])
    want = run(x, wide=True)
    assert torch.equal(got[0], want[0])
    assert same_bits(h.grad[:B], want[1].to(torch.bfloat16))
    assert same_bits(h.grad[B:], want[2].to(torch.bfloat16))
    assert torch.equal(got[3], want[3]) and torch.equal(got[4], want[4])


@pytest.mark.parametrize("need", list(itertools.product([False, True], repeat=4)),
                         ids=lambda n: "".join("SDWB"[i] if v else "-" for i, v in enumerate(n)))
def test_every_requires_grad_subset(need):
    x = inputs((7, 100, 3))
    got = run(x, need)
    compare(got, run(x, need, wide=True))
    for g, n in zip(got[1:], need):
        assert (g is not None) == n


def test_two_runs_are_bit_identical():
    import torch
    x = inputs((600, 100, 2))
    a, b = run(x), run(x)
    assert torch.equal(a[0], b[0]) and same_bits(a[1], b[1]) and same_bits(a[2], b[2])
    assert torch.equal(a[3], b[3]) and torch.equal(a[4], b[4])


@pytest.mark.parametrize("B", [0, 5])
def test_no_dst_rows(B):
    import torch
    from gnnflow_amd import ops
    D = 12
    src = torch.ones((B, D), device="cuda", dtype=torch.bfloat16, requires_grad=True)
    dst = torch.ones((0, D), device="cuda", dtype=torch.bfloat16, requires_grad=True)
    w = torch.ones((1, D), device="cuda", requires_grad=True)
    bias = torch.ones(1, device="cuda", requires_grad=True)
    out = ops.edge_score(src, dst, w, bias)
    assert tuple(out.shape) == (0, 1) and out.dtype == torch.float32
    out.sum().backward()
    for t in (src, dst, w, bias):
        assert t.grad.shape == t.shape and t.grad.dtype == t.dtype and not t.grad.any()


def test_mixed_and_other_dtypes_raise():
    import torch
    from gnnflow_amd import ops
    x = inputs((7, 100, 2))
    with pytest.raises(TypeError, match="float32.*bfloat16"):
        ops.edge_score(x["src"].float(), x["dst"], x["w"], x["bias"])
    with pytest.raises(TypeError):
        ops.edge_score(x["src"], x["dst"], x["w"].to(torch.bfloat16), x["bias"])
    with pytest.raises(TypeError):
        ops.edge_score(x["src"].half(), x["dst"].half(), x["w"], x["bias"])
