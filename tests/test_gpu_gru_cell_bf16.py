"""ops.gru_cell on bfloat16 gates (the uint16_t instantiations of csrc/gru_cell.hip) against the
float32 op on the widened gates, bit for bit: h_out, last and the gradient of hx with
torch.equal, the bfloat16 gradients of gi and gh against the float32 op's rounded once, on the
raw 16-bit patterns.  The float32 op is checked against float64 in tests/test_gpu_gru_cell.py; no
tolerance here."""
import itertools

import numpy as np
import pytest

from tests import gru_cell_ref as GR

pytestmark = pytest.mark.gpu

# H = 8: 16-byte accesses; H = 100: bfloat16 rows that are not 16-byte aligned (8-byte gate
# accesses); H = 7: element by element.  N on one thread's worth, around a wave, several
# workgroups.
CASES = [(N, H, R) for (N, R), H in itertools.product(((1, 1), (65, 17), (700, 0)), (8, 100, 7))]


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def same_bits(got, want):
    import torch
    assert got.dtype == torch.bfloat16 and want.dtype == torch.bfloat16
    assert got.shape == want.shape
    return torch.equal(got.contiguous().view(torch.int16), want.contiguous().view(torch.int16))


def inputs(case, saturated=False):
    """The case's gates rounded to bfloat16; hx, the residual and the gradient float32."""
    import torch
    c = GR.make_saturated(case) if saturated else GR.make_inputs(case)
    x = {k: _dev(c[k]) for k in ("gi", "gh", "hx", "residual", "g")}
    x["gi"], x["gh"] = x["gi"].to(torch.bfloat16), x["gh"].to(torch.bfloat16)
    x["R"] = c["R"]
    return x


def run(x, wide=False, residual="f32", need=(True,) * 4):
    """-> (h_out, last, d_gi, d_gh, d_hx, d_residual), None where no gradient was asked for."""
    import torch
    from gnnflow_amd import ops
    cast = (lambda t: t.float()) if wide else (lambda t: t.clone())
    gi, gh = cast(x["gi"]).requires_grad_(need[0]), cast(x["gh"]).requires_grad_(need[1])
    hx = x["hx"].clone().requires_grad_(need[2])
    res = None
    if residual is not None:
        res = x["residual"].to(torch.bfloat16) if residual == "bf16" else x["residual"].clone()
        res.requires_grad_(need[3])
    out, last = ops.gru_cell(gi, gh, hx, res, num_last=x["R"])
    assert out.dtype == torch.float32 and last.dtype == torch.float32
    if out.requires_grad:
        out.backward(x["g"])
    return (out.detach(), last, gi.grad, gh.grad, hx.grad, None if res is None else res.grad)


def compare(got, want):
    import torch
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    for g, w32 in zip(got[2:4], want[2:4]):
        assert (g is None) == (w32 is None)
        assert g is None or same_bits(g, w32.to(torch.bfloat16))
    for g, w32 in zip(got[4:], want[4:]):
        assert (g is None) == (w32 is None)
        assert g is None or (g.dtype == w32.dtype and torch.equal(g, w32))


@pytest.mark.parametrize("residual", [None, "f32", "bf16"])
@pytest.mark.parametrize("case", CASES, ids=GR.case_id)
def test_forward_and_backward_equal_the_float32_op(case, residual):
    import torch
    x = inputs(case)
    got = run(x, residual=residual)
    compare(got, run(x, wide=True, residual=residual))
    if residual == "bf16":
        assert got[5].dtype == torch.bfloat16
        assert same_bits(got[5], x["g"].to(torch.bfloat16))
    elif residual == "f32":
        assert torch.equal(got[5], x["g"])


@pytest.mark.parametrize("case", [(65, 100, 17), (65, 8, 17)], ids=GR.case_id)
def test_saturated_pre_activations(case):
    import torch
    x = inputs(case, saturated=True)
    got = run(x)
    compare(got, run(x, wide=True))
    for t in got:
        assert torch.isfinite(t.float()).all()


@pytest.mark.parametrize("H", [8, 100])
def test_misaligned_gates_take_a_narrower_path(H):
    """Gates that start 2 bytes past a 16-byte boundary: bit-equal to the aligned run."""
    import torch
    from gnnflow_amd import ops
    x = inputs((65, H, 17))
    aligned = run(x)

    def shifted(t):
        flat = torch.zeros(t.numel() + 1, device="cuda", dtype=t.dtype)
        v = flat[1:].view(*t.shape)
        v.copy_(t)
        assert v.is_contiguous() and v.data_ptr() % 16 == 2
        return v.requires_grad_(True)

    for which in ("gi", "gh"):
        gi = shifted(x["gi"]) if which == "gi" else x["gi"].clone().requires_grad_(True)
        gh = shifted(x["gh"]) if which == "gh" else x["gh"].clone().requires_grad_(True)
        hx = x["hx"].clone().requires_grad_(True)
        out, last = ops.gru_cell(gi, gh, hx, x["residual"], num_last=17)
        out.backward(x["g"])
        assert torch.equal(out.detach(), aligned[0]) and torch.equal(last, aligned[1])
        assert same_bits(gi.grad, aligned[2]) and same_bits(gh.grad, aligned[3])
        assert torch.equal(hx.grad, aligned[4])


@pytest.mark.parametrize("need", list(itertools.product([False, True], repeat=4)),
                         ids=lambda n: "".join("IHXR"[i] if v else "-" for i, v in enumerate(n)))
def test_every_requires_grad_subset(need):
    x = inputs((65, 100, 17))
    got = run(x, need=need)
    compare(got, run(x, wide=True, need=need))
    for g, n in zip(got[2:], need):
        assert (g is not None) == n


def test_two_runs_are_bit_identical():
    import torch
    x = inputs((700, 100, 0))
    a, b = run(x), run(x)
    assert torch.equal(a[0], b[0]) and same_bits(a[2], b[2]) and same_bits(a[3], b[3])
    assert torch.equal(a[4], b[4])


def test_no_rows():
    import torch
    from gnnflow_amd import ops
    H = 12
    gi = torch.ones((0, 3 * H), device="cuda", dtype=torch.bfloat16, requires_grad=True)
    gh = torch.ones((0, 3 * H), device="cuda", dtype=torch.bfloat16, requires_grad=True)
    hx = torch.ones((0, H), device="cuda", requires_grad=True)
    res = torch.ones((0, H), device="cuda", dtype=torch.bfloat16, requires_grad=True)
    out, last = ops.gru_cell(gi, gh, hx, res)
    assert tuple(out.shape) == (0, H) and out.dtype == torch.float32
    out.sum().backward()
    for t in (gi, gh, hx, res):
        assert t.grad.shape == t.shape and t.grad.dtype == t.dtype and not t.grad.any()


def test_mixed_and_other_dtypes_raise():
    import torch
    from gnnflow_amd import ops
    x = inputs((65, 100, 17))
    with pytest.raises(TypeError, match="float32.*bfloat16"):
        ops.gru_cell(x["gi"].float(), x["gh"], x["hx"])
    with pytest.raises(TypeError, match="float32.*bfloat16"):
        ops.gru_cell(x["gi"], x["gh"].float(), x["hx"])
    with pytest.raises(TypeError):
        ops.gru_cell(x["gi"], x["gh"], x["hx"].to(torch.bfloat16))
    with pytest.raises(TypeError):
        ops.gru_cell(x["gi"].half(), x["gh"].half(), x["hx"])
    with pytest.raises(TypeError):
        ops.gru_cell(x["gi"], x["gh"], x["hx"], x["residual"].half())
