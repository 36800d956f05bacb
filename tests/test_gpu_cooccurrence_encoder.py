"""nn.NeighborCooccurrenceEncoder on the GPU against the direct expression -- f applied to every
count, f(c) = Linear(dim, dim)(ReLU(Linear(1, dim)(c))), the two channels added and the padding
zeroed -- evaluated in float64: the output and the gradients of the four parameters.

Tolerance (test_gpu_gru_cell.py's rule): every tensor T must satisfy
e_op <= 2 e_direct32 + 2^-23 max |T_64|, where e_direct32 is the error of the same direct
expression in float32 on the same device, differentiated by autograd.  The padding is exactly
zero.  N = 7, L = 5, dim = 8.  The test prints its largest e_op / bound (run with -s)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import gru_cell_ref as GR

pytestmark = pytest.mark.gpu
N, L, DIM = 7, 5, 8
PARAMS = ("lift.weight", "lift.bias", "proj.weight", "proj.bias")


def _inputs():
    rng = np.random.RandomState(5)
    counts = rng.randint(0, L + 1, (N, 2, L, 2)).astype(np.int32)
    lengths = rng.randint(0, L + 1, (N, 2)).astype(np.int32)
    lengths[0], lengths[1] = (0, L), (L, 0)
    counts[2, 0, 0], counts[2, 0, 1] = (0, L), (L, L)
    g = rng.standard_normal((N, 2, L, DIM)).astype(np.float32)
    return (torch.from_numpy(counts).cuda(), torch.from_numpy(lengths).cuda(),
            torch.from_numpy(g).cuda())


def _direct(enc, counts, lengths, g, dtype):
    """f on every count, in `dtype`, with copies of enc's parameters; (out, grads)."""
    p = {k: v.detach().to(dtype).requires_grad_(True) for k, v in enc.named_parameters()}
    c = counts.to(dtype).unsqueeze(-1)                                    # [N, 2, L, 2, 1]
    hidden = torch.relu(F.linear(c, p["lift.weight"], p["lift.bias"]))
    f = F.linear(hidden, p["proj.weight"], p["proj.bias"])                # [N, 2, L, 2, dim]
    out = f[..., 0, :] + f[..., 1, :]
    filled = torch.arange(L, device=counts.device) < lengths.unsqueeze(2)
    out = out * filled.unsqueeze(3).to(dtype)
    out.backward(g.to(dtype))
    return out.detach(), {k: v.grad for k, v in p.items()}


def test_output_and_parameter_gradients_against_float64():
    import gnnflow_amd
    torch.manual_seed(11)
    enc = gnnflow_amd.NeighborCooccurrenceEncoder(DIM).cuda()
    counts, lengths, g = _inputs()
    out = enc(counts, lengths)
    assert out.dtype == torch.float32 and tuple(out.shape) == (N, 2, L, DIM) and out.is_cuda
    out.backward(g)
    got = dict(out=out.detach(), **{k: v.grad for k, v in enc.named_parameters()})
    o32, g32 = _direct(enc, counts, lengths, g, torch.float32)
    o64, g64 = _direct(enc, counts, lengths, g, torch.float64)
    t32, t64 = dict(out=o32, **g32), dict(out=o64, **g64)
    worst = 0.0
    for name in ("out",) + PARAMS:
        a, b, c = (x[name].cpu().numpy() for x in (got, t32, t64))
        assert np.abs(c).max() > 0, name
        r = GR.ratio(a, b, c)
        print("\n[e_op/bound] {}: {:.3g} (e_op {:.3g}, e_direct32 {:.3g})".format(
            name, r, GR.max_error(a, c), GR.max_error(b, c)))
        worst = max(worst, r)
    print("\n[e_op/bound] worst: {:.3g}".format(worst))
    for name in ("out",) + PARAMS:
        a, b, c = (x[name].cpu().numpy() for x in (got, t32, t64))
        assert GR.ratio(a, b, c) <= 1.0, name
    # the padding is exactly zero, and nothing else is masked
    filled = (torch.arange(L, device="cuda") < lengths.unsqueeze(2))
    assert (out[~filled] == 0).all() and (out[filled] != 0).any(1).all()
    assert (lengths == 0).any() and (lengths == L).any() and (counts == L).any()


def test_a_fixed_table_gives_the_same_rows():
    import gnnflow_amd
    torch.manual_seed(11)
    enc = gnnflow_amd.NeighborCooccurrenceEncoder(DIM).cuda()
    fixed = gnnflow_amd.NeighborCooccurrenceEncoder(DIM, max_count=L).cuda()
    fixed.load_state_dict(enc.state_dict())
    counts, lengths, _ = _inputs()
    assert torch.equal(enc(counts, lengths), fixed(counts, lengths))
    with pytest.raises(ValueError, match="max_count"):
        gnnflow_amd.NeighborCooccurrenceEncoder(DIM, max_count=L - 1).cuda()(counts, lengths)
