"""Float64 statement of ops.gru_cell (csrc/gru_cell.hip), the seeded inputs that the CPU and GPU
tests share, and the rule the GPU tests judge a float32 evaluation by.  Pure numpy.

    gi, gh [N, 3H] in the gate order r, z, n; hx [N, H]; residual [N, H] or none; g = d h_out

    r = sigma(gi_r + gh_r)      z = sigma(gi_z + gh_z)      n = tanh(gi_n + r gh_n)
    u = (1 - z) n + z hx        h_out = u (+ residual)      last = u[:R]

    a_n = g (1 - z)(1 - n^2)    a_z = g (hx - n) z (1 - z)  a_r = a_n gh_n r (1 - r)
    d_gi = [a_r, a_z, a_n]      d_gh = [a_r, a_z, a_n r]    d_hx = g z      d_residual = g

The float64 side is evaluated on the same fp32 inputs.  tests/test_gru_cell_ref.py checks it
against torch.nn.GRUCell in float64, forward and through autograd.

Tolerance.  The error of a float32 evaluation is dominated by the device's expf and tanhf, whose
error is not ours to assume, so nothing is derived a priori.  Each tensor T of the op is instead
measured against the same formula written with torch.sigmoid / torch.tanh in float32 on the same
device and differentiated by autograd:

    e_op = max |T_op - T_64|      e_torch = max |T_torch - T_64|
    e_op <= 2 e_torch + 2^-23 max |T_64|                                           (`bound`)

Both sides are valid float32 evaluations that differ in the transcendental functions and in the
association of the products, hence the factor 2; torch may land exactly, hence the floor of one
float32 spacing of the tensor's largest value.
"""
import numpy as np

from tests.layer_epilogue_ref import round_bf16  # noqa: F401  (re-exported)

# (N, H, R): the smallest shape; no `last` rows; one 4-column vector per chunk with R == N; the
# scalar path (H = 7) on a whole wave of rows; the model's H = 100 (float32: 16-byte path,
# bfloat16: the 8-byte one), one row past a wave; H = 8 (bfloat16: 16-byte path) over more than
# one workgroup; the edge width 172.
CASES = [(1, 1, 1), (3, 3, 0), (5, 4, 5), (64, 7, 64), (65, 100, 17), (257, 8, 64),
         (130, 172, 43)]
# pre-activations of the saturation case: the ends of sigma and tanh and their small-argument ends
EXTREMES = (100.0, -100.0, 0.0, 1e-4, -1e-4)

FLOOR = 2.0 ** -23


def case_id(case):
    return "N{}_H{}_R{}".format(*case)


def make_inputs(case, seed=None):
    """fp32 gi, gh [N, 3H], hx, residual, g [N, H] of a case, of unit scale."""
    N, H, R = case
    rng = np.random.RandomState(4000 + N + 7 * H + 31 * R if seed is None else seed)
    f = lambda *shape: rng.standard_normal(shape).astype(np.float32)      # noqa: E731
    return dict(gi=f(N, 3 * H), gh=f(N, 3 * H), hx=f(N, H), residual=f(N, H), g=f(N, H), R=R)


def make_saturated(case, seed=77):
    """A case whose pre-activations gi_r + gh_r, gi_z + gh_z and gi_n + r gh_n run through
    EXTREMES: gh is zero in the r and z chunks and gi carries the value, and in the n chunk gi_n
    carries it with gh_n zero on even columns and gi_n = 0 with gh_n = the value on odd ones (so
    the pre-activation is r times it)."""
    N, H, R = case
    c = make_inputs(case, seed)
    rng = np.random.RandomState(seed)
    pick = lambda: np.asarray(EXTREMES, np.float32)[rng.randint(0, len(EXTREMES), (N, H))]  # noqa
    gi, gh = np.zeros((N, 3 * H), np.float32), np.zeros((N, 3 * H), np.float32)
    gi[:, :H], gi[:, H:2 * H] = pick(), pick()
    v, odd = pick(), (np.arange(H) % 2 == 1)[None, :]
    gi[:, 2 * H:] = np.where(odd, 0, v)
    gh[:, 2 * H:] = np.where(odd, v, 0)
    c.update(gi=gi, gh=gh)
    return c


def sigmoid(x):
    """1 / (1 + exp(-x)) without an overflow warning: exp of the negative magnitude."""
    e = np.exp(-np.abs(x))
    return np.where(x >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


class Reference:
    """All float64 results of one case, computed once and left unchanged."""

    def __init__(self, gi, gh, hx, g, residual=None, R=0, input_dtype=np.float32):
        # input_dtype: what the inputs are rounded to before they are widened to float64
        gi, gh, hx, g = (np.asarray(a, input_dtype).astype(np.float64) for a in (gi, gh, hx, g))
        N, H = hx.shape
        assert gi.shape == gh.shape == (N, 3 * H) and g.shape == (N, H) and 0 <= R <= N
        ir, iz, i_n = gi[:, :H], gi[:, H:2 * H], gi[:, 2 * H:]
        hr, hz, hn = gh[:, :H], gh[:, H:2 * H], gh[:, 2 * H:]
        r, z = sigmoid(ir + hr), sigmoid(iz + hz)
        n = np.tanh(i_n + r * hn)
        self.r, self.z, self.n = r, z, n
        self.u = (1.0 - z) * n + z * hx
        self.h_out = self.u.copy()
        if residual is not None:
            self.h_out = self.u + np.asarray(residual, input_dtype).astype(np.float64)
        self.last = self.u[:R].copy()
        a_n = g * (1.0 - z) * (1.0 - n * n)
        a_z = g * (hx - n) * z * (1.0 - z)
        a_r = a_n * hn * r * (1.0 - r)
        self.d_gi = np.concatenate([a_r, a_z, a_n], 1)
        self.d_gh = np.concatenate([a_r, a_z, a_n * r], 1)
        self.d_hx = g * z
        self.d_residual = g.copy()

    def tensors(self):
        return dict(h_out=self.h_out, last=self.last, d_gi=self.d_gi, d_gh=self.d_gh,
                    d_hx=self.d_hx)


def reference(c, with_residual=True):
    return Reference(c["gi"], c["gh"], c["hx"], c["g"], c["residual"] if with_residual else None,
                     c["R"])


def max_error(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.isfinite(got).all()
    return float(np.abs(got - want).max()) if got.size else 0.0


def bound(torch_value, want, factor=2.0):
    """factor x e_torch + 2^-23 max |T_64|."""
    want = np.asarray(want, np.float64)
    top = float(np.abs(want).max()) if want.size else 0.0
    return factor * max_error(torch_value, want) + FLOOR * top


def ratio(got, torch_value, want):
    """e_op / bound; 0 when both are 0."""
    e, b = max_error(got, want), bound(torch_value, want)
    return 0.0 if e == 0.0 else (e / b if b > 0 else float("inf"))


def emulate_fp32(c, with_residual=True):
    """The formulas in numpy fp32 -> the op's five tensors.  Stands in for a float32 evaluation
    in the CPU tests."""
    f = np.float32
    gi, gh, hx, g, R = c["gi"], c["gh"], c["hx"], c["g"], c["R"]
    H = hx.shape[1]
    sg = lambda x: (f(1) / (f(1) + np.exp(-x, dtype=f))).astype(f)      # noqa: E731
    with np.errstate(over="ignore"):
        r, z = sg(gi[:, :H] + gh[:, :H]), sg(gi[:, H:2 * H] + gh[:, H:2 * H])
    hn = gh[:, 2 * H:]
    n = np.tanh(gi[:, 2 * H:] + r * hn, dtype=f)
    u = (f(1) - z) * n + z * hx
    a_n = g * (f(1) - z) * (f(1) - n * n)
    a_z = g * (hx - n) * z * (f(1) - z)
    a_r = a_n * hn * r * (f(1) - r)
    out = dict(h_out=u + c["residual"] if with_residual else u, last=u[:R],
               d_gi=np.concatenate([a_r, a_z, a_n], 1),
               d_gh=np.concatenate([a_r, a_z, a_n * r], 1), d_hx=g * z)
    assert all(v.dtype == f for v in out.values())
    return out
