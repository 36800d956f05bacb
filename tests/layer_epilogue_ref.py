"""Float64 reference of ops.dropout_relu_layer_norm (csrc/layer_epilogue.hip), the exact mask it
draws, a priori bounds on the error of its fp32 kernels, and the seeded inputs that the CPU and
the GPU tests share.  Pure numpy.

    T         = uint32(float64(p) * 2^32)            sc = fl32(1 / (1 - p))
    keep[r,d] = gf_philox4x32_10_first(seed, r * D + d, 0) >= T          (attention_dropout_ref)
    y[r,d]    = max(keep ? x * sc : 0, 0)
    mean[r]   = sum_d y / D      var[r] = sum_d (y - mean)^2 / D      rstd[r] = 1 / sqrt(var + eps)
    xhat      = (y - mean) rstd                      out = xhat gamma + beta
    g         = gout gamma       dy = rstd (g - sum_d g / D - xhat sum_d (g xhat) / D)
    gx        = y > 0 ? dy sc : 0
    ggamma[d] = sum_r gout xhat                      gbeta[d] = sum_r gout

The float64 side is evaluated on the same fp32 inputs, with sc the kernels' own fp32 constant and
eps the fp32 value they are handed.  u = 2^-24, gamma_k = k u / (1 - k u).  The library is built
with -ffp-contract=off and without fast-math, so every add, multiply, divide and square root is
one correctly rounded fp32 operation and a sum of n terms is within gamma_{n-1} sum |terms| of the
exact sum of the terms it is given, in ANY order (Higham, Accuracy and Stability, 4.2).  None of
the bounds therefore pins the kernels' layout.  Two rules carry every step, with b(a) the bound
already held on a computed a^ (first order would drop the products of bounds; they are kept):

    product   b(a b) = b(a) |b| + |a| b(b) + b(a) b(b) + u (|a| + b(a)) (|b| + b(b))
    sum       b(a + b) = b(a) + b(b) + u (|a + b| + b(a) + b(b))

Mask.  fl(x sc) has the sign of x sc and is zero only where x is (the inputs keep every product
a normal fp32), so y > 0 in the kernels exactly where it is here: the kernels' mask IS the exact
mask, and gx is exactly 0 where y is.  Where a bound is 0 error_ratio demands the exact value.

    y       one rounding where p > 0 (x sc), none at p = 0 (sc = 1):   b(y) = u y  or  0
    mean    D - 1 adds of terms >= 0 and one division:
            b(S) = sum b(y) + gamma_{D-1} sum (y + b(y)),  b(mean) = b(S) / D + u (mean + b(S) / D)
    dev     = y - mean by the sum rule
    var     the error of mean^ is one value e, |e| <= b(mean), common to the row's deviations, and
            sum_d dev = 0: it enters sum dev^2 as D e^2 only, not as 2 e sum |dev|.  With b_own =
            b(dev) - b(mean) the column's own part: sum over d of b(mean)^2 + 2 (|dev| + b(mean))
            b_own + b_own^2, one rounding per square, D - 1 adds and one division, as mean;
            var + eps by the sum rule
    s       = sqrt(var + eps) = sqrt(t):  |sqrt(t^) - sqrt(t)| <= b(t) / sqrt(t), one rounding more
    rstd    = 1 / s:  b(s) / (s (s - b(s))), one rounding more
    xhat    dev rstd by the product rule; out: one product with gamma, one sum with beta

The backward reads mean and rstd as the forward stored them and recomputes y, dev and xhat by the
same operations: the bounds above hold for them.  g = gout gamma is one rounding; its row sum and
that of g xhat are D - 1 adds and a division; dy is two sums, two products; gx one product more.
ggamma[d] is R products gout xhat^ and R - 1 adds however the rows are cut into waves, workgroups
and partial rows; gbeta[d] R - 1 adds of exact terms.

The inputs are drawn (make_inputs) with magnitudes in [2^-3, 4] on a grid of 2^-12, so no product
leaves the normal range; the special rows of the GPU tests (constant, negative, zero, one large
entry) are built from such values too.
"""
import numpy as np

from tests.attention_dropout_ref import philox_first, scale, threshold
from tests.block_ops_ref import U, error_ratio, gamma  # noqa: F401  (re-exported)

MAX_WIDTH = 1024


def keep_mask(R, D, p, seed):
    """bool [R, D]: element (r, d) draws counter r * D + d."""
    if np.float32(p) == 0:
        return np.ones((R, D), bool)
    u = philox_first(seed, np.arange(R * D, dtype=np.uint64), 0)
    return (u >= np.uint32(min(threshold(p), 0xFFFFFFFF))).reshape(R, D)


def round_bf16(a):
    """fp32 -> the nearest bfloat16 (ties to even) as fp32: the kernels' narrow() of bf16.hpp on
    finite values."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    b = a.view(np.uint32).astype(np.uint64)
    b = ((b + np.uint64(0x7FFF) + ((b >> np.uint64(16)) & np.uint64(1))) >> np.uint64(16)) \
        << np.uint64(16)
    return b.astype(np.uint32).view(np.float32).reshape(a.shape)


def _mul(a, ba, b, bb):
    a, b = np.abs(a), np.abs(b)
    return ba * b + a * bb + ba * bb + U * (a + ba) * (b + bb)


def _add(result, ba, bb):
    return ba + bb + U * (np.abs(result) + ba + bb)


def _rowsum(terms, b_terms, n):
    """(sum over the last axis) / n: bound of the kernels' n - 1 adds and one division."""
    s = terms.sum(-1)
    b_s = b_terms.sum(-1) + gamma(n - 1) * (np.abs(terms) + b_terms).sum(-1)
    return s / n, b_s / n + U * (np.abs(s) / n + b_s / n)


class Reference:
    """All float64 results and all bounds of one case, computed once and left unchanged."""

    def __init__(self, x, weight, bias, gout, eps=1e-5, p=0.0, seed=0):
        x32 = np.asarray(x, np.float32)
        R, D = x32.shape
        assert 1 <= D <= MAX_WIDTH
        x, w, b, g = (np.asarray(a, np.float32).astype(np.float64)
                      for a in (x32, weight, bias, gout))
        assert w.shape == b.shape == (D,) and g.shape == (R, D)
        self.R, self.D, self.p, self.seed = R, D, float(np.float32(p)), int(seed)
        eps = float(np.float32(eps))
        sc = float(scale(p))
        self.keep = keep_mask(R, D, p, seed)
        xs = np.where(self.keep, x * sc, 0.0)
        y = np.maximum(xs, 0.0)
        self.y, self.active = y, y > 0
        b_y = U * y if self.p > 0 else np.zeros_like(y)

        # ---- forward -------------------------------------------------------------------------
        mean, b_mean = _rowsum(y, b_y, D)
        dev = y - mean[:, None]
        b_dev = _add(dev, b_y, b_mean[:, None])
        # the error of mean^ is COMMON to the row's deviations: dev^ = dev + e + h with |e| <=
        # b(mean) the same in every column and |h| <= b_own its own; sum_d dev = 0, so
        # sum (dev + e + h)^2 - sum dev^2 = D e^2 + 2 sum (dev + e) h + sum h^2
        b_own = b_dev - b_mean[:, None]
        b_sq = b_mean[:, None] ** 2 + 2 * (np.abs(dev) + b_mean[:, None]) * b_own + b_own ** 2 \
            + U * (np.abs(dev) + b_dev) ** 2
        var, b_var = _rowsum(dev * dev, b_sq, D)
        t = var + eps
        b_t = _add(t, b_var, 0.0)
        s = np.sqrt(t)
        b_s = b_t / s
        b_s = b_s + U * (s + b_s)
        assert (b_s < s).all()
        rstd = 1.0 / s
        b_rstd = b_s / (s * (s - b_s))
        b_rstd = b_rstd + U * (rstd + b_rstd)
        xhat = dev * rstd[:, None]
        b_xhat = _mul(dev, b_dev, rstd[:, None], b_rstd[:, None])
        xg = xhat * w
        self.mean, self.b_mean, self.rstd, self.b_rstd = mean, b_mean, rstd, b_rstd
        self.xhat = xhat
        self.out = xg + b
        self.b_out = _add(self.out, _mul(xhat, b_xhat, w, 0.0), 0.0)

        # ---- backward ------------------------------------------------------------------------
        gg = g * w
        b_gg = U * np.abs(gg)
        m1, b_m1 = _rowsum(gg, b_gg, D)
        m2, b_m2 = _rowsum(gg * xhat, _mul(gg, b_gg, xhat, b_xhat), D)
        a = gg - m1[:, None]
        b_a = _add(a, b_gg, b_m1[:, None])
        h = xhat * m2[:, None]
        b_h = _mul(xhat, b_xhat, m2[:, None], b_m2[:, None])
        c = a - h
        b_c = _add(c, b_a, b_h)
        dy = rstd[:, None] * c
        b_dy = _mul(rstd[:, None], b_rstd[:, None], c, b_c)
        self.gx = np.where(self.active, dy * sc, 0.0)
        self.b_gx = np.where(self.active, _mul(dy, b_dy, sc, 0.0), 0.0)
        terms = g * xhat
        b_terms = _mul(g, 0.0, xhat, b_xhat)
        self.ggamma = terms.sum(0)
        self.b_ggamma = b_terms.sum(0) + gamma(R) * (np.abs(terms) + b_terms).sum(0)
        self.gbeta = g.sum(0)
        self.b_gbeta = gamma(R) * np.abs(g).sum(0)

    def ratios(self, out=None, mean=None, rstd=None, gx=None, ggamma=None, gbeta=None,
               scale=1.0):
        """{name: max error / (scale x bound)} of the results given."""
        got = dict(out=out, mean=mean, rstd=rstd, gx=gx, ggamma=ggamma, gbeta=gbeta)
        want = dict(out=(self.out, self.b_out), mean=(self.mean, self.b_mean),
                    rstd=(self.rstd, self.b_rstd), gx=(self.gx, self.b_gx),
                    ggamma=(self.ggamma, self.b_ggamma), gbeta=(self.gbeta, self.b_gbeta))
        return {k: error_ratio(np.asarray(v, np.float64).reshape(want[k][0].shape), want[k][0],
                               scale * want[k][1])
                for k, v in got.items() if v is not None}


# ---- seeded inputs shared by the CPU and the GPU tests ---------------------------------------
# (R, D).  Every D at R = 5: one lane used (1), a partial last chunk (3), both sides of the 64
# columns a wave covers with one column per lane (64, 65), the models' widths (100, 172), the
# last width with one chunk per lane (256) and the maximum, 16 columns per lane (1024).  Every R
# at D = 100: one row, fewer rows than a workgroup holds twice (5), more than one workgroup of the
# backward (257) and one more than the cap of the partial rows allows at one row each (1025).
WIDTHS = (1, 3, 64, 65, 100, 172, 256, 1024)
HEIGHTS = (1, 5, 257, 1025)
CASES = [(5, D) for D in WIDTHS] + [(R, 100) for R in HEIGHTS if R != 5] + [(1025, 1024)]
PS = (0.0, 0.2)
SEED = 0x5EEDC0FFEE123457          # above 2^32: both key words of the generator are in play
EPS = 1e-5


def case_id(case):
    return "R{}_D{}".format(*case)


def _draw(rng, *shape):
    """Signed magnitudes in [2^-3, 4] on a grid of 2^-12, fp32."""
    mag = rng.randint(1 << 9, (1 << 14) + 1, size=shape).astype(np.float64) / (1 << 12)
    return (mag * rng.choice([-1.0, 1.0], size=shape)).astype(np.float32)


def make_inputs(case, seed=None):
    """fp32 x [R, D], weight and bias [D] and gout [R, D] of a case."""
    R, D = case
    rng = np.random.RandomState(3000 + R + 7 * D if seed is None else seed)
    return dict(x=_draw(rng, R, D), weight=_draw(rng, D), bias=_draw(rng, D), gout=_draw(rng, R, D))


def reference(c, p=0.0, seed=SEED, eps=EPS):
    return Reference(c["x"], c["weight"], c["bias"], c["gout"], eps=eps, p=p, seed=seed)


def special_rows(D=100):
    """x [6, D] of rows that break a careless kernel: a constant positive row (variance 0; 1.5
    sums exactly, so mean is 1.5 and out is beta), an all-negative row (y = 0), a row with one
    1e4 entry among 1e-3 entries, a row with zeros among positive entries (relu's gradient at 0
    is 0), a row of large, nearly equal entries (E[y^2] - mean^2 cancels), an ordinary row."""
    rng = np.random.RandomState(77)
    x = np.abs(_draw(rng, 6, D))
    x[0] = 1.5
    x[1] = -x[1]
    x[2] = np.float32(1e-3)
    x[2, D // 3] = np.float32(1e4)
    x[3, ::3] = 0.0
    x[4] = np.float32(64.0) + x[4] / np.float32(4.0)
    x[5] = _draw(rng, D)
    return x.astype(np.float32)


def special_case():
    """special_rows() with seeded weight, bias and gout."""
    x = special_rows()
    rng = np.random.RandomState(78)
    D = x.shape[1]
    return dict(x=x, weight=_draw(rng, D), bias=_draw(rng, D), gout=_draw(rng, *x.shape))


ALL_DROPPED_SEED = 0      # asserted equal to find_all_dropped_seed(3, 0.9) on the CPU


def find_all_dropped_seed(D, p, R=4, limit=4096):
    """The first seed whose mask drops every element of some row of an [R, D] input."""
    for seed in range(limit):
        if (~keep_mask(R, D, p, seed)).all(axis=1).any():
            return seed
    raise AssertionError("no seed below {} drops a whole row".format(limit))


def emulate_fp32(c, p=0.0, seed=SEED, eps=EPS, one_pass_variance=False):
    """The kernels' arithmetic in numpy fp32 with serial sums -> dict of out, mean, rstd, gx,
    ggamma, gbeta.  Stands in for the GPU in the CPU tests.  one_pass_variance: the variance as
    E[y^2] - mean^2 instead, what the kernels must not do."""
    f = np.float32
    x, w, b, g = (np.asarray(c[k], f) for k in ("x", "weight", "bias", "gout"))
    R, D = x.shape
    sc, n = scale(p), f(D)
    keep = keep_mask(R, D, p, seed)
    y = np.maximum(np.where(keep, x * sc, f(0)), f(0))
    ssum = lambda a: np.cumsum(a, axis=1, dtype=f)[:, -1]      # noqa: E731
    mean = ssum(y) / n
    dev = y - mean[:, None]
    var = ssum(y * y) / n - mean * mean if one_pass_variance else ssum(dev * dev) / n
    rstd = f(1) / np.sqrt(var + f(eps))
    xhat = dev * rstd[:, None]
    out = xhat * w + b
    gg = g * w
    m1, m2 = ssum(gg) / n, ssum(gg * xhat) / n
    dy = rstd[:, None] * (gg - m1[:, None] - xhat * m2[:, None])
    gx = np.where(y > 0, dy * sc, f(0))
    ggamma = np.cumsum(g * xhat, axis=0, dtype=f)[-1]
    gbeta = np.cumsum(g, axis=0, dtype=f)[-1]
    res = dict(out=out, mean=mean, rstd=rstd, gx=gx, ggamma=ggamma, gbeta=gbeta)
    assert all(v.dtype == f for v in res.values())
    return res
