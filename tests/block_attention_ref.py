"""Float64 reference of ops.block_attention (csrc/block_attention.hip), a priori bounds on the
error of its fp32 kernels, and the seeded inputs that the CPU and GPU tests share.  Pure numpy.

    z[e,h] = sum_c q[row[e],h,c] k[e,h,c]     s = z > 0 ? z : slope z
    a      = softmax of s over the edges that share a destination
    out[d,h,c] = sum_e a[e,h] v[e,h,c]

`row` is taken as given (any order); no layout is assumed.  u, gamma_k and the float64 slack
are those of tests/block_ops_ref.py, and so is the argument that the bounds hold for any
summation order (no contraction, no fast-math).  The kernel's softmax is TWO PASSES over the
stored scores: max, then sum of __expf(s - m), then a = __expf(s - m) * (1 / sum); the bounds
below are for that scheme (there is no rescaling of partial sums to account for).

Every bound is first order in u with the second-order terms kept by using |x| + bound(x)
where a perturbed x is multiplied.
"""
import numpy as np

from tests.block_ops_ref import U, error_ratio, gamma  # noqa: F401  (re-exported)

U64 = 2.0 ** -53
TINY = 2.0 ** -126
KINK_MARGIN = 8.0        # min |z| >= KINK_MARGIN * bound(z): the inputs stay clear of the kink


def _slack(n):
    return 4.0 * np.asarray(n, dtype=np.float64) * U64


def _seg_sum(row, values, num_dst):
    out = np.zeros((num_dst,) + values.shape[1:])
    np.add.at(out, row, values)
    return out


def _seg_max(row, values, num_dst):
    out = np.full((num_dst,) + values.shape[1:], -np.inf)
    np.maximum.at(out, row, values)
    return out


def _f64(*arrays):
    return [np.asarray(a, dtype=np.float64) for a in arrays]


class Reference:
    """All float64 results and all bounds of one case, computed once and left unchanged.

    exact_z: the caller vouches that every product and partial sum of z is an integer below
    2^24 (checked here), so the kernel's z is exact, bound(z) = 0 and z == 0 may occur."""

    def __init__(self, row, num_dst, q, k, v, gout, slope=0.2, exact_z=False):
        row = np.asarray(row, dtype=np.int64).reshape(-1)
        q, k, v, g = _f64(q, k, v, gout)
        E, H, D = k.shape
        assert q.shape == (num_dst, H, D) and v.shape == k.shape and g.shape == q.shape
        assert len(row) == E and (E == 0 or (row.min() >= 0 and row.max() < num_dst))
        slope = float(np.float32(slope))            # the kernel's fp32 constant
        self.row, self.num_dst, self.slope = row, num_dst, slope
        n = np.bincount(row, minlength=num_dst)[row][:, None].astype(np.float64)   # [E, 1]
        qe, ge = q[row], g[row]

        # ---- forward -----------------------------------------------------------------------
        # z: D products and D - 1 adds in some order: gamma_{D+1} sum |q k| (as block_ops_ref
        # bounds its dot products, one spare rounding)
        self.z = (qe * k).sum(-1)
        absqk = np.abs(qe * k).sum(-1)
        if exact_z:
            assert np.array_equal(qe * k, np.round(qe * k)) and absqk.max(initial=0) < 2 ** 24
            self.bz = np.zeros_like(self.z)
        else:
            self.bz = (gamma(D + 1) + _slack(D)) * absqk
        pos = self.z > 0
        f = np.where(pos, 1.0, abs(slope))
        # s: the same branch as the reference (the precondition), one rounding of slope * z
        self.s = np.where(pos, self.z, slope * self.z)
        bs = f * self.bz + np.where(pos, 0.0, U * (np.abs(self.s) + f * self.bz))
        # a: softmax of perturbed scores.  With |s^ - s| <= bs, a^_k / a_k lies within
        # exp(+-(bs_k + max_j bs_j)) (numerator e^{+-bs_k}, denominator a convex combination
        # of e^{+-bs_j}).  On top, the fp32 evaluation as in block_ops_ref.softmax_fwd_bound:
        # t_k = u (3 |s_k - m| + 2) for the subtraction, the multiply by log2e and a 1-ulp
        # v_exp_f32, weighted mean of t for the sum, (n + 1) u for the n-term sum and 1 / sum;
        # |s^_k - m^| exceeds |s_k - m| by at most 2 max bs.
        m = _seg_max(row, self.s, num_dst)[row] if E else self.s
        ex = np.exp(self.s - m)
        self.att = ex / _seg_sum(row, ex, num_dst)[row] if E else ex
        bsmax = _seg_max(row, bs, num_dst)[row] if E else bs
        pert = np.expm1(bs + bsmax)
        t = U * (3.0 * (np.abs(self.s - m) + 2.0 * bsmax) + 2.0)
        fp = t + _seg_sum(row, self.att * t, num_dst)[row] + (n + 1) * U + _slack(n)
        self.b_att = self.att * (pert + fp * (1.0 + pert)) + TINY
        # out: n products, n - 1 adds of perturbed weights
        a_hi = self.att + self.b_att
        self.out = _seg_sum(row, self.att[:, :, None] * v, num_dst)
        nd = np.bincount(row, minlength=num_dst)[:, None, None].astype(np.float64)
        self.b_out = _seg_sum(row, self.b_att[:, :, None] * np.abs(v), num_dst) + \
            (gamma(nd + 1) + _slack(nd)) * _seg_sum(row, a_hi[:, :, None] * np.abs(v), num_dst)

        # ---- backward ----------------------------------------------------------------------
        # ga = sum_c gout v: gamma_{D+1} sum |gout v|
        ga = (ge * v).sum(-1)
        b_ga = (gamma(D + 1) + _slack(D)) * np.abs(ge * v).sum(-1)
        # gv = a gout: the error of a, and one multiply
        self.gv = self.att[:, :, None] * ge
        self.b_gv = (self.b_att + (U + U64) * a_hi)[:, :, None] * np.abs(ge)
        # dot = sum_e a ga: perturbed factors, then n products and n - 1 adds
        ga_hi = np.abs(ga) + b_ga
        dot = _seg_sum(row, self.att * ga, num_dst)[row] if E else ga
        per_dst = _seg_sum(row, self.b_att * np.abs(ga) + a_hi * b_ga, num_dst)
        b_dot = (per_dst[row] + (gamma(n + 1) + _slack(n)) *
                 _seg_sum(row, a_hi * ga_hi, num_dst)[row]) if E else ga
        # gs = a (ga - dot): one subtraction, one multiply
        tt = ga - dot
        b_tt = b_ga + b_dot + U * (np.abs(tt) + b_ga + b_dot)
        gs = self.att * tt
        b_gs = self.b_att * (np.abs(tt) + b_tt) + self.att * b_tt + \
            (U + U64) * a_hi * (np.abs(tt) + b_tt)
        # gz = gs * (z > 0 ? 1 : slope); slope also at z == 0, as torch.leaky_relu
        self.gz = gs * np.where(pos, 1.0, slope)
        b_gz = f * b_gs + np.where(pos, 0.0, (U + U64) * f * (np.abs(gs) + b_gs))
        gz_hi = np.abs(self.gz) + b_gz
        # gk = gz q: one multiply
        self.gk = self.gz[:, :, None] * qe
        self.b_gk = (b_gz + (U + U64) * gz_hi)[:, :, None] * np.abs(qe)
        # gq = sum_e gz k: n products, n - 1 adds
        self.gq = _seg_sum(row, self.gz[:, :, None] * k, num_dst)
        self.b_gq = _seg_sum(row, b_gz[:, :, None] * np.abs(k), num_dst) + \
            (gamma(nd + 1) + _slack(nd)) * _seg_sum(row, gz_hi[:, :, None] * np.abs(k), num_dst)
        self.exact_z = exact_z

    def assert_clear_of_kink(self):
        """The precondition of every bound above: no score within KINK_MARGIN bounds of 0
        (with exact_z: the kernel's z is the reference's, zeros included)."""
        if not self.exact_z and self.z.size:
            assert (np.abs(self.z) >= KINK_MARGIN * self.bz).all(), \
                "a score lies within {} error bounds of the leaky-ReLU kink".format(KINK_MARGIN)

    def ratios(self, out=None, att=None, gq=None, gk=None, gv=None):
        """{name: max error / bound} of the results given."""
        got = dict(out=out, att=att, gq=gq, gk=gk, gv=gv)
        want = dict(out=(self.out, self.b_out), att=(self.att, self.b_att),
                    gq=(self.gq, self.b_gq), gk=(self.gk, self.b_gk), gv=(self.gv, self.b_gv))
        return {name: error_ratio(np.asarray(x).reshape(want[name][0].shape), *want[name])
                for name, x in got.items() if x is not None}


# ---- seeded inputs shared by the CPU and the GPU tests ---------------------------------------
def rows_of(degs):
    degs = np.asarray(degs, dtype=np.int64)
    return np.repeat(np.arange(len(degs)), degs).astype(np.int64)


def make_inputs(row, num_dst, H, D, seed, slope=0.2):
    """Standard-normal fp32 q, k, v, gout for the block `row`.  A score that lands within
    4 KINK_MARGIN bounds of the leaky-ReLU kink is moved off it along q (k += +-0.5 q / |q|^2,
    |z| becomes about 0.5), so that the precondition holds for every block, the sampler's
    included, whose edges are not known before the GPU run; the callers still assert it."""
    rng = np.random.RandomState(seed)
    row = np.asarray(row, dtype=np.int64)
    E = len(row)
    q = rng.randn(num_dst, H, D).astype(np.float32)
    k = rng.randn(E, H, D).astype(np.float32)
    v = rng.randn(E, H, D).astype(np.float32)
    gout = rng.randn(num_dst, H, D).astype(np.float32)
    if E:
        qe = q[row].astype(np.float64)
        z = (qe * k).sum(-1)
        near = np.abs(z) < 4 * KINK_MARGIN * gamma(D + 1) * np.abs(qe * k).sum(-1) + 1e-30
        push = np.where(z >= 0, 0.5, -0.5) / np.maximum((qe * qe).sum(-1), 1e-30)
        k = np.where(near[:, :, None], k + (push[:, :, None] * qe), k).astype(np.float32)
    return dict(row=row, num_dst=num_dst, q=q, k=k, v=v, gout=gout, slope=slope)


def reference(c, **kw):
    r = Reference(c["row"], c["num_dst"], c["q"], c["k"], c["v"], c["gout"], c["slope"], **kw)
    r.assert_clear_of_kink()
    return r


SHAPES = [(1, 1), (1, 63), (1, 64), (1, 65), (2, 50), (3, 21), (4, 33), (8, 16), (16, 64),
          (2, 129)]


def shape_case(H, D):
    """About 40 destinations of degree 0-12, zero-degree ones first, last and in between."""
    rng = np.random.RandomState(900 + 7 * H + D)
    degs = rng.randint(0, 13, 40)
    degs[[0, 17, 39]] = 0
    degs[[16, 18]] = [3, 12]
    return make_inputs(rows_of(degs), 40, H, D, 1000 + 7 * H + D)


def long_segment_case():
    """One 3000-edge segment among 60 segments of 1-10 edges."""
    degs = np.random.RandomState(910).randint(1, 11, 61)
    degs[23] = 3000
    return make_inputs(rows_of(degs), 61, 2, 50, 911)


def unordered_case():
    """The edges of shape_case(3, 21) in a shuffled order: a block that needs `perm`."""
    c = shape_case(3, 21)
    p = np.random.RandomState(920).permutation(len(c["row"]))
    return dict(c, row=c["row"][p], k=c["k"][p], v=c["v"][p])


def exact_zero_case():
    """q, k in {-2..2} with D = 6: every z is an exactly representable integer and about one in
    seven is 0, where the gradient must take the slope branch."""
    rng = np.random.RandomState(930)
    degs = rng.randint(0, 9, 50)
    row = rows_of(degs)
    c = make_inputs(row, 50, 3, 6, 931)
    c["q"] = rng.randint(-2, 3, c["q"].shape).astype(np.float32)
    c["k"] = rng.randint(-2, 3, c["k"].shape).astype(np.float32)
    return c
