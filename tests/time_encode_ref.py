"""Float64 reference of ops.time_encode_cat (csrc/time_encode.hip), a priori bounds on the error
of its fp32 kernels, and the seeded inputs that the CPU and GPU tests share.  Pure numpy.

    out[i]   = [a[i] | b[i] | cos(w * t[i] + bias)]
    gw[j]    = - sum_i g[i,j] sin(w[j] t[i] + bias[j]) t[i]        g = the time columns of gout
    gbias[j] = - sum_i g[i,j] sin(w[j] t[i] + bias[j])
    ga, gb   = the column slices of gout

The float64 side is evaluated on the same fp32 inputs.  u = 2^-24.  The library is built with
-ffp-contract=off and without fast-math, so the argument is one correctly rounded multiply and
one correctly rounded add, and sums are plain fp32 adds in some order.

Copied columns: a copy does not round.  Bit-equal.

Time columns.  The kernel's argument is x^ = fl(fl(w t) + b): the product is off by at most
u |w t|, and the sum adds at most u |fl(w t) + b|, which is u |w t + b| to first order, so

    delta = |x^ - (w t + b)| <= u (|w t| + |w t + b|).

cos is 1-Lipschitz, so that is also the distance of the exact cosines; on top comes the error
of cosf itself, for which OpenCL's bound for cos is 4 ulp, at |value| <= 1 at most 4 * 2^-23:

    |got - cos64(w t + b)| <= delta + 4 * 2^-23.

gw[j].  Each term g sin(x^) t has a sine that is off by at most delta + 4 * 2^-23 (same
argument, sin is 1-Lipschitz, the same 4 ulp), which |g t| carries into the term; the two
multiplies of a term and the n - 1 adds of the sum, in ANY order, cost at most (n + 1) u
relative to sum |terms| <= sum |g t| to first order, and (n + 3) u leaves two spare roundings
(the partial rows are summed by a second pass, the total is negated exactly):

    |gw^[j] - gw[j]| <= sum_i |g_ij t_i| (delta_ij + 4 * 2^-23) + (n + 3) u sum_i |g_ij t_i|.

gbias[j]: the same without t_i.
"""
import numpy as np

from tests.block_ops_ref import U, error_ratio  # noqa: F401  (re-exported)

COS_ULP4 = 4.0 * 2.0 ** -23


def tgat_frequencies(T):
    """TimeEncode's initial weight: 1 / 10^linspace(0, 9, T), fp32."""
    return (1 / 10 ** np.linspace(0, 9, T, dtype=np.float32)).astype(np.float32)


class Reference:
    """All float64 results and all bounds of one case, computed once and left unchanged."""

    def __init__(self, parts, t, w, bias, gout):
        parts = [np.asarray(p, dtype=np.float64) for p in parts]
        t = np.asarray(t, dtype=np.float64).reshape(-1)
        w = np.asarray(w, dtype=np.float64).reshape(-1)
        bias = np.asarray(bias, dtype=np.float64).reshape(-1)
        gout = np.asarray(gout, dtype=np.float64)
        n, T = len(t), len(w)
        assert len(bias) == T and all(p.shape[0] == n for p in parts)
        self.widths = [p.shape[1] for p in parts]
        self.offset = sum(self.widths)
        assert gout.shape == (n, self.offset + T)
        wt = t[:, None] * w[None, :]
        arg = wt + bias[None, :]
        self.delta = U * (np.abs(wt) + np.abs(arg))
        self.enc = np.cos(arg)
        self.b_enc = self.delta + COS_ULP4
        self.copied = np.concatenate(parts, axis=1) if parts else np.zeros((n, 0))
        self.out = np.concatenate([self.copied, self.enc], axis=1)
        g = gout[:, self.offset:]
        s = np.sin(arg)
        gt = g * t[:, None]
        self.gw = -(gt * s).sum(0)
        self.gbias = -(g * s).sum(0)
        self.b_gw = (np.abs(gt) * self.b_enc).sum(0) + (n + 3) * U * np.abs(gt).sum(0)
        self.b_gbias = (np.abs(g) * self.b_enc).sum(0) + (n + 3) * U * np.abs(g).sum(0)
        self.gparts, off = [], 0
        for width in self.widths:
            self.gparts.append(gout[:, off:off + width])
            off += width

    def copied_equal(self, out):
        """The copied columns of an fp32 result are bit-equal to the parts."""
        out = np.asarray(out)
        return out.shape == self.out.shape and \
            np.array_equal(out[:, :self.offset].astype(np.float64), self.copied)

    def ratios(self, out=None, gw=None, gbias=None):
        """{name: max error / bound} of the results given (out: the time columns only)."""
        r = {}
        if out is not None:
            r["enc"] = error_ratio(np.asarray(out)[:, self.offset:], self.enc, self.b_enc)
        if gw is not None:
            r["gw"] = error_ratio(np.asarray(gw).reshape(-1), self.gw, self.b_gw)
        if gbias is not None:
            r["gbias"] = error_ratio(np.asarray(gbias).reshape(-1), self.gbias, self.b_gbias)
        return r


# ---- seeded inputs shared by the CPU and the GPU tests ---------------------------------------
# (n, T, part widths, kind of t).  Every n of {1, 63, 64, 65, 257, 70 001}, every T of {1, 3, 4,
# 20, 100}, every width tuple of {(), (1,), (3,), (4,), (32,), (100, 16), (3, 5)} and every kind
# of t occur.  The 16-byte path needs every width and T a multiple of 4: it runs with no part,
# one part and two parts; all other cases take the scalar path, with a row pitch that is odd
# (rows misaligned from row 1 on, n > 1), or a multiple of 4 made of odd widths (3 + 5 + 100).
# T <= 32 and T > 32 are the backward's two lane layouts, T = 132 > 128 its column loop;
# n = 70 001 gives every backward workgroup several row passes.
CASES = [
    (1, 1, (), "unit"),
    (63, 3, (1,), "negative"),
    (64, 4, (4,), "unit"),
    (65, 20, (32,), "large"),
    (257, 100, (100, 16), "large"),
    (257, 100, (3, 5), "unit"),
    (65, 4, (3,), "zero"),
    (257, 20, (1,), "negative"),
    (64, 100, (), "zero"),
    (65, 132, (4,), "unit"),
    (70001, 100, (100, 16), "unit"),
    (70001, 3, (3, 5), "large"),
]


def case_id(case):
    n, T, widths, kind = case
    return "n{}_T{}_{}_{}".format(n, T, "x".join(map(str, widths)) or "none", kind)


def make_inputs(case, seed=None):
    """fp32 parts, t, w, bias and gout of a case.

    unit: t in [0, 1] (the sampler's dt); negative: t in [-2, 0]; zero: t = 0 (bias is not);
    large: t up to 1e4 with the TGAT frequencies (arguments up to 1e4 rad)."""
    n, T, widths, kind = case
    rng = np.random.RandomState(1000 + n + 7 * T + 31 * sum(widths) if seed is None else seed)
    parts = [rng.randn(n, width).astype(np.float32) for width in widths]
    if kind == "large":
        t = (rng.rand(n) * 1e4).astype(np.float32)
        w = tgat_frequencies(T)
        bias = (0.1 * rng.randn(T)).astype(np.float32)
    else:
        t = {"unit": rng.rand(n), "negative": -2 * rng.rand(n), "zero": np.zeros(n)}[kind]
        t = t.astype(np.float32)
        w = rng.randn(T).astype(np.float32)
        bias = rng.randn(T).astype(np.float32)
    gout = rng.randn(n, sum(widths) + T).astype(np.float32)
    return dict(parts=parts, t=t, w=w, bias=bias, gout=gout)


def reference(c):
    return Reference(c["parts"], c["t"], c["w"], c["bias"], c["gout"])


def emulate_fp32(c):
    """The kernels' arithmetic in numpy fp32: one multiply, one add, libm cos / sin of the fp32
    argument rounded to fp32, serial fp32 sums.  Stands in for the GPU in the CPU tests."""
    t, w, bias = c["t"], c["w"], c["bias"]
    arg = (t[:, None] * w[None, :]).astype(np.float32) + bias[None, :]
    assert arg.dtype == np.float32
    enc = np.cos(arg.astype(np.float64)).astype(np.float32)
    out = np.concatenate(list(c["parts"]) + [enc], axis=1)
    g = c["gout"][:, out.shape[1] - len(w):]
    p = g * np.sin(arg.astype(np.float64)).astype(np.float32)
    assert p.dtype == np.float32
    gbias = -np.cumsum(p, axis=0, dtype=np.float32)[-1]
    gw = -np.cumsum(p * t[:, None], axis=0, dtype=np.float32)[-1]
    return out, gw, gbias
