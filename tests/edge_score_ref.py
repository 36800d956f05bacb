"""Float64 reference of ops.edge_score (csrc/edge_score.hip), a priori bounds on the error of its
fp32 kernels, the seeded inputs that the CPU and GPU tests share, and the same for the whole
nn.EdgePredictor around it.  Pure numpy.

    x[j,d]    = src[j mod B, d] + dst[j, d]                    M = r B rows, m = (x > 0)
    out[j]    = bias + sum_d w[d] relu(x[j,d])
    gdst[j,d] = g[j] w[d] m[j,d]
    gsrc[i,d] = gdst[i,d] + gdst[i+B,d] + ... + gdst[i+(r-1)B,d]
    gw[d]     = sum_j g[j] relu(x[j,d])
    gbias     = sum_j g[j]

The float64 side is evaluated on the same fp32 inputs.  u = 2^-24, gamma_k = k u / (1 - k u).
The library is built with -ffp-contract=off and without fast-math, so every add and multiply is
one correctly rounded fp32 operation and sums are plain fp32 adds in some order; a sum of n
terms, each of which carries e roundings of its own, is within gamma_{n-1+e} sum |terms| of the
exact one in ANY order (Higham, Accuracy and Stability, 3.1 and 4.2).  None of the bounds below
therefore pins the kernels' layout.

Mask.  fl(s + p) = (s + p)(1 + e), |e| <= u, and an fp32 sum that falls below the normal range
is exact (every subnormal sum of two floats is representable), so fl(s + p) is positive exactly
when s + p is, and zero exactly when s + p is.  The mask of the kernels IS the exact mask.

gdst, gsrc.  With the exact mask, gdst is one rounded multiply fl(g w) or zero, and gsrc the r
blocks of it added one after the other in ascending order: a fixed fp32 expression, restated
here in numpy fp32 (`gdst32`, `gsrc32`).  The kernel must be BIT-EQUAL to it.

out[j].  relu(fl(x)) carries one rounding, the product with w a second, the D - 1 adds of the
D terms and the add of bias D more: D + 2 roundings on any path through the sum, and D + 3
leaves one spare:

    |out^[j] - out[j]| <= gamma_{D+3} (|bias| + sum_d |w_d| relu(x_jd)).

gw[d].  A term g relu(fl(x)) carries two roundings and the sum of M terms M - 1 more, however
the rows are cut into lanes, phases and partial rows; M + 2 leaves one spare:

    |gw^[d] - gw[d]| <= gamma_{M+2} sum_j |g_j| relu(x_jd).

gbias.  M - 1 adds of exact terms:  |gbias^ - gbias| <= gamma_M sum_j |g_j|.

The inputs are drawn (make_inputs) so that every product stays a normal fp32: all magnitudes of
src, dst, w, bias and g lie in [2^-3, 4] on a grid of 2^-12, so a non-zero x is at least 2^-12
and every product at least 2^-15.  Denormal handling does not enter the bounds.
"""
import numpy as np

from tests.block_ops_ref import U, error_ratio, gamma  # noqa: F401  (re-exported)


class Reference:
    """All float64 results and all bounds of one case, computed once and left unchanged."""

    def __init__(self, src, dst, w, bias, g):
        src32, dst32 = np.asarray(src, np.float32), np.asarray(dst, np.float32)
        w32 = np.asarray(w, np.float32).reshape(-1)
        g32 = np.asarray(g, np.float32).reshape(-1)
        src, dst, w, g = (a.astype(np.float64) for a in (src32, dst32, w32, g32))
        bias = float(np.asarray(bias, np.float32).reshape(-1)[0])
        (B, D), M = src.shape, dst.shape[0]
        assert dst.shape == (M, D) and w.shape == (D,) and g.shape == (M,)
        assert D >= 1 and (M % B == 0 if B else M == 0)
        r = M // B if B else 0
        self.B, self.D, self.M, self.r = B, D, M, r
        rows = np.arange(M) % max(B, 1)
        x = src[rows] + dst
        self.mask = x > 0
        relu = np.where(self.mask, x, 0.0)
        self.out = (bias + relu @ w).reshape(M, 1)
        self.b_out = (gamma(D + 3) * (abs(bias) + relu @ np.abs(w))).reshape(M, 1)
        self.gdst = g[:, None] * w[None, :] * self.mask
        self.gsrc = self.gdst.reshape(r, B, D).sum(0) if M else np.zeros((B, D))
        self.gw = (g[:, None] * relu).sum(0)
        self.b_gw = gamma(M + 2) * (np.abs(g)[:, None] * relu).sum(0)
        self.gbias = np.array([g.sum()])
        self.b_gbias = np.array([gamma(M) * np.abs(g).sum()])
        # the fp32 restatement of gdst and gsrc: one multiply, the mask, sequential adds
        prod = g32[:, None] * w32[None, :]
        assert prod.dtype == np.float32
        self.mask32 = (src32[rows] + dst32) > 0
        self.gdst32 = np.where(self.mask, prod, np.float32(0))
        acc = np.zeros((B, D), np.float32)
        for k in range(r):
            acc = acc + self.gdst32[k * B:(k + 1) * B]
        assert acc.dtype == np.float32 and self.gdst32.dtype == np.float32
        self.gsrc32 = acc

    def exact_equal(self, gsrc=None, gdst=None):
        """The fp32 gsrc / gdst given are bit-equal to the restatement (as values: -0 == 0)."""
        ok = True
        if gsrc is not None:
            gsrc = np.asarray(gsrc)
            ok = ok and gsrc.dtype == np.float32 and np.array_equal(gsrc, self.gsrc32)
        if gdst is not None:
            gdst = np.asarray(gdst)
            ok = ok and gdst.dtype == np.float32 and np.array_equal(gdst, self.gdst32)
        return ok

    def ratios(self, out=None, gw=None, gbias=None, scale=1.0):
        """{name: max error / (scale x bound)} of the results given."""
        r = {}
        if out is not None:
            r["out"] = error_ratio(np.asarray(out).reshape(-1, 1), self.out, scale * self.b_out)
        if gw is not None:
            r["gw"] = error_ratio(np.asarray(gw).reshape(-1), self.gw, scale * self.b_gw)
        if gbias is not None:
            r["gbias"] = error_ratio(np.asarray(gbias).reshape(-1), self.gbias,
                                     scale * self.b_gbias)
        return r


# ---- seeded inputs shared by the CPU and the GPU tests ---------------------------------------
# (B, D, r).  Every B of {1, 3, 15, 16, 17, 63, 64, 65, 600} (around the forward's 16-row
# workgroup, the backward's 8-row groups and a wave), every D of {1, 3, 4, 100, 128, 172, 257}
# (scalar path: 1, 3, 257; 16-byte path: 4, 100, 128, 172; one pass of the 16 lanes x 4 columns
# is 64 columns, so 100, 128, 172 and 257 take 2, 2, 3 and 5 passes; the backward has 32 lanes
# over the columns up to D = 31 and 64 beyond, 1 to 5 passes) and every r of {1, 2, 3} occur,
# the boundary values of B paired with the boundary values of D.  TALL has more src rows than
# 1024 groups of 8, so the partial rows reach their cap and every backward workgroup owns 69 rows.
CASES = [
    (1, 1, 1), (1, 4, 2), (3, 3, 3), (15, 100, 2), (16, 128, 1), (17, 172, 3), (63, 257, 2),
    (64, 4, 3), (65, 3, 1), (15, 128, 3), (16, 257, 2), (17, 100, 1), (63, 172, 1), (64, 1, 2),
    (65, 128, 3), (600, 100, 2), (600, 172, 2), (600, 257, 3),
]
TALL = (70001, 8, 1)


def case_id(case):
    return "B{}_D{}_r{}".format(*case)


def _draw(rng, *shape):
    """Signed magnitudes in [2^-3, 4] on a grid of 2^-12, fp32."""
    mag = rng.randint(1 << 9, (1 << 14) + 1, size=shape).astype(np.float64) / (1 << 12)
    return (mag * rng.choice([-1.0, 1.0], size=shape)).astype(np.float32)


def make_inputs(case, seed=None):
    """fp32 src [B, D], dst [r B, D], w [D], bias [1] and g [r B] of a case.  One entry in 16 of
    dst is the negative of its src entry: x = 0 exactly, where the mask is off."""
    B, D, r = case
    rng = np.random.RandomState(2000 + B + 7 * D + 31 * r if seed is None else seed)
    src, dst = _draw(rng, B, D), _draw(rng, r * B, D)
    cancel = rng.randint(0, 16, size=dst.shape) == 0
    dst = np.where(cancel, -src[np.arange(r * B) % B], dst).astype(np.float32)
    return dict(src=src, dst=dst, w=_draw(rng, D), bias=_draw(rng, 1), g=_draw(rng, r * B))


def reference(c):
    return Reference(c["src"], c["dst"], c["w"], c["bias"], c["g"])


def emulate_fp32(c):
    """The kernels' arithmetic in numpy fp32 with serial sums -> (out, gsrc, gdst, gw, gbias).
    Stands in for the GPU in the CPU tests."""
    src, dst, w, bias, g = c["src"], c["dst"], c["w"], c["bias"], c["g"]
    (B, D), M = src.shape, dst.shape[0]
    x = src[np.arange(M) % B] + dst
    relu = np.where(x > 0, x, np.float32(0))
    assert relu.dtype == np.float32
    out = np.cumsum(w[None, :] * relu, axis=1, dtype=np.float32)[:, -1] + bias[0]
    gdst = np.where(x > 0, g[:, None] * w[None, :], np.float32(0))
    gsrc = np.zeros((B, D), np.float32)
    for k in range(M // B):
        gsrc = gsrc + gdst[k * B:(k + 1) * B]
    gw = np.cumsum(g[:, None] * relu, axis=0, dtype=np.float32)[-1]
    gbias = np.cumsum(g, dtype=np.float32)[-1:]
    assert out.dtype == gw.dtype == gbias.dtype == np.float32
    return out.reshape(M, 1), gsrc, gdst, gw, gbias


# ---- the whole EdgePredictor ------------------------------------------------------------------
class PredictorReference:
    """nn.EdgePredictor in float64 from a state dict {src_fc,dst_fc,out_fc}.{weight,bias} and
    h [3 B, K], with the gradients of sum(G * [pos; neg]) and a priori bounds on what an fp32
    evaluation (two Linear layers by any GEMM, then ops.edge_score or its torch expression) may
    differ by.  The bounds are those of ops.edge_score above, propagated through the Linears:

    A Linear is K products and K adds per element (the bias included), in any order:
        ds = gamma_{K+1} (|h| |W|^T + |b|)        the same for dd.
    relu is 1-Lipschitz, so the edge score sees x off by at most dx = ds + dd, and
        b_out = gamma_{D+3} (|bias| + sum_d |w_d| relu(x)) + sum_d |w_d| dx.
    No x of the case may lie within 4 dx of zero (`mask_is_stable`, asserted by the tests that
    use the bounds): then every fp32 evaluation has the mask of the exact one, the gradients are
    sums of products of the inputs, and a sum of n products whose factors carry e roundings is
    within gamma_{n+e} of sum |products|.  With gd = g w m (1 rounding) and gs = the r = 2 blocks
    of gd added (2 roundings):
        out_fc.weight   gamma_{M+2} sum_j |g| relu(x) + sum_j |g| dx
        out_fc.bias     gamma_M sum_j |g|
        dst_fc.weight   gamma_{M+2} |gd|^T |h_dst|          dst_fc.bias   gamma_{M+1} sum_j |gd|
        src_fc.weight   gamma_{B+3} |gs|^T |h_src|          src_fc.bias   gamma_{B+2} sum_i |gs|
        h               gamma_{D+3} |gs| |W_src|  and  gamma_{D+2} |gd| |W_dst|
    where |gs| stands for the sum of the blocks' |gd|."""

    def __init__(self, state, h, G):
        p = {k: np.asarray(v, np.float32).astype(np.float64) for k, v in state.items()}
        h = np.asarray(h, np.float32).astype(np.float64)
        G = np.asarray(G, np.float64).reshape(-1)
        Ws, bs, Wd, bd = (p[k] for k in ("src_fc.weight", "src_fc.bias", "dst_fc.weight",
                                         "dst_fc.bias"))
        w, bias = p["out_fc.weight"].reshape(-1), float(p["out_fc.bias"].reshape(-1)[0])
        n, K = h.shape
        assert n % 3 == 0 and G.shape == (2 * n // 3,)
        B, D, M = n // 3, len(w), 2 * n // 3
        hs, hd = h[:B], h[B:]
        s, d = hs @ Ws.T + bs, hd @ Wd.T + bd
        ds = gamma(K + 1) * (np.abs(hs) @ np.abs(Ws).T + np.abs(bs))
        dd = gamma(K + 1) * (np.abs(hd) @ np.abs(Wd).T + np.abs(bd))
        rows = np.arange(M) % B
        x, dx = s[rows] + d, ds[rows] + dd
        self.mask_is_stable = bool((np.abs(x) > 4 * dx).all())
        mask = x > 0
        relu = np.where(mask, x, 0.0)
        out = bias + relu @ w
        b_out = gamma(D + 3) * (abs(bias) + relu @ np.abs(w)) + dx @ np.abs(w)
        self.pos, self.neg = out[:B].reshape(B, 1), out[B:].reshape(B, 1)
        self.b_pos, self.b_neg = b_out[:B].reshape(B, 1), b_out[B:].reshape(B, 1)
        gd = G[:, None] * w[None, :] * mask
        gs = gd[:B] + gd[B:]
        agd = np.abs(gd)
        ags = agd[:B] + agd[B:]
        aG = np.abs(G)[:, None]
        self.grads = {
            "h": np.concatenate([gs @ Ws, gd @ Wd]),
            "src_fc.weight": gs.T @ hs, "src_fc.bias": gs.sum(0),
            "dst_fc.weight": gd.T @ hd, "dst_fc.bias": gd.sum(0),
            "out_fc.weight": (G[:, None] * relu).sum(0).reshape(1, D),
            "out_fc.bias": np.array([G.sum()]),
        }
        self.bounds = {
            "h": np.concatenate([gamma(D + 3) * (ags @ np.abs(Ws)),
                                 gamma(D + 2) * (agd @ np.abs(Wd))]),
            "src_fc.weight": gamma(B + 3) * (ags.T @ np.abs(hs)),
            "src_fc.bias": gamma(B + 2) * ags.sum(0),
            "dst_fc.weight": gamma(M + 2) * (agd.T @ np.abs(hd)),
            "dst_fc.bias": gamma(M + 1) * agd.sum(0),
            "out_fc.weight": (gamma(M + 2) * (aG * relu).sum(0) + (aG * dx).sum(0)).reshape(1, D),
            "out_fc.bias": np.array([gamma(M) * np.abs(G).sum()]),
        }

    def ratios(self, pos, neg, grads, scale=1.0):
        """{name: max error / (scale x bound)} of an fp32 evaluation."""
        r = {"pos": error_ratio(pos, self.pos, scale * self.b_pos),
             "neg": error_ratio(neg, self.neg, scale * self.b_neg)}
        for k, v in grads.items():
            r[k] = error_ratio(v, self.grads[k], scale * self.bounds[k])
        return r
