"""Float64 reference of ops.block_attention with attention dropout (the *_dropout kernels of
csrc/block_attention.hip), the exact mask it draws, and a priori bounds on the error of its fp32
kernels.  Pure numpy, built on tests/block_attention_ref.py (imported, unchanged).

The mask, for p = float32(dropout_p), a 64-bit seed, H heads and i the position of an edge in
the GROUPED order the kernel sees (stable sort of `row`):

    T          = uint32(float64(p) * 2^32)
    keep[i,h]  = gf_philox4x32_10_first(seed, i * H + h, 0) >= T      (include/gnnflow_rng.h)
    w[i,h]     = keep ? 1 / (1 - p) : 0
    out[d,h,c] = sum_e (a[e,h] w[e,h]) v[e,h,c]                        a: the softmax, as before
    ga = w (gout . v)    gv = (a w) gout    dot = sum_e a ga    gs = a (ga - dot)    gz, gq, gk as before

The reference takes w with the TRUE 1 / (1 - p) in float64; the kernels multiply by
sc = fl32(1 / (1 - p)).  delta = |sc - 1 / (1 - p)| is taken exactly from the two float64 values,
not bounded.  Bounds, derived as in the parent file (first order in u, |x| + bound(x) where a
perturbed x is multiplied; K = keep as 0 / 1; b_att and a_hi = a + b_att from the parent):

    aw = a w    kernel fl(a^ sc): the error of a times sc, delta times a, one rounding
                b_aw = K (b_att sc + a delta + u (a_hi sc))
    out         kernel sums the nk KEPT edges only (a dropped edge is skipped, exactly 0):
                sum b_aw |v| + gamma_{nk+1} sum (aw + b_aw) |v|
    ga_d        = gout . v as the parent's ga: b_gad = gamma_{D+1} sum |gout v|
    ga = w ga_d kernel fl(sc ga_d^): b_ga = K (sc b_gad + delta |ga_d| + u sc (|ga_d| + b_gad))
    gv          kernel fl(fl(a^ sc) gout): (b_aw + u (aw + b_aw)) |gout|; 0 where dropped
    dot         nk products and nk - 1 adds of perturbed factors (dropped edges add nothing):
                sum (b_att |ga| + a_hi b_ga) + gamma_{nk+1} sum a_hi (|ga| + b_ga)
    gs, gz, gk, gq   the parent's formulas on this ga and dot (a dropped edge has ga = 0 exactly
                and still takes -a dot)

Where the bound of an element is 0 (att_dropped and gv of a dropped edge, every result of a
destination whose edges are all dropped ...) error_ratio demands the exact value.  With p = 0:
sc = 1, delta = 0, K = 1, every value equals the parent Reference's and every bound is the
parent's plus the one extra rounding.
"""
import numpy as np

from tests import block_attention_ref as A
from tests.block_attention_ref import U, U64, _seg_sum, _slack, error_ratio, gamma

M32 = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)


def philox_first(seed, tid, call=0):
    """gf_philox4x32_10_first of include/gnnflow_rng.h in uint64 arithmetic; seed, tid and call
    are integers below 2^64 or arrays of them (broadcast).  Returns uint32."""
    seed, tid, call = (np.asarray(x, dtype=np.uint64) for x in (seed, tid, call))
    seed, tid, call = np.broadcast_arrays(seed, tid, call)
    c0, c1 = tid & M32, tid >> S32
    c2, c3 = call & M32, call >> S32
    k0, k1 = seed & M32, seed >> S32
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c0          # both factors below 2^32: no wrap
        p1 = np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> S32) ^ c1 ^ k0, p1 & M32, (p0 >> S32) ^ c3 ^ k1, p0 & M32
        k0 = (k0 + np.uint64(0x9E3779B9)) & M32
        k1 = (k1 + np.uint64(0xBB67AE85)) & M32
    return c0.astype(np.uint32)


def threshold(p):
    """T: an edge is kept when its draw is >= T."""
    p = np.float32(p)
    assert 0 <= p < 1
    return int(float(p) * 4294967296.0)


def scale(p):
    """The kernels' fp32 constant 1.0f / (1.0f - p)."""
    return np.float32(1) / (np.float32(1) - np.float32(p))


def keep_mask(E, H, p, seed):
    """bool [E, H], indexed by the edge's position in the grouped order."""
    u = philox_first(seed, np.arange(E * H, dtype=np.uint64), 0)
    return (u >= np.uint32(min(threshold(p), 0xFFFFFFFF))).reshape(E, H)


def grouped_position(row):
    """Position of each edge in the grouped order: its rank in the stable sort of `row`."""
    row = np.asarray(row, dtype=np.int64).reshape(-1)
    rank = np.empty(len(row), np.int64)
    rank[np.argsort(row, kind="stable")] = np.arange(len(row))
    return rank


class DropoutReference:
    """All float64 results and bounds of one case with the mask of (p, seed) applied; computed
    once and left unchanged.  `keep` is in the caller's edge order."""

    def __init__(self, row, num_dst, q, k, v, gout, slope=0.2, p=0.0, seed=0, exact_z=False):
        base = A.Reference(row, num_dst, q, k, v, gout, slope, exact_z=exact_z)
        self.base = base
        row = base.row
        q, k, v, g = A._f64(q, k, v, gout)
        E, H, D = k.shape
        self.row, self.num_dst, self.slope, self.exact_z = row, num_dst, base.slope, exact_z
        self.z, self.bz = base.z, base.bz
        self.p, self.seed = float(np.float32(p)), int(seed)
        self.keep = keep_mask(E, H, p, seed)[grouped_position(row)]
        sc = float(scale(p))
        true = 1.0 / (1.0 - self.p)
        delta = abs(sc - true)
        self.scale, self.delta = sc, delta
        K = self.keep.astype(np.float64)
        W = K * true
        att, b_att = base.att, base.b_att
        a_hi = att + b_att
        self.att, self.b_att = att, b_att
        qe, ge = q[row], g[row]
        nk = _seg_sum(row, K, num_dst)                       # [num_dst, H] kept edges
        nke = nk[row]

        # ---- forward -----------------------------------------------------------------------
        self.att_dropped = att * W
        b_aw = K * (b_att * sc + att * delta + (U + U64) * a_hi * sc)
        self.b_att_dropped = b_aw
        aw_hi = self.att_dropped + b_aw
        self.out = _seg_sum(row, self.att_dropped[:, :, None] * v, num_dst)
        self.b_out = _seg_sum(row, b_aw[:, :, None] * np.abs(v), num_dst) + \
            (gamma(nk + 1) + _slack(nk))[:, :, None] * \
            _seg_sum(row, aw_hi[:, :, None] * np.abs(v), num_dst)

        # ---- backward ----------------------------------------------------------------------
        ga_d = (ge * v).sum(-1)
        b_gad = (gamma(D + 1) + _slack(D)) * np.abs(ge * v).sum(-1)
        ga = W * ga_d
        b_ga = K * (sc * b_gad + delta * np.abs(ga_d) + (U + U64) * sc * (np.abs(ga_d) + b_gad))
        self.gv = self.att_dropped[:, :, None] * ge
        self.b_gv = (b_aw + (U + U64) * aw_hi)[:, :, None] * np.abs(ge)
        ga_hi = np.abs(ga) + b_ga
        dot = _seg_sum(row, att * ga, num_dst)[row]
        per_dst = _seg_sum(row, b_att * np.abs(ga) + a_hi * b_ga, num_dst)
        b_dot = per_dst[row] + (gamma(nke + 1) + _slack(nke)) * \
            _seg_sum(row, a_hi * ga_hi, num_dst)[row]
        tt = ga - dot
        b_tt = b_ga + b_dot + U * (np.abs(tt) + b_ga + b_dot)
        gs = att * tt
        b_gs = b_att * (np.abs(tt) + b_tt) + att * b_tt + (U + U64) * a_hi * (np.abs(tt) + b_tt)
        pos = base.z > 0
        f = np.where(pos, 1.0, abs(base.slope))
        self.gz = gs * np.where(pos, 1.0, base.slope)
        b_gz = f * b_gs + np.where(pos, 0.0, (U + U64) * f * (np.abs(gs) + b_gs))
        gz_hi = np.abs(self.gz) + b_gz
        self.gk = self.gz[:, :, None] * qe
        self.b_gk = (b_gz + (U + U64) * gz_hi)[:, :, None] * np.abs(qe)
        nd = np.bincount(row, minlength=num_dst)[:, None, None].astype(np.float64)
        self.gq = _seg_sum(row, self.gz[:, :, None] * k, num_dst)
        self.b_gq = _seg_sum(row, b_gz[:, :, None] * np.abs(k), num_dst) + \
            (gamma(nd + 1) + _slack(nd)) * _seg_sum(row, gz_hi[:, :, None] * np.abs(k), num_dst)

    def assert_clear_of_kink(self):
        self.base.assert_clear_of_kink()

    def ratios(self, out=None, att=None, att_dropped=None, gq=None, gk=None, gv=None):
        """{name: max error / bound} of the results given (att: the pre-dropout softmax)."""
        got = dict(out=out, att=att, att_dropped=att_dropped, gq=gq, gk=gk, gv=gv)
        want = dict(out=(self.out, self.b_out), att=(self.att, self.b_att),
                    att_dropped=(self.att_dropped, self.b_att_dropped),
                    gq=(self.gq, self.b_gq), gk=(self.gk, self.b_gk), gv=(self.gv, self.b_gv))
        return {name: error_ratio(np.asarray(x).reshape(want[name][0].shape), *want[name])
                for name, x in got.items() if x is not None}


def reference(c, p, seed, **kw):
    r = DropoutReference(c["row"], c["num_dst"], c["q"], c["k"], c["v"], c["gout"], c["slope"],
                         p=p, seed=seed, **kw)
    r.assert_clear_of_kink()
    return r


# ---- the (p, seed) pairs of the GPU tests; tests/test_attention_dropout_ref.py checks on the CPU
# that each mask keeps a fraction within 4 sqrt(p (1 - p) / n) of 1 - p -------------------------
SEED = 0x5EEDC0FFEE123457          # above 2^32: both key words of the generator are in play
SEED_B = 977
P_EXACT = (0.1, 0.5, 0.9)
P = 0.5
NC_SHAPE = (2, 129)                # the A.SHAPES entry with more than 128 columns: NC = 4
HEAD_SHAPES = [(1, 1), (1, 63), (1, 64), (1, 65), (3, 21), (8, 16), NC_SHAPE]
DEGENERATE = [[], [0], [0] * 5, [1] * 9, [4, 0, 7]]
ALL_DROPPED_DEGS = [2, 3, 2, 3, 1, 2, 3, 2]     # test 3: a degree-2 or -3 segment loses every edge


def degenerate_case(degs):
    row = A.rows_of(degs)
    return A.make_inputs(row, len(degs), 2, 5, 960 + len(degs))


def all_dropped_case():
    return A.make_inputs(A.rows_of(ALL_DROPPED_DEGS), len(ALL_DROPPED_DEGS), 2, 5, 975)


def find_all_dropped_seed(degs, H, p, limit=4096):
    """The first seed whose mask drops every edge of some (segment of degree 2 or 3, head)."""
    degs = np.asarray(degs)
    row = A.rows_of(degs)
    for seed in range(limit):
        kept = _seg_sum(row, keep_mask(len(row), H, p, seed).astype(np.float64), len(degs))
        if ((kept == 0) & (degs[:, None] >= 2)).any():
            return seed
    raise AssertionError("no seed below {} drops a whole segment".format(limit))


ALL_DROPPED_SEED = 0               # asserted equal to find_all_dropped_seed(...) on the CPU
