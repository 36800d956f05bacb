"""Float64 reference of ops.block_gat (csrc/block_gat.hip), the exact dropout mask it draws, a
priori bounds on the error of its fp32 kernels, and the seeded inputs that the CPU and GPU tests
share.  Pure numpy.

    z[e,h] = el[col[e],h] + er[row[e],h]       s = z > 0 ? z : slope z
    a      = softmax of s over the edges that share a destination
    out[d,h,c] = sum_e (a[e,h] w[e,h]) feat[col[e],h,c]           w = 1 without dropout
    gfeat[col[e]] += (a w) gout[row[e]]     ga = w (gout[row[e]] . feat[col[e]])
    dot = sum_e a ga     gs = a (ga - dot)     gz = gs (z > 0 ? 1 : slope)
    gel[col[e]] += gz    ger[d] = sum_e gz

`col` and `row` are taken as given (any order, repeated sources); no layout is assumed.  The mask
is that of tests/attention_dropout_ref.py (keep_mask, indexed by the edge's position in the
stable sort of `row`), computed on the CPU from the numpy Philox there.

Bounds.  u, gamma_k and the float64 slack are those of tests/block_ops_ref.py, and so is the
argument that they hold for ANY summation order (no contraction, no fast-math; adding an exact
zero is exact), which covers the atomic accumulation of the explicit-col path.  All are first
order in u with |x| + bound(x) wherever a perturbed x is multiplied.

    z       ONE fp32 add of two inputs: bound(z) = u |z|.  The computed z has the sign of the
            true z and is 0 exactly when it is, so the kernel and the reference always take the
            same leaky-ReLU branch; the seeded inputs still assert |z| >= KINK_MARGIN bound(z)
            (that is z != 0) and the exact-integer case has z == 0 on some edges.
    s, a    as tests/block_attention_ref.py: bs from bz, the softmax perturbation
            expm1(bs_k + max bs), the two-pass __expf evaluation t_k = u (3 |s_k - m| + 2), its
            weighted mean, (n + 1) u for the sum and 1 / sum, and 2^-126 for flushed terms.
    a w     p = 0: a itself.  Else as attention_dropout_ref: K (b_att sc + a delta + u a_hi sc)
            with sc = fl32(1 / (1 - p)) and delta = |sc - 1 / (1 - p)| taken exactly.
    out     the nk kept edges only: sum b_aw |f| + gamma_{nk+1} sum (aw + b_aw) |f|
    gfeat   per edge t = fl(aw^ gout): b_t = (b_aw + u aw_hi) |gout|; a source row read by m edges
            sums m terms with m - 1 adds: sum b_t + gamma_{m-1} sum (|t| + b_t); m = 0: exactly 0
    ga      gout . feat: gamma_{D+1} sum |gout f|, times w as attention_dropout_ref
    dot     the kernel may sum a ga over the edges (two sweeps) or, as csrc/block_gat.hip does,
            take gout[d] . out^[d] from the saved forward output (the two are equal in exact
            arithmetic, with dropout too).  Neither scheme's bound dominates the other, so b_dot
            is the LARGER of
              sweep    sum (b_att |ga| + a_hi b_ga) + gamma_{nk+1} sum a_hi (|ga| + b_ga)
              via out  sum_c |gout_c| b_out_c + gamma_{D+1} sum_c |gout_c| (|out_c| + b_out_c)
    gs, gz  the parent's formulas on this ga and dot
    gel     as gfeat with the terms gz:  sum b_gz + gamma_{m-1} sum (|gz| + b_gz)
    ger     n terms, n - 1 adds: sum b_gz + gamma_n sum (|gz| + b_gz)
"""
import numpy as np

from tests import attention_dropout_ref as R
from tests.block_attention_ref import KINK_MARGIN, TINY, U64, _f64, _seg_max, _seg_sum, rows_of
from tests.block_ops_ref import U, _layout, _slack, error_ratio, gamma  # noqa: F401

__all__ = ["Reference", "reference", "KINK_MARGIN"]


def _src_sum(col, values, num_src):
    out = np.zeros((num_src,) + values.shape[1:])
    np.add.at(out, col, values)
    return out


class Reference:
    """All float64 results and all bounds of one case, computed once and left unchanged.
    `keep` is in the caller's edge order.  exact_z: the caller vouches that el and er are small
    integers (checked), so z is exact in fp32 and z == 0 may occur."""

    def __init__(self, col, row, num_dst, num_src, feat, el, er, gout, slope=0.2, p=0.0, seed=0,
                 exact_z=False):
        col, row = _layout(col, row, num_dst, num_src)
        feat, el, er, g = _f64(feat, el, er, gout)
        E = len(row)
        _, H, D = feat.shape
        assert feat.shape[0] == num_src and el.shape == (num_src, H)
        assert er.shape == (num_dst, H) and g.shape == (num_dst, H, D)
        slope = float(np.float32(slope))            # the kernel's fp32 constant
        self.col, self.row, self.num_dst, self.num_src = col, row, num_dst, num_src
        self.slope, self.exact_z = slope, exact_z
        n = np.bincount(row, minlength=num_dst)[row][:, None].astype(np.float64)   # [E, 1]
        fe, ge = feat[col], g[row]

        # ---- forward: z, s, a -----------------------------------------------------------------
        self.z = el[col] + er[row]
        if exact_z:
            assert np.array_equal(el, np.round(el)) and np.array_equal(er, np.round(er))
            assert max(np.abs(el).max(initial=0), np.abs(er).max(initial=0)) < 2 ** 20
            self.bz = np.zeros_like(self.z)
        else:
            self.bz = (U + 2 * U64) * np.abs(self.z)
        pos = self.z > 0
        f = np.where(pos, 1.0, abs(slope))
        self.s = np.where(pos, self.z, slope * self.z)
        bs = f * self.bz + np.where(pos, 0.0, U * (np.abs(self.s) + f * self.bz))
        m = _seg_max(row, self.s, num_dst)[row] if E else self.s
        ex = np.exp(self.s - m)
        self.att = ex / _seg_sum(row, ex, num_dst)[row] if E else ex
        bsmax = _seg_max(row, bs, num_dst)[row] if E else bs
        pert = np.expm1(bs + bsmax)
        t = U * (3.0 * (np.abs(self.s - m) + 2.0 * bsmax) + 2.0)
        fp = t + (_seg_sum(row, self.att * t, num_dst)[row] if E else t) + (n + 1) * U + _slack(n)
        self.b_att = self.att * (pert + fp * (1.0 + pert)) + TINY
        att, b_att = self.att, self.b_att
        a_hi = att + b_att

        # ---- the mask ---------------------------------------------------------------------------
        self.p, self.seed = float(np.float32(p)), int(seed)
        self.keep = R.keep_mask(E, H, p, seed)[R.grouped_position(row)] if E else \
            np.ones((0, H), bool)
        sc = float(R.scale(p))
        true = 1.0 / (1.0 - self.p)
        delta = abs(sc - true)
        self.scale, self.delta = sc, delta
        K = self.keep.astype(np.float64)
        W = K * true
        nk = _seg_sum(row, K, num_dst)                       # [num_dst, H] kept edges
        nke = nk[row]

        # ---- forward: out -----------------------------------------------------------------------
        self.att_dropped = att * W
        if self.p == 0:
            b_aw = b_att
        else:
            b_aw = K * (b_att * sc + att * delta + (U + U64) * a_hi * sc)
        self.b_att_dropped = b_aw
        aw_hi = self.att_dropped + b_aw
        self.out = _seg_sum(row, self.att_dropped[:, :, None] * fe, num_dst)
        self.b_out = _seg_sum(row, b_aw[:, :, None] * np.abs(fe), num_dst) + \
            (gamma(nk + 1) + _slack(nk))[:, :, None] * \
            _seg_sum(row, aw_hi[:, :, None] * np.abs(fe), num_dst)

        # ---- backward -------------------------------------------------------------------------
        mcol = np.bincount(col, minlength=num_src).astype(np.float64)     # edges reading a row
        acc = gamma(np.maximum(mcol - 1, 0)) + np.where(mcol > 1, _slack(mcol), 0.0)
        term = self.att_dropped[:, :, None] * ge
        b_term = (b_aw + (U + U64) * aw_hi)[:, :, None] * np.abs(ge)
        self.gfeat = _src_sum(col, term, num_src)
        self.b_gfeat = _src_sum(col, b_term, num_src) + \
            acc[:, None, None] * _src_sum(col, np.abs(term) + b_term, num_src)

        ga_d = (ge * fe).sum(-1)
        b_gad = (gamma(D + 1) + _slack(D)) * np.abs(ge * fe).sum(-1)
        ga = W * ga_d
        if self.p == 0:
            b_ga = b_gad
        else:
            b_ga = K * (sc * b_gad + delta * np.abs(ga_d) +
                        (U + U64) * sc * (np.abs(ga_d) + b_gad))
        ga_hi = np.abs(ga) + b_ga
        dot = _seg_sum(row, att * ga, num_dst)[row] if E else ga
        sweep = _seg_sum(row, b_att * np.abs(ga) + a_hi * b_ga, num_dst) + \
            (gamma(nk + 1) + _slack(nk)) * _seg_sum(row, a_hi * ga_hi, num_dst)
        via_out = (np.abs(g) * self.b_out).sum(-1) + \
            (gamma(D + 1) + _slack(D)) * (np.abs(g) * (np.abs(self.out) + self.b_out)).sum(-1)
        b_dot = np.maximum(sweep, via_out)[row] if E else ga
        tt = ga - dot
        b_tt = b_ga + b_dot + U * (np.abs(tt) + b_ga + b_dot)
        gs = att * tt
        b_gs = b_att * (np.abs(tt) + b_tt) + att * b_tt + (U + U64) * a_hi * (np.abs(tt) + b_tt)
        self.gz = gs * np.where(pos, 1.0, slope)
        b_gz = f * b_gs + np.where(pos, 0.0, (U + U64) * f * (np.abs(gs) + b_gs))
        gz_hi = np.abs(self.gz) + b_gz
        self.gel = _src_sum(col, self.gz, num_src)
        self.b_gel = _src_sum(col, b_gz, num_src) + acc[:, None] * _src_sum(col, gz_hi, num_src)
        nd = np.bincount(row, minlength=num_dst)[:, None].astype(np.float64)
        self.ger = _seg_sum(row, self.gz, num_dst)
        self.b_ger = _seg_sum(row, b_gz, num_dst) + \
            (gamma(nd) + _slack(nd)) * _seg_sum(row, gz_hi, num_dst)
        self.unread = mcol == 0                      # source rows no edge reads

    def assert_clear_of_kink(self):
        """The precondition: |z| >= KINK_MARGIN bound(z), which with bound(z) = u |z| says that
        no score is 0 (with exact_z the kernel's z is the reference's, zeros included)."""
        if not self.exact_z and self.z.size:
            assert (np.abs(self.z) >= KINK_MARGIN * self.bz).all() and (self.z != 0).all(), \
                "a score lies on the leaky-ReLU kink"

    def ratios(self, out=None, att=None, att_dropped=None, gfeat=None, gel=None, ger=None):
        """{name: max error / bound} of the results given (att: the pre-dropout softmax)."""
        got = dict(out=out, att=att, att_dropped=att_dropped, gfeat=gfeat, gel=gel, ger=ger)
        want = dict(out=(self.out, self.b_out), att=(self.att, self.b_att),
                    att_dropped=(self.att_dropped, self.b_att_dropped),
                    gfeat=(self.gfeat, self.b_gfeat), gel=(self.gel, self.b_gel),
                    ger=(self.ger, self.b_ger))
        return {name: error_ratio(np.asarray(x).reshape(want[name][0].shape), *want[name])
                for name, x in got.items() if x is not None}


def reference(c, p=0.0, seed=0, **kw):
    r = Reference(c["col"], c["row"], c["num_dst"], c["num_src"], c["feat"], c["el"], c["er"],
                  c["gout"], c["slope"], p=p, seed=seed, **kw)
    r.assert_clear_of_kink()
    return r


# ---- seeded inputs shared by the CPU and the GPU tests ---------------------------------------
SEED = R.SEED                      # above 2^32: both key words of the generator are in play
SEED_B = R.SEED_B
PS = (0.2, 0.5)
NUM_DST = 7
# every group width (8, 16, 32, 64) and NC = 2, 8, 16
HEAD_SHAPES = [(1, 1), (3, 5), (8, 8), (2, 16), (2, 17), (1, 64), (2, 100), (1, 300), (1, 1024)]
DEGENERATE = [[], [0], [0] * 5, [1] * 9, [4, 0, 7]]


def make_inputs(col, row, num_dst, num_src, H, D, seed, slope=0.2):
    """Standard-normal fp32 feat, el, er, gout for the block (col, row)."""
    rng = np.random.RandomState(seed)
    return dict(col=np.asarray(col, np.int64), row=np.asarray(row, np.int64), num_dst=num_dst,
                num_src=num_src, slope=slope,
                feat=rng.randn(num_src, H, D).astype(np.float32),
                el=rng.randn(num_src, H).astype(np.float32),
                er=rng.randn(num_dst, H).astype(np.float32),
                gout=rng.randn(num_dst, H, D).astype(np.float32))


def sampler_case(degs, H, D, seed):
    """The sampler's layout over the given degrees: col = num_dst + arange(E)."""
    row = rows_of(degs)
    nd, E = len(degs), len(row)
    return make_inputs(nd + np.arange(E, dtype=np.int64), row, nd, nd + E, H, D, seed)


def shape_degs(H, D):
    """NUM_DST degrees 0-12 with a zero-degree destination first and in between."""
    degs = np.random.RandomState(300 + 7 * H + D).randint(1, 13, NUM_DST)
    degs[[0, 4]] = 0
    return degs


def shape_case(H, D):
    return sampler_case(shape_degs(H, D), H, D, 400 + 7 * H + D)


def segment_degs(G):
    """Segment lengths around the group width G: 0, 1, G - 1, G, G + 1."""
    return [0, 1, G - 1, G, G + 1]


def segment_case(G):
    return sampler_case(segment_degs(G), 2, {8: 5, 64: 40}[G], 500 + G)


def long_segment_case():
    """One 3000-edge segment among 12 segments of 1-10 edges."""
    degs = np.random.RandomState(510).randint(1, 11, 13)
    degs[5] = 3000
    return sampler_case(degs, 2, 20, 511)


def degenerate_case(degs):
    return sampler_case(degs, 2, 5, 560 + len(degs))


def unordered_case():
    """A hand-built block: 9 destinations (one without in-edges), 14 sources of which each of
    the first 13 may feed several edges and the last feeds NONE, edges in a shuffled order."""
    rng = np.random.RandomState(520)
    degs = np.array([3, 0, 5, 1, 9, 2, 4, 7, 6])
    row = rows_of(degs)
    col = rng.randint(0, 13, len(row)).astype(np.int64)
    p = rng.permutation(len(row))
    c = make_inputs(col[p], row[p], len(degs), 14, 3, 21, 521)
    assert (np.bincount(c["col"], minlength=14) >= 2).any() and 13 not in c["col"]
    assert (np.diff(c["row"]) < 0).any()
    return c


def exact_zero_case():
    """el, er in {-2..2}: every z is an exactly representable integer and about one in five
    is 0, where forward and backward must take the slope branch."""
    rng = np.random.RandomState(530)
    c = sampler_case(rng.randint(0, 9, 20), 3, 6, 531)
    c["el"] = rng.randint(-2, 3, c["el"].shape).astype(np.float32)
    c["er"] = rng.randint(-2, 3, c["er"].shape).astype(np.float32)
    return c
