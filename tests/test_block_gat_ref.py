"""tests/block_gat_ref.py checked on the CPU before any GPU run: an fp32 emulation of the
kernels of csrc/block_gat.hip -- lane-strided score pass, two-pass softmax with v_exp_f32
perturbed by +-1 ulp, the dropout mask, dot taken from the saved fp32 output, ger as lane-strided
sums and a butterfly, gfeat / gel accumulated in a shuffled (atomic) order -- stays within every
bound on the inputs that tests/test_gpu_block_gat.py feeds the kernels, and seeded mistakes
break a bound, so the bounds are neither wrong nor vacuous."""
import numpy as np
import pytest

from tests import attention_dropout_ref as R
from tests import block_gat_ref as Gr
from tests.test_block_attention_ref import _butterfly, _exp_f32, _group, _head_dot

F32 = np.float32


def emulate(c, p=0.0, seed=0, rseed=0, two_sweeps=False, kink_ge=False, no_dot=False,
            scale_twice=False, drop_last=False):
    """fp32 forward + backward of the kernels on case `c`; keyword flags seed one mistake
    (two_sweeps is no mistake: the other admissible way to form dot)."""
    row, col, nd, ns = c["row"], c["col"], c["num_dst"], c["num_src"]
    feat, el, er, g = (c[x].astype(F32) for x in ("feat", "el", "er", "gout"))
    E = len(row)
    _, H, D = feat.shape
    slope = F32(c["slope"])
    order = np.argsort(row, kind="stable")            # what block.segments() does
    rs, cs = row[order], col[order]
    degs = np.bincount(row, minlength=nd)
    starts = np.r_[0, np.cumsum(degs)][:-1]
    pos = np.arange(E) - starts[rs]                   # position within the segment
    G, _ = _group(D)
    rng = np.random.RandomState(rseed)
    keep = R.keep_mask(E, H, p, seed) if E else np.ones((0, H), bool)
    w = np.where(keep, R.scale(p), F32(0)).astype(F32)
    maxdeg = int(degs.max()) if E else 0

    z = (el[cs] + er[rs]).astype(F32)
    s = np.where(z > 0, z, (slope * z).astype(F32)).astype(F32)
    m = np.full((nd, H), -np.finfo(F32).max, F32)
    np.maximum.at(m, rs, s)
    ex = _exp_f32((s - m[rs]).astype(F32), rng)

    def lane_sums(x):
        """lane j % G adds edge j of its segment; then the butterfly"""
        lanes = np.zeros((nd, H, G), F32)
        for j in range(maxdeg):
            sel = pos == j
            lanes[rs[sel], :, j % G] = (lanes[rs[sel], :, j % G] + x[sel]).astype(F32)
        return _butterfly(lanes)

    with np.errstate(divide="ignore"):
        inv = (F32(1) / lane_sums(ex)).astype(F32)
    att = (ex * inv[rs]).astype(F32)
    aw = (att * w).astype(F32) if p > 0 else att
    if scale_twice:
        aw = (aw * w).astype(F32)

    fs, gs_ = feat[cs], g[rs]
    out = np.zeros((nd, H, D), F32)
    for j in range(maxdeg):                           # serial, in edge order, kept edges only
        sel = (pos == j) & ((pos < degs[rs] - 1) if drop_last else True)
        new = (out[rs[sel]] + (aw[sel][:, :, None] * fs[sel]).astype(F32)).astype(F32)
        out[rs[sel]] = np.where(keep[sel][:, :, None], new, out[rs[sel]])

    ga = _head_dot(gs_, fs) if E else np.zeros((0, H), F32)
    if p > 0:
        ga = np.where(keep, (w * ga).astype(F32), F32(0))
    if two_sweeps:
        dot = np.zeros((nd, H), F32)
        for j in range(maxdeg):
            sel = pos == j
            new = (dot[rs[sel]] + (att[sel] * ga[sel]).astype(F32)).astype(F32)
            dot[rs[sel]] = np.where(keep[sel], new, dot[rs[sel]])
    else:
        dot = _head_dot(g, out)                       # gout[d] . out^[d]
    gsc = (att * (ga if no_dot else (ga - dot[rs]).astype(F32))).astype(F32)
    unit = (z >= 0) if kink_ge else (z > 0)
    gz = np.where(unit, gsc, (gsc * slope).astype(F32)).astype(F32)
    ger = lane_sums(gz) if E else np.zeros((nd, H), F32)

    # gfeat, gel: one fp32 add per edge into zeros, in a shuffled order (atomics; a sampler
    # block adds once per row, which is the plain store)
    gfeat, gel = np.zeros((ns, H, D), F32), np.zeros((ns, H), F32)
    term = (aw[:, :, None] * gs_).astype(F32)
    for i in rng.permutation(E):
        gfeat[cs[i]] = np.where(keep[i][:, None], (gfeat[cs[i]] + term[i]).astype(F32),
                                gfeat[cs[i]])
        gel[cs[i]] = (gel[cs[i]] + gz[i]).astype(F32)

    back = np.empty(E, np.int64)
    back[order] = np.arange(E)
    return dict(out=out, att=att[back], att_dropped=np.where(keep, aw, F32(0))[back],
                gfeat=gfeat, gel=gel, ger=ger)


CASES = [("shape{}x{}".format(H, D), lambda H=H, D=D: Gr.shape_case(H, D)) for H, D in Gr.HEAD_SHAPES] + \
        [("segments{}".format(G), lambda G=G: Gr.segment_case(G)) for G in (8, 64)] + \
        [("long_segment", Gr.long_segment_case), ("unordered", Gr.unordered_case)] + \
        [("degenerate{}".format(i), lambda d=d: Gr.degenerate_case(d))
         for i, d in enumerate(Gr.DEGENERATE)]
_REF = {}


def _case(name, p=0.0, seed=0):
    """(inputs, reference), computed once per session and shared."""
    key = (name, p, seed)
    if key not in _REF:
        c = dict(CASES + [("exact_zero", Gr.exact_zero_case)])[name]()
        _REF[key] = (c, Gr.reference(c, p, seed, exact_z=name == "exact_zero"))
    return _REF[key]


@pytest.mark.parametrize("p", (0.0,) + Gr.PS)
@pytest.mark.parametrize("name", [n for n, _ in CASES] + ["exact_zero"])
def test_emulation_within_bounds(name, p):
    """Also asserts the precondition of every shared case (in Gr.reference) -- the seeds are
    checked here, on the CPU -- and min att > 2^-100, so that `dropped <=> the returned
    attention is exactly 0` holds."""
    c, ref = _case(name, p, Gr.SEED)
    assert ref.att.min(initial=1.0) > 2.0 ** -100
    worst = {}
    for rseed in range(3):          # three draws of the +-1 ulp perturbation and the add order
        for two in (False, True):
            got = emulate(c, p, Gr.SEED, rseed, two_sweeps=two)
            assert np.array_equal(got["att_dropped"] == 0, ~ref.keep)
            assert not got["gfeat"][ref.unread].any() and not got["gel"][ref.unread].any()
            for what, r in ref.ratios(**got).items():
                worst[what] = max(worst.get(what, 0.0), r)
    print("\n[error/bound] {} p={}: {}".format(
        name, p, " ".join("{}={:.3g}".format(k, v) for k, v in sorted(worst.items()))))
    assert set(worst) == {"out", "att", "att_dropped", "gfeat", "gel", "ger"}
    assert max(worst.values()) <= 1.0, worst


def test_cases_are_what_the_gpu_tests_need():
    assert [_group(D) for _, D in Gr.HEAD_SHAPES] == \
        [(8, 1), (8, 1), (8, 1), (16, 1), (32, 1), (64, 1), (64, 2), (64, 8), (64, 16)]
    for H, D in Gr.HEAD_SHAPES:
        assert len(Gr.shape_degs(H, D)) == Gr.NUM_DST == 7 and H * D <= 1024
    assert Gr.segment_degs(8) == [0, 1, 7, 8, 9] and Gr.segment_degs(64) == [0, 1, 63, 64, 65]
    assert _group(Gr.segment_case(8)["feat"].shape[2])[0] == 8
    assert _group(Gr.segment_case(64)["feat"].shape[2])[0] == 64
    assert np.bincount(Gr.long_segment_case()["row"]).max() == 3000
    c, ref = _case("unordered")
    assert ref.unread.sum() >= 1 and ref.unread[13]
    assert not ref.gfeat[13].any() and not ref.b_gfeat[13].any()     # exact zeros are demanded
    assert not ref.gel[13].any() and not ref.b_gel[13].any()
    ref = _case("shape2x16")[1]
    assert ref.unread[:7].all() and not ref.unread[7:].any()        # the sampler layout


def test_exact_zero_case_has_zeros():
    c, ref = _case("exact_zero")
    assert ref.exact_z and (ref.z == 0).sum() >= 20
    assert (np.abs(ref.gz[ref.z == 0]) > 0).any()


def test_p_zero_is_the_reference_without_dropout():
    c = Gr.shape_case(2, 17)
    plain, ref = Gr.reference(c), Gr.reference(c, 0.0, Gr.SEED)
    assert ref.keep.all() and ref.scale == 1.0 and ref.delta == 0.0
    for f in ("out", "att", "att_dropped", "gfeat", "gel", "ger", "b_out", "b_gfeat", "b_gel"):
        assert np.array_equal(getattr(ref, f), getattr(plain, f)), f


def test_dot_is_gout_times_out_with_dropout_too():
    c, ref = _case("shape3x5", 0.5, Gr.SEED)
    assert 0 < ref.keep.sum() < ref.keep.size
    K = ref.keep / (1 - 0.5)
    fe, ge = c["feat"].astype(np.float64)[ref.col], c["gout"].astype(np.float64)[ref.row]
    sweep = Gr._seg_sum(ref.row, ref.att * K * (ge * fe).sum(-1), ref.num_dst)
    assert np.allclose(sweep, (c["gout"] * ref.out).sum(-1), rtol=1e-12, atol=1e-13)


@pytest.mark.parametrize("mistake,broken", [("drop_last", "out"), ("no_dot", "gel"),
                                            ("scale_twice", "out")])
def test_mistake_breaks_a_bound(mistake, broken):
    for name in ("shape3x5", "shape2x100", "unordered"):
        c, ref = _case(name, 0.5, Gr.SEED)
        r = ref.ratios(**emulate(c, 0.5, Gr.SEED, **{mistake: True}))
        assert r[broken] > 1.0, (name, r)


def test_mistake_slope_branch_at_exact_zero_breaks_bound():
    """Factor 1 instead of slope where z == 0: the forward cannot tell, gel and ger can."""
    c, ref = _case("exact_zero")
    r = ref.ratios(**emulate(c, kink_ge=True))
    assert r["out"] <= 1.0 and r["att"] <= 1.0 and r["gfeat"] <= 1.0
    assert r["gel"] > 1.0 and r["ger"] > 1.0


def test_wrong_seed_breaks_the_mask():
    c, ref = _case("shape3x5", 0.5, Gr.SEED)
    r = ref.ratios(**emulate(c, 0.5, Gr.SEED_B))
    assert r["att_dropped"] == float("inf") and r["out"] > 1.0
