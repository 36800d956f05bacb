"""tests/attention_dropout_ref.py checked on the CPU before any GPU run: the numpy Philox against
the Random123 known answers and the oracle, the mask's threshold and keep fractions for the
(p, seed) pairs the GPU tests use, p = 0 against the parent reference, and an fp32 emulation of
the dropout kernels of csrc/block_attention.hip within every bound on the shared cases."""
import numpy as np
import pytest

from tests import attention_dropout_ref as R
from tests import block_attention_ref as A
from tests.test_block_attention_ref import _butterfly, _exp_f32, _group, _head_dot

F32 = np.float32
FULL = 0xFFFFFFFFFFFFFFFF


def test_philox_known_answers():
    """The Random123 kat_vectors used in tests/test_gpu_sampler_parity.py."""
    assert int(R.philox_first(0, 0, 0)) == 0x6627E8D5
    assert int(R.philox_first(FULL, FULL, FULL)) == 0x408F276D
    tid = (0x85A308D3 << 32) | 0x243F6A88
    call = (0x03707344 << 32) | 0x13198A2E
    seed = (0x299F31D0 << 32) | 0xA4093822
    assert int(R.philox_first(seed, tid, call)) == 0xD16CFE09


def test_philox_matches_the_oracle():
    from oracle import oracle as O
    rng = np.random.RandomState(7)
    t = rng.randint(0, 1 << 63, size=(300, 3)).astype(np.uint64) * 2 + \
        rng.randint(0, 2, size=(300, 3)).astype(np.uint64)
    got = R.philox_first(t[:, 0], t[:, 1], t[:, 2])
    assert got.dtype == np.uint32
    want = np.array([O.philox_first(int(s), int(i), int(c)) for s, i, c in t], dtype=np.uint32)
    assert np.array_equal(got, want)
    small = np.array([O.philox_first(R.SEED, i, 0) for i in range(64)], dtype=np.uint32)
    assert np.array_equal(R.philox_first(R.SEED, np.arange(64), 0), small)


def test_threshold_and_scale():
    assert R.threshold(0.0) == 0 and R.keep_mask(500, 3, 0.0, R.SEED).all()
    assert R.scale(0.0) == 1 and R.scale(0.5) == 2 and R.scale(0.5).dtype == np.float32
    assert R.threshold(0.5) == 1 << 31
    ps = np.sort(np.r_[np.random.RandomState(1).rand(200), 0.0, np.nextafter(F32(1), F32(0))])
    ts = [R.threshold(p) for p in ps]
    assert all(a <= b for a, b in zip(ts, ts[1:])) and ts[-1] < 1 << 32
    # a larger threshold only ever drops more of the same draws
    masks = [R.keep_mask(400, 2, p, R.SEED) for p in (0.1, 0.5, 0.9)]
    assert (masks[0] | ~masks[1]).all() and (masks[1] | ~masks[2]).all()


def _cases_of_the_gpu_tests():
    c = A.shape_case(2, 50)
    n = c["k"].shape[0] * 2
    todo = [("exact p={}".format(p), n, p, R.SEED) for p in R.P_EXACT]
    todo.append(("seed B", n, R.P, R.SEED_B))
    for H, D in R.HEAD_SHAPES:
        todo.append(("{}x{}".format(H, D), A.shape_case(H, D)["k"].shape[0] * H, R.P, R.SEED))
    todo.append(("long", A.long_segment_case()["k"].shape[0] * 2, R.P, R.SEED))
    todo.append(("unordered", A.unordered_case()["k"].shape[0] * 3, R.P, R.SEED))
    return todo


def test_keep_fraction_of_the_gpu_tests_masks():
    """Deterministic: the seeds were picked so that it holds, and this is where it is checked."""
    for name, n, p, seed in _cases_of_the_gpu_tests():
        frac = R.keep_mask(n, 1, p, seed).mean()
        assert abs(frac - (1 - p)) <= 4 * np.sqrt(p * (1 - p) / n), (name, frac)


def test_masks_of_two_seeds_differ():
    a, b = R.keep_mask(228, 2, R.P, R.SEED), R.keep_mask(228, 2, R.P, R.SEED_B)
    assert (a != b).sum() > 100


def test_all_dropped_seed():
    """The seed of the GPU test drops every edge of a (degree 2 or 3 segment, head) pair."""
    assert R.find_all_dropped_seed(R.ALL_DROPPED_DEGS, 2, R.P) == R.ALL_DROPPED_SEED
    ref = R.reference(R.all_dropped_case(), R.P, R.ALL_DROPPED_SEED)
    kept = A._seg_sum(ref.row, ref.keep.astype(np.float64), ref.num_dst)
    d, h = np.argwhere((kept == 0) & (np.array(R.ALL_DROPPED_DEGS)[:, None] >= 2))[0]
    assert not ref.out[d, h].any() and not ref.b_out[d, h].any()
    assert not ref.gq[d, h].any() and not ref.b_gq[d, h].any()      # exact zeros are demanded
    assert ref.att.min() > 2.0 ** -100


def test_grouped_position():
    row = np.array([2, 0, 2, 1, 0])
    assert R.grouped_position(row).tolist() == [3, 0, 4, 2, 1]
    c, base = A.unordered_case(), A.shape_case(3, 21)
    ref, bref = R.reference(c, R.P, R.SEED), R.reference(base, R.P, R.SEED)
    p = np.random.RandomState(920).permutation(len(base["row"]))
    # a shuffle is not a stable sort: within a segment the edges meet the mask in another order,
    # so only the multiset of decisions is shared, not the per-edge result
    assert ref.keep.sum() == bref.keep.sum() and not np.array_equal(ref.keep, bref.keep[p])
    order = np.argsort(c["row"], kind="stable")
    assert np.array_equal(ref.keep[order], R.keep_mask(len(order), 3, R.P, R.SEED))


@pytest.mark.parametrize("name", ["shape2x50", "unordered", "degree_one"])
def test_p_zero_is_the_parent_reference(name):
    c = {"shape2x50": lambda: A.shape_case(2, 50), "unordered": A.unordered_case,
         "degree_one": lambda: A.make_inputs(np.arange(9), 9, 2, 5, 940)}[name]()
    parent, ref = A.reference(c), R.reference(c, 0.0, R.SEED)
    assert ref.keep.all() and ref.scale == 1.0 and ref.delta == 0.0
    for f in ("out", "att", "gq", "gk", "gv", "gz", "z"):
        assert np.array_equal(getattr(ref, f), getattr(parent, f)), f
    assert np.array_equal(ref.att_dropped, parent.att)
    for f in ("b_out", "b_att", "b_gq", "b_gk", "b_gv"):         # one more rounding, no less
        mine, theirs = getattr(ref, f), getattr(parent, f)
        assert (mine >= theirs).all() and (mine <= 1.5 * theirs).all(), f


def emulate(c, p, seed, rseed=0, ignore_mask_in_dot=False, scale_twice=False):
    """fp32 forward + backward of the dropout kernels on case `c`: the parent emulation's lane
    groups, butterflies and +-1 ulp v_exp_f32, with w applied where the kernels apply it."""
    row, nd = c["row"], c["num_dst"]
    q, k, v, g = (c[x].astype(F32) for x in ("q", "k", "v", "gout"))
    E, H, D = k.shape
    slope = F32(c["slope"])
    order = np.argsort(row, kind="stable")
    rs, ks, vs = row[order], k[order], v[order]
    degs = np.bincount(row, minlength=nd)
    starts = np.r_[0, np.cumsum(degs)][:-1]
    pos = np.arange(E) - starts[rs]
    G, _ = _group(D)
    rng = np.random.RandomState(rseed)
    keep = R.keep_mask(E, H, p, seed)
    sc = R.scale(p)
    w = np.where(keep, sc, F32(0)).astype(F32)

    z = _head_dot(q[rs], ks)
    s = np.where(z > 0, z, (slope * z).astype(F32)).astype(F32)
    m = np.full((nd, H), -np.finfo(F32).max, F32)
    np.maximum.at(m, rs, s)
    ex = _exp_f32((s - m[rs]).astype(F32), rng)
    lanes = np.zeros((nd, H, G), F32)
    for j in range(int(degs.max()) if E else 0):
        sel = pos == j
        lanes[rs[sel], :, j % G] = (lanes[rs[sel], :, j % G] + ex[sel]).astype(F32)
    with np.errstate(divide="ignore"):
        inv = (F32(1) / _butterfly(lanes)).astype(F32)
    att = (ex * inv[rs]).astype(F32)
    aw = (att * w).astype(F32)
    if scale_twice:
        aw = (aw * w).astype(F32)

    def seg_serial(wt, x, only=None):
        """acc += wt * x in edge order; `only`: [E, H] edges whose term is skipped when False"""
        acc = np.zeros((nd, H) + x.shape[2:], F32)
        for j in range(int(degs.max()) if E else 0):
            sel = pos == j
            term = (wt[sel][(...,) + (None,) * (x.ndim - 2)] * x[sel]).astype(F32)
            new = (acc[rs[sel]] + term).astype(F32)
            if only is not None:
                new = np.where(only[sel].reshape(only[sel].shape + (1,) * (x.ndim - 2)),
                               new, acc[rs[sel]])
            acc[rs[sel]] = new
        return acc

    out = seg_serial(aw, vs, keep)
    ga = (w * _head_dot(g[rs], vs)).astype(F32)
    gv = (aw[:, :, None] * g[rs]).astype(F32)
    dot = seg_serial(att, _head_dot(g[rs], vs) if ignore_mask_in_dot else ga,
                     None if ignore_mask_in_dot else keep)
    gs = (att * (ga - dot[rs]).astype(F32)).astype(F32)
    gz = np.where(z > 0, gs, (gs * slope).astype(F32)).astype(F32)
    gk = (gz[:, :, None] * q[rs]).astype(F32)
    gq = seg_serial(gz, ks)

    back = np.empty(E, np.int64)
    back[order] = np.arange(E)
    return dict(out=out, att=att[back], att_dropped=aw[back], gq=gq, gk=gk[back], gv=gv[back])


CASES = [("shape{}x{}".format(H, D), lambda H=H, D=D: A.shape_case(H, D), R.P, R.SEED)
         for H, D in R.HEAD_SHAPES] + \
        [("exact_p{}".format(p), lambda: A.shape_case(2, 50), p, R.SEED) for p in R.P_EXACT] + \
        [("long_segment", A.long_segment_case, R.P, R.SEED),
         ("unordered", A.unordered_case, R.P, R.SEED),
         ("all_dropped", R.all_dropped_case, R.P, R.ALL_DROPPED_SEED)] + \
        [("degenerate{}".format(i), lambda d=d: R.degenerate_case(d), R.P, R.SEED)
         for i, d in enumerate(R.DEGENERATE)]
_REF = {}


def _case(name):
    if name not in _REF:
        _, make, p, seed = next(x for x in CASES if x[0] == name)
        c = make()
        _REF[name] = (c, R.reference(c, p, seed), p, seed)
    return _REF[name]


@pytest.mark.parametrize("name", [x[0] for x in CASES])
def test_emulation_within_bounds(name):
    """Also asserts the preconditions of the GPU tests on the CPU: clear of the kink (in
    R.reference) and min att > 2^-100."""
    c, ref, p, seed = _case(name)
    assert ref.att.min(initial=1.0) > 2.0 ** -100
    worst = {}
    for rseed in range(3):
        got = emulate(c, p, seed, rseed)
        assert np.array_equal(got["att_dropped"] == 0, ~ref.keep)
        assert not got["gv"][~ref.keep].any()
        for what, r in ref.ratios(**got).items():
            worst[what] = max(worst.get(what, 0.0), r)
    print("\n[error/bound] {}: {}".format(
        name, " ".join("{}={:.3g}".format(k, v) for k, v in sorted(worst.items()))))
    assert set(worst) == {"out", "att", "att_dropped", "gq", "gk", "gv"}
    assert max(worst.values()) <= 1.0, worst


@pytest.mark.parametrize("mistake,broken", [("ignore_mask_in_dot", "gk"), ("scale_twice", "out")])
def test_mistake_breaks_a_bound(mistake, broken):
    """The softmax Jacobian fed the undropped ga, and the scale applied twice, each leave a
    bound: the bounds are not vacuous."""
    c, ref, p, seed = _case("shape3x21")
    assert ref.ratios(**emulate(c, p, seed, **{mistake: True}))[broken] > 1.0


def test_wrong_seed_breaks_the_mask():
    c, ref, p, seed = _case("shape3x21")
    r = ref.ratios(**emulate(c, p, R.SEED_B))
    assert r["att_dropped"] == float("inf") and r["out"] > 1.0


def test_invalid_p_is_an_error_from_both_entry_points():
    """p outside [0, 1) or NaN: GF_ERR_INVALID_ARGUMENT before any pointer is looked at."""
    import ctypes
    from gnnflow_amd import _build, _capi
    _build.build()
    lib = _capi.load()
    for p in (1.0, -0.1, 1.5, float("nan")):
        rc = lib.gf_block_attention_dropout(None, 0, 0, 2, 4, None, None, None,
                                            ctypes.c_float(0.2), ctypes.c_float(p), 1, None, None,
                                            None, 0, None)
        assert rc == _capi.GF_ERR_INVALID_ARGUMENT, p
        assert b"dropout" in lib.gf_last_error()
        rc = lib.gf_block_attention_dropout_backward(
            None, 0, 0, 2, 4, None, None, None, None, ctypes.c_float(0.2), ctypes.c_float(p), 1,
            None, None, None, None, 0, None)
        assert rc == _capi.GF_ERR_INVALID_ARGUMENT, p
    # a valid p gets as far as the next check
    rc = lib.gf_block_attention_dropout(None, 0, 0, 2, 4, None, None, None, ctypes.c_float(0.2),
                                        ctypes.c_float(0.5), 1, None, None, None, 0, None)
    assert rc == _capi.GF_ERR_INVALID_ARGUMENT and b"offsets" in lib.gf_last_error()
