"""The float64 reference and error bounds of tests/block_attention_ref.py, checked on the CPU
before any GPU run: an fp32 emulation of the kernels of csrc/block_attention.hip -- the same
lane groups, butterfly sums, two-pass softmax and v_exp_f32 perturbed by +-1 ulp -- stays
within every bound on the inputs that tests/test_gpu_block_attention.py feeds the kernels, and
seeded mistakes in that algorithm break a bound, so the bounds are neither wrong nor vacuous."""
import ctypes

import numpy as np
import pytest

from tests import block_attention_ref as A

F32 = np.float32
LOG2E = F32(1.4426950408889634)


def _group(D):
    """(G, NC) as csrc/block_attention.hip dispatches a D-column head."""
    for g in (8, 16, 32, 64):
        if D <= g:
            return g, 1
    nc = 2
    while 64 * nc < D:
        nc *= 2
    return 64, nc


def _butterfly(p):
    G = p.shape[-1]
    idx = np.arange(G)
    off = G // 2
    while off:
        p = (p + p[..., idx ^ off]).astype(F32)
        off //= 2
    return p[..., 0]


def _head_dot(a, b):
    """[n, H, D] x [n, H, D] -> [n, H]: lane `c mod G` sums its NC products serially, then the
    xor butterfly over the group."""
    n, H, D = a.shape
    G, NC = _group(D)
    pad = ((0, 0), (0, 0), (0, G * NC - D))
    a = np.pad(a.astype(F32), pad).reshape(n, H, NC, G)
    b = np.pad(b.astype(F32), pad).reshape(n, H, NC, G)
    p = np.zeros((n, H, G), F32)
    for j in range(NC):
        p = (p + (a[:, :, j] * b[:, :, j]).astype(F32)).astype(F32)
    return _butterfly(p)


def _exp_f32(x, rng):
    """__expf(x) = v_exp_f32(log2e * x), v_exp_f32 off by up to one ulp either way."""
    t = (x.astype(F32) * LOG2E).astype(F32)
    e = np.exp2(t.astype(np.float64)).astype(F32)
    step = np.where(e >= np.finfo(F32).tiny, rng.randint(-1, 2, e.shape), 0)
    e = np.where(step > 0, np.nextafter(e, F32(np.inf)), e)
    return np.where(step < 0, np.nextafter(e, F32(0)), e).astype(F32)


def _head_mod(x):
    """View [n, H, D] as if column c belonged to head c % H (the seeded indexing mistake)."""
    n, H, D = x.shape
    return np.ascontiguousarray(x.reshape(n, D, H).transpose(0, 2, 1))


def _head_mod_back(x, H, D):
    return np.ascontiguousarray(x.transpose(0, 2, 1)).reshape(x.shape[0], H, D)


def emulate(c, seed=0, drop_last=False, head_mod=False, kink_ge=False, no_dot=False,
            gq_drop_last=False):
    """fp32 forward + backward of the kernels on case `c`; keyword flags seed one mistake."""
    row, nd = c["row"], c["num_dst"]
    q, k, v, g = (c[x].astype(F32) for x in ("q", "k", "v", "gout"))
    E, H, D = k.shape
    if head_mod:
        q, k, v, g = (_head_mod(x) for x in (q, k, v, g))
        H, D = q.shape[1:]
    slope = F32(c["slope"])
    order = np.argsort(row, kind="stable")            # what ops.block_attention's perm does
    rs, ks, vs = row[order], k[order], v[order]
    degs = np.bincount(row, minlength=nd)
    starts = np.r_[0, np.cumsum(degs)][:-1]
    pos = np.arange(E) - starts[rs]                   # position within the segment
    G, _ = _group(D)
    rng = np.random.RandomState(seed)

    z = _head_dot(q[rs], ks)
    s = np.where(z > 0, z, (slope * z).astype(F32)).astype(F32)
    m = np.full((nd, H), -np.finfo(F32).max, F32)
    np.maximum.at(m, rs, s)
    ex = _exp_f32((s - m[rs]).astype(F32), rng)
    lanes = np.zeros((nd, H, G), F32)
    for j in range(int(degs.max()) if E else 0):      # lane j % G takes edge j of a segment
        sel = pos == j
        lanes[rs[sel], :, j % G] = (lanes[rs[sel], :, j % G] + ex[sel]).astype(F32)
    with np.errstate(divide="ignore"):
        inv = (F32(1) / _butterfly(lanes)).astype(F32)
    att = (ex * inv[rs]).astype(F32)

    def seg_serial(w, x, drop):
        acc = np.zeros((nd, H, D), F32)
        for j in range(int(degs.max()) if E else 0):
            sel = (pos == j) & ((pos < degs[rs] - 1) if drop else True)
            acc[rs[sel]] = (acc[rs[sel]] + (w[sel][:, :, None] * x[sel]).astype(F32)).astype(F32)
        return acc

    out = seg_serial(att, vs, drop_last)
    ga = _head_dot(g[rs], vs)
    gv = (att[:, :, None] * g[rs]).astype(F32)
    dot = np.zeros((nd, H), F32)
    for j in range(int(degs.max()) if E else 0):
        sel = pos == j
        dot[rs[sel]] = (dot[rs[sel]] + (att[sel] * ga[sel]).astype(F32)).astype(F32)
    gs = (att * (ga if no_dot else (ga - dot[rs]).astype(F32))).astype(F32)
    unit = (z >= 0) if kink_ge else (z > 0)
    gz = np.where(unit, gs, (gs * slope).astype(F32)).astype(F32)
    gk = (gz[:, :, None] * q[rs]).astype(F32)
    gq = seg_serial(gz, ks, gq_drop_last)

    back = np.empty(E, np.int64)
    back[order] = np.arange(E)
    res = dict(out=out, att=att[back], gq=gq, gk=gk[back], gv=gv[back])
    if head_mod:
        Ht, Dt = c["k"].shape[1:]
        res = {n: (x if n == "att" else _head_mod_back(x, Ht, Dt)) for n, x in res.items()}
        res.pop("att")        # per-head values: no column layout to map back
    return res


CASES = [("shape{}x{}".format(H, D), lambda H=H, D=D: A.shape_case(H, D)) for H, D in A.SHAPES] + \
        [("long_segment", A.long_segment_case), ("unordered", A.unordered_case)]
_REF = {}


def _case(name):
    """(inputs, reference), computed once per session and shared."""
    if name not in _REF:
        c = dict(CASES + [("exact_zero", A.exact_zero_case)])[name]()
        _REF[name] = (c, A.reference(c, exact_z=name == "exact_zero"))
    return _REF[name]


@pytest.mark.parametrize("name", [n for n, _ in CASES] + ["exact_zero"])
def test_emulation_within_bounds(name):
    """Also asserts the precondition min |z| >= 8 bound(z) of every shared case (in
    A.reference) -- the seeds are checked here, on the CPU."""
    c, ref = _case(name)
    worst = {}
    for seed in range(3):           # three draws of the +-1 ulp perturbation
        for what, r in ref.ratios(**emulate(c, seed)).items():
            worst[what] = max(worst.get(what, 0.0), r)
    print("\n[error/bound] {}: {}".format(
        name, " ".join("{}={:.3g}".format(k, v) for k, v in sorted(worst.items()))))
    assert set(worst) == {"out", "att", "gq", "gk", "gv"}
    assert max(worst.values()) <= 1.0, worst


def test_reference_takes_row_as_given():
    """The unordered case is the ordered one with its edges shuffled: same per-destination
    results, per-edge results shuffled alike."""
    c, ref = _case("unordered")
    base, bref = _case("shape3x21")
    p = np.random.RandomState(920).permutation(len(base["row"]))
    assert np.allclose(ref.out, bref.out, rtol=1e-13, atol=0)
    assert np.allclose(ref.att, bref.att[p], rtol=1e-13, atol=0)
    assert np.allclose(ref.gk, bref.gk[p], rtol=0, atol=1e-12)     # ga - dot cancels


def test_degree_one_is_exact():
    c = A.make_inputs(np.arange(9), 9, 2, 5, 940)
    ref = A.reference(c)
    assert (ref.att == 1).all() and np.array_equal(ref.out, c["v"].astype(np.float64))
    got = emulate(c)
    assert (got["att"] == 1).all() and np.array_equal(got["out"], c["v"])


def test_exact_zero_case_has_zeros():
    c, ref = _case("exact_zero")
    assert ref.exact_z and (ref.z == 0).sum() >= 20
    assert (np.abs(ref.gz[ref.z == 0]) > 0).any()


MISTAKES = ["drop_last", "head_mod", "no_dot", "gq_drop_last"]


@pytest.mark.parametrize("mistake", MISTAKES)
def test_mistake_breaks_a_bound(mistake):
    """The dropped last edge, head = c % H, the softmax backward without its sum a ga term and
    gq without its last edge each leave some bound, on every shared case they can touch."""
    broken = {"drop_last": "out", "no_dot": "gk", "gq_drop_last": "gq"}
    for name, _ in CASES:
        c, ref = _case(name)
        H, D = c["k"].shape[1:]
        if mistake == "head_mod" and (H == 1 or D == 1):
            continue                # c % H == c // D there
        r = ref.ratios(**emulate(c, **{mistake: True}))
        if mistake == "head_mod":
            assert max(r.values()) > 1.0, name
        else:
            assert r[broken[mistake]] > 1.0, (name, r)


def test_mistake_slope_branch_at_exact_zero_breaks_bound():
    """Factor 1 instead of slope where z == 0: the forward cannot tell, gq and gk can."""
    c, ref = _case("exact_zero")
    r = ref.ratios(**emulate(c, kink_ge=True))
    assert r["out"] <= 1.0 and r["att"] <= 1.0 and r["gv"] <= 1.0
    assert r["gk"] > 1.0 and r["gq"] > 1.0


def test_width_limit_is_an_error_not_a_fallback():
    """heads * head_dim above GF_BLOCK_ATTENTION_MAX_WIDTH: GF_ERR_INVALID_ARGUMENT and a
    message, from both entry points, before any pointer is looked at."""
    from gnnflow_amd import _build, _capi, ops
    _build.build()
    lib = _capi.load()
    assert ops.MAX_ATTENTION_WIDTH == 1024
    for H, D in ((1, 1025), (1025, 1), (33, 32), (0, 4), (4, 0)):
        rc = lib.gf_block_attention(None, 0, 0, H, D, None, None, None, ctypes.c_float(0.2),
                                    None, None, 0, None)
        assert rc == _capi.GF_ERR_INVALID_ARGUMENT, (H, D)
        assert b"block_attention" in lib.gf_last_error()
        rc = lib.gf_block_attention_backward(None, 0, 0, H, D, None, None, None, None,
                                             ctypes.c_float(0.2), None, None, None, None, 0, None)
        assert rc == _capi.GF_ERR_INVALID_ARGUMENT, (H, D)
