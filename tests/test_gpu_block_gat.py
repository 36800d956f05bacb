"""ops.block_gat (csrc/block_gat.hip) against the float64 reference and the exact numpy mask of
tests/block_gat_ref.py, within its a priori fp32 bounds, forward and backward.  The shared cases
and their preconditions are checked on the CPU in tests/test_block_gat_ref.py.

Two ways in: `run` goes through ops.block_gat on a hand-built block, which always carries an
explicit col (the atomic path, also when col happens to be num_dst + arange); `direct` calls the
C entry points with a NULL col, the sampler's layout, on the same inputs.  Real sampler blocks go
through ops.block_gat with segments()[1] None.  Each test prints its largest error-to-bound
ratio (run with -s)."""
import ctypes
import itertools

import numpy as np
import pytest

from tests import block_gat_ref as Gr

pytestmark = pytest.mark.gpu
NAMES = ("feat", "el", "er")


class _Margin:
    def __init__(self):
        self.worst = 0.0

    def check(self, what, ref, **got):
        for name, r in ref.ratios(**{n: x for n, x in got.items() if x is not None}).items():
            self.worst = max(self.worst, r)
            assert r <= 1.0, "{} {}: error / bound = {:.3g}".format(what, name, r)


@pytest.fixture
def margin(request):
    m = _Margin()
    yield m
    print("\n[error/bound] {}: {:.3g}".format(request.node.name, m.worst))


def _np(t):
    return t.detach().cpu().numpy()


def _dev(a, grad=False):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda().requires_grad_(grad)


def _block(c):
    from gnnflow_amd import MFGBlock
    return MFGBlock(c["num_src"], c["num_dst"], _dev(c["col"]), _dev(c["row"]))


_REFS = {}


def _ref(key, c, p=0.0, seed=0, **kw):
    """The float64 reference of a shared case: computed once, never modified."""
    key = (key, p, seed)
    if key not in _REFS:
        _REFS[key] = Gr.reference(c, p, seed, **kw)
        assert _REFS[key].att.min(initial=1.0) > 2.0 ** -100
    return _REFS[key]


def run(b, c, need=NAMES, p=0.0, seed=None, no_grad=False):
    """Forward + backward through ops.block_gat -> dict of numpy results (None: no grad)."""
    import torch
    from gnnflow_amd import ops
    feat, el, er = (_dev(c[n], n in need) for n in NAMES)
    kw = dict(dropout_p=p, dropout_seed=seed) if p else {}
    with torch.no_grad() if no_grad else torch.enable_grad():
        out, att = ops.block_gat(b, feat, el, er, negative_slope=c["slope"],
                                 return_attention=True, **kw)
    assert out.shape == c["gout"].shape and att.shape == (len(c["row"]), c["el"].shape[1])
    assert not att.requires_grad
    if need:
        out.backward(_dev(c["gout"]))
    res = dict(out=_np(out), att_dropped=_np(att))
    if not p:
        res["att"] = res["att_dropped"]
    for n, t in zip(NAMES, (feat, el, er)):
        assert (t.grad is not None) == (n in need)
        res["g" + n] = _np(t.grad) if t.grad is not None else None
    return res


def direct(c, p=0.0, seed=0, null_col=True):
    """Both C entry points on a case whose edges are grouped; NULL col = the sampler's layout."""
    import torch
    from gnnflow_amd import _capi
    lib = _capi.load()
    row, nd, ns = c["row"], c["num_dst"], c["num_src"]
    assert (np.diff(row) >= 0).all()
    if null_col:
        assert np.array_equal(c["col"], nd + np.arange(len(row)))
    offsets = _dev(np.r_[0, np.cumsum(np.bincount(row, minlength=nd))].astype(np.int64))
    col = None if null_col else _dev(c["col"])
    feat, el, er, g = (_dev(c[n]) for n in NAMES + ("gout",))
    E, (_, H, D) = len(row), feat.shape
    # poisoned outputs: whatever the kernels and the memsets leave unwritten shows up
    out, att, drp = (torch.full(s, float("nan"), device="cuda")
                     for s in ((nd, H, D), (E, H), (E, H)))
    gfeat, gel, ger = (torch.full_like(t, float("nan")) for t in (feat, el, er))
    ptr = lambda t: t.data_ptr() if t is not None and t.numel() else None     # noqa: E731
    head = (ptr(offsets), nd, E, ptr(col), ns, H, D, ptr(feat), ptr(el), ptr(er))
    mid = (ctypes.c_float(c["slope"]), ctypes.c_float(p), seed)
    tail = (0, _capi.current_stream(feat.device))
    _capi.check(lib.gf_block_gat(*head, *mid, ptr(out), ptr(att), ptr(drp), *tail))
    _capi.check(lib.gf_block_gat_backward(*head, ptr(att), ptr(out), *mid, ptr(g), ptr(gfeat),
                                          ptr(gel), ptr(ger), *tail))
    torch.cuda.synchronize()
    return dict(out=_np(out), att=_np(att), att_dropped=_np(drp), gfeat=_np(gfeat),
                gel=_np(gel), ger=_np(ger))


def _check_layout_zeros(res, nd):
    """Sampler layout: the rows of the destinations themselves are exact zeros."""
    assert not res["gfeat"][:nd].any() and not res["gel"][:nd].any()


def _check_mask(res, ref):
    assert np.array_equal(res["att_dropped"] == 0, ~ref.keep)


def _sampler_blocks(strategy):
    from gnnflow_amd import DynamicGraph, TemporalSampler
    rng = np.random.RandomState(20)
    N, E = 300, 5000
    src, dst = rng.randint(0, N, E), rng.randint(0, N, E)
    ts = np.sort(rng.rand(E)).astype(np.float32)
    g = DynamicGraph(1 << 20, 64 << 20, "cuda", 16, 64, "insert")
    g.add_edges(src.astype(np.int64), dst.astype(np.int64), ts, add_reverse=True)
    rng = np.random.RandomState(22)
    mfgs = TemporalSampler(g, [10, 10], strategy, seed=5).sample(
        rng.randint(0, N, 150).astype(np.int64), rng.uniform(0.6, 1.0, 150).astype(np.float32))
    return [b for layer in mfgs for b in layer]


@pytest.mark.parametrize("strategy", ["recent", "uniform"])
def test_sampler_blocks(margin, strategy):
    checked = 0
    for li, b in enumerate(_sampler_blocks(strategy)):
        assert b.segments()[1] is None and b.segments()[2] is None
        if b.num_edges() == 0:
            continue
        checked += 1
        col, row = (_np(x) for x in b.edges())
        nd = b.num_dst_nodes()
        c = Gr.make_inputs(col, row, nd, b.num_src_nodes(), 2, 50, 950 + li)
        for p, seed in ((0.0, None), (0.5, Gr.SEED)):
            ref = Gr.reference(c, p, seed or 0)
            first, second = run(b, c, p=p, seed=seed), run(b, c, p=p, seed=seed)
            margin.check("layer {} p={}".format(li, p), ref, **first)
            _check_layout_zeros(first, nd)
            _check_mask(first, ref)
            for n in first:                       # no atomics: the same bits, the same seed too
                assert np.array_equal(first[n], second[n]), n
    assert checked == 2


@pytest.mark.parametrize("H,D", Gr.HEAD_SHAPES, ids=["{}x{}".format(*s) for s in Gr.HEAD_SHAPES])
def test_head_shapes(margin, H, D):
    c = Gr.shape_case(H, D)
    assert c["num_dst"] == 7
    ref = _ref(("shape", H, D), c)
    margin.check("col", ref, **run(_block(c), c))
    res = direct(c)
    margin.check("sampler layout", ref, **res)
    _check_layout_zeros(res, 7)
    assert np.array_equal(res["att"], res["att_dropped"])         # p == 0: w = 1


@pytest.mark.parametrize("G", [8, 64])
def test_segment_lengths_around_the_group_width(margin, G):
    c = Gr.segment_case(G)
    assert np.bincount(c["row"], minlength=5).tolist() == [0, 1, G - 1, G, G + 1]
    for p, seed in ((0.0, 0), (0.5, Gr.SEED)):
        ref = _ref(("segments", G), c, p, seed)
        margin.check("col p={}".format(p), ref, **run(_block(c), c, p=p, seed=seed))
        res = direct(c, p, seed)
        margin.check("sampler layout p={}".format(p), ref, **res)
        _check_layout_zeros(res, 5)
        assert not res["out"][0].any() and not res["ger"][0].any()


def test_long_segment_among_short(margin):
    c = Gr.long_segment_case()
    assert np.bincount(c["row"]).max() == 3000
    for p, seed in ((0.0, 0), (0.2, Gr.SEED)):
        ref = _ref("long", c, p, seed)
        margin.check("col", ref, **run(_block(c), c, p=p, seed=seed))
        margin.check("sampler layout", ref, **direct(c, p, seed))


@pytest.mark.parametrize("degs", Gr.DEGENERATE,
                         ids=["no_dst", "no_edge", "all_degree_0", "all_degree_1", "gap"])
def test_degenerate_blocks(margin, degs):
    c = Gr.degenerate_case(degs)
    for p, seed in ((0.0, 0), (0.5, Gr.SEED)):
        ref = Gr.reference(c, p, seed)
        res = run(_block(c), c, p=p, seed=seed)
        margin.check("ops", ref, **res)
        if len(c["row"]) == 0:
            assert all(not res[n].any() for n in ("out", "gfeat", "gel", "ger"))
        else:
            raw = direct(c, p, seed)
            margin.check("sampler layout", ref, **raw)
            _check_layout_zeros(raw, len(degs))
        if degs == [1] * 9 and p == 0:
            assert (res["att"] == 1).all() and np.array_equal(res["out"], c["feat"][9:])
        if degs == [4, 0, 7]:
            assert not res["out"][1].any() and not res["ger"][1].any()


def test_unordered_block_with_repeated_sources(margin):
    """perm and the atomic path; the source no edge reads gets exact zeros."""
    c = Gr.unordered_case()
    b = _block(c)
    assert b.segments()[1] is not None and b.segments()[2] is not None
    for p, seed in ((0.0, 0), (0.5, Gr.SEED)):
        ref = _ref("unordered", c, p, seed)
        res = run(b, c, p=p, seed=seed)
        margin.check("p={}".format(p), ref, **res)           # att in the caller's order
        _check_mask(res, ref)
        assert ref.unread[13] and not res["gfeat"][ref.unread].any() \
            and not res["gel"][ref.unread].any()


def test_exact_zero_scores_take_the_slope(margin):
    c = Gr.exact_zero_case()
    ref = _ref("zero", c, exact_z=True)
    assert (ref.z == 0).sum() >= 20
    margin.check("col", ref, **run(_block(c), c))
    margin.check("sampler layout", ref, **direct(c))


SUBSETS = [s for k in range(4) for s in itertools.combinations(NAMES, k)]


@pytest.mark.parametrize("need", SUBSETS, ids=["+".join(s) or "no_grad" for s in SUBSETS])
def test_gradient_subsets(margin, need):
    """run() asserts that exactly the inputs that require grad get one; the empty subset is the
    forward alone under no_grad."""
    c = Gr.shape_case(2, 100)
    for p, seed in ((0.0, 0), (0.5, Gr.SEED)):
        ref = _ref(("shape", 2, 100), c, p, seed)
        margin.check("p={}".format(p), ref,
                     **run(_block(c), c, need, p=p, seed=seed, no_grad=not need))


@pytest.mark.parametrize("p", Gr.PS)
def test_dropout_against_the_cpu_mask(margin, p):
    """out, the gradients and the returned DROPPED attention a * w against the reference with
    the mask computed on the CPU; the pre-dropout softmax from the entry point."""
    for key, c in ((("shape", 2, 17), Gr.shape_case(2, 17)), (("shape", 8, 8), Gr.shape_case(8, 8))):
        ref = _ref(key, c, p, Gr.SEED)
        assert 0 < ref.keep.sum() < ref.keep.size
        res = run(_block(c), c, p=p, seed=Gr.SEED)
        _check_mask(res, ref)
        margin.check("col", ref, **res)
        raw = direct(c, p, Gr.SEED)
        _check_mask(raw, ref)
        assert (raw["att"] > 0).all()
        margin.check("sampler layout", ref, **raw)
        _check_layout_zeros(raw, 7)
        other = run(_block(c), c, p=p, seed=Gr.SEED_B)
        assert not np.array_equal(other["att_dropped"] == 0, ~ref.keep)


def test_p_zero_is_the_plain_call_and_runs_repeat():
    import torch
    from gnnflow_amd import ops
    c = Gr.long_segment_case()
    b = _block(c)

    def via_ops(**kw):
        feat, el, er = (_dev(c[n], True) for n in NAMES)
        out, att = ops.block_gat(b, feat, el, er, c["slope"], return_attention=True, **kw)
        out.backward(_dev(c["gout"]))
        return dict(out=out.detach(), att=att, gfeat=feat.grad, gel=el.grad, ger=er.grad)

    plain = via_ops()
    for kw in (dict(dropout_p=0.0), dict(dropout_p=0.0, dropout_seed=Gr.SEED)):
        got = via_ops(**kw)
        for n in plain:
            assert torch.equal(plain[n], got[n]), (kw, n)
    # the sampler layout: two runs, and two runs with one seed, give the same bits
    for p, seed in ((0.0, 0), (0.5, Gr.SEED)):
        first, second = direct(c, p, seed), direct(c, p, seed)
        for n in first:
            assert np.array_equal(first[n], second[n]), (p, n)
    assert np.array_equal(direct(c)["out"], _np(plain["out"]))


def test_nan_row_on_a_dropped_edge_does_not_propagate():
    c = Gr.shape_case(2, 17)
    ref = _ref(("shape", 2, 17), c, 0.5, Gr.SEED)
    gone = np.flatnonzero(~ref.keep.any(axis=1))          # edges dropped for every head
    assert len(gone) >= 1
    bad = dict(c, feat=c["feat"].copy())
    bad["feat"][c["col"][gone]] = np.nan
    for got, clean in ((run(_block(bad), bad, p=0.5, seed=Gr.SEED),
                        run(_block(c), c, p=0.5, seed=Gr.SEED)),
                       (direct(bad, 0.5, Gr.SEED), direct(c, 0.5, Gr.SEED))):
        for n in ("out", "gfeat", "gel", "ger"):
            assert np.isfinite(got[n]).all(), n
            assert np.array_equal(got[n], clean[n]), n   # the rows were never read


def test_composed_chain_cross_check(margin):
    """The chain of GATConv.forward on the same inputs: el[col] + er[row] -> leaky_relu ->
    ops.edge_softmax -> ops.block_reduce, gradients by autograd.  Both sides within their own
    bounds of one reference: |fused - composed| <= bound(fused) + bound(composed).  The chain's
    attention has the fused bound (one add, the same two-pass softmax); its out and gfeat have
    block_reduce's own bounds on its fp32 weights plus the weights' error; its gel and ger follow
    the reference's formulas with dot summed over the edges (covered by b_dot) and ga summed with
    gamma_{D+2} where the reference has gamma_{D+1}, so (D + 2) / (D + 1) times the reference's
    bound covers every term."""
    import torch.nn.functional as F
    from gnnflow_amd import ops
    from tests import block_ops_ref as Ro
    c = Gr.unordered_case()
    ref = _ref("unordered", c)
    b = _block(c)
    fused = run(b, c)
    margin.check("fused", ref, **fused)
    feat, el, er = (_dev(c[n], True) for n in NAMES)
    col, row = b.edges()
    att = ops.edge_softmax(b, F.leaky_relu(el[col] + er[row], c["slope"]))
    out = ops.block_reduce(b, feat, att)
    out.backward(_dev(c["gout"]))
    lay = (c["col"], c["row"], c["num_dst"], c["num_src"])
    H, D = c["feat"].shape[1:]
    a32 = _np(att)
    b_out = Ro.reduce_fwd_bound(*lay, c["feat"], a32).reshape(ref.out.shape) + \
        Gr._seg_sum(c["row"], ref.b_att[:, :, None] * np.abs(c["feat"][c["col"]]), c["num_dst"])
    b_gfeat = Ro.reduce_bwd_bound(*lay, c["feat"], a32, False, c["gout"])[0] \
        .reshape(ref.gfeat.shape) + \
        Gr._src_sum(c["col"], ref.b_att[:, :, None] * np.abs(c["gout"][c["row"]]), c["num_src"])
    k = (D + 2.0) / (D + 1.0)
    for name, mine, theirs, bound in (
            ("att", fused["att"], a32, 2 * ref.b_att),
            ("out", fused["out"], _np(out), ref.b_out + b_out),
            ("gfeat", fused["gfeat"], _np(feat.grad), ref.b_gfeat + b_gfeat),
            ("gel", fused["gel"], _np(el.grad), (1 + k) * ref.b_gel),
            ("ger", fused["ger"], _np(er.grad), (1 + k) * ref.b_ger)):
        r = Gr.error_ratio(mine, theirs.astype(np.float64), bound)
        margin.worst = max(margin.worst, r)
        assert r <= 1.0, (name, r)
