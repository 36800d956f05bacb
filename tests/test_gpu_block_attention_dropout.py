"""ops.block_attention with dropout_p / dropout_seed (the *_dropout kernels of
csrc/block_attention.hip) against the float64 reference and the exact numpy mask of
tests/attention_dropout_ref.py, within its a priori fp32 bounds, forward and backward.  The
(p, seed) pairs, their keep fractions and the preconditions are checked on the CPU in
tests/test_attention_dropout_ref.py.  Each test prints its largest error-to-bound ratio (-s)."""
import ctypes

import numpy as np
import pytest

from tests import attention_dropout_ref as R
from tests import block_attention_ref as A

pytestmark = pytest.mark.gpu


class _Margin:
    def __init__(self):
        self.worst = 0.0

    def check(self, what, ref, **got):
        for name, r in ref.ratios(**got).items():
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


def _block(row, num_dst):
    from gnnflow_amd import MFGBlock
    E = len(row)
    return MFGBlock(num_dst + E, num_dst, _dev(num_dst + np.arange(E, dtype=np.int64)),
                    _dev(np.asarray(row, np.int64)))


_REFS = {}


def _ref(key, c, p, seed):
    """The float64 reference of a shared case: computed once, never modified.  Every test
    needs min att > 2^-100, so that `dropped <=> the returned attention is exactly 0` holds."""
    key = (key, p, seed)
    if key not in _REFS:
        _REFS[key] = R.reference(c, p, seed)
        assert _REFS[key].att.min(initial=1.0) > 2.0 ** -100
    return _REFS[key]


def run(b, c, p, seed, need=("q", "k", "v"), no_grad=False, **kw):
    """Forward + backward of the op with dropout -> dict of numpy results."""
    import torch
    from gnnflow_amd import ops
    q, k, v = (_dev(c[n], n in need) for n in ("q", "k", "v"))
    with torch.no_grad() if no_grad else torch.enable_grad():
        out, att = ops.block_attention(b, q, k, v, negative_slope=c["slope"],
                                       return_attention=True, dropout_p=p, dropout_seed=seed, **kw)
    assert out.shape == c["q"].shape and att.shape == c["k"].shape[:2]
    assert not att.requires_grad
    if need:
        out.backward(_dev(c["gout"]))
    res = dict(out=_np(out), att_dropped=_np(att))
    for n, t in (("q", q), ("k", k), ("v", v)):
        assert (t.grad is not None) == (n in need)
        res["g" + n] = _np(t.grad) if t.grad is not None else None
    return res


def _given(res):
    return {n: x for n, x in res.items() if x is not None}


def _check_mask(res, ref):
    """Exactly the dropped entries are 0, and their gv rows are exact zeros."""
    assert np.array_equal(res["att_dropped"] == 0, ~ref.keep)
    if res.get("gv") is not None:
        assert not res["gv"][~ref.keep].any()


@pytest.mark.parametrize("p", R.P_EXACT)
def test_exact_mask(margin, p):
    c = A.shape_case(2, 50)
    ref = _ref("shape2x50", c, p, R.SEED)
    res = run(_block(c["row"], 40), c, p, R.SEED)
    _check_mask(res, ref)
    assert 0 < ref.keep.sum() < ref.keep.size
    # the kept entries against a * scale (att_dropped's bound is that of a * w)
    margin.check("p={}".format(p), ref, **res)


@pytest.mark.parametrize("H,D", R.HEAD_SHAPES, ids=["{}x{}".format(*s) for s in R.HEAD_SHAPES])
def test_head_shapes(margin, H, D):
    c = A.shape_case(H, D)
    ref = _ref(("shape", H, D), c, R.P, R.SEED)
    res = run(_block(c["row"], 40), c, R.P, R.SEED)
    _check_mask(res, ref)
    margin.check("", ref, **res)


@pytest.mark.parametrize("degs", R.DEGENERATE,
                         ids=["no_dst", "no_edge", "all_degree_0", "all_degree_1", "gap"])
def test_degenerate_blocks(margin, degs):
    c = R.degenerate_case(degs)
    row = c["row"]
    ref = R.reference(c, R.P, R.SEED)
    assert ref.att.min(initial=1.0) > 2.0 ** -100
    res = run(_block(row, len(degs)), c, R.P, R.SEED)
    _check_mask(res, ref)
    margin.check("", ref, **res)
    if len(row) == 0:
        assert all(not res[n].any() for n in ("out", "gq", "gk", "gv"))
    if degs == [1] * 9:
        assert ref.keep.any() and not ref.keep.all()
        want = np.where(ref.keep[:, :, None], R.scale(R.P) * c["v"], np.float32(0))
        assert np.array_equal(res["out"], want)           # exactly scale * v, or exactly 0
    if degs == [4, 0, 7]:
        assert not res["out"][1].any() and not res["gq"][1].any()


def test_segment_with_every_edge_dropped(margin):
    c = R.all_dropped_case()
    seed = R.ALL_DROPPED_SEED
    ref = _ref("all_dropped", c, R.P, seed)
    kept = A._seg_sum(ref.row, ref.keep.astype(np.float64), ref.num_dst)
    lost = (kept == 0) & (np.array(R.ALL_DROPPED_DEGS)[:, None] >= 2)
    assert lost.any()                                     # the chosen seed does have one
    res = run(_block(c["row"], c["num_dst"]), c, R.P, seed)
    _check_mask(res, ref)
    margin.check("", ref, **res)
    assert not res["out"][lost].any() and not res["gq"][lost].any()
    assert not res["gk"][lost[ref.row]].any()


def test_long_segment_among_short(margin):
    c = A.long_segment_case()
    assert np.bincount(c["row"]).max() == 3000
    ref = _ref("long", c, R.P, R.SEED)
    res = run(_block(c["row"], c["num_dst"]), c, R.P, R.SEED)
    _check_mask(res, ref)
    margin.check("", ref, **res)


def test_unordered_block_goes_through_perm(margin):
    c = A.unordered_case()
    b = _block(c["row"], c["num_dst"])
    assert b.segments()[2] is not None
    ref = _ref("unordered", c, R.P, R.SEED)
    # the mask index is the position after the stable sort by destination
    order = np.argsort(c["row"], kind="stable")
    want = np.empty_like(ref.keep)
    want[order] = R.keep_mask(len(order), 3, R.P, R.SEED)
    assert np.array_equal(want, ref.keep)
    assert not np.array_equal(want, R.keep_mask(len(order), 3, R.P, R.SEED))
    res = run(b, c, R.P, R.SEED)
    _check_mask(res, ref)                                 # att_dropped, gv in the caller's order
    margin.check("", ref, **res)


@pytest.mark.parametrize("need", [("q",), ("k",), ("v",), ("q", "k", "v"), ()],
                         ids=["q", "k", "v", "qkv", "no_grad"])
def test_gradient_subsets(margin, need):
    """run() asserts that exactly the inputs that require grad get one."""
    c = A.shape_case(2, 50)
    ref = _ref("shape2x50", c, R.P, R.SEED)
    res = run(_block(c["row"], 40), c, R.P, R.SEED, need, no_grad=not need)
    _check_mask(res, ref)
    margin.check("+".join(need), ref, **_given(res))


def test_determinism_and_seeds():
    c = A.long_segment_case()
    b = _block(c["row"], c["num_dst"])
    first, second = run(b, c, R.P, R.SEED), run(b, c, R.P, R.SEED)
    for n in first:
        assert np.array_equal(first[n], second[n]), n
    other = run(b, c, R.P, R.SEED_B)
    assert not np.array_equal(first["att_dropped"] == 0, other["att_dropped"] == 0)
    assert np.array_equal(other["att_dropped"] == 0,
                          ~R.keep_mask(len(c["row"]), 2, R.P, R.SEED_B))


def _direct(lib_fwd, lib_bwd, c, extra):
    """Both C entry points of one flavour on the sorted case `c`; extra: the arguments between
    negative_slope and the outputs."""
    import torch
    from gnnflow_amd import _capi
    b = _block(c["row"], c["num_dst"])
    offsets = b.segments()[0]
    q, k, v, g = (_dev(c[n]) for n in ("q", "k", "v", "gout"))
    E, H, D = k.shape
    out, att = torch.empty_like(q), torch.empty((E, H), device="cuda")
    gq, gk, gv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
    head = (offsets.data_ptr(), c["num_dst"], E, H, D, q.data_ptr(), k.data_ptr(), v.data_ptr())
    slope = ctypes.c_float(c["slope"])
    tail = (0, _capi.current_stream(q.device))
    fwd_out = (out.data_ptr(), att.data_ptr()) + ((None,) if extra else ())
    _capi.check(lib_fwd(*head, slope, *extra, *fwd_out, *tail))
    _capi.check(lib_bwd(*head, att.data_ptr(), slope, *extra, g.data_ptr(), gq.data_ptr(),
                        gk.data_ptr(), gv.data_ptr(), *tail))
    torch.cuda.synchronize()
    return dict(out=out, att=att, gq=gq, gk=gk, gv=gv)


def test_p_zero_is_the_op_without_dropout():
    import torch
    from gnnflow_amd import _capi, ops
    c = A.shape_case(2, 129)

    def via_ops(**kw):
        q, k, v = (_dev(c[n], True) for n in ("q", "k", "v"))
        out, att = ops.block_attention(_block(c["row"], 40), q, k, v, negative_slope=c["slope"],
                                       return_attention=True, **kw)
        out.backward(_dev(c["gout"]))
        return dict(out=out.detach(), att=att, gq=q.grad, gk=k.grad, gv=v.grad)

    plain = via_ops()
    for kw in (dict(dropout_p=0.0), dict(dropout_p=0.0, dropout_seed=R.SEED)):
        got = via_ops(**kw)
        for n in plain:
            assert torch.equal(plain[n], got[n]), (kw, n)
    lib = _capi.load()
    for cc in (c, A.shape_case(3, 21), A.long_segment_case()):
        old = _direct(lib.gf_block_attention, lib.gf_block_attention_backward, cc, ())
        new = _direct(lib.gf_block_attention_dropout, lib.gf_block_attention_dropout_backward, cc,
                      (ctypes.c_float(0.0), R.SEED))
        for n in old:
            assert torch.equal(old[n], new[n]), n


def test_pre_dropout_attention_from_the_entry_point(margin):
    """d_att of gf_block_attention_dropout is the pre-dropout softmax (within att's bound), and
    it is what the backward needs: gq, gk, gv from it are within bounds."""
    from gnnflow_amd import _capi
    c = A.shape_case(2, 50)
    ref = _ref("shape2x50", c, R.P, R.SEED)
    lib = _capi.load()
    got = _direct(lib.gf_block_attention_dropout, lib.gf_block_attention_dropout_backward, c,
                  (ctypes.c_float(R.P), R.SEED))
    margin.check("", ref, **{n: _np(t) for n, t in got.items()})
    assert (_np(got["att"]) > 0).all()


def test_composed_chain_cross_check(margin):
    """edge_softmax -> multiply by the numpy mask * scale (uploaded) -> block_reduce on the same
    inputs: both paths within their bounds of the same DropoutReference (the chain's dropped
    attention within att_dropped's bound -- same softmax, the same one multiply --, its output
    within block_reduce's bound given its own fp32 messages)."""
    import torch
    import torch.nn.functional as F
    from gnnflow_amd import ops
    from tests import block_ops_ref as Ro
    c = A.shape_case(2, 50)
    ref = _ref("shape2x50", c, R.P, R.SEED)
    b = _block(c["row"], 40)
    margin.check("fused", ref, **run(b, c, R.P, R.SEED))
    q, k, v = (_dev(c[n], True) for n in ("q", "k", "v"))
    row, E = b.edges()[1], len(c["row"])
    w = _dev(np.where(ref.keep, R.scale(R.P), np.float32(0)).astype(np.float32))
    att = ops.edge_softmax(b, F.leaky_relu((q[row] * k).sum(2), c["slope"])) * w
    msg = (v * att[:, :, None]).reshape(E, -1)
    out = ops.block_reduce(b, torch.cat([torch.zeros((40, msg.shape[1]), device=msg.device), msg]))
    out.backward(_dev(c["gout"]).reshape(40, -1))
    margin.check("composed", ref, att_dropped=_np(att), gq=_np(q.grad), gk=_np(k.grad),
                 gv=_np(v.grad))
    col = 40 + np.arange(E)
    src = np.concatenate([np.zeros((40, msg.shape[1]), np.float32), _np(msg)])
    bound = Ro.reduce_fwd_bound(col, c["row"], 40, 40 + E, src) + \
        A._seg_sum(c["row"], ((ref.b_att_dropped + 2 * A.U * ref.att_dropped)[:, :, None] *
                              np.abs(c["v"])).reshape(E, -1), 40)
    r = A.error_ratio(_np(out), ref.out.reshape(40, -1), bound)
    margin.worst = max(margin.worst, r)
    assert r <= 1.0, r


def test_error_paths():
    from gnnflow_amd import _capi, ops
    c = A.shape_case(2, 50)
    b = _block(c["row"], 40)
    q, k, v = (_dev(c[n]) for n in ("q", "k", "v"))
    for p in (-0.1, 1.0, 1.5, float("nan")):
        with pytest.raises(ValueError):
            ops.block_attention(b, q, k, v, dropout_p=p, dropout_seed=1)
    with pytest.raises(ValueError):
        ops.block_attention(b, q, k, v, dropout_p=0.5)              # no seed
    for seed in (-1, 2 ** 64):
        with pytest.raises(ValueError):
            ops.block_attention(b, q, k, v, dropout_p=0.5, dropout_seed=seed)
    ops.block_attention(b, q, k, v, dropout_p=0.5, dropout_seed=2 ** 64 - 1)
    lib = _capi.load()
    rc = lib.gf_block_attention_dropout(
        b.segments()[0].data_ptr(), 40, len(c["row"]), 2, 50, q.data_ptr(), k.data_ptr(),
        v.data_ptr(), ctypes.c_float(0.2), ctypes.c_float(1.0), 1, None, None, None, 0, None)
    assert rc == _capi.GF_ERR_INVALID_ARGUMENT and b"dropout" in lib.gf_last_error()
