"""ops.block_attention (csrc/block_attention.hip) against the float64 reference of
tests/block_attention_ref.py, within its a priori fp32 bounds, forward and backward: sampler
blocks, head shapes around the lane-group sizes, degenerate blocks, one long segment, an
unordered block, exact-zero scores, every gradient subset, non-contiguous inputs, the composed
chain of existing ops, determinism and the error paths.  Each test prints its largest
error-to-bound ratio (run with -s)."""
import numpy as np
import pytest

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
    """A hand-built block over `row` (the op never reads col); sorted rows take no perm."""
    from gnnflow_amd import MFGBlock
    E = len(row)
    return MFGBlock(num_dst + E, num_dst, _dev(num_dst + np.arange(E, dtype=np.int64)),
                    _dev(np.asarray(row, np.int64)))


_REFS = {}


def _ref(key, c, **kw):
    """The float64 reference of a shared case: computed once, never modified."""
    if key not in _REFS:
        _REFS[key] = A.reference(c, **kw)
    return _REFS[key]


def run(b, c, need=("q", "k", "v"), slope=None):
    """Forward + backward of the fused op -> dict of numpy results (None where no grad)."""
    from gnnflow_amd import ops
    q, k, v = (_dev(c[n], n in need) for n in ("q", "k", "v"))
    out, att = ops.block_attention(b, q, k, v, negative_slope=c["slope"], return_attention=True)
    assert out.shape == c["q"].shape and att.shape == c["k"].shape[:2]
    assert not att.requires_grad
    if need:
        out.backward(_dev(c["gout"]))
    res = dict(out=_np(out), att=_np(att))
    for n, t in (("q", q), ("k", k), ("v", v)):
        assert (t.grad is not None) == (n in need)
        res["g" + n] = _np(t.grad) if t.grad is not None else None
    return res


def _assert_sampler_layout(b):
    import torch
    col, row = b.edges()
    nd, E = b.num_dst_nodes(), b.num_edges()
    assert torch.equal(col, nd + torch.arange(E, device=col.device))
    assert E < 2 or bool((row[1:] >= row[:-1]).all())
    offsets, seg_col, perm = b.segments()
    assert seg_col is None and perm is None        # the col-less, perm-less path


@pytest.mark.parametrize("strategy", ["recent", "uniform"])
def test_sampler_blocks(margin, strategy):
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
    checked = 0
    for li, layer in enumerate(mfgs):
        for b in layer:
            _assert_sampler_layout(b)
            if b.num_edges() == 0:
                continue
            checked += 1
            c = A.make_inputs(_np(b.edges()[1]), b.num_dst_nodes(), 2, 50, 950 + li)
            margin.check("layer {}".format(li), A.reference(c), **run(b, c))
    assert checked == 2


@pytest.mark.parametrize("H,D", A.SHAPES, ids=["{}x{}".format(*s) for s in A.SHAPES])
def test_head_shapes(margin, H, D):
    c = A.shape_case(H, D)
    degs = np.bincount(c["row"], minlength=40)
    assert degs.min() == 0 and degs.max() == 12
    margin.check("", _ref(("shape", H, D), c), **run(_block(c["row"], 40), c))


@pytest.mark.parametrize("degs", [[], [0], [0] * 5, [1] * 9, [4, 0, 7]],
                         ids=["no_dst", "no_edge", "all_degree_0", "all_degree_1", "gap"])
def test_degenerate_blocks(margin, degs):
    row = A.rows_of(degs)
    c = A.make_inputs(row, len(degs), 2, 5, 960 + len(degs))
    res = run(_block(row, len(degs)), c)
    margin.check("", A.reference(c), **res)
    if len(row) == 0:
        assert all(not res[n].any() for n in ("out", "gq", "gk", "gv"))
    if degs == [1] * 9:
        assert (res["att"] == 1).all() and np.array_equal(res["out"], c["v"])
    if degs == [4, 0, 7]:
        assert not res["out"][1].any() and not res["gq"][1].any()


def test_long_segment_among_short(margin):
    c = A.long_segment_case()
    assert np.bincount(c["row"]).max() == 3000
    margin.check("", _ref("long", c), **run(_block(c["row"], c["num_dst"]), c))


def test_unordered_block_goes_through_perm(margin):
    c = A.unordered_case()
    b = _block(c["row"], c["num_dst"])
    assert b.segments()[2] is not None
    margin.check("", _ref("unordered", c), **run(b, c))      # att, gk, gv in the caller's order


def test_exact_zero_scores_take_the_slope(margin):
    c = A.exact_zero_case()
    ref = _ref("zero", c, exact_z=True)
    assert (ref.z == 0).sum() >= 20
    margin.check("", ref, **run(_block(c["row"], c["num_dst"]), c))


@pytest.mark.parametrize("need", [("q",), ("k",), ("v",), ("q", "k", "v")],
                         ids=["q", "k", "v", "qkv"])
def test_gradient_subsets(margin, need):
    """run() asserts that exactly the inputs that require grad get one (the others None)."""
    c = A.shape_case(2, 50)
    margin.check("+".join(need), _ref(("shape", 2, 50), c),
                 **{n: x for n, x in run(_block(c["row"], 40), c, need).items() if x is not None})


def test_forward_only_without_grad(margin):
    c = A.shape_case(2, 50)
    margin.check("", _ref(("shape", 2, 50), c), **{n: x for n, x in run(
        _block(c["row"], 40), c, need=()).items() if x is not None})


def test_non_contiguous_and_2d_inputs(margin):
    """q as a transposed view, k as a slice of a wider tensor, v 2-D with heads=."""
    import torch
    from gnnflow_amd import ops
    c = A.shape_case(3, 21)
    ref = _ref(("shape", 3, 21), c)
    b = _block(c["row"], 40)
    E = len(c["row"])
    q = _dev(c["q"].transpose(1, 0, 2)).transpose(0, 1).requires_grad_(True)
    wide = _dev(np.concatenate([c["k"], c["k"]], axis=2))
    k = wide[:, :, :21].requires_grad_(True)
    assert not q.is_contiguous() and not k.is_contiguous()
    out, att = ops.block_attention(b, q, k, _dev(c["v"]), c["slope"], return_attention=True)
    out.backward(_dev(c["gout"]))
    margin.check("views", ref, out=_np(out), att=_np(att), gq=_np(q.grad), gk=_np(k.grad))
    flat = [_dev(c[n].reshape(len(c[n]), -1)) for n in ("q", "k", "v")]
    out2 = ops.block_attention(b, *flat, negative_slope=c["slope"], heads=3)
    assert out2.shape == (40, 3, 21) and torch.equal(out2, out)
    with pytest.raises(ValueError):
        ops.block_attention(b, *flat, heads=4)            # 63 columns, 4 heads
    with pytest.raises(ValueError):
        ops.block_attention(b, *flat)                     # 2-D without heads=
    assert E == att.shape[0]


def test_composed_chain_cross_check(margin):
    """The chain of existing ops the fused op replaces, on the same inputs: both within their
    own bounds of the same reference (the chain's attention within the fused op's bound for
    att -- same two-pass softmax --, its output within block_reduce's bound given its att)."""
    import torch
    import torch.nn.functional as F
    from gnnflow_amd import ops
    from tests import block_ops_ref as R
    c = A.shape_case(2, 50)
    ref = _ref(("shape", 2, 50), c)
    b = _block(c["row"], 40)
    fused = run(b, c)
    margin.check("fused", ref, **fused)
    q, k, v = (_dev(c[n], True) for n in ("q", "k", "v"))
    row, E = b.edges()[1], len(c["row"])
    att = ops.edge_softmax(b, F.leaky_relu((q[row] * k).sum(2), c["slope"]))
    msg = (v * att[:, :, None]).reshape(E, -1)
    out = ops.block_reduce(b, torch.cat([torch.zeros((40, msg.shape[1]), device=msg.device), msg]))
    out.backward(_dev(c["gout"]).reshape(40, -1))
    margin.check("composed", ref, att=_np(att), gq=_np(q.grad), gk=_np(k.grad), gv=_np(v.grad))
    # out = sum of the chain's own fp32 messages: block_reduce's bound on those, plus the
    # bound of the messages themselves (att's error and one multiply)
    col = 40 + np.arange(E)
    src = np.concatenate([np.zeros((40, msg.shape[1]), np.float32), _np(msg)])
    bound = R.reduce_fwd_bound(col, c["row"], 40, 40 + E, src) + \
        A._seg_sum(c["row"], ((ref.b_att + 2 * A.U * ref.att)[:, :, None] *
                              np.abs(c["v"])).reshape(E, -1), 40)
    r = A.error_ratio(_np(out), ref.out.reshape(40, -1), bound)
    margin.worst = max(margin.worst, r)
    assert r <= 1.0, r


def test_two_runs_are_bit_identical():
    c = A.long_segment_case()
    b = _block(c["row"], c["num_dst"])
    first, second = run(b, c), run(b, c)
    for n in first:
        assert np.array_equal(first[n], second[n]), n


def test_error_paths():
    import torch
    from gnnflow_amd import ops
    c = A.shape_case(2, 50)
    b = _block(c["row"], 40)
    q, k, v = (_dev(c[n]) for n in ("q", "k", "v"))
    with pytest.raises(TypeError):
        ops.block_attention(b, q.double(), k, v)
    with pytest.raises(TypeError):
        ops.block_attention(b, q, k.half(), v)
    with pytest.raises(ValueError):
        ops.block_attention(b, q[:-1], k, v)              # rows of q != num_dst
    with pytest.raises(ValueError):
        ops.block_attention(b, q, k[:-1], v)              # rows of k != num_edges
    with pytest.raises(ValueError):
        ops.block_attention(b, q, k, v[1:])
    with pytest.raises(ValueError):
        ops.block_attention(b, q, k[:, :1], v)            # [H, D] differ
    with pytest.raises(ValueError):
        ops.block_attention(b, q, k, v.reshape(-1, 50, 2))
    E = len(c["row"])
    wide = ops.MAX_ATTENTION_WIDTH // 2 + 1
    big = [torch.zeros((n, 2, wide), device="cuda") for n in (40, E, E)]
    with pytest.raises(ValueError, match="limit"):
        ops.block_attention(b, *big)
