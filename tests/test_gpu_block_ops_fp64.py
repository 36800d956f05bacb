"""The block ops (csrc/block_ops.hip) against float64 references, within a priori fp32 error
bounds (tests/block_ops_ref.py), forward and backward.

Blocks come from the real samplers, whose col-less layout (source of edge k = row
num_dst + k) takes the kernels' non-atomic paths, and from hand-built shapes: feature and
per-head widths around the 64-lane stride, many heads, the thread/wave switch of the softmax,
one long segment among short ones, ties in max, shifted and masked logits, degenerate blocks.
Each test prints its largest error-to-bound ratio (run with -s)."""
import numpy as np
import pytest

from tests import block_ops_ref as R

pytestmark = pytest.mark.gpu

MODES = ["copy_sum", "copy_mean", "mul_sum", "mul_mean"]
GRAD_CASES = [("src",), ("w",), ("src", "w")]


class _Margin:
    def __init__(self):
        self.worst = 0.0

    def check(self, what, got, want, bound):
        r = R.error_ratio(got, want, bound)
        self.worst = max(self.worst, r)
        assert r <= 1.0, "{}: error / bound = {:.3g}".format(what, r)

    def exact(self, what, got, want):
        assert np.array_equal(np.asarray(got, np.float64), np.asarray(want, np.float64)), what


@pytest.fixture
def margin(request):
    m = _Margin()
    yield m
    print("\n[error/bound] {}: {:.3g}".format(request.node.name, m.worst))


def _np(t):
    return t.detach().cpu().numpy()


def _2d(a):
    """[n, ...] -> [n, prod(...)], also for n = 0."""
    return a.reshape(a.shape[0], int(np.prod(a.shape[1:])))


def _dev(a, grad=False):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda().requires_grad_(grad)


def _explicit(col, row, num_dst, num_src):
    """A hand-made block: its ops pass `col` explicitly (the general, atomic path)."""
    from gnnflow_amd import MFGBlock
    return MFGBlock(num_src, num_dst, _dev(np.asarray(col, np.int64)),
                    _dev(np.asarray(row, np.int64)))


def _assert_sampler_layout(b):
    """The invariant the col-less kernels rely on, and that the block does take that path."""
    import torch
    col, row = b.edges()
    nd, E = b.num_dst_nodes(), b.num_edges()
    dev = col.device
    assert torch.equal(col, nd + torch.arange(E, device=dev))
    assert E < 2 or bool((row[1:] >= row[:-1]).all())
    assert b.num_src_nodes() == nd + E
    offsets, seg_col, perm = b.segments()
    assert seg_col is None and perm is None
    want = torch.searchsorted(row, torch.arange(nd + 1, device=dev)) if E else \
        torch.zeros(nd + 1, dtype=torch.int64, device=dev)
    assert torch.equal(offsets, want)


def _col_less(col, row, num_dst, num_src):
    """A hand-built block in the sampler's layout, set up as MFGBlock.segments() sets up a
    sampler block (col = None): its ops take the col-less kernel path."""
    b = _explicit(col, row, num_dst, num_src)
    offsets, _, perm = b.segments()
    assert perm is None
    b._segments = (offsets, None, None)
    _assert_sampler_layout(b)
    return b


def _blocks(c):
    """The blocks over case `c`'s layout: col-less and explicit when it is the sampler's."""
    L = (c["col"], c["row"], c["num_dst"], c["num_src"])
    sampler = np.array_equal(c["col"], c["num_dst"] + np.arange(len(c["col"])))
    return ([("col-less", _col_less(*L))] if sampler else []) + [("explicit", _explicit(*L))]


def _layout(b):
    col, row = b.edges()
    return _np(col), _np(row), b.num_dst_nodes(), b.num_src_nodes()


# ---- the op checks --------------------------------------------------------------------------------
def check_reduce(margin, tag, b, src, w, grad, modes=MODES):
    """block_reduce forward + backward in each mode; mul modes with each gradient case."""
    from gnnflow_amd import ops
    L = _layout(b)
    nd = L[2]
    for mode in modes:
        mean, weighted = mode.endswith("mean"), mode.startswith("mul")
        wr = w if weighted else None
        args = L + (src, wr, mean)
        want, bound = R.reduce_fwd(*args), R.reduce_fwd_bound(*args)
        want_s, want_w = R.reduce_bwd(*args, grad)
        bound_s, bound_w = R.reduce_bwd_bound(*args, grad)
        for need in GRAD_CASES if weighted else GRAD_CASES[:1]:
            what = "{} {} needs {}".format(tag, mode, "+".join(need))
            vs = _dev(src, "src" in need)
            vw = _dev(wr, "w" in need) if weighted else None
            out = ops.block_reduce(b, vs, vw, mean=mean)
            assert out.shape == (nd,) + src.shape[1:]
            margin.check(what + " forward", _2d(_np(out)), want, bound)
            out.backward(_dev(grad))
            if "src" in need:
                margin.check(what + " grad_src", _2d(_np(vs.grad)), want_s, bound_s)
            if "w" in need:
                margin.check(what + " grad_w", _np(vw.grad).reshape(want_w.shape), want_w, bound_w)


def check_softmax(margin, tag, b, logits, grad_y):
    """edge_softmax forward + backward; masked (-inf) logits give exactly 0 and no gradient,
    fully masked segments NaN wherever the reference does."""
    from gnnflow_amd import ops
    L = _layout(b)
    x = _dev(logits, True)
    y = ops.edge_softmax(b, x)
    yn = _2d(_np(y))
    want = R.softmax_fwd(*L, logits)
    margin.check(tag + " softmax forward", yn, want, R.softmax_fwd_bound(*L, logits))
    y.backward(_dev(grad_y))
    gx = _2d(_np(x.grad))
    gy = _2d(grad_y)
    margin.check(tag + " softmax backward", gx, R.softmax_bwd(*L, yn, gy),
                 R.softmax_bwd_bound(*L, yn, gy))
    dead = np.isneginf(_2d(logits)) & ~np.isnan(want)
    assert (yn[dead] == 0).all() and (gx[dead] == 0).all(), tag
    return yn


def check_max(margin, tag, b, src, grad):
    """block_max: forward exactly, gradient to the lowest tied edge within the bound (exact
    unless a source row feeds several edges)."""
    from gnnflow_amd import ops
    L = _layout(b)
    vs = _dev(src, True)
    out = ops.block_max(b, vs)
    want, arg = R.max_fwd(*L, src)
    margin.exact(tag + " max forward", _np(out).reshape(want.shape), want)
    out.backward(_dev(grad))
    margin.check(tag + " max backward", _2d(_np(vs.grad)),
                 R.max_bwd(*L, arg, grad), R.max_bwd_bound(*L, arg, grad))


# ---- blocks from the real samplers --------------------------------------------------------------
def _graph(dense):
    from gnnflow_amd import DynamicGraph
    rng = np.random.RandomState(21 if dense else 20)
    N, E = (60, 20000) if dense else (300, 5000)
    src, dst = rng.randint(0, N, E), rng.randint(0, N, E)
    ts = np.sort(rng.rand(E)).astype(np.float32)
    g = DynamicGraph(1 << 20, 64 << 20, "cuda", 16, 64, "insert")
    g.add_edges(src.astype(np.int64), dst.astype(np.int64), ts, add_reverse=True)
    return g, N


def _check_sampled(margin, mfgs, expect_wave=False):
    rng = np.random.RandomState(31)
    H, P = 4, 20
    checked = 0
    for layer in mfgs:
        for b in layer:
            _assert_sampler_layout(b)
            L = _layout(b)
            nd, ns, E = L[2], L[3], len(L[0])
            if E == 0:
                continue
            checked += 1
            if expect_wave:
                assert E > 32 * nd          # the wave softmax kernels run
            src = rng.randn(ns, H, P).astype(np.float32)
            w = rng.randn(E, H, 1).astype(np.float32)
            grad = rng.randn(nd, H, P).astype(np.float32)
            logits = (3 * rng.randn(E, H)).astype(np.float32)
            grad_y = rng.randn(E, H).astype(np.float32)
            twin = _explicit(*L)            # same col / row, explicit-col path
            for tag, blk in (("sampled", b), ("twin", twin)):
                check_reduce(margin, tag, blk, src, w, grad)
                check_softmax(margin, tag, blk, logits, grad_y)
                check_max(margin, tag, blk, src.reshape(ns, -1), grad.reshape(nd, -1))
    assert checked


SAMPLERS = [("recent", 1, [10, 10], False), ("uniform", 1, [10, 10], False),
            ("recent", 2, [10, 10], False), ("uniform", 2, [10, 10], False),
            ("recent", 1, [50], True), ("uniform", 1, [50], True)]


@pytest.mark.parametrize("strategy,snapshots,fanouts,dense", SAMPLERS,
                         ids=["{}-{}snap-{}".format(s, n, "x".join(map(str, f)))
                              for s, n, f, _ in SAMPLERS])
def test_sampler_blocks(margin, strategy, snapshots, fanouts, dense):
    from gnnflow_amd import TemporalSampler
    g, N = _graph(dense)
    sampler = TemporalSampler(g, fanouts, strategy, num_snapshots=snapshots,
                              snapshot_time_window=0.25 if snapshots > 1 else 0.0, seed=5)
    rng = np.random.RandomState(22)
    R_ = 100 if dense else 150
    mfgs = sampler.sample(rng.randint(0, N, R_).astype(np.int64),
                          rng.uniform(0.6, 1.0, R_).astype(np.float32))
    _check_sampled(margin, mfgs, expect_wave=dense)


def test_partitioned_sampler_blocks(margin):
    from gnnflow_amd import TemporalSampler
    from gnnflow_amd.dist import DevicePartitionedSampler
    g, N = _graph(False)
    part = DevicePartitionedSampler(TemporalSampler(g, [10, 10], "recent"))
    rng = np.random.RandomState(23)
    mfgs = part.sample(rng.randint(0, N, 150).astype(np.int64), np.full(150, 2.0, np.float32))
    _check_sampled(margin, mfgs)


# ---- hand-built shapes ---------------------------------------------------------------------------
@pytest.mark.parametrize("sampler_layout", [True, False], ids=["sampler", "general"])
@pytest.mark.parametrize("dim", [1, 63, 64, 65, 129, 172, 256])
def test_feature_widths(margin, dim, sampler_layout):
    c = R.width_case(dim, sampler_layout)
    for tag, b in _blocks(c):
        check_reduce(margin, tag, b, c["src"], c["w"], c["grad"])
        check_max(margin, tag, b, c["src"], c["grad"])


@pytest.mark.parametrize("sampler_layout", [True, False], ids=["sampler", "general"])
@pytest.mark.parametrize("heads", [1, 3, 4, 8])
@pytest.mark.parametrize("per_head", [1, 63, 64, 65])
def test_per_head_widths(margin, per_head, heads, sampler_layout):
    c = R.head_case(per_head, heads, sampler_layout)
    E = len(c["col"])
    for tag, b in _blocks(c):
        for shape in ((E, heads), (E, heads, 1)):
            check_reduce(margin, "{} w{}".format(tag, shape), b, c["src"], c["w"].reshape(shape),
                         c["grad"], modes=["mul_sum", "mul_mean"])
            check_softmax(margin, "{} logits{}".format(tag, shape), b,
                          c["logits"].reshape(shape), c["grad_y"].reshape(shape))


@pytest.mark.parametrize("heads", [1, 4])
@pytest.mark.parametrize("extra", [0, 1], ids=["thread", "wave"])
def test_softmax_thread_wave_switch(margin, extra, heads):
    c = R.softmax_switch_case(extra, heads)
    E = len(c["col"])
    assert E == 32 * c["num_dst"] + extra
    for tag, b in _blocks(c):
        for shape in ((E, heads), (E, heads, 1)):
            check_softmax(margin, "{} logits{}".format(tag, shape), b,
                          c["logits"].reshape(shape), c["grad_y"].reshape(shape))


@pytest.mark.parametrize("sampler_layout", [True, False], ids=["sampler", "general"])
def test_long_segment_among_short(margin, sampler_layout):
    c = R.long_segment_case(sampler_layout)
    assert len(c["col"]) <= 32 * c["num_dst"]     # the thread softmax kernels run
    assert R.degrees(c["row"], c["num_dst"]).max() == 3000
    ns, nd = c["num_src"], c["num_dst"]
    for tag, b in _blocks(c):
        check_reduce(margin, tag, b, c["src"], c["w"], c["grad"])
        check_softmax(margin, tag, b, c["logits"], c["grad_y"])
        check_max(margin, tag, b, c["src"].reshape(ns, -1), c["grad"].reshape(nd, -1))


@pytest.mark.parametrize("degs", [[7], [0], [0] * 5], ids=["one_dst", "one_dst_no_edge",
                                                         "no_edges"])
def test_degenerate_blocks(margin, degs):
    col, row, nd, ns = R.block_layout(degs, True, 0)
    rng = np.random.RandomState(40 + len(degs))
    E, H, P = len(col), 2, 3
    c = dict(col=col, row=row, num_dst=nd, num_src=ns)
    src = rng.randn(ns, H, P).astype(np.float32)
    grad = rng.randn(nd, H, P).astype(np.float32)
    for tag, b in _blocks(c):
        check_reduce(margin, tag, b, src, rng.randn(E, H).astype(np.float32), grad)
        check_softmax(margin, tag, b, rng.randn(E, H).astype(np.float32),
                      rng.randn(E, H).astype(np.float32))
        check_max(margin, tag, b, src.reshape(ns, -1), grad.reshape(nd, -1))


# ---- ties in max ----------------------------------------------------------------------------------
@pytest.mark.parametrize("sampler_layout", [True, False], ids=["sampler", "general"])
def test_max_ties_go_to_lowest_edge(margin, sampler_layout):
    """Integer features in {0, 1, 2}: the gradient of a tied max goes to the lowest edge of
    the segment (exactly, where each source row feeds one edge).  The tie share is a
    condition that keeps the test meaningful, not a measurement."""
    c = R.tie_case(sampler_layout)
    L = (c["col"], c["row"], c["num_dst"], c["num_src"])
    assert R.tie_fraction(*L, c["src"]) >= 0.25
    for tag, b in _blocks(c):
        check_max(margin, tag, b, c["src"], c["grad"])


def test_sage_pool_layer_gradient_on_sampler_block(margin):
    """SAGEConv('pool') on a sampled block against a float64 evaluation of the same layer.

    Integer inputs and an integer fc_pool make relu(fc_pool(x)) exact in fp32 and full of tied
    zeros, so the max routes its gradient by the lowest-edge rule in both evaluations.  The
    remaining fp32 work is GEMMs and sums: each result is bounded by gamma_K times the same
    chain evaluated on absolute values, K the total length of the sums along the chain."""
    import torch
    from gnnflow_amd import TemporalSampler
    from gnnflow_amd import nn as gnn
    g, N = _graph(False)
    rng = np.random.RandomState(50)
    b = TemporalSampler(g, [10], "recent").sample(
        rng.randint(0, N, 200).astype(np.int64), np.full(200, 2.0, np.float32))[0][0]
    _assert_sampler_layout(b)
    col, row, nd, ns = _layout(b)
    fin, fout = 12, 8
    torch.manual_seed(51)
    layer = gnn.SAGEConv(fin, fout, "pool").cuda().eval()
    with torch.no_grad():
        layer.fc_pool.weight.copy_(_dev(rng.randint(-1, 2, (fin, fin)).astype(np.float32)))
        layer.fc_pool.bias.copy_(_dev(rng.randint(-1, 2, fin).astype(np.float32)))
        layer.bias.copy_(_dev(rng.randn(fout).astype(np.float32)))
    x = rng.randint(0, 2, (ns, fin)).astype(np.float32)
    G = rng.randn(nd, fout).astype(np.float32)
    out = layer(b, _dev(x))
    (out * _dev(G)).sum().backward()

    p = {k: _np(v).astype(np.float64) for k, v in layer.named_parameters()}
    x64, G64 = x.astype(np.float64), G.astype(np.float64)
    Wp, bp, Ws, Wn, bias = (p["fc_pool.weight"], p["fc_pool.bias"], p["fc_self.weight"],
                            p["fc_neigh.weight"], p["bias"])
    L = (col, row, nd, ns)
    pre = x64 @ Wp.T + bp
    z = np.maximum(pre, 0)
    pooled, arg = R.max_fwd(*L, z)
    assert R.tie_fraction(*L, z) >= 0.25
    live = (pre > 0).astype(np.float64)
    dpre = R.max_bwd(*L, arg, G64 @ Wn) * live
    adpre = R.max_bwd(*L, arg, np.abs(G64) @ np.abs(Wn)) * live
    ax, aG = np.abs(x64), np.abs(G64)

    def bound(K, a):
        return (R.gamma(K) + 4 * K * R.U64) * a

    margin.check("out", _np(out), x64[:nd] @ Ws.T + pooled @ Wn.T + bias,
                 bound(fin + 2, ax[:nd] @ np.abs(Ws).T + pooled @ np.abs(Wn).T + np.abs(bias)))
    grads = {k: _np(v.grad) for k, v in layer.named_parameters()}
    margin.check("fc_self", grads["fc_self.weight"], G64.T @ x64[:nd], bound(nd, aG.T @ ax[:nd]))
    margin.check("fc_neigh", grads["fc_neigh.weight"], G64.T @ pooled, bound(nd, aG.T @ pooled))
    margin.check("bias", grads["bias"], G64.sum(0), bound(nd, aG.sum(0)))
    margin.check("fc_pool.weight", grads["fc_pool.weight"], dpre.T @ x64,
                 bound(ns + fout, adpre.T @ ax))
    margin.check("fc_pool.bias", grads["fc_pool.bias"], dpre.sum(0), bound(ns + fout, adpre.sum(0)))


# ---- softmax edges ---------------------------------------------------------------------------------
@pytest.mark.parametrize("wave", [False, True], ids=["thread", "wave"])
@pytest.mark.parametrize("kind", ["shift", "masked", "all_masked"])
def test_softmax_shifted_and_masked_logits(margin, kind, wave):
    c = R.softmax_edge_case(kind, wave)
    E, nd = len(c["col"]), c["num_dst"]
    assert (E > 32 * nd) == wave
    for tag, b in _blocks(c):
        y = check_softmax(margin, tag, b, c["logits"], c["grad_y"])
        if kind == "all_masked":
            assert np.isnan(y).any()
