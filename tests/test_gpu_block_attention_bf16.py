"""ops.block_attention on bfloat16 q, k, v (csrc/block_attention.hip) against the float32 op
on the widened inputs, bit for bit, forward and backward, with and without dropout:

    bf16_op(x.bfloat16(), ...)  ==  fp32_op(x.bfloat16().float(), ...).to(torch.bfloat16)

on the raw 16-bit patterns (NaNs by position); the float32 attention with torch.equal.  The
library is built with -ffp-contract=off and without fast-math and the bfloat16 kernels run the
float32 kernels' arithmetic in the same order, so no tolerance is involved; the float32 op itself
is checked against float64 in tests/test_gpu_block_attention*.py."""
import numpy as np
import pytest

from tests import attention_dropout_ref as R
from tests import block_attention_ref as A

pytestmark = pytest.mark.gpu

NAMES = ("q", "k", "v")


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _block(row, num_dst):
    from gnnflow_amd import MFGBlock
    E = len(row)
    return MFGBlock(num_dst + E, num_dst, _dev(num_dst + np.arange(E, dtype=np.int64)),
                    _dev(np.asarray(row, np.int64)))


def same_bits(got, want):
    """Two bfloat16 tensors hold the same 16-bit patterns; NaNs are compared by position."""
    import torch
    assert got.dtype == torch.bfloat16 and want.dtype == torch.bfloat16
    assert got.shape == want.shape
    ng, nw = got.isnan(), want.isnan()
    return torch.equal(ng, nw) and \
        torch.equal(got.contiguous().view(torch.int16)[~ng], want.contiguous().view(torch.int16)[~nw])


def bf16_inputs(c):
    """q, k, v, gout of a case rounded to bfloat16 (what both sides start from)."""
    import torch
    return {n: _dev(c[n]).to(torch.bfloat16) for n in NAMES + ("gout",)}


def run(b, x, slope, need=NAMES, wide=False, **kw):
    """Forward + backward on the bfloat16 tensors of `x`, or on their widening -> dict."""
    import torch
    from gnnflow_amd import ops
    cast = (lambda t: t.float()) if wide else (lambda t: t.clone())
    q, k, v = (cast(x[n]).requires_grad_(n in need) for n in NAMES)
    out, att = ops.block_attention(b, q, k, v, negative_slope=slope, return_attention=True, **kw)
    assert out.dtype == q.dtype and att.dtype == torch.float32 and not att.requires_grad
    assert out.shape == q.shape
    if need:
        out.backward(cast(x["gout"]))
    res = dict(out=out.detach(), att=att)
    for n, t in zip(NAMES, (q, k, v)):
        assert (t.grad is not None) == (n in need)
        if t.grad is not None:
            assert t.grad.dtype == t.dtype
            res["g" + n] = t.grad
    return res


def check(b, c, need=NAMES, **kw):
    """The acceptance criterion on one case; returns the bfloat16 results."""
    import torch
    x = bf16_inputs(c)
    got = run(b, x, c["slope"], need, **kw)
    want = run(b, x, c["slope"], need, wide=True, **kw)
    assert sorted(got) == sorted(want)
    for n in got:
        if n == "att":
            assert torch.equal(got[n], want[n]), n
        else:
            assert same_bits(got[n], want[n].to(torch.bfloat16)), n
    return got


@pytest.fixture(scope="module")
def sampler_blocks():
    """150 roots, fanout [10, 10], as tests/test_gpu_block_attention.py builds them."""
    from gnnflow_amd import DynamicGraph, TemporalSampler
    rng = np.random.RandomState(20)
    N, E = 300, 5000
    src, dst = rng.randint(0, N, E), rng.randint(0, N, E)
    ts = np.sort(rng.rand(E)).astype(np.float32)
    g = DynamicGraph(1 << 20, 64 << 20, "cuda", 16, 64, "insert")
    g.add_edges(src.astype(np.int64), dst.astype(np.int64), ts, add_reverse=True)
    rng = np.random.RandomState(22)
    mfgs = TemporalSampler(g, [10, 10], "recent", seed=5).sample(
        rng.randint(0, N, 150).astype(np.int64), rng.uniform(0.6, 1.0, 150).astype(np.float32))
    blocks = [b for layer in mfgs for b in layer if b.num_edges()]
    assert len(blocks) == 2
    return blocks


def _sampler_case(b, li):
    return A.make_inputs(b.edges()[1].cpu().numpy(), b.num_dst_nodes(), 2, 50, 950 + li)


def test_sampler_blocks(sampler_blocks):
    for li, b in enumerate(sampler_blocks):
        assert b.segments()[1] is None and b.segments()[2] is None
        check(b, _sampler_case(b, li))


@pytest.mark.parametrize("H,D", A.SHAPES, ids=["{}x{}".format(*s) for s in A.SHAPES])
def test_head_shapes(H, D):
    """Every lane-group size G = 8 .. 64, the sizes around them, NC = 2 (65) and NC = 4 (129)."""
    c = A.shape_case(H, D)
    check(_block(c["row"], 40), c)


@pytest.mark.parametrize("H,D", [(1, 300), (1, 1024)], ids=["1x300", "1x1024"])
def test_many_columns_per_lane(H, D):
    """NC = 8 and NC = 16, the widest head."""
    c = A.make_inputs(A.rows_of([3, 0, 1, 5]), 4, H, D, 940 + D)
    check(_block(c["row"], 4), c)


@pytest.mark.parametrize("degs", [[], [0], [0] * 5, [1], [1] * 9, [4, 0, 7]],
                         ids=["no_dst", "no_edge", "all_degree_0", "single_edge", "all_degree_1",
                              "gap"])
def test_degenerate_blocks(degs):
    import torch
    row = A.rows_of(degs)
    c = A.make_inputs(row, len(degs), 2, 5, 960 + len(degs))
    got = check(_block(row, len(degs)), c)
    if len(row) == 0:      # bfloat16 zeros and bfloat16 zero gradients
        for n in ("out", "gq", "gk", "gv"):
            assert got[n].dtype == torch.bfloat16 and not got[n].any(), n
    if degs in ([1], [1] * 9):
        assert (got["att"] == 1).all()
        assert same_bits(got["out"], bf16_inputs(c)["v"])
    if degs == [4, 0, 7]:
        assert not got["out"][1].any() and not got["gq"][1].any()


def test_long_segment_among_short():
    c = A.long_segment_case()
    assert np.bincount(c["row"]).max() == 3000          # far more than 64 edges
    check(_block(c["row"], c["num_dst"]), c)


def test_unordered_block_goes_through_perm():
    c = A.unordered_case()
    b = _block(c["row"], c["num_dst"])
    assert b.segments()[2] is not None
    check(b, c)                                          # att, gk, gv in the caller's order
    check(b, c, dropout_p=R.P, dropout_seed=R.SEED)


@pytest.mark.parametrize("need", [("q",), ("k", "v"), NAMES, ()], ids=["q", "kv", "qkv", "none"])
def test_gradient_subsets(need):
    c = A.shape_case(2, 50)
    check(_block(c["row"], 40), c, need)
    check(_block(c["row"], 40), c, need, dropout_p=R.P, dropout_seed=R.SEED)


def test_2d_inputs_and_non_contiguous_k():
    import torch
    from gnnflow_amd import ops
    c = A.shape_case(3, 21)
    b = _block(c["row"], 40)
    x = bf16_inputs(c)
    base = run(b, x, c["slope"])
    wide = torch.cat([x["k"], x["k"]], dim=2)
    k = wide[:, :, :21].requires_grad_(True)
    qT = x["q"].transpose(0, 1).contiguous().transpose(0, 1).requires_grad_(True)
    assert not k.is_contiguous() and not qT.is_contiguous()
    out = ops.block_attention(b, qT, k, x["v"], c["slope"])
    out.backward(x["gout"])
    assert same_bits(out.detach(), base["out"])
    assert same_bits(k.grad, base["gk"]) and same_bits(qT.grad, base["gq"])
    flat = [x[n].reshape(x[n].shape[0], -1) for n in NAMES]
    out2 = ops.block_attention(b, *flat, negative_slope=c["slope"], heads=3)
    assert out2.shape == (40, 3, 21) and same_bits(out2, base["out"])
    with pytest.raises(ValueError):
        ops.block_attention(b, *flat)                    # 2-D without heads=


@pytest.mark.parametrize("p", [0.5, 2.0 ** -7], ids=["p0.5", "p_near_0"])
def test_dropout_on_sampler_blocks(sampler_blocks, p):
    """check() compares the returned attention too: with dropout that is the DROPPED attention."""
    for li, b in enumerate(sampler_blocks):
        c = _sampler_case(b, li)
        got = check(b, c, dropout_p=p, dropout_seed=R.SEED)
        keep = R.keep_mask(len(c["row"]), 2, p, R.SEED)   # sorted rows: grouped order = given
        assert np.array_equal(got["att"].cpu().numpy() != 0, keep)
        assert not keep.all()
        assert not got["gv"][_dev(~keep)].any()


@pytest.mark.parametrize("H,D", [(1, 65), (2, 129)], ids=["1x65", "2x129"])
def test_dropout_with_several_columns_per_lane(H, D):
    c = A.shape_case(H, D)
    check(_block(c["row"], 40), c, dropout_p=R.P, dropout_seed=R.SEED)


DISPATCH_ROWS = [(2, 8), (2, 16), (2, 32), (2, 64), (2, 65), (2, 129), (2, 257), (1, 513)]


@pytest.mark.parametrize("H,D", DISPATCH_ROWS, ids=["{}x{}".format(*s) for s in DISPATCH_ROWS])
def test_dropout_on_every_dispatch_row(H, D):
    """A kernel template is compiled only where it is instantiated: every (G, NC) the dispatch can
    choose, for both element types, forward and backward, with dropout, on a block with a
    destination without in-edges and one whose 70 edges take a 64-lane group round twice.  The
    rows without dropout are run by test_head_shapes and test_many_columns_per_lane."""
    degs = [2, 0, 70, 1, 3]
    c = A.make_inputs(A.rows_of(degs), len(degs), H, D, 970 + D)
    got = check(_block(c["row"], len(degs)), c, dropout_p=R.P, dropout_seed=R.SEED)
    assert not got["out"][1].any() and not got["gq"][1].any()


def test_non_finite_v_on_a_dropped_edge_does_not_propagate():
    import torch
    c = A.shape_case(2, 50)
    keep = R.keep_mask(len(c["row"]), 2, R.P, R.SEED)
    dropped = np.argwhere(~keep)
    assert len(dropped) >= 3
    c = dict(c, v=c["v"].copy())
    for (e, h), bad in zip(dropped[:3], (np.inf, -np.inf, np.nan)):
        c["v"][e, h, :] = bad
    got = check(_block(c["row"], 40), c, dropout_p=R.P, dropout_seed=R.SEED)
    for n in ("out", "gq", "gk", "gv"):
        assert torch.isfinite(got[n].float()).all(), n


def test_two_runs_are_bit_identical():
    import torch
    c = A.long_segment_case()
    b = _block(c["row"], c["num_dst"])
    x = bf16_inputs(c)
    for kw in ({}, dict(dropout_p=R.P, dropout_seed=R.SEED_B)):
        first, second = run(b, x, c["slope"], **kw), run(b, x, c["slope"], **kw)
        for n in first:
            assert torch.equal(first[n].view(torch.int16) if n != "att" else first[n],
                               second[n].view(torch.int16) if n != "att" else second[n]), n


def test_mixed_and_other_dtypes_raise():
    c = A.shape_case(2, 50)
    b = _block(c["row"], 40)
    x = bf16_inputs(c)
    with pytest.raises(TypeError, match="float32.*bfloat16"):
        from gnnflow_amd import ops
        ops.block_attention(b, x["q"].float(), x["k"], x["v"])
    with pytest.raises(TypeError):
        ops.block_attention(b, x["q"].half(), x["k"].half(), x["v"].half())
