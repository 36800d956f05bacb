"""ops.block_reduce and ops.block_max on bfloat16 source rows (csrc/block_ops.hip) against
the float32 ops on the widened inputs, bit for bit, forward and backward:

    bf16_op(x, ...)  ==  fp32_op(x.float(), ...).to(torch.bfloat16)        x bfloat16

on the raw 16-bit patterns; the float32 results (the gradient of the edge weights, the argmax)
with torch.equal.  The gradient fed to the float32 op is the bfloat16 gradient widened.  The
library is built with -ffp-contract=off and without fast-math and the bfloat16 kernels run the
float32 kernels' arithmetic in the same order, so no tolerance is involved; the float32 ops are
checked against float64 in tests/test_gpu_block_ops_fp64.py.

Three blocks over the in-degrees [0, 1, 3, 10, 2, 5, 0]: the sampler's layout (col None: direct
bfloat16 stores), an explicit col that reads every source at most once and some not at all (the
float32 scratch; one add into zero per element, so the order of atomics cannot matter), and the
same with its edges shuffled (the perm path).  A fourth block lets several edges read one source;
there the inputs are multiples of 1/8 so that every sum is exact and bit equality still holds."""
import numpy as np
import pytest

from tests import block_ops_ref as R
from tests.test_gpu_block_attention_bf16 import same_bits
from tests.test_gpu_block_ops_fp64 import _col_less, _explicit

pytestmark = pytest.mark.gpu

DEGS = [0, 1, 3, 10, 2, 5, 0]
DIMS = [1, 63, 64, 65, 130]
UNREAD = 3            # sources of the explicit-col blocks that no edge reads, besides the rest


def layouts():
    """name -> (col, row, num_dst, num_src) on the host."""
    col, row, nd, ns = R.block_layout(DEGS, True, 0)
    E = len(row)
    rng = np.random.RandomState(70)
    num_src = ns + UNREAD
    pcol = rng.permutation(num_src)[:E].astype(np.int64)      # every source at most once
    shuffle = rng.permutation(E)
    return {"sampler": (col, row, nd, ns), "permutation": (pcol, row, nd, num_src),
            "unordered": (pcol[shuffle], row[shuffle], nd, num_src)}


@pytest.fixture(scope="module")
def blocks():
    L = layouts()
    out = {"sampler": _col_less(*L["sampler"]), "permutation": _explicit(*L["permutation"]),
           "unordered": _explicit(*L["unordered"])}
    assert out["sampler"].segments()[1] is None
    assert out["permutation"].segments()[1] is not None
    assert out["permutation"].segments()[2] is None and out["unordered"].segments()[2] is not None
    for name in ("permutation", "unordered"):
        reads = np.bincount(L[name][0], minlength=L[name][3])
        assert reads.max() == 1 and (reads == 0).sum() >= UNREAD
    return out


def _bf16(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda().to(torch.bfloat16)


def _f32(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def run_reduce(b, x, w, g, mean, need, wide):
    """block_reduce forward + backward on bfloat16 x and g, or on their widening."""
    import torch
    from gnnflow_amd import ops
    cast = (lambda t: t.float()) if wide else (lambda t: t.clone())
    xs = cast(x).requires_grad_("src" in need)
    ws = w.clone().requires_grad_("w" in need) if w is not None else None
    out = ops.block_reduce(b, xs, ws, mean=mean)
    assert out.dtype == xs.dtype and out.shape == (b.num_dst_nodes(),) + tuple(x.shape[1:])
    out.backward(cast(g))
    res = dict(out=out.detach())
    if "src" in need:
        assert xs.grad.dtype == xs.dtype
        res["gsrc"] = xs.grad
    if "w" in need:
        assert ws.grad.dtype == torch.float32
        res["gw"] = ws.grad
    return res


def check_reduce(b, x, w, g, mean, need=("src",)):
    import torch
    got = run_reduce(b, x, w, g, mean, need, wide=False)
    want = run_reduce(b, x, w, g, mean, need, wide=True)
    assert sorted(got) == sorted(want)
    for n in got:
        if n == "gw":
            assert torch.equal(got[n], want[n]), n
        else:
            assert same_bits(got[n], want[n].to(torch.bfloat16)), n
    return got


def run_max(b, x, g, wide):
    from gnnflow_amd import ops
    cast = (lambda t: t.float()) if wide else (lambda t: t.clone())
    xs = cast(x).requires_grad_()
    out = ops.block_max(b, xs)
    assert out.dtype == xs.dtype
    arg = out.grad_fn.saved_tensors[0]          # the winning edge per element, as saved
    out.backward(cast(g))
    assert xs.grad.dtype == xs.dtype
    return dict(out=out.detach(), arg=arg, gsrc=xs.grad)


def check_max(b, x, g):
    import torch
    got, want = run_max(b, x, g, wide=False), run_max(b, x, g, wide=True)
    assert torch.equal(got["arg"], want["arg"])
    for n in ("out", "gsrc"):
        assert same_bits(got[n], want[n].to(torch.bfloat16)), n
    return got


def _unread(b):
    col = b.edges()[0].cpu().numpy()
    return np.flatnonzero(np.bincount(col, minlength=b.num_src_nodes()) == 0)


@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("name", ["sampler", "permutation", "unordered"])
def test_copy_reduce_and_max(blocks, name, dim):
    import torch
    b = blocks[name]
    rng = np.random.RandomState(1000 + dim)
    x = _bf16(rng.randn(b.num_src_nodes(), dim))
    g = _bf16(rng.randn(b.num_dst_nodes(), dim))
    unread = torch.from_numpy(_unread(b)).cuda()
    for mean in (False, True):
        got = check_reduce(b, x, None, g, mean)
        assert not got["out"][[0, 6]].any()                 # the empty first and last segment
        assert not got["gsrc"][unread].any()                # rows no edge reads: exact zeros
    got = check_max(b, x, g)
    assert not got["out"][[0, 6]].any() and not got["out"][[0, 6]].view(torch.int16).any()  # +0
    assert (got["arg"][[0, 6]] == -1).all() and (got["arg"][1:6] >= 0).all()
    assert not got["gsrc"][unread].any()


@pytest.mark.parametrize("dim,heads", [(130, 2), (64, 64), (6, 3)])
@pytest.mark.parametrize("name", ["sampler", "permutation", "unordered"])
def test_weighted_reduce(blocks, name, dim, heads):
    b = blocks[name]
    rng = np.random.RandomState(2000 + dim)
    x = _bf16(rng.randn(b.num_src_nodes(), dim))
    g = _bf16(rng.randn(b.num_dst_nodes(), dim))
    w = _f32(rng.randn(b.num_edges(), heads))
    for mean in (False, True):
        for need in (("src", "w"), ("src",), ("w",)):
            check_reduce(b, x, w, g, mean, need)
    # the [E, heads, 1] weights GATConv passes, and a 3-D source
    got = check_reduce(b, x.reshape(-1, heads, dim // heads), w.reshape(-1, heads, 1),
                       g.reshape(-1, heads, dim // heads), False, ("src", "w"))
    assert got["out"].shape == (b.num_dst_nodes(), heads, dim // heads)


def test_ties_in_max_go_to_the_lowest_edge(blocks):
    """Values in {0, 1, 2}: many ties, and +0 against -0 (equal, so the lower edge keeps it)."""
    rng = np.random.RandomState(3000)
    for name, b in blocks.items():
        x = rng.randint(0, 3, (b.num_src_nodes(), 65)).astype(np.float32)
        x[rng.rand(*x.shape) < 0.2] = -0.0
        check_max(b, _bf16(x), _bf16(rng.randn(b.num_dst_nodes(), 65)))


def _eighths(rng, shape):
    return rng.randint(-32, 33, shape).astype(np.float32) / 8.0


@pytest.mark.parametrize("dim,heads", [(65, 1), (130, 2), (6, 3)])
def test_several_edges_reading_one_source_exact_arithmetic(dim, heads):
    """An explicit col in which a source feeds up to 8 edges: float32 atomic adds into the
    scratch in an order that is not fixed.  Inputs, weights and gradients are k / 8 with
    |k| <= 32, mean=False: every product is a multiple of 1/64 below 16 and every sum stays far
    below 2^24 / 64, hence exact in float32 whatever the order, and bit equality is required."""
    col, row, nd, ns = R.block_layout(DEGS, False, 71)
    reads = np.bincount(col, minlength=ns)
    assert 2 <= reads.max() <= 8 and (reads == 0).any()
    rng = np.random.RandomState(72)
    p = rng.permutation(len(row))
    for b in (_explicit(col, row, nd, ns), _explicit(col[p], row[p], nd, ns)):
        x, g = _bf16(_eighths(rng, (ns, dim))), _bf16(_eighths(rng, (nd, dim)))
        w = _f32(_eighths(rng, (len(row), heads)))
        assert np.array_equal(x.float().cpu().numpy() * 8, np.round(x.float().cpu().numpy() * 8))
        check_reduce(b, x, None, g, False)
        got = check_reduce(b, x, w, g, False, ("src", "w"))
        assert not got["gsrc"][np.flatnonzero(reads == 0)].any()
        check_max(b, x, g)


def test_no_edges_and_wrong_gradient_dtype():
    import torch
    from gnnflow_amd import ops
    col, row, nd, ns = R.block_layout([0, 0, 0], True, 0)
    b = _explicit(col, row, nd, ns)
    x = _bf16(np.ones((ns, 5))).requires_grad_()
    for out in (ops.block_reduce(b, x), ops.block_max(b, x)):
        assert out.dtype == torch.bfloat16 and out.shape == (3, 5) and not out.any()
        x.grad = None
        out.backward(torch.ones_like(out))
        assert x.grad.dtype == torch.bfloat16 and not x.grad.any()
    b = _explicit(*R.block_layout([2, 1], True, 0))
    x = _bf16(np.ones((5, 4))).requires_grad_()
    for op in (ops.block_reduce, ops.block_max):
        out = op(b, x)
        with pytest.raises(TypeError, match="bfloat16.*float32"):
            out.grad_fn.apply(torch.ones(2, 4, device="cuda"))      # a float32 gradient


def test_update_all_takes_bfloat16_rows(blocks):
    import torch
    import gnnflow_amd.function as fn
    b = blocks["sampler"]
    rng = np.random.RandomState(4000)
    x = _bf16(rng.randn(b.num_src_nodes(), 2, 9))
    a = _f32(rng.rand(b.num_edges(), 2, 1))
    b.srcdata["v"], b.edata["a"] = x, a
    b.update_all(fn.u_mul_e("v", "a", "m"), fn.sum("m", "h"))
    from gnnflow_amd import ops
    assert same_bits(b.dstdata["h"], ops.block_reduce(b, x.float(), a).to(torch.bfloat16))
    b.update_all(fn.copy_src("v", "m"), fn.max("m", "h"))
    assert same_bits(b.dstdata["h"], ops.block_max(b, x.float()).to(torch.bfloat16))
