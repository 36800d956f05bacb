"""ops.block_gat on a bfloat16 feat (csrc/block_gat.hip) against the float32 op on the
widened feat, bit for bit, forward and backward, with and without dropout:

    out, grad_feat:            bf16_op(x)  ==  fp32_op(x.float()).to(torch.bfloat16)
    att, grad_el, grad_er:     torch.equal

el and er are float32 on both sides; the gradient fed to the float32 op is the bfloat16 gradient
widened.  No tolerance: the same float32 instruction sequence on the same values (the float32 op
is checked against float64 in tests/test_gpu_block_gat.py).  The backward's dot = gout . out uses
the forward's out BEFORE rounding, or grad_el / grad_er would not be equal.

Blocks as in tests/test_gpu_block_ops_bf16.py (sampler layout, an explicit col reading each
source at most once, the same shuffled).  Where several edges read one source the float32
atomics' order is not fixed and the softmax is not exact: that block is checked within half a
bfloat16 step plus the bound the float32 op is granted."""
import numpy as np
import pytest

from tests import block_gat_ref as Gr
from tests.test_gpu_block_attention_bf16 import same_bits
from tests.test_gpu_block_ops_bf16 import _bf16, _f32, _unread, blocks, layouts  # noqa: F401

pytestmark = pytest.mark.gpu

NAMES = ("feat", "el", "er")
SEED = Gr.SEED


def run(b, x, need, wide, return_attention=True, **kw):
    import torch
    from gnnflow_amd import ops
    feat = (x["feat"].float() if wide else x["feat"].clone()).requires_grad_("feat" in need)
    el = x["el"].clone().requires_grad_("el" in need)
    er = x["er"].clone().requires_grad_("er" in need)
    res = ops.block_gat(b, feat, el, er, negative_slope=0.2, return_attention=return_attention,
                        **kw)
    out, att = res if return_attention else (res, None)
    assert out.dtype == feat.dtype and out.shape == (b.num_dst_nodes(),) + tuple(feat.shape[1:])
    out.backward(x["gout"].float() if wide else x["gout"])
    got = dict(out=out.detach())
    if att is not None:
        assert att.dtype == torch.float32 and not att.requires_grad
        got["att"] = att
    for n, t in zip(NAMES, (feat, el, er)):
        assert (t.grad is not None) == (n in need)
        if t.grad is not None:
            assert t.grad.dtype == t.dtype
            got["g" + n] = t.grad
    return got


def check(b, x, need=NAMES, **kw):
    import torch
    got, want = run(b, x, need, False, **kw), run(b, x, need, True, **kw)
    assert sorted(got) == sorted(want)
    for n in got:
        if n in ("out", "gfeat"):
            assert same_bits(got[n], want[n].to(torch.bfloat16)), n
        else:
            assert torch.equal(got[n], want[n]), n
    return got


def inputs(b, H, D, seed):
    rng = np.random.RandomState(seed)
    return dict(feat=_bf16(rng.randn(b.num_src_nodes(), H, D)),
                el=_f32(rng.randn(b.num_src_nodes(), H)), er=_f32(rng.randn(b.num_dst_nodes(), H)),
                gout=_bf16(rng.randn(b.num_dst_nodes(), H, D)))


# one D per branch of the dispatch that matters: G = 8, 16, 64 with NC = 1 (50), NC = 2 (100) and
# NC = 4 with a ragged last chunk (130)
@pytest.mark.parametrize("D", [3, 16, 50, 100, 130])
@pytest.mark.parametrize("H", [1, 3])
def test_bit_contract(blocks, H, D):
    import torch
    for name, b in blocks.items():
        x = inputs(b, H, D, 5000 + 10 * D + H)
        unread = torch.from_numpy(_unread(b)).cuda()
        for kw in ({}, dict(dropout_p=0.5, dropout_seed=SEED)):
            got = check(b, x, **kw)
            assert not got["out"][[0, 6]].any() and not got["ger"][[0, 6]].any()
            assert not got["gfeat"][unread].any() and not got["gel"][unread].any()
            if kw:
                assert (got["att"] == 0).any() and (got["att"] != 0).any()
            check(b, x, return_attention=False, **kw)
            for need in NAMES:
                check(b, x, (need,), **kw)


def test_two_runs_on_the_sampler_layout_are_bit_identical(blocks):
    import torch
    b = blocks["sampler"]
    x = inputs(b, 3, 50, 5100)
    for kw in ({}, dict(dropout_p=0.5, dropout_seed=SEED)):
        first, second = run(b, x, NAMES, False, **kw), run(b, x, NAMES, False, **kw)
        for n in first:
            a, c = first[n], second[n]
            if a.dtype == torch.bfloat16:
                a, c = a.view(torch.int16), c.view(torch.int16)
            assert torch.equal(a, c), n


def test_several_edges_reading_one_source():
    """The shuffled block of tests/block_gat_ref.py: 13 sources feed several edges each, one feeds
    none.  feat and the gradient are strictly positive, so nothing cancels in grad_feat.  The
    bfloat16 op's grad_feat is its float32 sum rounded once: half a bfloat16 step, 2^-8 |r|, from
    it, and that sum and the float32 op's r differ by the order of the float32 adds, for which
    tests/test_gpu_block_gat.py grants the float32 op the a priori bound of
    tests/block_gat_ref.py (taken here on the same widened inputs).  The same for grad_el."""
    import torch
    from tests.test_gpu_block_gat import _block
    c = Gr.unordered_case()
    rng = np.random.RandomState(5200)
    for n in ("feat", "gout"):
        c[n] = _bf16(rng.uniform(0.5, 2.0, c[n].shape)).float().cpu().numpy()
    b = _block(c)
    assert b.segments()[1] is not None and b.segments()[2] is not None
    x = dict(feat=_bf16(c["feat"]), el=_f32(c["el"]), er=_f32(c["er"]), gout=_bf16(c["gout"]))
    assert np.array_equal(x["feat"].float().cpu().numpy(), c["feat"])
    for p, seed in ((0.0, 0), (0.5, SEED)):
        kw = dict(dropout_p=p, dropout_seed=seed) if p else {}
        ref = Gr.reference(c, p, seed)
        got, r = run(b, x, NAMES, False, **kw), run(b, x, NAMES, True, **kw)
        assert same_bits(got["out"], r["out"].to(torch.bfloat16))
        assert torch.equal(got["att"], r["att"]) and torch.equal(got["ger"], r["ger"])
        for n, bound in (("gfeat", ref.b_gfeat), ("gel", ref.b_gel)):
            mine, theirs = (t.float().cpu().numpy().astype(np.float64) for t in (got[n], r[n]))
            tol = 2.0 ** -8 * np.abs(theirs) + bound.reshape(theirs.shape)
            worst = float((np.abs(mine - theirs) / np.maximum(tol, 1e-300)).max())
            print("\n[error/tolerance] p={} {}: {:.3g}".format(p, n, worst))
            assert (np.abs(mine - theirs) <= tol).all(), (p, n, worst)
        assert ref.unread[13]                              # rows no edge reads: exact zeros
        assert not got["gfeat"][13].any() and not got["gel"][13].any()


def test_no_edges_and_wrong_gradient_dtype():
    import torch
    from gnnflow_amd import ops
    from tests.test_gpu_block_ops_fp64 import _explicit
    from tests import block_ops_ref as R
    b = _explicit(*R.block_layout([0, 0, 0], True, 0))
    x = inputs(b, 2, 5, 5300)
    feat = x["feat"].requires_grad_()
    out, att = ops.block_gat(b, feat, x["el"], x["er"], return_attention=True)
    assert out.dtype == torch.bfloat16 and not out.any() and att.shape == (0, 2)
    out.sum().backward()
    assert feat.grad.dtype == torch.bfloat16 and not feat.grad.any()
    b = _explicit(*R.block_layout([2, 1], True, 0))
    x = inputs(b, 2, 5, 5301)
    out = ops.block_gat(b, x["feat"].requires_grad_(), x["el"], x["er"])
    with pytest.raises(TypeError, match="bfloat16.*float32"):
        out.grad_fn.apply(torch.ones(2, 2, 5, device="cuda"), None)
