"""models.SAGE and models.GAT on the GPU, on a 2-layer synthetic block pair whose 4 positive edges
give 12 roots at neg_sample_ratio 1 and 20 at 3: output shapes, equality with a plain-torch
restatement of the forward on the same parameters (float32, the tolerance of
tests/test_gpu_block_ops.py), one optimiser step under bfloat16 autocast, and the example with
--model gat --amp."""
import importlib.util
import math
import os

import numpy as np
import pytest

from tests.test_gpu_block_ops import TOL, _block, ref_edge_softmax, ref_reduce

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POS, DIM_IN, DIM_OUT = 4, 20, 12


def _mfgs(ratio, seed=90):
    """[[outer block], [roots' block]] with srcdata['h'] on the outer one."""
    import torch
    rng = np.random.RandomState(seed + ratio)
    roots = POS * (ratio + 2)
    inner = _block(roots, rng.randint(0, 6, roots), seed + 1)
    outer = _block(inner.num_src_nodes(), rng.randint(0, 6, inner.num_src_nodes()), seed + 2)
    outer.srcdata['h'] = torch.from_numpy(
        rng.randn(outer.num_src_nodes(), DIM_IN).astype(np.float32)).cuda()
    return [[outer], [inner]]


def _score(model, h, ratio):
    src, pos, neg = h[:POS], h[POS:2 * POS], h[2 * POS:]
    return model.predictor(src * pos), model.predictor(src.tile(ratio, 1) * neg)


def _sage_by_hand(model, mfgs, ratio):
    import torch.nn.functional as F
    h = mfgs[0][0].srcdata['h']
    for l in range(2):
        layer, b = model.layers['l{}h0'.format(l)], mfgs[l][0]
        col, row = b.edges()
        nd = b.num_dst_nodes()
        neigh = ref_reduce(col, row, h, None, nd, True)
        h = layer.fc_self(h[:nd]) + layer.fc_neigh(neigh) + layer.bias
        if l == 0:
            h = F.relu(h)
    return _score(model, h, ratio)


def _gat_by_hand(model, mfgs, ratio):
    import torch
    import torch.nn.functional as F
    h = mfgs[0][0].srcdata['h']
    for l in range(2):
        layer, b = model.layers['l{}h0'.format(l)], mfgs[l][0]
        col, row = b.edges()
        nd, H = b.num_dst_nodes(), layer._num_heads
        ft = layer.fc(h).view(-1, H, DIM_OUT)
        el, er = (ft * layer.attn_l).sum(-1), (ft[:nd] * layer.attn_r).sum(-1)
        a = ref_edge_softmax(row, F.leaky_relu(el[col] + er[row], 0.2), nd)
        h = torch.zeros(nd, H, DIM_OUT, device="cuda").index_add(0, row, ft[col] * a[:, :, None])
        h = h + layer.bias.view(1, H, DIM_OUT)
        h = F.elu(h).flatten(1) if l == 0 else h.mean(1)
    return _score(model, h, ratio)


def _model(name):
    import torch
    from gnnflow_amd import models
    torch.manual_seed(91)
    model = models.SAGE(DIM_IN, DIM_OUT) if name == "sage" else \
        models.GAT(DIM_IN, DIM_OUT, attn_head=[2, 1])
    with torch.no_grad():
        for layer in model.layers.values():
            layer.bias.uniform_(-1, 1)
    return model.cuda()


@pytest.mark.parametrize("ratio", [1, 3])
@pytest.mark.parametrize("name", ["sage", "gat"])
def test_forward_matches_a_plain_torch_restatement(name, ratio):
    import torch
    model = _model(name)
    mfgs = _mfgs(ratio)
    assert mfgs[1][0].num_dst_nodes() == {1: 12, 3: 20}[ratio]
    pos, neg = model(mfgs, neg_sample_ratio=ratio)
    assert pos.shape == (POS, 1) and neg.shape == (POS * ratio, 1)
    with torch.no_grad():
        want_pos, want_neg = (_sage_by_hand if name == "sage" else _gat_by_hand)(
            model, _mfgs(ratio), ratio)
    assert torch.allclose(pos, want_pos, **TOL) and torch.allclose(neg, want_neg, **TOL)
    assert pos.abs().sum() > 0 and not torch.equal(neg[:POS], pos)
    assert 'h' in mfgs[1][0].srcdata                      # written for the inner block


@pytest.mark.parametrize("ratio", [1, 3])
@pytest.mark.parametrize("name", ["sage", "gat"])
def test_one_optimiser_step_under_autocast(name, ratio):
    import torch
    import torch.nn.functional as F
    model = _model(name).train()
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    before = [p.detach().clone() for p in model.parameters()]
    with torch.autocast("cuda", dtype=torch.bfloat16):
        pos, neg = model(_mfgs(ratio), neg_sample_ratio=ratio)
        loss = F.binary_cross_entropy_with_logits(pos, torch.ones_like(pos)) + \
            F.binary_cross_entropy_with_logits(neg, torch.zeros_like(neg))
    assert pos.shape == (POS, 1) and neg.shape == (POS * ratio, 1)
    opt.zero_grad()
    loss.backward()
    assert torch.isfinite(loss)
    for k, p in model.named_parameters():
        assert p.grad is not None and p.grad.dtype == torch.float32, k
        assert torch.isfinite(p.grad).all(), k
    opt.step()
    assert all(torch.isfinite(p).all() for p in model.parameters())
    assert any(not torch.equal(a, p) for a, p in zip(before, model.parameters()))


def test_example_trains_gat_under_autocast():
    spec = importlib.util.spec_from_file_location(
        "train_edge_prediction", os.path.join(ROOT, "examples", "train_edge_prediction.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    losses = mod.main(num_batches=3, verbose=False, amp=True, model='gat')
    assert len(losses) == 3 and all(math.isfinite(x) for x in losses)
