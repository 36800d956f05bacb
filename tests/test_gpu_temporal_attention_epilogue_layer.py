"""nn.TemporalAttentionLayer with `fused_epilogue`: the last line layer_norm(relu(dropout(w_out(
rst)))) as one ops.dropout_relu_layer_norm call, against the same layer with the flag off.

Everything in front of the epilogue is the same code in both runs, so z = w_out(rst) is bit-equal
(asserted) and the two outputs are two fp32 evaluations of the same expression of z.  Each lies
within the a priori bound of tests/layer_epilogue_ref.py (Reference, evaluated on z), so they
differ by at most twice that bound: out by 2 b_out, the gradients of layer_norm.weight / .bias by
2 b_ggamma / 2 b_gbeta, the gradient gz of z by bz = 2 b_gx.  Through w_out (z = rst W^T + c, R rows,
K inputs, D outputs, any GEMM: n products and n - 1 adds are within gamma_{n+1} of the sum of
magnitudes, on either side):

    grad W      = gz^T rst     |difference| <= bz^T |rst| + 2 gamma_{R+1} (|gz| + bz)^T |rst|
    grad c      = sum_r gz                     sum_r bz + 2 gamma_R sum_r (|gz| + bz)
    grad rst    = gz W                         bz |W| + 2 gamma_{D+1} (|gz| + bz) |W|

Upstream of rst (w_q, w_k, w_v, the time encoding, the features h) the gradients are G = L(grad
rst) with L the linear map of the unchanged backward (attention, the three Linears, the time
encoding) at the forward both runs share.  Its magnitude |L| is taken from that backward itself,
one unit vector of grad rst at a time (_upstream), so with B the bound on grad rst above:

    |G_on - G_off| <= (1 + 2^-10) (|L| B + 2 gamma_N |L| max(|grad rst|))

The first term is the difference of the inputs carried through L.  The second is the rounding of
the two fp32 evaluations of L, each within gamma_N |L| |grad rst| to first order, with N the
roundings on the longest path: the E edge rows a weight gradient sums, two reductions over the
widest row (a Linear's input gradient, a head's dot product), the largest segment and 16 single
operations.  |L| is the composite Jacobian; 2^-10 covers its own fp32 evaluation and the sum of
its rst.numel() non-negative terms.

The block is the one-layer sampler block of batch 0 of tests/test_gpu_models.py's world (a
tests/synth.py power-law graph of 600 edges): 36 destinations, about 100 edges."""
import itertools

import numpy as np
import pytest

from tests import layer_epilogue_ref as LE
from tests.test_gpu_models import BATCH, _World

pytestmark = pytest.mark.gpu

FLAGS = ("fused_attention", "fused_attention_dropout", "fused_time_encode")


@pytest.fixture(scope="module")
def world():
    return _World()


def _block(world, dim_node=12, dim_edge=6):
    """The one-layer sampler block of batch 0 (36 destinations, about 100 edges) with 'h' and 'f'
    cut to the layer's widths; 'h' asks for a gradient."""
    b = world.mfgs(dict(num_layers=1, num_snapshots=1, dim_node=0), 0)[0][0]
    assert b.num_edges() > 0 and b.num_dst_nodes() == 3 * BATCH
    b.srcdata['h'] = world.nfeat[b.srcdata['ID']][:, :dim_node].contiguous().requires_grad_(True)
    b.edata['f'] = world.efeat[b.edata['ID']][:, :dim_edge].contiguous()
    return b


def _layer(dim_out, heads=2, dropout=0.0, att_dropout=0.0, seed=3):
    import torch
    from gnnflow_amd import nn as gnn
    torch.manual_seed(seed)
    layer = gnn.TemporalAttentionLayer(12, 6, 8, dim_out, heads, dropout, att_dropout).cuda()
    with torch.no_grad():      # an affine layer norm that is seen to be used
        layer.layer_norm.weight.uniform_(0.5, 1.5)
        layer.layer_norm.bias.uniform_(-1, 1)
    return layer


def _np(t):
    return t.detach().float().cpu().numpy().astype(np.float64)


def _run(layer, world, fused, seed=None, backward=True):
    """One forward (+ backward of sum(out * G)) -> dict of out, z, rst, gz, grst, G and grads."""
    import torch
    layer.fused_epilogue = fused
    layer.zero_grad()
    b = _block(world)
    seen = {}

    def hook(_m, inp, out):
        seen["rst"], seen["z"] = inp[0], out
        if out.requires_grad:
            out.register_hook(lambda g: seen.__setitem__("gz", g))
            inp[0].register_hook(lambda g: seen.__setitem__("grst", g))
    handle = layer.w_out.register_forward_hook(hook)
    if seed is not None:
        torch.manual_seed(seed)
    out = layer(b)
    handle.remove()
    seen["out"] = out
    if backward:
        gen = torch.Generator().manual_seed(9)
        seen["G"] = torch.randn(out.shape, generator=gen).cuda()
        (out * seen["G"]).sum().backward()
        seen["grads"] = {k: p.grad.clone() for k, p in layer.named_parameters()}
        seen["gh"] = b.srcdata['h'].grad
        for k, g in seen["grads"].items():
            assert torch.isfinite(g).all(), k
        assert torch.isfinite(seen["gh"]).all()
    return seen


def _within(name, a, b, bound):
    ratio = LE.error_ratio(_np(a), _np(b), bound)
    print("[difference / bound] {}: {:.3g}".format(name, ratio))
    assert ratio <= 1.0, (name, ratio)


def _compare(layer, world, on, off, p=0.0, seed=0):
    import torch
    assert torch.equal(on["z"], off["z"]) and torch.equal(on["rst"], off["rst"])
    ln = layer.layer_norm
    r = LE.Reference(_np(on["z"]), _np(ln.weight), _np(ln.bias), _np(on["G"]), eps=ln.eps, p=p,
                     seed=seed)
    _within("out", on["out"], off["out"], 2 * r.b_out)
    _within("layer_norm.weight", on["grads"]["layer_norm.weight"],
            off["grads"]["layer_norm.weight"], 2 * r.b_ggamma)
    _within("layer_norm.bias", on["grads"]["layer_norm.bias"], off["grads"]["layer_norm.bias"],
            2 * r.b_gbeta)
    bz = 2 * r.b_gx
    _within("z", on["gz"], off["gz"], bz)
    R, D = r.R, r.D
    agz = np.maximum(np.abs(_np(on["gz"])), np.abs(_np(off["gz"]))) + bz
    rst, W = np.abs(_np(on["rst"])), np.abs(_np(layer.w_out.weight))
    _within("w_out.weight", on["grads"]["w_out.weight"], off["grads"]["w_out.weight"],
            bz.T @ rst + 2 * LE.gamma(R + 1) * (agz.T @ rst))
    _within("w_out.bias", on["grads"]["w_out.bias"], off["grads"]["w_out.bias"],
            bz.sum(0) + 2 * LE.gamma(R) * agz.sum(0))
    b_rst = bz @ W + 2 * LE.gamma(D + 1) * (agz @ W)
    _within("rst", on["grst"], off["grst"], b_rst)
    a_rst = np.maximum(np.abs(_np(on["grst"])), np.abs(_np(off["grst"])))
    lb, la, n = _upstream(layer, world, b_rst, a_rst)
    assert set(lb) == {k for k in on["grads"] if not k.startswith(("w_out.", "layer_norm."))} | {"h"}
    for k in lb:
        bound = (1 + 2.0 ** -10) * (lb[k] + 2 * LE.gamma(n) * la[k])
        _within(k, on["gh"] if k == "h" else on["grads"][k],
                off["gh"] if k == "h" else off["grads"][k], bound)
    return r


def _upstream(layer, world, b_rst, a_rst):
    """(|L| b_rst, |L| a_rst, N) per upstream parameter and for h, L: grad rst -> gradient, from
    one backward per element of rst through the part of the layer in front of w_out."""
    import torch
    layer.fused_epilogue = False
    b = _block(world)
    seen = {}
    handle = layer.w_out.register_forward_hook(lambda _m, inp, _o: seen.__setitem__("rst", inp[0]))
    layer(b)
    handle.remove()
    rst = seen["rst"]
    names = [k for k, _ in layer.named_parameters() if not k.startswith(("w_out.", "layer_norm."))]
    params = dict(layer.named_parameters())
    inputs = [params[k] for k in names] + [b.srcdata['h']]
    acc_b = [torch.zeros_like(t) for t in inputs]
    acc_a = [torch.zeros_like(t) for t in inputs]
    wb, wa = b_rst.ravel().tolist(), a_rst.ravel().tolist()
    e = torch.zeros(rst.numel(), device=rst.device, dtype=rst.dtype)
    for j in range(rst.numel()):
        e[j] = 1
        if j:
            e[j - 1] = 0
        g = torch._foreach_abs(torch.autograd.grad(rst, inputs, grad_outputs=e.view_as(rst),
                                                   retain_graph=True))
        torch._foreach_add_(acc_b, g, alpha=wb[j])
        torch._foreach_add_(acc_a, g, alpha=wa[j])
    deg = int(np.bincount(b.edges()[1].cpu().numpy()).max())
    width = max(t.shape[-1] for t in inputs)
    n = b.num_edges() + 2 * max(width, layer.dim_out) + deg + 16
    keys = names + ["h"]
    return dict(zip(keys, map(_np, acc_b))), dict(zip(keys, map(_np, acc_a))), n


@pytest.mark.parametrize("mode", ["eval", "train"])
@pytest.mark.parametrize("dim_out", [100, 6])
def test_flag_on_against_flag_off_without_dropout(world, dim_out, mode):
    layer = _layer(dim_out)
    layer.train(mode == "train")
    off, on = _run(layer, world, False), _run(layer, world, True)
    assert on["out"].dtype == off["out"].dtype and on["out"].shape == (3 * BATCH, dim_out)
    _compare(layer, world, on, off)


def test_eval_mode_ignores_the_dropout(world):
    import torch
    layer = _layer(100, dropout=0.3).eval()
    state = torch.random.get_rng_state()
    off, on = _run(layer, world, False), _run(layer, world, True)
    assert torch.equal(torch.random.get_rng_state(), state)      # no seed drawn
    _compare(layer, world, on, off)


@pytest.mark.parametrize("dim_out", [100, 6])
def test_training_dropout_under_manual_seed(world, dim_out):
    """Two forwards with the same seed are bit-equal, and the output is the op's own on the
    layer's z with the seed the layer drew (the first draw after manual_seed), which in turn is
    the torch expression with the reference's mask within the two sides' bounds."""
    import torch
    import torch.nn.functional as F
    from gnnflow_amd import ops
    from tests.attention_dropout_ref import scale
    p = 0.2
    layer = _layer(dim_out, dropout=p).train()
    a, b = _run(layer, world, True, seed=21), _run(layer, world, True, seed=21)
    assert torch.equal(a["out"], b["out"])
    assert all(torch.equal(a["grads"][k], b["grads"][k]) for k in a["grads"])
    assert not torch.equal(a["out"], _run(layer, world, True, seed=22, backward=False)["out"])
    torch.manual_seed(21)
    seed = int(torch.randint(0, 2 ** 63 - 1, (1,), dtype=torch.int64))
    ln = layer.layer_norm
    z = a["z"].detach()
    assert torch.equal(a["out"], ops.dropout_relu_layer_norm(z, ln.weight, ln.bias, ln.eps,
                                                             dropout_p=p, dropout_seed=seed))
    r = LE.Reference(_np(z), _np(ln.weight), _np(ln.bias), _np(a["G"]), eps=ln.eps, p=p, seed=seed)
    keep = torch.from_numpy(r.keep.astype(np.float32)).cuda()
    want = F.layer_norm(F.relu(z * keep * float(scale(p))), (dim_out,), ln.weight, ln.bias, ln.eps)
    _within("out against torch with the mask", a["out"], want, 2 * r.b_out)
    # flag off: torch's generator stream is untouched by the epilogue (nn.Dropout on the GPU
    # draws from the device generator), and no CPU seed is drawn
    state = torch.random.get_rng_state()
    _run(layer, world, False, backward=False)
    assert torch.equal(torch.random.get_rng_state(), state)


def test_state_dict_does_not_know_the_flag(world):
    import torch
    on, off = _layer(100), _layer(100, seed=4)
    on.fused_epilogue, off.fused_epilogue = True, False
    assert "fused_epilogue" not in "".join(on.state_dict())
    assert list(on.state_dict()) == list(off.state_dict())
    off.load_state_dict(on.state_dict())
    assert off.fused_epilogue is False and on.fused_epilogue is True
    assert all(torch.equal(a, b) for a, b in zip(on.state_dict().values(),
                                                 off.state_dict().values()))
    on.load_state_dict(off.state_dict())
    from gnnflow_amd import nn as gnn
    assert gnn.FUSED_EPILOGUE_DEFAULT is _layer(6).fused_epilogue


@pytest.mark.parametrize("flags", list(itertools.product((False, True), repeat=3)),
                         ids=lambda f: "".join("01"[x] for x in f))
def test_autocast_every_flag_combination(world, flags):
    """Under bfloat16 autocast, attention dropout active, the other three switches in every
    combination, `fused_epilogue` on against off.  tests/test_gpu_autocast_layers.py holds no
    numeric bound to borrow (it asserts bit-equality with a hand composition), so the comparison
    is the one above: z is the same bfloat16 tensor in both runs, torch widens it and runs its
    fp32 layer_norm, the op widens it in the kernel, and both are within the fp32 bound of the
    reference evaluated on z."""
    import torch
    layer = _layer(100, att_dropout=0.2).train()
    for f, v in zip(FLAGS, flags):
        setattr(layer, f, v)
    runs = {}
    for fused in (False, True):
        with torch.autocast("cuda", dtype=torch.bfloat16):
            layer.fused_epilogue = fused
            runs[fused] = _run(layer, world, fused, seed=31, backward=False)
        out = runs[fused]["out"]
        assert out.dtype == torch.float32 and torch.isfinite(out).all()
        assert runs[fused]["z"].dtype == torch.bfloat16
    # backward outside the region, as loss.backward() is
    on, off = runs[True], runs[False]
    assert torch.equal(on["z"], off["z"])
    G = torch.randn(on["out"].shape, generator=torch.Generator().manual_seed(9)).cuda()
    grads = {}
    for fused, run in runs.items():
        layer.zero_grad()
        (run["out"] * G).sum().backward()
        grads[fused] = {k: p.grad.clone() for k, p in layer.named_parameters()}
        assert all(torch.isfinite(g).all() and g.dtype == torch.float32
                   for g in grads[fused].values())
    ln = layer.layer_norm
    r = LE.Reference(_np(on["z"]), _np(ln.weight), _np(ln.bias), _np(G), eps=ln.eps)
    _within("out", on["out"], off["out"], 2 * r.b_out)
    for k, bound in (("layer_norm.weight", r.b_ggamma), ("layer_norm.bias", r.b_gbeta)):
        _within(k, grads[True][k], grads[False][k], 2 * bound)
    # the gradient of z is bfloat16: each side's fp32 value (within b_gx of the reference) rounded
    # once, within 2^-9 of itself.  Everything upstream then runs through bfloat16 GEMMs on
    # gradients that may differ by a bfloat16 ulp; those are required to be finite above.
    gz_on, gz_off = _np(on["gz"]), _np(off["gz"])
    assert on["gz"].dtype == off["gz"].dtype == torch.bfloat16
    _within("z", on["gz"], off["gz"],
            2 * r.b_gx + 2.0 ** -9 * (np.abs(gz_on) + np.abs(gz_off) + 2 * r.b_gx) * r.active)


def test_autocast_training_dropout_is_the_op_on_z(world):
    """Under bfloat16 autocast with dropout 0.2: the layer's output is the op's on the bfloat16 z
    with the seed the layer drew, bit for bit, and float32."""
    import torch
    from gnnflow_amd import ops
    layer = _layer(100, dropout=0.2).train()
    with torch.autocast("cuda", dtype=torch.bfloat16):
        a = _run(layer, world, True, seed=51, backward=False)
    torch.manual_seed(51)
    seed = int(torch.randint(0, 2 ** 63 - 1, (1,), dtype=torch.int64))
    ln, z = layer.layer_norm, a["z"].detach()
    assert z.dtype == torch.bfloat16 and a["out"].dtype == torch.float32
    assert torch.equal(a["out"], ops.dropout_relu_layer_norm(z, ln.weight, ln.bias, ln.eps,
                                                             dropout_p=0.2, dropout_seed=seed))
    (a["out"] * torch.randn(a["out"].shape, generator=torch.Generator().manual_seed(9)).cuda()
     ).sum().backward()
    assert all(torch.isfinite(p.grad).all() for p in layer.parameters())


def test_what_the_op_does_not_take_is_the_torch_line(world, monkeypatch):
    """dim_out above the op's width, a layer norm without affine parameters and dropout.p == 1
    take torch's kernels with the flag set: the op is not called and the output is bit-equal."""
    import torch
    from gnnflow_amd import ops

    def refuse(*a, **k):
        raise AssertionError("ops.dropout_relu_layer_norm was called")
    wide = _layer(1025, heads=1)
    wide.fused_attention = False      # ops.block_attention stops at 1024 columns too
    plain = _layer(100)
    plain.layer_norm = torch.nn.LayerNorm(100, elementwise_affine=False).cuda()
    ones = _layer(100, dropout=1.0).train()
    for layer in (wide, plain, ones):
        off = _run(layer, world, False, seed=41, backward=False)["out"]
        monkeypatch.setattr(ops, "dropout_relu_layer_norm", refuse)
        on = _run(layer, world, True, seed=41, backward=False)["out"]
        monkeypatch.undo()
        assert torch.equal(on, off)


@pytest.mark.parametrize("name", ["tgn", "two_snapshots"])
def test_dgnn_trains_with_the_flag_on_every_layer(world, name):
    """Forward, backward and one optimiser step of models.DGNN (TGN, and the two-snapshot DySAT
    shape) with `fused_epilogue` set on every layer: the op is called once per layer and
    snapshot, every parameter gets a finite gradient and the step moves the model."""
    import torch
    import torch.nn.functional as F
    from gnnflow_amd import ops
    from tests.test_gpu_autocast_layers import _dgnn
    model, kw = _dgnn(name)
    model.train()
    layers = [m for m in model.modules() if hasattr(m, "fused_epilogue")]
    assert len(layers) == kw["num_layers"] * kw["num_snapshots"]
    for m in layers:
        m.fused_epilogue = True
    calls, op = [], ops.dropout_relu_layer_norm

    def counted(*a, **k):
        calls.append(k.get("dropout_p", 0.0))
        return op(*a, **k)
    ops.dropout_relu_layer_norm = counted
    try:
        opt = torch.optim.Adam(model.parameters(), lr=1e-3)
        mfgs = world.mfgs(kw, 0)
        if model.has_memory():
            model.memory.prepare_input(mfgs[0][0])
            model.last_updated = model.memory_updater(mfgs[0][0])
        pos, neg = model(mfgs)
    finally:
        ops.dropout_relu_layer_norm = op
    assert len(calls) == len(layers) and all(p == kw["dropout"] for p in calls)
    loss = F.binary_cross_entropy_with_logits(pos, torch.ones_like(pos)) + \
        F.binary_cross_entropy_with_logits(neg, torch.zeros_like(neg))
    loss.backward()
    before = {k: v.detach().clone() for k, v in model.named_parameters()}
    for k, v in model.named_parameters():
        assert v.grad is not None and torch.isfinite(v.grad).all(), k
    opt.step()
    assert torch.isfinite(loss)
    assert any(not torch.equal(v, before[k]) for k, v in model.named_parameters())


N_DOWNSTREAM = 512


@pytest.mark.parametrize("name", ["tgn", "two_snapshots"])
def test_dgnn_loss_matches_the_flag_off_model(world, name):
    """models.DGNN in training mode without dropout (with it the two paths draw different masks by
    design), `fused_epilogue` on every layer against the same model with it off: same state dict,
    same blocks.  The loss is a function of every epilogue's output; call c's output differs
    between the two paths by at most 2 b_out_c for the z it is given, and the loss moves by that
    times its gradient G_c at the output.  What lies downstream of an epilogue (a second layer,
    the combiner, the predictor, BCE) runs in both models on inputs that differ, so its fp32
    roundings differ too: each evaluation is within gamma_N of the magnitudes it carries, taken to
    first order as <|G_c|, |out_c|>, with N = 512 above the roundings on the longest such path
    (about 300: Linears of at most 68 inputs, segments of 3 edges, heads of 8 columns, layer norms
    of 16, the RNN, the predictor, BCE's B + 8).  So

        |loss_on - loss_off| <= sum_c <|G_c|, 2 b_out_c> + 2 gamma_N sum_c <|G_c|, |out_c|>
                                + 2 gamma_{B+8} loss."""
    import torch
    import torch.nn.functional as F
    from gnnflow_amd import ops
    from tests.test_gpu_autocast_layers import _dgnn
    losses, calls, op = {}, [], ops.dropout_relu_layer_norm

    def recorded(x, w, b, eps, **k):
        out = op(x, w, b, eps, **k)
        call = dict(z=x.detach(), w=w.detach(), b=b.detach(), eps=eps, out=out.detach())
        out.register_hook(lambda g: call.__setitem__("G", g))
        calls.append(call)
        return out
    state = None
    for fused in (False, True):
        model, kw = _dgnn(name, dropout=0.0, att_dropout=0.0)
        if state is not None:
            model.load_state_dict(state)
        state = {k: v.clone() for k, v in model.state_dict().items()}
        model.train()
        layers = [m for m in model.modules() if hasattr(m, "fused_epilogue")]
        for m in layers:
            m.fused_epilogue = fused
        mfgs = world.mfgs(kw, 0)
        if model.has_memory():
            model.memory.prepare_input(mfgs[0][0])
            model.last_updated = model.memory_updater(mfgs[0][0])
        ops.dropout_relu_layer_norm = recorded
        try:
            pos, neg = model(mfgs)
        finally:
            ops.dropout_relu_layer_norm = op
        loss = F.binary_cross_entropy_with_logits(pos, torch.ones_like(pos)) + \
            F.binary_cross_entropy_with_logits(neg, torch.zeros_like(neg))
        loss.backward()
        losses[fused] = float(loss.detach())
        assert len(calls) == (len(layers) if fused else 0)
    bound = 2 * LE.gamma(BATCH + 8) * max(losses.values())
    for c in calls:
        G = np.abs(_np(c["G"]))
        r = LE.Reference(_np(c["z"]), _np(c["w"]), _np(c["b"]), G, eps=c["eps"])
        bound += (G * 2 * r.b_out).sum() + 2 * LE.gamma(N_DOWNSTREAM) * (G * np.abs(_np(c["out"]))).sum()
    diff = abs(losses[True] - losses[False])
    print("\n[loss] {}: off {:.9g}, on {:.9g}, difference / bound = {:.3g}".format(
        name, losses[False], losses[True], diff / bound))
    assert diff <= bound
