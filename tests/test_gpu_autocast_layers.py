"""nn.TemporalAttentionLayer, nn.EdgePredictor, nn.GRUMemoryUpdater and models.DGNN under
torch.autocast('cuda', dtype=torch.bfloat16).

Wiring, not numerics: each module's output must equal, bit for bit, the same computation written
out here from the public ops and F.linear / F.layer_norm under the same autocast region, with the
dtypes the modules document; every parameter must get a finite gradient from a backward that runs
outside the region.  The numerics rest on the op-level equalities of
tests/test_gpu_{block_attention,time_encode,edge_score}_bf16.py.  Then every combination of the
fused switches runs, and DGNN trains two steps in its TGN, TGAT and two-snapshot shapes."""
import pytest

from tests.test_gpu_models import BATCH, N, _World

pytestmark = pytest.mark.gpu


def autocast():
    import torch
    return torch.autocast("cuda", dtype=torch.bfloat16)


@pytest.fixture(scope="module")
def world():
    return _World()


def _layer_block(world, dim_node, dim_edge):
    """The one-layer sampler block of batch 0 with 'h' and 'f' cut to the layer's widths."""
    b = world.mfgs(dict(num_layers=1, num_snapshots=1, dim_node=0), 0)[0][0]
    assert b.num_edges() > 0 and b.segments()[2] is None
    if dim_node:
        b.srcdata['h'] = world.nfeat[b.srcdata['ID']][:, :dim_node].contiguous()
    b.edata['f'] = world.efeat[b.edata['ID']][:, :dim_edge].contiguous()
    return b


def _hand_layer(layer, b):
    """TemporalAttentionLayer.forward with attention dropout inactive, spelled out."""
    import torch
    import torch.nn.functional as F
    from gnnflow_amd import ops
    E, R, dev = b.num_edges(), b.num_dst_nodes(), b.device
    parts_q, parts_kv, h_dst = [], [], None
    if layer.use_node_feat:
        h = b.srcdata['h']
        h_dst = h[:R]
        parts_q.append(h_dst)
        parts_kv.append(h[R:])
    if layer.use_edge_feat:
        parts_kv.append(b.edata['f'])
    zeros = torch.zeros(R, dtype=torch.float32, device=dev)
    if layer.use_time_enc:
        w = layer.time_enc.w
        if layer.fused_time_encode:
            q_in = ops.time_encode_cat(parts_q, zeros, w.weight, w.bias, out_dtype=torch.bfloat16)
            kv = ops.time_encode_cat(parts_kv, b.edata['dt'], w.weight, w.bias,
                                     out_dtype=torch.bfloat16)
            assert q_in.dtype == kv.dtype == torch.bfloat16
        else:
            q_in = torch.cat(parts_q + [ops.time_encode(zeros, w.weight, w.bias)], dim=1)
            kv = torch.cat(parts_kv + [ops.time_encode(b.edata['dt'], w.weight, w.bias)], dim=1)
    else:
        kv = torch.cat(parts_kv, dim=1)
        q_in = torch.cat(parts_q, dim=1) if parts_q else None
    H = layer.num_head
    if q_in is None:      # w_q is the identity over a row of ones
        q = torch.ones((R, layer.dim_out), device=dev, dtype=torch.bfloat16)
    else:
        q = F.linear(q_in, layer.w_q.weight, layer.w_q.bias)
    k = F.linear(kv, layer.w_k.weight, layer.w_k.bias)
    v = F.linear(kv, layer.w_v.weight, layer.w_v.bias)
    assert q.dtype == k.dtype == v.dtype == torch.bfloat16
    agg = ops.block_attention(b, q.reshape(R, H, -1), k.reshape(E, H, -1), v.reshape(E, H, -1),
                              negative_slope=0.2)
    assert agg.dtype == torch.bfloat16
    agg = agg.reshape(R, -1)
    rst = torch.cat([agg, h_dst.to(torch.bfloat16)], dim=1) if layer.use_node_feat else agg
    assert rst.dtype == torch.bfloat16
    out = F.linear(rst, layer.w_out.weight, layer.w_out.bias)
    ln = layer.layer_norm
    return F.layer_norm(F.relu(out), ln.normalized_shape, ln.weight, ln.bias, ln.eps)


def _finite_grads(module):
    import torch
    for name, p in module.named_parameters():
        assert p.grad is not None, name
        assert p.grad.dtype == p.dtype == torch.float32, name
        assert torch.isfinite(p.grad).all(), name


@pytest.mark.parametrize("dims,fused_te", [((12, 6, 8), True), ((12, 6, 8), False),
                                           ((0, 6, 8), True), ((12, 6, 0), True),
                                           ((0, 6, 0), True)],
                         ids=["full", "full_unfused_time", "no_node_feat", "no_time_enc",
                              "edge_feat_only"])
def test_temporal_attention_layer_wiring(world, dims, fused_te):
    import torch
    from gnnflow_amd import nn as gnn
    dim_node, dim_edge, dim_time = dims
    torch.manual_seed(3)
    layer = gnn.TemporalAttentionLayer(dim_node, dim_edge, dim_time, 16, 2, 0.0, 0.0).cuda()
    layer.fused_time_encode = fused_te
    with torch.no_grad():      # a bias that is not zero, so that it is seen to be used
        if dim_time:
            layer.time_enc.w.bias.uniform_(-1, 1)
    b = _layer_block(world, dim_node, dim_edge)
    with autocast():
        out = layer(b)
        want = _hand_layer(layer, b)
    assert out.dtype == torch.float32 and out.shape == (b.num_dst_nodes(), 16)
    assert torch.equal(out, want) and torch.isfinite(out).all() and out.abs().sum() > 0
    out.square().sum().backward()      # outside the autocast region, as loss.backward() is
    _finite_grads(layer)
    # outside autocast the layer is what it was: float32 all the way
    assert layer(b).dtype == torch.float32


def test_edge_predictor_wiring():
    import torch
    import torch.nn.functional as F
    from gnnflow_amd import nn as gnn
    from gnnflow_amd import ops
    torch.manual_seed(4)
    model = gnn.EdgePredictor(16).cuda()
    assert model.fused_score
    B = 7
    h = torch.randn(3 * B, 16, device="cuda", requires_grad=True)
    with autocast():
        pos, neg = model(h)
        s = F.linear(h[:B], model.src_fc.weight, model.src_fc.bias)
        d = F.linear(h[B:], model.dst_fc.weight, model.dst_fc.bias)
        assert s.dtype == d.dtype == torch.bfloat16
        want = ops.edge_score(s, d, model.out_fc.weight, model.out_fc.bias)
        # bfloat16 rows, as the RNN combiner hands them over under autocast
        pos16, neg16 = model(h.detach().to(torch.bfloat16))
    assert pos.dtype == neg.dtype == torch.float32 and pos.shape == neg.shape == (B, 1)
    assert torch.equal(pos, want[:B]) and torch.equal(neg, want[B:])
    assert pos16.dtype == torch.float32 and torch.isfinite(pos16).all() and \
        torch.isfinite(neg16).all()
    (pos.sum() - 2 * neg.sum()).backward()
    _finite_grads(model)
    assert h.grad.dtype == torch.float32 and torch.isfinite(h.grad).all()


def _dgnn(name, **over):
    import torch
    from gnnflow_amd.models import DGNN
    kw = dict(dim_node=32, dim_edge=16, dim_time=20, dim_embed=16, num_layers=2, num_snapshots=1,
              att_head=2, dropout=0.1, att_dropout=0.1, use_memory=False)
    if name == "tgn":
        kw.update(use_memory=True, dim_memory=16, num_nodes=N)
    elif name == "two_snapshots":
        kw.update(num_snapshots=2)
    else:
        assert name == "tgat"
    kw.update(over)
    torch.manual_seed(11)
    return DGNN(**kw).cuda(), kw


@pytest.mark.parametrize("fused_te", [False, True], ids=["cat", "fused_time_encode"])
def test_gru_memory_updater_wiring(world, fused_te):
    import torch
    from gnnflow_amd import ops
    model, kw = _dgnn("tgn")
    up = model.memory_updater
    up.fused_time_encode = fused_te
    with torch.no_grad():      # a memory that is not all zeros
        model.memory.node_memory.normal_()
        model.memory.mailbox.normal_()
    blocks = [world.mfgs(kw, 0)[0][0] for _ in range(2)]
    for b in blocks:
        model.memory.prepare_input(b)
    b, hand = blocks
    R = b.num_dst_nodes()
    with autocast():
        last = up(b)
        x, dt = hand.srcdata['mem_input'], hand.srcdata['ts'] - hand.srcdata['mem_ts']
        w = up.time_enc.w
        if fused_te:
            x = ops.time_encode_cat((x,), dt, w.weight, w.bias)
        else:
            x = torch.cat([x, ops.time_encode(dt, w.weight, w.bias)], dim=1)
        updated = up.updater(x, hand.srcdata['mem'])
        assert updated.dtype == torch.bfloat16
        updated = updated.float()
        want_h = updated + up.node_feat_proj(hand.srcdata['h'])
    assert last["last_updated_memory"].dtype == torch.float32
    assert torch.equal(last["last_updated_memory"], updated[:R])
    assert b.srcdata['h'].dtype == torch.float32 and torch.equal(b.srcdata['h'], want_h)
    assert torch.isfinite(b.srcdata['h']).all()
    b.srcdata['h'].square().sum().backward()
    _finite_grads(up)


FLAGS = ("fused_attention", "fused_attention_dropout", "fused_time_encode")


@pytest.mark.parametrize("off", (None,) + FLAGS, ids=("all_on",) + FLAGS)
def test_every_flag_combination_runs(world, off):
    """Training mode with attention dropout active, the three switches off one at a time."""
    import torch
    from gnnflow_amd import nn as gnn
    torch.manual_seed(5)
    layer = gnn.TemporalAttentionLayer(12, 6, 8, 16, 2, 0.1, 0.2).cuda().train()
    for f in FLAGS:
        setattr(layer, f, f != off)
    b = _layer_block(world, 12, 6)
    with autocast():
        out = layer(b)
    assert out.dtype == torch.float32 and torch.isfinite(out).all() and out.abs().sum() > 0
    out.square().sum().backward()
    _finite_grads(layer)


def _train_two_steps(world, name, fused):
    import torch
    import torch.nn.functional as F
    model, kw = _dgnn(name)
    model.train()
    if fused:
        for m in model.modules():
            for f in FLAGS:
                if hasattr(m, f):
                    setattr(m, f, True)
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    scores = []
    for batch in range(2):
        mfgs = world.mfgs(kw, batch)
        opt.zero_grad()
        with autocast():
            if model.has_memory():
                model.memory.prepare_input(mfgs[0][0])
                model.last_updated = model.memory_updater(mfgs[0][0])
            pos, neg = model(mfgs)
            loss = F.binary_cross_entropy_with_logits(pos, torch.ones_like(pos)) + \
                F.binary_cross_entropy_with_logits(neg, torch.zeros_like(neg))
        assert pos.shape == neg.shape == (BATCH, 1)
        loss.backward()
        for k, p in model.named_parameters():
            assert p.grad is not None and torch.isfinite(p.grad).all(), k
        opt.step()
        if model.has_memory():
            # (a 2-layer model's outer block: whole (src, dst, neg) thirds only, update_mem_mail
            # refuses a remainder; it read none of those rows when it still let them through)
            last = model.last_updated
            whole = last["last_updated_nid"].shape[0] // 3 * 3
            with torch.no_grad():
                model.memory.update_mem_mail(**{k: v[:whole] for k, v in last.items()},
                                             edge_feats=None, neg_sample_ratio=1)
        scores += [pos.detach().float().clone(), neg.detach().float().clone()]
        assert torch.isfinite(loss) and all(torch.isfinite(s).all() for s in scores)
    assert all(torch.isfinite(p).all() for p in model.parameters())
    if model.has_memory():
        mem = model.memory
        for t in (mem.node_memory, mem.mailbox, mem.node_memory_ts, mem.mailbox_ts):
            assert t.dtype == torch.float32 and torch.isfinite(t).all()
        assert mem.node_memory.abs().sum() > 0
    return scores


@pytest.mark.parametrize("fused", [False, True], ids=["defaults", "all_fused"])
@pytest.mark.parametrize("name", ["tgn", "tgat", "two_snapshots"])
def test_dgnn_trains_under_autocast(world, name, fused):
    """Forward, loss, backward, Adam step and update_mem_mail under autocast, twice; without the
    bfloat16 ops the first forward raises TypeError.  The same seed gives the same scores."""
    import torch
    first = _train_two_steps(world, name, fused)
    second = _train_two_steps(world, name, fused)
    assert all(torch.equal(a, b) for a, b in zip(first, second))
