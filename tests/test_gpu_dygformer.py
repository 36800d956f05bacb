"""GPU: models.DyGFormer.forward_graph on DynamicGraph.pair_sequence's finished parts against
forward() on neighbor_cooccurrence's outputs and the tables: L = 8 slots, 120 pairs, dim = 4, on
a 4 000-edge power-law graph with reverse edges.  In eval() the two are the same expression from
the channels' Linear layers on, so the results are equal bit for bit -- provided the reader's parts
are, bit for bit, what forward() assembles in torch with the zero-row rule and masked_fill.  The
scores against the torch EdgePredictor expression on the same src_fc / dst_fc outputs within
test_gpu_edge_score.py's bound for that comparison: twice edge_score_ref's a priori fp32 bound
of the fused kernel, gamma(D + 3) (|bias| + sum_d |w_d| relu(x_d)), one for each side."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import edge_score_ref as ES
from tests import synth

pytestmark = pytest.mark.gpu

L, ROWS, DIM = 8, 120, 4
NUM_NODES, NUM_EDGES = 300, 4000


class Setup:
    pass


@pytest.fixture(scope="module")
def setup():
    import gnnflow_amd
    s = Setup()
    src, dst, ts, eid = synth.powerlaw_graph(NUM_NODES, NUM_EDGES, seed=9, tie_levels=500)
    s.graph = gnnflow_amd.DynamicGraph(1 << 20, 1 << 28, "cuda", 8, 128, "insert")
    synth.ingest_chunks(s.graph, src, dst, ts, eid, 1500, add_reverse=True)
    q_src, qts = synth.random_roots(NUM_NODES, ROWS, 1000.0, seed=4, extra_ids=(-1, NUM_NODES))
    q_dst, _ = synth.random_roots(NUM_NODES, ROWS, 1000.0, seed=5, extra_ids=(3, 4, -2))
    q_dst[10:14] = q_src[10:14]
    s.src, s.dst = torch.from_numpy(q_src).cuda(), torch.from_numpy(q_dst).cuda()
    s.ts = torch.from_numpy(qts).cuda()
    torch.manual_seed(0)
    # tables short of the ids in use: some nodes and edges have no row
    s.node_feats = torch.randn(NUM_NODES - 40, DIM, device="cuda")
    s.edge_feats = torch.randn(NUM_EDGES - 500, DIM, device="cuda")
    return s


def _model(dim_node=DIM, dim_edge=DIM, **kw):
    from gnnflow_amd.models import DyGFormer
    torch.manual_seed(1)
    return DyGFormer(dim_node, dim_edge, dim_time=DIM, channel_dim=DIM, max_length=L,
                     dim_embed=DIM, **kw).cuda()


def _torch_inputs(setup):
    """forward()'s arguments from the reader that was there before pair_sequence."""
    c = setup.graph.neighbor_cooccurrence(setup.src, setup.dst, setup.ts, length=L,
                                          include_self=True)
    assert (c.lengths == 1).any() and (c.lengths == L).any()
    assert ((c.lengths > 1) & (c.lengths < L)).any()
    assert (c.nodes >= NUM_NODES - 40).any() and (c.eids >= NUM_EDGES - 500).any()
    delta_t = setup.ts[:, None, None] - c.times
    return c.nodes, c.eids, delta_t, c.counts, c.lengths


@pytest.mark.parametrize("patch", [1, 2, L])
def test_forward_graph_equals_forward_bit_for_bit(setup, patch):
    model = _model(patch_size=patch).eval()
    nodes, eids, delta_t, counts, lengths = _torch_inputs(setup)
    with torch.no_grad():
        got = model.forward_graph(setup.graph, setup.src, setup.dst, setup.ts, setup.node_feats,
                                  setup.edge_feats)
        want = model(nodes, eids, delta_t, counts, lengths, setup.node_feats, setup.edge_feats)
        # forward() replaces the padded slots: junk there changes nothing, and it is not a copy
        # of the reader's zeros that makes the two agree
        pad = torch.arange(L, device="cuda") >= lengths.unsqueeze(2)
        again = model(nodes.masked_fill(pad, 5), eids.masked_fill(pad, 5),
                      delta_t.masked_fill(pad, float("nan")), counts, lengths, setup.node_feats,
                      setup.edge_feats)
        emb = model.forward_graph(setup.graph, setup.src, setup.dst, setup.ts, setup.node_feats,
                                  setup.edge_feats, return_embed=True)
        emb_want = model(nodes, eids, delta_t, counts, lengths, setup.node_feats,
                         setup.edge_feats, return_embed=True)
    assert tuple(got.shape) == (ROWS, 1) and torch.isfinite(got).all()
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    assert torch.equal(got.view(torch.int32), again.view(torch.int32))
    for a, b in zip(emb, emb_want):
        assert tuple(a.shape) == (ROWS, DIM)
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("dn,de", [(0, DIM), (DIM, 0), (0, 0)])
def test_dropped_channels_and_since(setup, dn, de):
    model = _model(dn, de).eval()
    c = setup.graph.neighbor_cooccurrence(setup.src, setup.dst, setup.ts, since=300.0, length=L)
    delta_t = setup.ts[:, None, None] - c.times
    with torch.no_grad():
        got = model.forward_graph(setup.graph, setup.src, setup.dst, setup.ts, setup.node_feats,
                                  setup.edge_feats, since=300.0)
        want = model(c.nodes, c.eids, delta_t, c.counts, c.lengths, setup.node_feats,
                     setup.edge_feats)
    assert torch.isfinite(got).all()
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))


def test_scores_are_the_edge_predictor_expression(setup):
    model = _model().eval()
    head = model.edge_predictor
    assert head.fused_score
    with torch.no_grad():
        got = model.forward_graph(setup.graph, setup.src, setup.dst, setup.ts, setup.node_feats,
                                  setup.edge_feats)
        emb_src, emb_dst = model.forward_graph(setup.graph, setup.src, setup.dst, setup.ts,
                                               setup.node_feats, setup.edge_feats,
                                               return_embed=True)
        src_h, dst_h = head.src_fc(emb_src), head.dst_fc(emb_dst)
        want = head.out_fc(F.relu(src_h + dst_h))
        head.fused_score = False
        unfused = model.score(emb_src, emb_dst)
        head.fused_score = True
    assert torch.equal(unfused, want)
    ref = ES.Reference(src_h.cpu().numpy(), dst_h.cpu().numpy(),
                       head.out_fc.weight.detach().cpu().numpy(),
                       head.out_fc.bias.detach().cpu().numpy(), np.zeros(ROWS, np.float32))
    ratio = ES.error_ratio(got.cpu().numpy(), want.cpu().numpy(), 2 * ref.b_out)
    print("\n[difference / (2 x bound)] {:.3g}".format(ratio))
    assert ratio <= 1.0, "difference / (2 x bound) = {:.3g}".format(ratio)
    assert ES.error_ratio(got.cpu().numpy(), ref.out, ref.b_out) <= 1.0


def test_one_backward_pass_reaches_every_parameter(setup):
    model = _model(dropout=0.0).train()
    score = model.forward_graph(setup.graph, setup.src, setup.dst, setup.ts, setup.node_feats,
                                setup.edge_feats)
    F.binary_cross_entropy_with_logits(score, torch.ones_like(score)).backward()
    named = dict(model.named_parameters())
    assert len(named) > 30 and not any(n.startswith("time_enc") for n in named)
    for name, p in named.items():
        assert p.grad is not None and torch.isfinite(p.grad).all(), name
        assert p.grad.abs().sum() > 0, name


def test_learn_time_trains_the_encoder_and_starts_from_the_fixed_one(setup):
    fixed = _model().eval()
    learn = _model(learn_time=True).eval()
    state = {k: v for k, v in fixed.state_dict().items() if not k.startswith("time_enc")}
    missing = learn.load_state_dict(state, strict=False)
    assert sorted(missing.missing_keys) == ["time_enc.w.bias", "time_enc.w.weight"]
    assert torch.equal(learn.time_enc.w.weight.detach(), fixed.time_enc.weight)
    assert not learn.time_enc.w.bias.detach().any()
    with torch.no_grad():
        a = fixed.forward_graph(setup.graph, setup.src, setup.dst, setup.ts, setup.node_feats,
                                setup.edge_feats)
        b = learn.forward_graph(setup.graph, setup.src, setup.dst, setup.ts, setup.node_feats,
                                setup.edge_feats)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    learn.train()
    learn.forward_graph(setup.graph, setup.src, setup.dst, setup.ts, setup.node_feats,
                        setup.edge_feats).square().sum().backward()
    for p in learn.time_enc.parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all() and p.grad.abs().sum() > 0


def test_wrong_length_is_refused(setup):
    model = _model()
    c = setup.graph.neighbor_cooccurrence(setup.src, setup.dst, setup.ts, length=L + 1)
    with pytest.raises(ValueError, match="max_length is 8"):
        model(c.nodes, c.eids, c.times, c.counts, c.lengths, setup.node_feats, setup.edge_feats)
