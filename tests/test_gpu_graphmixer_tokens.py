"""GPU: models.GraphMixer.forward_tokens on DynamicGraph.neighbor_sequence's finished tokens
against forward() on the same call's edge features, time deltas and lengths: K = 8 tokens, 150
rows, dim = 4, on a 4 000-edge power-law graph with reverse edges.  In eval() the two are the same
expression from the first Linear on, so the embeddings are equal bit for bit -- provided the
reader's tokens are, bit for bit, what forward() assembles: [edge_x | time_enc(delta_t)] with the
padded slots zero."""
import numpy as np
import pytest
import torch

from tests import synth

pytestmark = pytest.mark.gpu

K, ROWS, DIM = 8, 150, 4
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
    nodes, qts = synth.random_roots(NUM_NODES, ROWS, 1000.0, seed=4, extra_ids=(-1, NUM_NODES))
    s.nodes, s.ts = torch.from_numpy(nodes).cuda(), torch.from_numpy(qts).cuda()
    torch.manual_seed(0)
    s.edge_feats = torch.randn(NUM_EDGES, DIM, device="cuda")
    s.node_x = torch.randn(ROWS, DIM, device="cuda")
    s.nbr_mean = torch.randn(ROWS, DIM, device="cuda")
    return s


def _model(dim_edge):
    from gnnflow_amd.models import GraphMixer
    torch.manual_seed(1)
    return GraphMixer(DIM, dim_edge, dim_time=DIM, dim_embed=DIM, num_tokens=K).cuda()


def test_forward_tokens_equals_forward_bit_for_bit(setup):
    model = _model(DIM).eval()
    seq = setup.graph.neighbor_sequence(setup.nodes, setup.ts, length=K,
                                        edge_feats=setup.edge_feats,
                                        time_encoder=model.time_enc)
    assert tuple(seq.tokens.shape) == (ROWS, K, 2 * DIM)
    assert (seq.lengths == 0).any() and (seq.lengths == K).any()
    assert ((seq.lengths > 0) & (seq.lengths < K)).any()
    edge_x = seq.tokens[..., :DIM]
    with torch.no_grad():
        got = model.forward_tokens(seq.tokens, setup.node_x, setup.nbr_mean, return_embed=True)
        want = model(edge_x, seq.delta_t, seq.lengths, setup.node_x, setup.nbr_mean,
                     return_embed=True)
        # forward() replaces the padded slots: junk there changes nothing, and it is not a copy
        # of the reader's zeros that makes the two agree
        junk = torch.where((torch.arange(K, device="cuda")[None, :] < seq.lengths[:, None])
                           [..., None], edge_x, torch.full_like(edge_x, float("nan")))
        again = model(junk, seq.delta_t, seq.lengths, setup.node_x, setup.nbr_mean,
                      return_embed=True)
    assert tuple(got.shape) == (ROWS, DIM) and torch.isfinite(got).all()
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    assert torch.equal(got.view(torch.int32), again.view(torch.int32))
    # and the edge predictor's path: rows laid out [src | dst | negatives]
    with torch.no_grad():
        pos, neg = model.forward_tokens(seq.tokens, setup.node_x, setup.nbr_mean)
        pos_w, neg_w = model(edge_x, seq.delta_t, seq.lengths, setup.node_x, setup.nbr_mean)
    assert tuple(pos.shape) == (ROWS // 3, 1) and tuple(neg.shape) == (ROWS // 3, 1)
    assert torch.equal(pos, pos_w) and torch.equal(neg, neg_w)


def test_time_only_tokens_when_dim_edge_is_zero(setup):
    model = _model(0).eval()
    seq = setup.graph.neighbor_sequence(setup.nodes, setup.ts, length=K,
                                        time_encoder=model.time_enc)
    assert tuple(seq.tokens.shape) == (ROWS, K, DIM)
    with torch.no_grad():
        got = model.forward_tokens(seq.tokens, setup.node_x, setup.nbr_mean, return_embed=True)
        want = model(None, seq.delta_t, seq.lengths, setup.node_x, setup.nbr_mean,
                     return_embed=True)
    assert torch.isfinite(got).all()
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))


def test_forward_tokens_rejects_another_shape(setup):
    model = _model(DIM)
    for shape in ((ROWS, K + 1, 2 * DIM), (ROWS, K, DIM), (ROWS, K * 2 * DIM)):
        with pytest.raises(ValueError, match="tokens must be"):
            model.forward_tokens(torch.zeros(shape, device="cuda"), setup.node_x, setup.nbr_mean)


def test_gradients_reach_link_in_and_the_mixers(setup):
    model = _model(DIM).train()
    seq = setup.graph.neighbor_sequence(setup.nodes, setup.ts, length=K,
                                        edge_feats=setup.edge_feats,
                                        time_encoder=model.time_enc)
    assert not seq.tokens.requires_grad
    embed = model.forward_tokens(seq.tokens, setup.node_x, setup.nbr_mean, return_embed=True)
    embed.square().sum().backward()
    named = dict(model.named_parameters())
    reached = [name for name in named if name.startswith(("link_in.", "mixers."))]
    assert "link_in.weight" in reached and len(reached) > 10
    for name in reached:
        grad = named[name].grad
        assert grad is not None and torch.isfinite(grad).all() and grad.abs().sum() > 0, name
    assert np.isfinite(float(embed.detach().sum()))
