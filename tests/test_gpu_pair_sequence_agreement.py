"""GPU: DynamicGraph.pair_sequence against the readers that were there before it, on the toy of
test_gpu_pair_sequence.py and on a sampler-grade random graph (power-law sources, 4 000 edges with
heavy ties, ingested in chunks, with and without reverse edges):

- lengths, nodes, eids, times and counts are neighbor_cooccurrence(include_self=True)'s, element
  for element, floats by their bits, the padding included;
- positions 1 .. of each side are neighbor_sequence(length=L - 1) of that side's node: the four
  planes, delta_t, and each part against the matching columns of the tokens, bit for bit;
- lengths - 1 is temporal_degree capped at L - 1."""
import numpy as np
import pytest
import torch

from tests import synth
from tests import test_gpu_neighbor_sequence as T
from tests import test_gpu_pair_sequence as P

pytestmark = pytest.mark.gpu

LENGTHS = [2, 9, 33, 129, 512]
NUM_NODES, NUM_EDGES = 300, 4000
DN, DE, DT = 5, 8, 4


class Case:
    pass


def _case(graph, src, dst, ts, num_edges, table_rows):
    c = Case()
    c.graph, c.ts_host = graph, ts
    c.src, c.dst = torch.from_numpy(src).cuda(), torch.from_numpy(dst).cuda()
    c.ts = torch.from_numpy(ts).cuda()
    rng = np.random.RandomState(5)
    # tables a little short of the ids in use, so that some ids have no row
    c.edge_tab = torch.from_numpy(rng.randn(num_edges - 100, DE).astype(np.float32)).cuda()
    c.node_tab = torch.from_numpy(rng.randn(table_rows, DN).astype(np.float32)).cuda()
    c.enc = (torch.from_numpy(rng.randn(DT, 1).astype(np.float32)).cuda(),
             torch.from_numpy((rng.rand(DT) + 0.25).astype(np.float32)).cuda())
    return c


@pytest.fixture(scope="module", params=["toy", "powerlaw", "powerlaw-undirected"])
def case(request):
    if request.param == "toy":
        graph = T._new_graph(T._edges())
        src, dst, ts = P._queries()
        return _case(graph, src, dst, ts, graph.num_edges(), T.NODE_ROWS)
    src, dst, ts, eid = synth.powerlaw_graph(NUM_NODES, NUM_EDGES, seed=7, tie_levels=200)
    graph = T._new_graph()
    synth.ingest_chunks(graph, src, dst, ts, eid, 997,
                        add_reverse=request.param.endswith("undirected"))
    q_src, qts = synth.random_roots(NUM_NODES, 600, 1000.0, seed=3,
                                    extra_ids=(-1, NUM_NODES, NUM_NODES + 5, 1 << 40))
    q_dst, _ = synth.random_roots(NUM_NODES, 600, 1000.0, seed=4,
                                  extra_ids=(5, 6, -2, 7, NUM_NODES))
    qts[10:20] = ts[1000:1010]                                   # on stored times: ties
    qts[20] = np.nan
    q_src[30:38] = np.bincount(src).argmax()                     # the busiest source, after it all
    q_dst[34:42] = q_src[34:42]                                  # and pairs with itself
    qts[30:38] = 1100.0
    return _case(graph, q_src, q_dst, qts, NUM_EDGES, NUM_NODES - 50)


def _since(case, kind):
    return T._d_since(kind, case.ts_host)


def _bits(x):
    return x.view(torch.int32) if x.dtype == torch.float32 else x


@pytest.mark.parametrize("kind", T.KINDS)
@pytest.mark.parametrize("length", LENGTHS)
def test_the_shared_planes_are_neighbor_cooccurrence(case, length, kind):
    since = _since(case, kind)
    seq = case.graph.pair_sequence(case.src, case.dst, case.ts, since=since, length=length)
    pair = case.graph.neighbor_cooccurrence(case.src, case.dst, case.ts, since=since,
                                            length=length, include_self=True)
    assert (seq.lengths > 1).any() and (seq.lengths == 1).any()
    for name in pair._fields:
        assert torch.equal(_bits(getattr(seq, name)), _bits(getattr(pair, name))), name
    assert (seq.counts.sum(3) > 1).any()


@pytest.mark.parametrize("kind", T.KINDS)
@pytest.mark.parametrize("length", LENGTHS)
def test_positions_behind_the_self_slot_are_neighbor_sequence(case, length, kind):
    since = _since(case, kind)
    seq = case.graph.pair_sequence(case.src, case.dst, case.ts, since=since, length=length,
                                   node_feats=case.node_tab, edge_feats=case.edge_tab,
                                   time_encoder=case.enc)
    for side, end in ((0, case.src), (1, case.dst)):
        one = case.graph.neighbor_sequence(end, case.ts, since=since, length=length - 1,
                                           edge_feats=case.edge_tab, node_feats=case.node_tab,
                                           time_encoder=case.enc)
        assert one.lengths.any()
        assert torch.equal(seq.lengths[:, side] - 1, one.lengths)
        for name in ("nodes", "eids", "times", "delta_t"):
            assert torch.equal(_bits(getattr(seq, name)[:, side, 1:]),
                               _bits(getattr(one, name))), name
        tok = one.tokens.view(torch.int32)
        assert torch.equal(seq.edge[:, side, 1:].view(torch.int32), tok[..., :DE])
        assert torch.equal(seq.node[:, side, 1:].view(torch.int32), tok[..., DE:DE + DN])
        assert torch.equal(seq.time[:, side, 1:].view(torch.int32), tok[..., DE + DN:])


@pytest.mark.parametrize("kind", T.KINDS)
def test_lengths_are_temporal_degree_capped(case, kind):
    since = _since(case, kind)
    degree = torch.stack([case.graph.temporal_degree(end, case.ts, since=since)
                          for end in (case.src, case.dst)], dim=1)
    assert (degree > 128).any()
    for length in LENGTHS:
        seq = case.graph.pair_sequence(case.src, case.dst, case.ts, since=since, length=length)
        assert torch.equal(seq.lengths.long() - 1, degree.clamp(max=length - 1))
