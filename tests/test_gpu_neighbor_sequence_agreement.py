"""GPU: DynamicGraph.neighbor_sequence against the readers that were there before it, on the toy
of test_gpu_neighbor_sequence.py and on a sampler-grade random graph (power-law sources, 4 000
edges with heavy ties, ingested in chunks, with and without reverse edges):

- lengths, nodes, eids and times are neighbor_cooccurrence's side 0 with the node on both sides
  and include_self=False, element for element, the padding included;
- lengths is temporal_degree clamped to the length;
- the edge part of the tokens is edge_feats[eids] where the slot is filled and the eid has a row;
- the node part, summed over the positions by a sequential float32 loop on the host, is
  neighbor_aggregate(max_history=L, reduce="sum").node bit for bit (a padded slot and an id without
  a row add +0.0, which changes no bit of a sum that started from +0.0)."""
import numpy as np
import pytest
import torch

from tests import synth
from tests import test_gpu_neighbor_sequence as T

pytestmark = pytest.mark.gpu

LENGTHS = [1, 8, 65, 512]
NUM_NODES, NUM_EDGES = 300, 4000


class Case:
    pass


def _case(graph, nodes, ts, num_edges, table_rows):
    c = Case()
    c.graph, c.ts_host = graph, ts
    c.nodes, c.ts = torch.from_numpy(nodes).cuda(), torch.from_numpy(ts).cuda()
    rng = np.random.RandomState(5)
    # tables a little short of the ids in use, so that some ids have no row
    c.edge_tab = torch.from_numpy(rng.randn(num_edges - 100, 8).astype(np.float32)).cuda()
    c.node_tab = torch.from_numpy(rng.randn(table_rows, 5).astype(np.float32)).cuda()
    return c


@pytest.fixture(scope="module", params=["toy", "powerlaw", "powerlaw-undirected"])
def case(request):
    if request.param == "toy":
        graph = T._new_graph(T._edges())
        nodes, ts = T._queries()
        return _case(graph, nodes, ts, graph.num_edges(), T.NODE_ROWS)
    src, dst, ts, eid = synth.powerlaw_graph(NUM_NODES, NUM_EDGES, seed=7, tie_levels=200)
    graph = T._new_graph()
    synth.ingest_chunks(graph, src, dst, ts, eid, 997,
                        add_reverse=request.param.endswith("undirected"))
    nodes, qts = synth.random_roots(NUM_NODES, 600, 1000.0, seed=3,
                                    extra_ids=(-1, NUM_NODES, NUM_NODES + 5, 1 << 40))
    qts[10:20] = ts[1000:1010]                                   # on stored times: ties
    qts[20] = np.nan
    nodes[30:38] = np.bincount(src).argmax()                     # the busiest source, after it all
    qts[30:38] = 1100.0
    return _case(graph, nodes, qts, NUM_EDGES, NUM_NODES - 50)


def _since(case, kind):
    return T._d_since(kind, case.ts_host)


@pytest.mark.parametrize("kind", T.KINDS)
@pytest.mark.parametrize("length", LENGTHS)
def test_planes_are_neighbor_cooccurrence_side_0(case, length, kind):
    since = _since(case, kind)
    seq = case.graph.neighbor_sequence(case.nodes, case.ts, since=since, length=length)
    pair = case.graph.neighbor_cooccurrence(case.nodes, case.nodes, case.ts, since=since,
                                            length=length, include_self=False)
    assert seq.lengths.any() and (seq.lengths == 0).any()
    assert torch.equal(seq.lengths, pair.lengths[:, 0])
    assert torch.equal(seq.nodes, pair.nodes[:, 0]) and torch.equal(seq.eids, pair.eids[:, 0])
    assert torch.equal(seq.times.view(torch.int32), pair.times[:, 0].view(torch.int32))
    want = case.ts[:, None] - pair.times[:, 0]
    filled = torch.arange(length, device="cuda")[None, :] < seq.lengths[:, None]
    assert torch.equal(seq.delta_t[filled].view(torch.int32), want[filled].view(torch.int32))
    assert not seq.delta_t[~filled].view(torch.int32).any()


@pytest.mark.parametrize("kind", T.KINDS)
def test_lengths_are_temporal_degree_clamped(case, kind):
    since = _since(case, kind)
    degree = case.graph.temporal_degree(case.nodes, case.ts, since=since)
    assert (degree > 65).any()
    for length in LENGTHS:
        seq = case.graph.neighbor_sequence(case.nodes, case.ts, since=since, length=length)
        assert torch.equal(seq.lengths.long(), degree.clamp(max=length))


@pytest.mark.parametrize("kind,length", [("none", 8), ("tensor", 65), ("scalar", 512)])
def test_edge_part_is_the_indexed_table(case, kind, length):
    seq = case.graph.neighbor_sequence(case.nodes, case.ts, since=_since(case, kind),
                                       length=length, edge_feats=case.edge_tab,
                                       node_feats=case.node_tab)
    rows = case.edge_tab.shape[0]
    filled = torch.arange(length, device="cuda")[None, :] < seq.lengths[:, None]
    has_row = filled & (seq.eids < rows)
    assert has_row.any() and (filled & ~has_row).any()
    gathered = case.edge_tab[seq.eids.clamp(0, rows - 1)]
    assert torch.equal(seq.tokens[..., :8][has_row].view(torch.int32),
                       gathered[has_row].view(torch.int32))
    assert not seq.tokens[..., :8][~has_row].view(torch.int32).any()


@pytest.mark.parametrize("kind,length", [("none", 8), ("tensor", 65), ("scalar", 512),
                                         ("none", 1)])
def test_node_part_summed_in_order_is_neighbor_aggregate(case, kind, length):
    since = _since(case, kind)
    seq = case.graph.neighbor_sequence(case.nodes, case.ts, since=since, length=length,
                                       node_feats=case.node_tab)
    agg = case.graph.neighbor_aggregate(case.nodes, case.ts, node_feats=case.node_tab,
                                        since=since, max_history=length, reduce="sum")
    assert torch.equal(agg.count, seq.lengths.long())
    part = seq.tokens.cpu().numpy()
    start = np.zeros((part.shape[0], 1, part.shape[2]), np.float32)
    total = np.cumsum(np.concatenate([start, part], axis=1), axis=1, dtype=np.float32)[:, -1]
    assert total.dtype == np.float32 and total.any()
    assert np.array_equal(total.view(np.int32), agg.node.view(torch.int32).cpu().numpy())
