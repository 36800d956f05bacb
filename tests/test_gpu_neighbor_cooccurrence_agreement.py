"""DynamicGraph.neighbor_cooccurrence against the readers that were there before it, on
test_gpu_neighbor_cooccurrence.py's graph and queries, with no restatement in between and zero
tolerance: under the same window (t, since, H = length - include_self)

- lengths - self is common_neighbors' n_src / n_dst and min(temporal_degree, H);
- a position's count in channel 0 is pair_history(src, its node).count, in channel 1
  pair_history(dst, its node).count, plus the self slot's one occurrence where the node is that
  end itself (and not negative: a negative id is not counted);
- without the self slot, the nodes with both counts > 0 are common_neighbors' common ones."""
import numpy as np
import pytest
import torch

from tests.test_gpu_neighbor_cooccurrence import _d_since, _edges, _new_graph, _queries

pytestmark = pytest.mark.gpu


class Toy:
    pass


@pytest.fixture(scope="module", params=[False, True], ids=["directed", "reverse"])
def toy(request):
    t = Toy()
    src, dst, ts = _queries()
    t.graph = _new_graph(_edges(), add_reverse=request.param)
    t.ts = ts
    t.src, t.dst, t.t = (torch.from_numpy(x).cuda() for x in (src, dst, ts))
    return t


@pytest.mark.parametrize("kind", ["none", "tensor"])
@pytest.mark.parametrize("L,self_slot", [(1, False), (2, True), (33, True), (128, False),
                                         (512, True)])
def test_lengths_are_the_window_sizes(toy, L, self_slot, kind):
    since = _d_since(kind, toy.ts)
    H = L - int(self_slot)
    out = toy.graph.neighbor_cooccurrence(toy.src, toy.dst, toy.t, since=since, length=L,
                                          include_self=self_slot)
    cn = toy.graph.common_neighbors(toy.src, toy.dst, toy.t, since=since, max_history=H,
                                    max_common=0)
    n = out.lengths - int(self_slot)
    assert torch.equal(n[:, 0], cn.n_src) and torch.equal(n[:, 1], cn.n_dst)
    for side, end in ((0, toy.src), (1, toy.dst)):
        deg = toy.graph.temporal_degree(end, toy.t, since=since)
        assert torch.equal(n[:, side].long(), deg.clamp(max=H))
    assert (n > 0).any() and (n == 0).any() and (n == H).any()
    # the filled slots are the first ones, and only they hold an edge
    filled = torch.arange(L, device="cuda") < out.lengths[:, :, None]
    has_edge = filled.clone()
    if self_slot:
        has_edge[:, :, 0] = False
    assert torch.equal(out.eids >= 0, has_edge)
    assert (out.nodes[~filled] == -1).all() and (out.counts[~filled] == 0).all()
    assert (out.times[~filled] == 0).all()


@pytest.mark.parametrize("L,self_slot", [(33, True), (40, False)])
def test_the_counts_are_pair_historys(toy, L, self_slot):
    since = _d_since("tensor", toy.ts)
    H = L - int(self_slot)
    out = toy.graph.neighbor_cooccurrence(toy.src, toy.dst, toy.t, since=since, length=L,
                                          include_self=self_slot)
    assert ((out.counts[..., 0] >= 2) & (out.counts[..., 1] >= 2)).any()
    corrected = 0
    for side in (0, 1):
        for p in range(L):
            z = out.nodes[:, side, p].contiguous()
            for channel, end in ((0, toy.src), (1, toy.dst)):
                count = toy.graph.pair_history(end, z, toy.t, since=since, max_history=H).count
                own = (z == end) & (z >= 0) if self_slot else torch.zeros_like(z, dtype=torch.bool)
                corrected += int(own.sum())
                assert torch.equal(out.counts[:, side, p, channel].long() - own.long(), count), \
                    (side, p, channel)
    assert (corrected > 0) == self_slot


@pytest.mark.parametrize("H", [5, 32, 129, 512])
def test_the_nodes_on_both_sides_are_the_common_neighbours(toy, H):
    K = 64
    since = _d_since("tensor", toy.ts)
    out = toy.graph.neighbor_cooccurrence(toy.src, toy.dst, toy.t, since=since, length=H,
                                          include_self=False)
    cn = toy.graph.common_neighbors(toy.src, toy.dst, toy.t, since=since, max_history=H,
                                    max_common=K)
    nodes, counts = out.nodes.cpu().numpy(), out.counts.cpu().numpy()
    common, cn_nodes = cn.common.cpu().numpy(), cn.nodes.cpu().numpy()
    both = (nodes >= 0) & (counts[..., 0] > 0) & (counts[..., 1] > 0)
    compared = 0
    for i in range(len(nodes)):
        mine = set(nodes[i, 0][both[i, 0]].tolist())
        assert mine == set(nodes[i, 1][both[i, 1]].tolist()), i      # the same set on either side
        assert len(mine) == common[i], i
        if common[i] <= K:
            assert mine == set(cn_nodes[i][cn_nodes[i] >= 0].tolist()), i
            compared += common[i] > 0
    assert compared >= 8 and (common > K).any() == (H >= 129)
