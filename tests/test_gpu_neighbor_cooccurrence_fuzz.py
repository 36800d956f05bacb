"""DynamicGraph.neighbor_cooccurrence on the stores the sampler is tested on: the four seeds of
test_gpu_common_neighbors_fuzz.py, which between them have an offload in the middle of the stream,
a hub of more than 8192 edges, the `replace` block policy and negative (and signed-zero) times.
The stores are built with scripts/fuzz_history.py's draw and build_store; the drawn queries (src,
dst, ts) are taken as pairs, and so is every drawn source with the row before's (two nodes that
both have histories, hubs among them), each with the draw's own lower end and with none, at length
5 and 512, and compared with tests/neighbor_cooccurrence_ref.py over histories read with
graph.get_temporal_neighbors: all five outputs exactly equal.  include_self alternates over the
four settings so that both values meet both pairings.

The rolled pairing without a lower end and without the self slot must give at least 50 rows with
a neighbour counted on both sides.  From the restatement over the drawn edge lists (no GPU) that
setting gives 561, 468, 262 and 109 such rows at length 5 and 566, 525, 267 and 255 at length 512
for the seeds 25, 54, 115 and 238."""
import os
import sys

import numpy as np
import pytest
import torch

from tests import neighbor_cooccurrence_ref as R
from tests.test_history_fuzz_inputs import SEEDS

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

COOC_SEEDS = [25, 54, 115, 238]      # test_gpu_common_neighbors_fuzz.py checks what they cover


@pytest.fixture(scope="module", params=COOC_SEEDS)
def store(request):
    import fuzz_history as F
    assert request.param in SEEDS
    d = F.draw(request.param)
    g = F.build_store(d)
    hist = R.from_graph(g, d.q_src)
    hist.update(R.from_graph(g, d.q_dst))
    return d, g, hist


@pytest.mark.parametrize("L", [5, 512])
def test_fuzzed_pairs_match_the_reference(store, L):
    d, g, hist = store
    src, ts = torch.from_numpy(d.q_src).cuda(), torch.from_numpy(d.q_ts).cuda()
    rolled = np.roll(d.q_src, 1)
    settings = [(None, rolled, False), (None, d.q_dst, True)]
    if d.since is not None:
        settings += [(d.since, rolled, True), (d.since, d.q_dst, False)]
    for since, q_dst, self_slot in settings:
        d_since = torch.from_numpy(since).cuda() if isinstance(since, np.ndarray) else since
        out = g.neighbor_cooccurrence(src, torch.from_numpy(q_dst).cuda(), ts, since=d_since,
                                      length=L, include_self=self_slot)
        want = R.neighbor_cooccurrence(hist, d.q_src, q_dst, d.q_ts, since, L, self_slot)
        R.same(tuple(x.cpu().numpy() for x in out), want)
        lengths, nodes, _, _, counts = want
        if since is None and not self_slot:
            both = int(R.has_cooccurrence(nodes, counts).sum())
            print("\nseed {} length {}: {} rows with a neighbour on both sides".format(
                d.seed, L, both))
            assert both >= 50, (d.seed, L, both)
            assert (lengths == 0).any() and (lengths > 0).any()
            if L == 5:
                deg = g.temporal_degree(src, ts).cpu().numpy()
                assert ((lengths[:, 0] == L) & (deg > L)).any()      # the bound cuts
    torch.cuda.synchronize()
