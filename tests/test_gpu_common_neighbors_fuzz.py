"""DynamicGraph.common_neighbors and temporal_degree on the stores the sampler is tested on: four
of the seeds tests/test_history_fuzz_inputs.py vouches for, which between them have an offload in
the middle of the stream, a hub of more than 8192 edges, the `replace` block policy and negative
(and signed-zero) times.  The stores are built with scripts/fuzz_history.py's draw and
build_store; the drawn queries (src, dst, ts) are taken as pairs, and so is every drawn source
with the row before's (two nodes that both have histories, hubs among them: hundreds of rows with
common neighbours, where a drawn destination often has no history at all), each with the draw's
own lower end and with none, and compared with tests/common_neighbors_ref.py over histories read
with graph.get_temporal_neighbors: all eight outputs exactly equal."""
import os
import sys

import numpy as np
import pytest
import torch

from tests import common_neighbors_ref as R
from tests.test_history_fuzz_inputs import DRAWN, SEEDS

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

CN_SEEDS = [25, 54, 115, 238]
K = 5


def test_the_seeds_cover_the_store_features():
    import fuzz_history as F
    assert set(CN_SEEDS) <= set(SEEDS)
    for feature in ("offload", "hub", "replace", "negative"):
        assert any(feature in F.features(F.draw(s)) for s in CN_SEEDS), feature
        assert any(feature in DRAWN[s].split() for s in CN_SEEDS), feature


@pytest.fixture(scope="module", params=CN_SEEDS)
def store(request):
    import fuzz_history as F
    d = F.draw(request.param)
    g = F.build_store(d)
    ends = np.concatenate([d.q_src, d.q_dst])
    hist = R.from_graph(g, ends)
    return d, g, hist


@pytest.mark.parametrize("H", [5, 512])
def test_fuzzed_pairs_match_the_reference(store, H):
    d, g, hist = store
    src, ts = torch.from_numpy(d.q_src).cuda(), torch.from_numpy(d.q_ts).cuda()
    lower_ends = [d.since] + ([None] if d.since is not None else [])
    some_common = 0
    for since, q_dst in [(s, q) for s in lower_ends for q in (d.q_dst, np.roll(d.q_src, 1))]:
        d_since = torch.from_numpy(since).cuda() if isinstance(since, np.ndarray) else since
        out = g.common_neighbors(src, torch.from_numpy(q_dst).cuda(), ts, since=d_since,
                                 max_history=H, max_common=K)
        got = tuple(x.cpu().numpy() for x in out)
        want = R.common_neighbors(hist, d.q_src, q_dst, d.q_ts, since, H, K)
        for name, a, b in zip(out._fields, got, want):
            bad = np.flatnonzero((a != b).reshape(len(a), -1).any(1))
            assert a.dtype == b.dtype and a.shape == b.shape and len(bad) == 0, \
                "seed {} {}: rows {} got {} want {}".format(d.seed, name, bad[:5], a[bad[:5]],
                                                            b[bad[:5]])
        some_common += int((want[4] > 0).sum())
        deg = g.temporal_degree(src, ts, since=d_since).cpu().numpy()
        assert np.array_equal(deg, R.temporal_degree(hist, d.q_src, d.q_ts, since))
        if since is None:
            assert (deg > 0).any() and (deg == 0).any()
            assert (want[0] > 0).any()
            if H == 5:
                assert ((want[0] == H) & (deg > H)).any()            # the bound cuts
    assert some_common >= 50, d.seed
    torch.cuda.synchronize()
