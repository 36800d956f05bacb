"""The four edge-history readers (DynamicGraph.pair_history, DynamicGraph.seen_mask,
DeviceBatchStream's historical negatives, DynamicGraph.temporal_random_walk) on the stores the
sampler is tested on: a slice of scripts/fuzz_history.py in the suite, and three scenarios that
do not depend on a draw.  Every comparison is exact (ids, counts and mask words equal, last_ts and
walk times bit for bit), against the readers' numpy restatements (check A) and against what
TemporalSampler(graph, [k], "recent") samples for the same rows (check B).

Check B runs on all rows, the rows that tie with an edge included: the sampler's upper end is
strict, as the readers'.  On a store with negative times it samples with a window of 4e6 and
leaves out the rows at t = +inf (fuzz_history's docstring has the reasons).

The 16 seeds are those tests/test_history_fuzz_inputs.py vouches for; run(seed, conditions=True)
asserts the same conditions once more on the histories the store holds, the seeds with an
offload included."""
import os
import sys

import numpy as np
import pytest
import torch

from tests import synth
from tests.test_history_fuzz_inputs import SEEDS

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))


@pytest.mark.parametrize("seed", SEEDS)
def test_history_fuzz(seed):
    import fuzz_history
    fuzz_history.run(seed, conditions=True)


def _newest_edges(src, dst, ts):
    """Per node that has an edge: (node, the destination and the time of its newest edge)."""
    order = np.lexsort((np.arange(len(src)), ts, src))
    last = order[np.flatnonzero(np.append(src[order][1:] != src[order][:-1], True))]
    return src[last], dst[last], ts[last]


def _around(t):
    """The float32 below t, t and the float32 above t."""
    t = np.asarray(t, np.float32)
    return np.nextafter(t, np.float32(-np.inf)), t, np.nextafter(t, np.float32(np.inf))


@pytest.mark.parametrize("max_history", [0, 5])
def test_negative_times_and_rows_around_the_newest_edge(max_history):
    """The reader-side twin of the sampler's test of that name: half of the times are negative,
    and every node is asked at, one float below and one float above its newest edge's time (the
    last_ts_bits shortcut is taken only above), for that edge's destination; the remaining rows
    are anywhere, some before the node's first edge, and -0.0 / +0.0 against a node whose edges
    are at both."""
    import fuzz_history as F
    N, E = 300, 6000
    src, dst, ts, eid = synth.powerlaw_graph(N, E, seed=31, tie_levels=700)
    ts = (ts - np.float32(500.0)).astype(np.float32)                # [-500, 500)
    z = int(np.searchsorted(ts, 0.0))
    src[z - 2:z + 2] = 7
    ts[z - 2:z], ts[z:z + 2] = np.float32(-0.0), np.float32(0.0)
    dst[z - 1] = dst[z]      # one destination at -0.0 and at +0.0: the last row below meets both
    g = F.new_graph(8, "insert", True)
    g.add_edges(src, dst, ts, eid)
    v, d, t = _newest_edges(src, dst, ts)
    assert len(v) > 200 and (t < 0).any() and (t > 0).any()
    rng = np.random.RandomState(3)
    pick = rng.randint(0, E, 300)
    q_src = np.concatenate([v, v, v, src[pick], [7, 7, 7]])
    q_dst = np.concatenate([d, d, d, dst[rng.randint(0, E, 300)], dst[z - 2:z + 1]])
    q_ts = np.concatenate(list(_around(t)) + [rng.uniform(-600.0, 600.0, 300).astype(np.float32),
                                              np.array([-0.0, 0.0, 1.0], np.float32)])
    a = F.arguments(q_src, q_dst, q_ts, dst, True, max_history=max_history,
                    since=F.since_tensor(q_ts), cands=np.unique(dst)[:130].copy(), first_row=77,
                    epoch=5)
    # not vacuous: the three rows of a node differ where its newest edge is the only match
    n = len(v)
    want = F.P.pair_history(F.P.from_graph(g, q_src), a.q_src, a.q_dst, a.q_ts, None, max_history)
    if max_history == 0:
        assert (want[0][:n] < want[0][2 * n:3 * n]).all()
    assert (want[2][n:2 * n] != want[2][2 * n:3 * n]).all()          # a tie is not history
    # the latest of equal times is told by the store's order: +0.0 here, after -0.0
    assert want[0][-1] >= 2 and want[1][-1] == 0 and not np.signbit(want[1][-1])
    assert want[2][-1] == eid[z]
    assert F.check_readers(g, a, "negative times") >= (len(q_src) if max_history else 100)


@pytest.mark.parametrize("max_history", [0, 5])
def test_replace_policy_small_chunks_and_an_offload_inside_the_hubs_run(max_history):
    """`replace` policy, minimum block size 1, chunks of 7 edges, and an offload whose cut lies
    between the hub's first and newest edge of the first half: the hub's one block stays whole,
    the blocks of nodes whose newest edge is older than the cut go, and the stream goes on."""
    import fuzz_history as F
    N, E, HUB = 200, 2500, 3
    src, dst, ts, eid = synth.powerlaw_graph(N, E, seed=17, alpha=1.6, tie_levels=60)
    rng = np.random.RandomState(4)
    at = np.sort(rng.choice(E, 700, replace=False))
    src[at], dst[at] = HUB, rng.randint(0, 12, 700)
    g = F.new_graph(1, "replace", True)
    half = (E // 2 // 7) * 7
    synth.ingest_chunks(g, src[:half], dst[:half], ts[:half], eid[:half], 7)
    hub_ts = ts[:half][src[:half] == HUB]
    cut = float(np.median(hub_ts))
    assert hub_ts[0] < cut < hub_ts[-1]
    edges_before = g.num_edges()
    assert g.offload_old_blocks(cut) > 0 and g.num_edges() < edges_before
    synth.ingest_chunks(g, src[half:], dst[half:], ts[half:], eid[half:], 7)
    assert g.out_degree(np.array([HUB]))[0] == np.count_nonzero(src == HUB)
    q_src, q_ts = synth.random_roots(N, 600, 1000.0, seed=9, extra_ids=[N + 2, -1])
    q_dst = dst[rng.randint(0, E, 600)]
    pick = rng.randint(0, E, 600)
    own = np.arange(600) % 3 == 0
    q_src[own], q_dst[own], q_ts[own] = src[pick[own]], dst[pick[own]], ts[pick[own]]
    q_ts[np.arange(600) % 3 == 1] = np.float32(1e6)
    q_src[5:40], q_dst[5:40] = HUB, rng.randint(0, 12, 35)
    a = F.arguments(q_src, q_dst, q_ts, dst, False, max_history=max_history, since=float(cut),
                    cands=np.arange(65, dtype=np.int64), K=3, Kh=1, L=8, W=1)
    F.check_readers(g, a, "replace and offload")
    torch.cuda.synchronize()


@pytest.mark.parametrize("max_history", [0, 1000])
def test_a_hub_of_8192_edges_and_a_far_source_id(max_history):
    """A hub long enough that pair_history strides more than 100 trips per lane and the search
    takes 14 halvings, in a store whose node table has 70 000 empty entries before its last
    source."""
    import fuzz_history as F
    N, E, HUB, FAR = 50, 2000, 11, 50 + 70000
    src, dst, ts, eid = synth.powerlaw_graph(N, E, seed=23, tie_levels=5000)
    rng = np.random.RandomState(6)
    n = 8192 + 150
    src = np.concatenate([src, np.full(n, HUB, np.int64)])
    dst = np.concatenate([dst, rng.randint(20, 40, n)])
    ts = np.concatenate([ts, np.floor(np.sort(rng.uniform(0, 1000, n)) * 5) / 5]).astype(np.float32)
    order = np.argsort(ts, kind="stable")
    src, dst, ts = src[order], dst[order], ts[order]
    E = len(src)
    far_at = np.array([100, E // 2, E - 50])
    src[far_at] = FAR
    g = F.new_graph(8, "insert", True)
    synth.ingest_chunks(g, src, dst, ts, np.arange(E), 6000)
    assert g.max_vertex_id() == FAR and g.out_degree(np.array([HUB]))[0] >= 8192
    q_src, q_ts = synth.random_roots(N, 400, 1000.0, seed=2, extra_ids=[N + 2, -1, FAR + 1])
    q_dst = dst[rng.randint(0, E, 400)]
    hub_rows = np.arange(400) % 2 == 1
    q_src[hub_rows], q_dst[hub_rows] = HUB, rng.randint(20, 41, 200)
    q_src[10:16], q_dst[10:16] = FAR, np.tile(dst[far_at], 2)
    q_ts[10:16] = np.concatenate([ts[far_at], [1e6, ts[far_at[1]] + 1, -1.0]])
    q_ts[np.arange(400) % 8 == 3] = np.float32(1e6)
    a = F.arguments(q_src, q_dst, q_ts, dst, False, max_history=max_history,
                    since=F.since_tensor(q_ts), cands=np.arange(15, 80, dtype=np.int64),
                    recency=4, first_row=1 << 40)
    want = F.P.pair_history(F.P.from_graph(g, q_src), a.q_src, a.q_dst, a.q_ts, None, max_history)
    # with the whole history some lane holds three or more matches
    assert want[0][hub_rows].max() > (20 if max_history else 128) and (want[0][10:16] > 0).any()
    F.check_readers(g, a, "hub and far id")
