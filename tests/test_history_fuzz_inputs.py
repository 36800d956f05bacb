"""The draws of scripts/fuzz_history.py, without a GPU: that the exact comparisons of
tests/test_gpu_history_readers_fuzz.py are not vacuous on the 16 seeds it runs.

SEEDS are those 16.  They were chosen, among the seeds 0 .. 399, so that fuzz_history.check_inputs
holds for each of them:

  - at least 10 % of the rows have count > 0 and at least 10 % have count == 0;
  - each of three restatements that are wrong on purpose (<= for <, the oldest n for the newest
    n, max_history + 1 for max_history) differs from the expected output on at least 1 % of the
    rows;
  - on the seeds with negative times a window taken to start at the node's first edge whenever
    since <= 0 differs on at least one row, and rows at -0.0 and at +0.0 ask for the node whose
    history holds both;
  - at least one row is on its node's newest edge's time.

No seed with max_history == 0 can be among them, since without a bound the oldest n are the
newest n; the pinned scenarios of the GPU module run with max_history == 0.

The histories here come from the drawn edge lists through temporal_walk_ref.from_chunks, which
restates the store's order call by call, under either block policy, but not an offload (that
takes the block policy).  So this file asserts check_inputs on the seeds WITHOUT an offload,
NO_OFFLOAD below; on the eight others it asserts what the draw alone shows, and the GPU module
asserts check_inputs for all 16 on the histories the store holds (run(seed, conditions=True)).
"""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import fuzz_history as F      # noqa: E402
from tests import temporal_walk_ref as T      # noqa: E402

SEEDS = [2, 9, 19, 25, 54, 59, 96, 112, 115, 143, 235, 238, 259, 268, 278, 316]
NO_OFFLOAD = [2, 9, 19, 54, 143, 238, 268, 316]
# the store features of each seed, of fuzz_history.FEATURES
DRAWN = {
    2: "negative replace", 9: "shuffle hub", 19: "replace", 25: "replace offload shuffle far",
    54: "negative far hub", 59: "negative offload hub", 96: "negative replace offload",
    112: "replace offload shuffle hub", 115: "negative replace offload hub", 143: "",
    235: "negative offload far", 238: "negative replace shuffle hub", 259: "replace offload hub",
    268: "negative", 278: "negative offload shuffle hub", 316: "negative replace far",
}


def test_the_seeds_cover_every_store_feature_twice():
    assert len(SEEDS) == len(set(SEEDS)) == 16 and sorted(DRAWN) == SEEDS
    for seed in SEEDS:
        d = F.draw(seed)
        assert " ".join(F.features(d)) == DRAWN[seed], seed
        assert (seed in NO_OFFLOAD) == (not d.offload), seed
    for feature in F.FEATURES:
        assert sum(feature in DRAWN[s].split() for s in SEEDS) >= 2, feature
    # and the reader arguments vary: every kind of lower end, bounds below and above a wave
    draws = [F.draw(s) for s in SEEDS]
    assert {d.since_kind for d in draws} == {"none", "scalar", "tensor"}
    assert {1, 5, 64, 65, 1000} <= {d.max_history for d in draws}
    assert {d.chunk for d in draws} == {7, 333, 6000}
    assert {d.min_block for d in draws} == {1, 4, 62}


@pytest.mark.parametrize("seed", SEEDS)
def test_a_draw_is_a_valid_stream_and_holds_its_special_rows(seed):
    d = F.draw(seed)
    same = F.draw(seed)
    assert all(np.array_equal(getattr(d, k), getattr(same, k), equal_nan=True)
               for k in ("src", "dst", "ts", "eid", "q_src", "q_dst", "q_ts"))
    assert d.E <= 20000 and d.B <= 1500 and sorted(d.eid) == list(range(d.E))
    # call after call the times ascend, whatever the order inside a call
    lows = [d.ts[i:i + d.chunk].min() for i in range(0, d.E, d.chunk)]
    highs = [d.ts[i:i + d.chunk].max() for i in range(0, d.E, d.chunk)]
    assert all(h <= l for h, l in zip(highs[:-1], lows[1:]))
    inside = [np.all(np.diff(d.ts[i:i + d.chunk]) >= 0) for i in range(0, d.E, d.chunk)]
    assert all(inside) == (not d.shuffle)
    assert (d.ts < 0).any() == d.negative
    if d.negative:
        z = d.ts[d.zero_rows]
        assert (d.src[d.zero_rows] == d.zero_node).all() and (z == 0).all()
        assert np.signbit(z).any() and not np.signbit(z).all()
        rows = d.q_src == d.zero_node
        assert (rows & (d.q_ts == 0) & np.signbit(d.q_ts)).any()
        assert (rows & (d.q_ts == 0) & ~np.signbit(d.q_ts)).any()
    if d.far:
        assert np.count_nonzero(d.src == d.N + F.FAR) >= 1
    if d.hub >= 0:
        assert np.count_nonzero(d.src == d.hub) >= F.HUB_EDGES
        # pair_history strides more than 100 trips per lane over such a run
        assert np.count_nonzero(d.src == d.hub) / 64 > 100
    assert np.isneginf(d.q_ts).any() and np.isposinf(d.q_ts).any() and np.isnan(d.q_ts).any()
    assert (d.q_ts == np.float32(F.LATE)).mean() > 0.2 and (d.kind == 0).mean() > 0.2
    assert d.q_src[0] == d.N + 2 and d.q_src[1] == -1
    assert d.max_history > 0


@pytest.mark.parametrize("seed", NO_OFFLOAD)
def test_the_comparisons_of_a_seed_are_not_vacuous(seed):
    d = F.draw(seed)
    out = F.check_inputs(d, F.edge_histories(d))
    print(F.describe(d), out)
    if d.hub >= 0:      # count_before takes 14 halvings over the hub's run
        assert len(F.edge_histories(d)[d.hub][1]).bit_length() >= 14


def test_from_chunks_is_from_edges_call_after_call():
    """One call: from_edges.  Several: every call's from_edges in turn, appended."""
    d = F.draw(19)      # in time order: any chunking is a valid stream
    edges = tuple(x[:500] for x in (d.src, d.dst, d.ts, d.eid))
    for reverse in (False, True):
        one, one_len = T.from_edges(*edges, reverse)
        got, got_len = T.from_chunks(*edges, 500, reverse)
        assert got_len == one_len and sorted(got) == [v for v in one if len(one[v][0])]
        for v in got:
            assert all(np.array_equal(x, y) for x, y in zip(got[v], one[v]))
        chunk = 70      # the last call is a short one
        want = {}
        for i in range(0, 500, chunk):
            part, _ = T.from_edges(*(x[i:i + chunk] for x in edges), reverse)
            for v, h in part.items():
                if len(h[0]):
                    want[v] = h if v not in want else tuple(
                        np.concatenate([a, b]) for a, b in zip(want[v], h))
        got, _ = T.from_chunks(*edges, chunk, reverse)
        assert sorted(got) == sorted(want)
        for v in got:
            assert all(np.array_equal(x, y) for x, y in zip(got[v], want[v]))
            assert np.all(np.diff(got[v][1]) >= 0)


def test_the_wrong_restatements_are_wrong_where_they_should_be():
    """On a history of five edges: a tie, the bound and its direction."""
    h = {0: (np.array([7, 8, 7, 9, 7]), np.array([1, 2, 3, 3, 5], np.float32), np.arange(5))}
    q = (np.zeros(3, np.int64), np.array([7, 9, 7]), np.array([3.0, 3.0, 9.0], np.float32))
    assert [x.tolist() for x in F.restate(h, *q)] == [[1, 0, 3], [1.0, -np.inf, 5.0], [0, -1, 4]]
    assert F.restate(h, *q, 0, "le")[0].tolist() == [2, 1, 3]
    assert F.restate(h, *q, 2)[0].tolist() == [1, 0, 1]
    assert F.restate(h, *q, 2, "oldest")[0].tolist() == [1, 0, 1]
    assert F.restate(h, *q, 2, "oldest")[2].tolist() == [0, -1, 0]
    assert F.restate(h, *q, 2, "off_by_one")[0].tolist() == [1, 0, 2]
