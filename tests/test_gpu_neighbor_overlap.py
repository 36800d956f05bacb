"""gnnflow_amd.NeighborOverlap on the GPU against tests/common_neighbors_ref.overlap_scores: cn,
jaccard and pa equal after the one rounding to float32, aa and ra within 1e-10 relative in
float64 before it (at most 512 positive terms, each a correctly rounded division or a logarithm
and a division off by a few units of 2^-53, summed in another order: the bound is loose by three
orders); its output shapes and what LinkMetrics makes of them; and the two examples that use it.

The graph has 30 nodes and 900 edges among them at whole-numbered times in [0, 100), built with
reverse edges, so that two nodes share neighbours and those have degrees well above 2.  The batch
is every eighteenth edge of the stream, 48 edges from early ones to late ones, each with three
negatives of which some are unknown to the graph."""
import importlib.util
import math
import os

import numpy as np
import pytest
import torch

from tests import common_neighbors_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, KMAX, WINDOW = 48, 3, 20.0


def _edges():
    rng = np.random.RandomState(8)
    n = 900
    src = rng.choice(30, n)
    dst = (src + rng.choice(12, n) + 1) % 30
    t = np.sort(np.floor(rng.rand(n) * 100))
    return src.astype(np.int64), dst.astype(np.int64), t.astype(np.float32)


class Toy:
    pass


@pytest.fixture(scope="module")
def toy():
    import gnnflow_amd
    t = Toy()
    src, dst, ts = _edges()
    t.graph = gnnflow_amd.DynamicGraph(1 << 20, 1 << 28, "cuda", 8, 128, "insert")
    t.graph.add_edges(src, dst, ts, add_reverse=True)
    rng = np.random.RandomState(9)
    rows = np.arange(36, 900, 18)
    t.src, t.dst, t.ts = src[rows], dst[rows], ts[rows]
    t.neg = rng.choice(36, KMAX * B).astype(np.int64)      # k-major; 30 .. 35 are unknown
    t.hist = R.from_graph(t.graph, np.arange(36))
    roots = np.concatenate([t.src, t.dst, t.neg])
    t.roots, t.d_ts = torch.from_numpy(roots).cuda(), torch.from_numpy(np.tile(t.ts, 5)).cuda()
    t.pairs = (np.tile(t.src, 1 + KMAX), roots[B:], np.tile(t.ts, 1 + KMAX))
    t.d_pairs = tuple(torch.from_numpy(x).cuda() for x in t.pairs)
    t.ref = {}
    return t


def _want(toy, score, H, K, window):
    key = (score, H, K, window)
    if key not in toy.ref:
        toy.ref[key] = R.overlap_scores(toy.hist, *toy.pairs, score, H, K, window)
    return toy.ref[key]


def test_the_batch_exercises_the_scores(toy):
    assert len(toy.src) == B and (toy.neg >= 30).sum() >= 5
    cn = _want(toy, "cn", 64, 64, None)
    assert (cn == 0).sum() >= 5 and (cn >= 5).sum() >= 20
    jac = _want(toy, "jaccard", 64, 64, None)
    assert ((jac > 0) & (jac < 1)).sum() >= 20 and (jac == 0).sum() >= 5
    # quotients that float32 cannot hold: the one rounding is seen
    assert (jac.astype(np.float32).astype(np.float64) != jac).sum() >= 10
    for score in ("aa", "ra"):
        full, cut = _want(toy, score, 64, 64, None), _want(toy, score, 64, 2, None)
        assert (full > 0).sum() >= 20 and (cut <= full).all() and (cut < full).sum() >= 10
        assert (_want(toy, score, 64, 64, WINDOW) != full).sum() >= 10      # the window matters
    assert (_want(toy, "pa", 5, 64, None) <= 25).all() and _want(toy, "pa", 64, 64, None).max() > 25
    assert (_want(toy, "cn", 5, 64, None) <= cn).all() and _want(toy, "cn", 5, 64, None).sum() < \
        cn.sum()


@pytest.mark.parametrize("window", [None, WINDOW])
@pytest.mark.parametrize("H,K", [(64, 64), (5, 64), (64, 2), (512, 512), (33, 0)])
@pytest.mark.parametrize("score", R.SCORES)
def test_scores_match_the_reference(toy, score, H, K, window):
    import gnnflow_amd
    base = gnnflow_amd.NeighborOverlap(toy.graph, score, max_history=H, max_common=K,
                                       window=window)
    want = _want(toy, score, H, K, window)
    got64 = base.scores_float64(*toy.d_pairs)
    got = base.score_pairs(*toy.d_pairs)
    assert got64.dtype == torch.float64 and got.dtype == torch.float32
    assert tuple(got.shape) == tuple(got64.shape) == ((1 + KMAX) * B,)
    assert torch.isfinite(got).all() and torch.equal(got, got64.float())
    got64 = got64.cpu().numpy()
    if score in ("cn", "jaccard", "pa"):
        assert np.array_equal(got.cpu().numpy(), want.astype(np.float32))
    else:
        err = np.abs(got64 - want)
        assert (err <= 1e-10 * want).all(), "largest relative error {}".format(
            (err / np.maximum(want, 1e-300)).max())
        assert np.array_equal(got64 == 0, want == 0)


@pytest.mark.parametrize("K", [0, 1, 3])
def test_predict_has_edge_predictors_shapes(toy, K):
    import gnnflow_amd
    base = gnnflow_amd.NeighborOverlap(toy.graph, "jaccard")
    want = _want(toy, "jaccard", 64, 64, None).astype(np.float32)
    roots, ts = toy.roots[:(2 + K) * B], toy.d_ts[:(2 + K) * B]
    pos, neg = base.predict(roots, ts, neg_sample_ratio=K)
    assert pos.dtype == neg.dtype == torch.float32
    assert tuple(pos.shape) == (B, 1) and tuple(neg.shape) == (K * B, 1)
    assert np.array_equal(pos.cpu().numpy()[:, 0], want[:B])
    assert np.array_equal(neg.cpu().numpy()[:, 0], want[B:(1 + K) * B])
    # ts with only the B edge times, and host arrays as get_batch yields them
    pos2, neg2 = base.predict(roots.cpu().numpy(), ts[:B].cpu().numpy(), K)
    assert torch.equal(pos2, pos) and torch.equal(neg2, neg)


@pytest.mark.parametrize("score", R.SCORES)
def test_link_metrics_take_the_scores_as_they_are(toy, score):
    import gnnflow_amd
    base = gnnflow_amd.NeighborOverlap(toy.graph, score)
    metrics = gnnflow_amd.LinkMetrics(torch.device("cuda", 0))
    for K in (1, 3):
        pos, neg = base.predict(toy.roots[:(2 + K) * B], toy.d_ts[:B], K)
        assert torch.isfinite(pos).all() and torch.isfinite(neg).all()
        metrics.update(pos, neg, sigmoid=False)
    r = metrics.compute()
    assert r["nonfinite"] == 0 and r["batches"] == 2
    assert math.isfinite(r["ap"]) and math.isfinite(r["auc"])
    assert 0.0 < r["auc"] <= 1.0 and 0.0 < r["ap"] <= 1.0


def test_an_empty_batch(toy):
    import gnnflow_amd
    for score in ("cn", "aa"):
        base = gnnflow_amd.NeighborOverlap(toy.graph, score, window=WINDOW)
        pos, neg = base.predict(torch.zeros(0, dtype=torch.int64, device="cuda"),
                                torch.zeros(0, device="cuda"), 2)
        assert tuple(pos.shape) == (0, 1) and tuple(neg.shape) == (0, 1)
        assert pos.dtype == torch.float32


def _example(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "examples", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_neighbor_baselines_example(capsys):
    mod = _example("neighbor_baselines")
    r = mod.main(num_batches=3, batch_size=100, neg_ratio=2, num_edges=6000, verbose=True)
    out = capsys.readouterr().out
    assert set(r) == set(R.SCORES) and all("NeighborOverlap " + s in out for s in R.SCORES)
    for s in R.SCORES:
        assert r[s]["batches"] == 3 and r[s]["nonfinite"] == 0
        assert all(math.isfinite(r[s][k]) and 0.0 < r[s][k] <= 1.0 for k in ("ap", "auc", "mrr"))
    w = mod.main(num_batches=2, batch_size=100, neg_ratio=1, num_edges=6000, verbose=False,
                 scores=("ra",), max_history=512, max_common=8, window=1e5, hist_negatives=1)
    assert set(w) == {"ra"} and w["ra"]["batches"] == 2 and w["ra"]["nonfinite"] == 0


def test_evaluate_edge_prediction_is_unchanged_without_the_flag(capsys):
    mod = _example("evaluate_edge_prediction")
    plain = mod.main(num_batches=2, verbose=False)
    assert "neighbor_overlap" not in plain
    both = mod.main(num_batches=2, neighbor_overlap="pa")
    out = capsys.readouterr().out
    assert "NeighborOverlap (pa" in out and "EdgeBank" not in out
    assert [l for l in out.splitlines() if l.startswith("ap ")]
    base = both.pop("neighbor_overlap")
    assert set(both) == set(plain)
    for k in plain:      # the model's pass does not know about the baseline
        assert both[k] == plain[k] or (math.isnan(both[k]) and math.isnan(plain[k])), k
    assert base["batches"] == 2 and base["nonfinite"] == 0
    assert math.isfinite(base["ap"]) and math.isfinite(base["auc"])
