"""gnnflow_amd.EdgeBank on the GPU against tests/pair_history_ref.edge_bank_scores, exactly; its
output shapes and what LinkMetrics makes of them; and the two examples that use it.

The graph has 30 sources, 32 destinations and 600 edges at whole-numbered times in [0, 100), with
pairs that repeat.  The batch is every twelfth edge of the stream, 48 edges from early ones, whose
pair is new, to late ones, each with three negatives of which some are nodes the source has met,
some it has not, and some are unknown to the graph."""
import importlib.util
import math
import os

import numpy as np
import pytest
import torch

from tests import pair_history_ref as P

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, KMAX, WINDOW = 48, 3, 20.0


def _edges():
    rng = np.random.RandomState(5)
    n = 600
    src = rng.choice(30, n)
    dst = (src + rng.choice(8, n) + 1) % 32      # eight partners per source: pairs repeat
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
    t.graph.add_edges(src, dst, ts)
    rng = np.random.RandomState(6)
    rows = np.arange(24, 600, 12)                 # B edges from early (no history yet) to late
    t.src, t.dst, t.ts = src[rows], dst[rows], ts[rows]
    t.neg = rng.choice(40, KMAX * B).astype(np.int64)      # k-major; 32 .. 39 are unknown
    t.hist = P.from_graph(t.graph, np.arange(40))
    return t


def _batch(toy, K):
    """(roots, ts) in get_batch's layout on the device, and the pairs they mean on the host."""
    roots = np.concatenate([toy.src, toy.dst, toy.neg[:K * B]])
    ts = np.tile(toy.ts, 2 + K)
    pairs = (np.tile(toy.src, 1 + K), roots[B:], np.tile(toy.ts, 1 + K))
    return torch.from_numpy(roots).cuda(), torch.from_numpy(ts).cuda(), pairs


def test_the_batch_exercises_the_bank(toy):
    src, dst, ts = _batch(toy, KMAX)[2]
    count = P.pair_history(toy.hist, src, dst, ts)[0]
    assert (count[:B] >= 3).sum() >= 5 and (count[:B] == 0).sum() >= 1     # positives both ways
    assert (count[B:] > 0).sum() >= 5 and (count[B:] == 0).sum() >= 5      # negatives both ways
    assert ((count > 0) & (count < 3)).sum() >= 5                          # min_count = 3 matters
    windowed = P.pair_history(toy.hist, src, dst, ts, ts - np.float32(WINDOW))[0]
    assert (windowed <= count).all() and 0 < windowed.sum() < count.sum()  # the window matters
    assert (toy.neg >= 32).sum() >= 5


@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("min_count", [1, 3])
@pytest.mark.parametrize("score", ["seen", "count"])
@pytest.mark.parametrize("mode", ["unlimited", "time_window"])
def test_scores_match_the_reference(toy, mode, score, min_count, K):
    import gnnflow_amd
    window = WINDOW if mode == "time_window" else None
    bank = gnnflow_amd.EdgeBank(toy.graph, mode, window=window, min_count=min_count, score=score)
    roots, ts, (src, dst, t) = _batch(toy, K)
    want = P.edge_bank_scores(toy.hist, src, dst, t, mode=mode, window=window,
                              min_count=min_count, score=score)
    got = bank.score_pairs(*(torch.from_numpy(x).cuda() for x in (src, dst, t)))
    assert got.dtype == torch.float32 and tuple(got.shape) == ((1 + K) * B,)
    assert np.array_equal(got.cpu().numpy(), want)
    pos, neg = bank.predict(roots, ts, neg_sample_ratio=K)
    assert pos.dtype == neg.dtype == torch.float32
    assert tuple(pos.shape) == (B, 1) and tuple(neg.shape) == (K * B, 1)
    assert np.array_equal(pos.cpu().numpy()[:, 0], want[:B])
    assert np.array_equal(neg.cpu().numpy()[:, 0], want[B:])
    # ts with only the B edge times, and host arrays as get_batch yields them
    pos2, neg2 = bank.predict(roots.cpu().numpy(), ts[:B].cpu().numpy(), K)
    assert torch.equal(pos2, pos) and torch.equal(neg2, neg)


def test_max_history_bounds_the_bank(toy):
    import gnnflow_amd
    _, _, (src, dst, t) = _batch(toy, KMAX)
    bank = gnnflow_amd.EdgeBank(toy.graph, max_history=4, score="count")
    got = bank.score_pairs(*(torch.from_numpy(x).cuda() for x in (src, dst, t)))
    want = P.edge_bank_scores(toy.hist, src, dst, t, max_history=4, score="count")
    assert np.array_equal(got.cpu().numpy(), want)
    assert want.sum() < P.edge_bank_scores(toy.hist, src, dst, t, score="count").sum()


def test_a_window_wider_than_the_span_is_unlimited_memory(toy):
    import gnnflow_amd
    roots, ts, _ = _batch(toy, KMAX)
    for score in ("seen", "count"):
        a = gnnflow_amd.EdgeBank(toy.graph, score=score).predict(roots, ts, KMAX)
        b = gnnflow_amd.EdgeBank(toy.graph, "time_window", window=1000.0,
                                 score=score).predict(roots, ts, KMAX)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        c = gnnflow_amd.EdgeBank(toy.graph, "time_window", window=WINDOW,
                                 score=score).predict(roots, ts, KMAX)
        assert not (torch.equal(a[0], c[0]) and torch.equal(a[1], c[1]))


@pytest.mark.parametrize("score", ["seen", "count"])
def test_link_metrics_take_the_scores_as_they_are(toy, score):
    import gnnflow_amd
    bank = gnnflow_amd.EdgeBank(toy.graph, score=score)
    metrics = gnnflow_amd.LinkMetrics(torch.device("cuda", 0))
    for K in (1, 3):
        roots, ts, _ = _batch(toy, K)
        pos, neg = bank.predict(roots, ts, K)
        assert tuple(pos.shape) == (B, 1) and tuple(neg.shape) == (K * B, 1)
        assert torch.isfinite(pos).all() and torch.isfinite(neg).all()
        metrics.update(pos, neg, sigmoid=False)
    r = metrics.compute()
    assert r["nonfinite"] == 0 and r["batches"] == 2
    assert math.isfinite(r["ap"]) and math.isfinite(r["auc"])
    assert 0.5 < r["auc"] <= 1.0 and 0.0 < r["ap"] <= 1.0      # repeats dominate this stream


def test_an_empty_batch(toy):
    import gnnflow_amd
    bank = gnnflow_amd.EdgeBank(toy.graph, "time_window", window=WINDOW)
    pos, neg = bank.predict(torch.zeros(0, dtype=torch.int64, device="cuda"),
                            torch.zeros(0, device="cuda"), 2)
    assert tuple(pos.shape) == (0, 1) and tuple(neg.shape) == (0, 1)
    with pytest.raises(ValueError, match="multiple"):
        bank.predict(torch.zeros(7, dtype=torch.int64, device="cuda"), torch.zeros(7, device="cuda"))
    with pytest.raises(ValueError, match="edge times"):
        bank.predict(torch.zeros(6, dtype=torch.int64, device="cuda"), torch.zeros(1, device="cuda"))


def _example(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "examples", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_edge_bank_example(capsys):
    mod = _example("edge_bank")
    r = mod.main(num_batches=3, batch_size=100, neg_ratio=2, num_edges=6000, verbose=True)
    assert "EdgeBank unlimited" in capsys.readouterr().out
    assert r["batches"] == 3 and r["mrr_batches"] == 3 and r["nonfinite"] == 0
    assert all(math.isfinite(r[k]) and 0.0 < r[k] <= 1.0 for k in ("ap", "auc", "mrr"))
    assert r["auc"] > 0.5                                      # the synthetic stream repeats pairs
    w = mod.main(num_batches=3, batch_size=100, neg_ratio=2, num_edges=6000, verbose=False,
                 mode="time_window", score="count", hist_negatives=1)
    assert w["batches"] == 3 and w["nonfinite"] == 0 and math.isfinite(w["ap"])


def test_evaluate_edge_prediction_is_unchanged_without_the_flag(capsys):
    mod = _example("evaluate_edge_prediction")
    plain = mod.main(num_batches=2, verbose=False)
    assert "edge_bank" not in plain
    both = mod.main(num_batches=2, edge_bank=True)
    out = capsys.readouterr().out
    assert "EdgeBank" in out and [l for l in out.splitlines() if l.startswith("ap ")]
    bank = both.pop("edge_bank")
    assert set(both) == set(plain)
    for k in plain:      # the model's pass does not know about the baseline
        assert both[k] == plain[k] or (math.isnan(both[k]) and math.isnan(plain[k])), k
    assert bank["batches"] == 2 and bank["nonfinite"] == 0
    assert math.isfinite(bank["ap"]) and math.isfinite(bank["auc"]) and bank["auc"] > 0.5
