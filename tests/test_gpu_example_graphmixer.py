"""GPU: examples/graphmixer.py -- neighbor_cooccurrence's sequences and neighbor_aggregate's mean
-> models.GraphMixer -> LinkLoss, an optimiser step, LinkMetrics -- composes on its smallest
setting: 2 batches of 50 edges, K = 8 tokens, H = 16 history edges, a 5 000-edge stream."""
import importlib.util
import math
import os

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_example_runs_and_its_results_are_finite(capsys):
    spec = importlib.util.spec_from_file_location(
        "graphmixer_example", os.path.join(ROOT, "examples", "graphmixer.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    out = mod.main(num_batches=2, batch_size=50, num_tokens=8, max_history=16, dim=4,
                   num_edges=5000)
    assert "GraphMixer, 2 steps" in capsys.readouterr().out
    assert len(out["batches"]) == 2
    for b in out["batches"]:
        assert b["edge_x"] == (150, 8, 4) and b["delta_t"] == (150, 8)
        assert b["nbr_mean"] == (150, 4)
        assert b["pred_pos"] == (50, 1) and b["pred_neg"] == (50, 1)
        assert math.isfinite(b["loss"]) and b["loss"] > 0
        assert 0 < b["mean_tokens"] <= 8 and 0 < b["mean_history"] <= 16
    loss, metrics = out["loss"], out["metrics"]
    assert loss["batches"] == 2 and loss["nonfinite"] == 0 and math.isfinite(loss["mean_loss"])
    assert metrics["batches"] == 2 and metrics["nonfinite"] == 0
    for key in ("ap", "auc", "mrr"):
        assert math.isfinite(metrics[key]) and 0 <= metrics[key] <= 1
