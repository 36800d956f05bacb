"""GPU: examples/dygformer.py -- pair_sequence's finished channels -> models.DyGFormer ->
LinkLoss, an optimiser step, LinkMetrics on a held-out tail -- composes on its smallest setting:
2 training batches and 1 held-out batch of 40 edges, 2 negatives per source, L = 8 slots in
patches of 2, a 5 000-edge stream."""
import importlib.util
import math
import os

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_example_runs_and_its_results_are_finite(capsys):
    spec = importlib.util.spec_from_file_location(
        "dygformer_example", os.path.join(ROOT, "examples", "dygformer.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    out = mod.main(num_batches=2, eval_batches=1, batch_size=40, negatives=2, length=8,
                   patch_size=2, dim=4, num_edges=5000)
    assert "DyGFormer, 2 steps" in capsys.readouterr().out
    assert [b["train"] for b in out["batches"]] == [True, True, False]
    for b in out["batches"]:
        assert b["score"] == (120, 1) and b["pred_pos"] == (40, 1) and b["pred_neg"] == (80, 1)
        if b["train"]:
            assert math.isfinite(b["loss"]) and b["loss"] > 0
    loss, metrics = out["loss"], out["metrics"]
    assert loss["batches"] == 2 and loss["nonfinite"] == 0 and math.isfinite(loss["mean_loss"])
    assert metrics["batches"] == 1 and metrics["nonfinite"] == 0
    for key in ("ap", "auc", "mrr"):
        assert math.isfinite(metrics[key]) and 0 <= metrics[key] <= 1
