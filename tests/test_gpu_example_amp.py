"""GPU: examples/train_edge_prediction.py with amp=True (bfloat16 autocast around the forward and
the loss, no GradScaler) runs a few batches and gives finite losses."""
import importlib.util
import math
import os

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_training_example_runs_under_autocast():
    spec = importlib.util.spec_from_file_location(
        "train_edge_prediction", os.path.join(ROOT, "examples", "train_edge_prediction.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    losses = mod.main(num_batches=3, verbose=False, amp=True)
    assert len(losses) == 3 and all(math.isfinite(x) for x in losses)
