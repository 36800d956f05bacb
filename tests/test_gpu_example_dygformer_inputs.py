"""GPU: examples/dygformer_inputs.py -- neighbor_cooccurrence -> the LRU feature cache ->
time deltas -> NeighborCooccurrenceEncoder -- composes on its smallest setting, in a fresh child
process under a timeout; both pairings, the bipartite stream's and the previous-source one, where
two users share communities."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = """
import importlib.util, json, sys
spec = importlib.util.spec_from_file_location("dygformer_inputs", sys.argv[1])
mod = importlib.util.module_from_spec(spec)
spec.loader.exec_module(mod)
out = {}
for pair in ("stream", "previous"):
    out[pair] = mod.main(num_batches=2, batch_size=50, length=8, dim=4, pair=pair,
                         num_edges=4000, verbose=(pair == "stream"))
print(json.dumps(out))
"""


def test_example_runs_and_its_tensors_have_the_documented_shapes():
    import json
    p = subprocess.run([sys.executable, "-c", CHILD,
                        os.path.join(ROOT, "examples", "dygformer_inputs.py")],
                       capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    assert "slots filled" in p.stdout
    out = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
    for pair in ("stream", "previous"):
        assert len(out[pair]) == 2
        for r in out[pair]:
            assert r["node_x"] == r["edge_x"] == r["cooc_x"] == [50, 2, 8, 4]
            assert r["delta_t"] == [50, 2, 8] and r["finite"] and r["min_delta_t"] >= 0
            assert 1 <= r["mean_length"] <= 8
            assert 0 <= r["cooccurrence_share"] <= 1
    assert any(r["cooccurrence_share"] > 0 for r in out["previous"])
