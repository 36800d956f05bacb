"""Writes tests/golden/temporal_attention_state_dict.json: the state_dict keys and shapes of the
reference's TransfomerAttentionLayer (gnnflow/models/modules/layers.py) for the four
configurations tests/test_gpu_temporal_attention_layer.py covers.  Names and shapes only.

    python tests/golden/make_temporal_attention_fixture.py /path/to/GNNFlow
"""
import importlib.util
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

CONFIGS = [(32, 16, 20), (0, 16, 20), (32, 0, 0), (0, 16, 0)]
DIM_OUT, NUM_HEAD = 24, 2


def main(ref_root):
    from gnnflow_amd import dgl_compat
    dgl_compat.install()
    spec = importlib.util.spec_from_file_location(
        "_ref_layers", os.path.join(ref_root, "gnnflow", "models", "modules", "layers.py"))
    layers = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(layers)
    out = {}
    for cfg in CONFIGS:
        layer = layers.TransfomerAttentionLayer(*cfg, DIM_OUT, NUM_HEAD, 0.1, 0.1)
        out["{}_{}_{}".format(*cfg)] = {k: list(v.shape) for k, v in layer.state_dict().items()}
    with open(os.path.join(HERE, "temporal_attention_state_dict.json"), "w") as f:
        json.dump({"dim_out": DIM_OUT, "num_head": NUM_HEAD, "configs": out}, f, indent=1,
                  sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main(sys.argv[1])
