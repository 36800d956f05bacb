"""Writes tests/golden/dgnn_state_dict.json: the state_dict keys and shapes of the reference's
DGNN (gnnflow/models/dgnn.py) for the configurations the model tests cover.  Names and shapes
only.

Route used: the reference PACKAGE is imported as tests/test_pybind_import.py does it (the pybind
`libgnnflow` module of this repository and gnnflow_amd.dgl_compat stand in for the native module
and for dgl), and `gnnflow.models.dgnn.DGNN` is constructed with its memory on the CPU.

    python tests/golden/make_dgnn_fixture.py /path/to/GNNFlow
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.dont_write_bytecode = True

DIM_EDGE, DIM_TIME, DIM_EMBED, HEADS, DIM_MEMORY, NUM_NODES = 16, 20, 24, 2, 24, 300
# name -> (dim_node, num_layers, num_snapshots, use_memory)
CONFIGS = {
    "tgn_nonode": (0, 1, 1, True),
    "tgn_node32": (32, 1, 1, True),
    "tgat": (32, 2, 1, False),
    "dysat": (32, 2, 3, False),
}


def kwargs(name):
    dim_node, layers, snapshots, use_memory = CONFIGS[name]
    kw = dict(dim_node=dim_node, dim_edge=DIM_EDGE, dim_time=DIM_TIME, dim_embed=DIM_EMBED,
              num_layers=layers, num_snapshots=snapshots, att_head=HEADS, dropout=0.1,
              att_dropout=0.1, use_memory=use_memory)
    if use_memory:
        kw.update(dim_memory=DIM_MEMORY, num_nodes=NUM_NODES)
    return kw


def main(ref_root):
    from gnnflow_amd import _build, dgl_compat
    sys.path[:0] = [os.path.dirname(_build.build_pybind()), ref_root]
    dgl_compat.install(force=True)
    from gnnflow.models.dgnn import DGNN
    out = {}
    for name in CONFIGS:
        model = DGNN(memory_device="cpu", **kwargs(name))
        out[name] = {k: list(v.shape) for k, v in model.state_dict().items()}
    with open(os.path.join(HERE, "dgnn_state_dict.json"), "w") as f:
        json.dump({"dim_edge": DIM_EDGE, "dim_time": DIM_TIME, "dim_embed": DIM_EMBED,
                   "att_head": HEADS, "dim_memory": DIM_MEMORY, "num_nodes": NUM_NODES,
                   "configs": out}, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main(sys.argv[1])
