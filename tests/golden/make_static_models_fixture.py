"""Writes tests/golden/static_models_state_dict.json: the state_dict keys and shapes of the
reference's static models, SAGE (gnnflow/models/graphsage.py) and GAT (gnnflow/models/gat.py),
for the configurations tests/test_static_models.py covers.  Names and shapes only.

Route used: that of make_dgnn_fixture.py.  The reference PACKAGE is imported with the pybind
`libgnnflow` module of this repository and gnnflow_amd.dgl_compat standing in for the native
module and for dgl, so `dglnn.SAGEConv` / `dglnn.GATConv` inside the reference's classes are this
repository's layers: what the fixture pins is the models' own structure (layer keys, widths per
layer, the predictor).

    python tests/golden/make_static_models_fixture.py /path/to/GNNFlow
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.dont_write_bytecode = True

DIM_IN, DIM_OUT = 20, 12
# name -> constructor arguments after (DIM_IN, DIM_OUT)
SAGE_CONFIGS = {"sage_{}_{}".format(agg, layers): dict(num_layers=layers, aggregator=agg)
                for agg in ("mean", "gcn", "pool") for layers in (2, 3)}
GAT_CONFIGS = {"gat_8_1": dict(num_layers=2, attn_head=[8, 1]),
               "gat_2_2_1": dict(num_layers=3, attn_head=[2, 2, 1])}


def main(ref_root):
    from gnnflow_amd import _build, dgl_compat
    sys.path[:0] = [os.path.dirname(_build.build_pybind()), ref_root]
    dgl_compat.install(force=True)
    from gnnflow.models.gat import GAT
    from gnnflow.models.graphsage import SAGE
    out = {}
    for cls, configs in ((SAGE, SAGE_CONFIGS), (GAT, GAT_CONFIGS)):
        for name, kw in configs.items():
            model = cls(DIM_IN, DIM_OUT, **kw)
            out[name] = {k: list(v.shape) for k, v in model.state_dict().items()}
    with open(os.path.join(HERE, "static_models_state_dict.json"), "w") as f:
        json.dump({"dim_in": DIM_IN, "dim_out": DIM_OUT, "configs": out}, f, indent=1,
                  sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main(sys.argv[1])
