"""models.SAGE and models.GAT without a GPU: state-dict names and shapes against the reference's
own (tests/golden/static_models_state_dict.json), the constructor errors, and the reference's
import lines with the package name swapped."""
import json
import os

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def fixture():
    with open(os.path.join(GOLDEN, "static_models_state_dict.json")) as f:
        return json.load(f)


def test_both_import_paths():
    from gnnflow_amd import models
    from gnnflow_amd.models.gat import GAT
    from gnnflow_amd.models.graphsage import SAGE
    assert models.SAGE is SAGE and models.GAT is GAT
    assert {"DGNN", "SAGE", "GAT"} <= set(models.__all__)


def test_state_dicts_match_the_reference():
    from gnnflow_amd.models import GAT, SAGE
    from tests.golden.make_static_models_fixture import GAT_CONFIGS, SAGE_CONFIGS
    fix = fixture()
    assert set(fix["configs"]) == set(SAGE_CONFIGS) | set(GAT_CONFIGS)
    for cls, configs in ((SAGE, SAGE_CONFIGS), (GAT, GAT_CONFIGS)):
        for name, kw in configs.items():
            model = cls(fix["dim_in"], fix["dim_out"], **kw)
            got = {k: list(v.shape) for k, v in model.state_dict().items()}
            assert got == fix["configs"][name], name
            assert list(model.layers) == ["l{}h0".format(l) for l in range(kw["num_layers"])]
            assert model.dim_out == fix["dim_out"] and model.num_layers == kw["num_layers"]
            assert model.reset() is None


def test_defaults_are_the_references():
    import torch.nn as nn
    from gnnflow_amd.models import GAT, SAGE
    sage, gat = SAGE(20, 12), GAT(20, 12)
    assert sage.num_layers == gat.num_layers == 2
    assert sage.layers["l0h0"]._aggre_type == "mean"
    assert [gat.layers[k]._num_heads for k in gat.layers] == [8, 1]
    assert gat.layers["l0h0"].activation is not None and gat.layers["l1h0"].activation is None
    assert all(layer._allow_zero_in_degree for layer in gat.layers.values())
    assert not any(layer.fused_attention for layer in gat.layers.values())
    for model in (sage, gat):
        kinds = [type(m) for m in model.predictor]
        assert kinds == [nn.Linear, nn.ReLU, nn.Linear, nn.ReLU, nn.Linear]
        assert model.predictor[-1].out_features == 1


def test_constructor_errors():
    from gnnflow_amd.models import GAT, SAGE
    with pytest.raises(ValueError, match="aggregator sum is not in"):
        SAGE(20, 12, aggregator="sum")
    with pytest.raises(NotImplementedError, match="lstm"):
        SAGE(20, 12, aggregator="lstm")
    for layers, heads in ((2, [8]), (3, [8, 1]), (1, [2, 2])):
        with pytest.raises(ValueError, match="must equal to num_layers"):
            GAT(20, 12, num_layers=layers, attn_head=heads)
