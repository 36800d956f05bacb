"""nn.EdgePredictor, nn.MLP and models.DGNN without a GPU: the reference's recorded EdgePredictor
run reproduced on the CPU, state-dict names and shapes of the memory-free DGNN configurations
against the reference's own, the import lines of the reference with the package name swapped,
and the memory calls as no-ops without memory."""
import json
import os

import numpy as np
import pytest

from tests import edge_score_ref as ES

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def predictor_fixture():
    with np.load(os.path.join(GOLDEN, "edge_predictor_reference.npz")) as z:
        return {k: z[k] for k in z.files}


def dgnn_fixture():
    with open(os.path.join(GOLDEN, "dgnn_state_dict.json")) as f:
        return json.load(f)


def dgnn_kwargs(fix, name):
    """The constructor arguments tests/golden/make_dgnn_fixture.py used for `name`."""
    from tests.golden.make_dgnn_fixture import CONFIGS, kwargs
    assert set(CONFIGS) == set(fix["configs"])
    kw = kwargs(name)
    assert (kw["dim_edge"], kw["dim_time"], kw["dim_embed"], kw["att_head"]) == \
        (fix["dim_edge"], fix["dim_time"], fix["dim_embed"], fix["att_head"])
    return kw


def load_predictor(fix):
    import torch
    from gnnflow_amd import nn as gnn
    model = gnn.EdgePredictor(fix["h"].shape[1])
    state = {k[len("state."):]: torch.from_numpy(v) for k, v in fix.items()
             if k.startswith("state.")}
    model.load_state_dict(state, strict=True)
    return model


def test_edge_predictor_reproduces_the_reference_on_the_cpu(monkeypatch):
    import torch
    from gnnflow_amd import nn as gnn
    from gnnflow_amd import ops
    fix = predictor_fixture()
    assert fix["h"].shape == (21, 12)

    def never(*a, **k):
        raise AssertionError("ops.edge_score called for CPU tensors")
    monkeypatch.setattr(ops, "edge_score", never)
    for fused in (False, True):
        model = load_predictor(fix)
        assert model.fused_score is gnn.FUSED_EDGE_SCORE_DEFAULT
        assert "fused_score" not in model.state_dict()
        model.fused_score = fused
        h = torch.from_numpy(fix["h"]).requires_grad_(True)
        pos, neg = model(h)
        (pos.sum() - 2 * neg.sum()).backward()
        torch.testing.assert_close(pos.detach(), torch.from_numpy(fix["pos"]))
        torch.testing.assert_close(neg.detach(), torch.from_numpy(fix["neg"]))
        torch.testing.assert_close(h.grad, torch.from_numpy(fix["grad.h"]))
        for k, v in model.named_parameters():
            torch.testing.assert_close(v.grad, torch.from_numpy(fix["grad." + k]))


def test_recorded_run_obeys_the_propagated_bounds():
    """The fixture itself against the float64 reference of the whole module: the recorded fp32
    run is inside the bounds the GPU test relies on, and no pre-activation is close enough to
    zero for an fp32 evaluation to take another side of the relu."""
    fix = predictor_fixture()
    state = {k[len("state."):]: v for k, v in fix.items() if k.startswith("state.")}
    G = np.r_[np.ones(7), -2 * np.ones(7)]
    ref = ES.PredictorReference(state, fix["h"], G)
    assert ref.mask_is_stable
    grads = {k[len("grad."):]: v for k, v in fix.items() if k.startswith("grad.")}
    ratios = ref.ratios(fix["pos"], fix["neg"], grads)
    print("\n[error/bound] recorded run: {:.3g}".format(max(ratios.values())))
    assert max(ratios.values()) <= 1.0, ratios


def test_edge_predictor_rejects_rows_not_a_multiple_of_three():
    import torch
    from gnnflow_amd import nn as gnn
    model = gnn.EdgePredictor(4)
    for fused in (False, True):
        model.fused_score = fused
        with pytest.raises(ValueError, match="multiple of 3"):
            model(torch.zeros(7, 4))
    pos, neg = model(torch.zeros(0, 4))
    assert pos.shape == neg.shape == (0, 1)


def test_mlp_is_the_reference_head():
    import torch
    import torch.nn.functional as F
    from gnnflow_amd import nn as gnn
    torch.manual_seed(3)
    mlp = gnn.MLP(6, 5, 3)
    assert {k: tuple(v.shape) for k, v in mlp.state_dict().items()} == {
        "fc1.weight": (5, 6), "fc1.bias": (5,), "fc2.weight": (3, 5), "fc2.bias": (3,)}
    x = torch.randn(4, 6)
    assert torch.equal(mlp(x), mlp.fc2(F.relu(mlp.fc1(x))))


def test_reference_import_lines_with_the_package_name_swapped():
    import gnnflow_amd
    from gnnflow_amd import memory
    from gnnflow_amd import nn as gnn
    from gnnflow_amd.models import DGNN
    from gnnflow_amd.models.dgnn import DGNN as DGNN2
    from gnnflow_amd.models.modules.layers import (MLP, EdgePredictor, TimeEncode,
                                                    TransfomerAttentionLayer)
    from gnnflow_amd.models.modules.memory import Memory
    from gnnflow_amd.models.modules.memory_updater import GRUMemeoryUpdater
    assert DGNN is DGNN2
    assert EdgePredictor is gnn.EdgePredictor is gnnflow_amd.EdgePredictor
    assert MLP is gnn.MLP is gnnflow_amd.MLP
    assert TimeEncode is gnn.TimeEncode and TransfomerAttentionLayer is gnn.TemporalAttentionLayer
    assert Memory is memory.Memory and GRUMemeoryUpdater is gnn.GRUMemoryUpdater


@pytest.mark.parametrize("name", ["tgat", "dysat"])
def test_dgnn_state_dict_matches_the_reference_fixture(name):
    import torch
    from gnnflow_amd import nn as gnn
    from gnnflow_amd.models import DGNN
    fix = dgnn_fixture()
    kw = dgnn_kwargs(fix, name)
    assert not kw["use_memory"]
    model = DGNN(**kw)
    got = {k: list(v.shape) for k, v in model.state_dict().items()}
    assert got == fix["configs"][name]
    assert ("combiner.weight_ih_l0" in got) == (kw["num_snapshots"] > 1)
    assert sorted(model.layers) == sorted("l{}h{}".format(l, h) for l in range(kw["num_layers"])
                                          for h in range(kw["num_snapshots"]))
    assert all(isinstance(m, gnn.TemporalAttentionLayer) for m in model.layers.values())
    assert isinstance(model.edge_predictor, gnn.EdgePredictor)
    assert model.last_updated is None and not model.has_memory()
    assert (model.dim_node, model.dim_node_input, model.dim_edge, model.dim_time,
            model.dim_embed, model.num_layers, model.num_snapshots, model.att_head) == \
        (kw["dim_node"],) * 2 + (kw["dim_edge"], kw["dim_time"], kw["dim_embed"],
                                 kw["num_layers"], kw["num_snapshots"], kw["att_head"])
    if name == "dysat":
        assert isinstance(model.combiner, torch.nn.RNN)
    # without memory every memory call is a no-op
    assert model.reset() is None and model.resize(10 ** 6) is None
    assert model.backup_memory() == {} and model.restore_memory({}) is None
    assert not hasattr(model, "memory") and not hasattr(model, "memory_updater")


def test_dgnn_accepts_the_reference_signature():
    from gnnflow_amd.models import DGNN
    # positional up to kvstore_client, then *args and **kwargs that the reference swallows
    model = DGNN(8, 4, 6, 8, 1, 1, 2, 0.1, 0.1, False, None, None, 'cuda', False, None, "extra",
                 unknown_option=1)
    assert not model.has_memory()
    with pytest.raises(AssertionError, match="multiple snapshots"):
        DGNN(8, 4, 6, 8, 1, 2, 2, 0.1, 0.1, True, dim_memory=8, num_nodes=10)
    with pytest.raises(AssertionError, match="dim_memory"):
        DGNN(8, 4, 6, 8, 1, 1, 2, 0.1, 0.1, True, num_nodes=10)
    with pytest.raises(AssertionError, match="num_nodes"):
        DGNN(8, 4, 6, 8, 1, 1, 2, 0.1, 0.1, True, dim_memory=8)
