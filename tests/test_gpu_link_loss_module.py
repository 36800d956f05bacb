"""nn.LinkLoss on the GPU: its epoch sums against tests/link_loss_ref.py, the accumulator as a
non-persistent buffer, two training steps of a small models.DGNN against the torch criterion,
and the example's --fused-loss loop."""
import importlib.util
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import link_loss_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_compute_reset_and_state_dict():
    import gnnflow_amd
    from gnnflow_amd import metrics, nn
    assert gnnflow_amd.LinkLoss is nn.LinkLoss and metrics.LinkLoss is nn.LinkLoss
    crit = nn.LinkLoss().cuda()
    assert crit.state is None and math.isnan(crit.compute()["mean_loss"])
    mine, theirs = R.Accumulator(), R.Accumulator()
    for k, (P, N) in enumerate(((600, 600), (600, 5400), (37, 111), (1, 9))):
        pos, neg = R.make_logits(P, N, seed=60 + k)
        x = torch.from_numpy(pos).cuda().reshape(P, 1).requires_grad_()
        loss = crit(x, torch.from_numpy(neg).cuda().reshape(N, 1))
        assert loss.shape == () and loss.dtype == torch.float32
        loss.backward()
        mine.add(pos, neg, loss=float(loss.detach()))
        theirs.add(pos, neg)
    out, want = crit.compute(), theirs.compute()
    assert out == mine.compute()      # the same float64 adds of the same float32 losses
    assert out["batches"] == 4 and out["nonfinite"] == 0
    for key in ("mean_loss", "edge_weighted_loss"):
        assert abs(out[key] - want[key]) <= R.LOSS_RTOL * want[key]
    assert out["mean_loss"] != out["edge_weighted_loss"]
    # the accumulator: a buffer, moved with the module, not saved with it
    assert crit.state.dtype == torch.float64 and crit.state.shape == (5,) and crit.state.is_cuda
    assert "state" in dict(crit.named_buffers()) and crit.state_dict() == {}
    crit.load_state_dict({})
    # a NaN batch is counted and nothing else moves
    kept = crit.state.clone()
    assert torch.isnan(crit(torch.full((3, 1), float("nan"), device="cuda"),
                            torch.zeros(2, 1, device="cuda")))
    assert crit.compute()["nonfinite"] == 1 and torch.equal(crit.state[:3], kept[:3])
    crit.reset()
    assert not crit.state.any() and crit.compute()["batches"] == 0
    # what is not float32 / bfloat16 takes the torch expression and is not counted
    x64 = torch.randn(5, 1, device="cuda", dtype=torch.float64)
    y64 = torch.randn(7, 1, device="cuda", dtype=torch.float64)
    want64 = F.binary_cross_entropy_with_logits(x64, torch.ones_like(x64)) + \
        F.binary_cross_entropy_with_logits(y64, torch.zeros_like(y64))
    assert torch.equal(crit(x64, y64), want64) and crit.compute()["batches"] == 0


def test_dgnn_trains_two_steps_as_with_the_torch_criterion():
    """The same two SGD steps from the same seed, once with nn.LinkLoss and once with the torch
    expression: the losses agree at assert_close's float32 defaults.  SGD, so that the last-bit
    differences of the first step's gradients move the parameters by lr times as little."""
    from gnnflow_amd import nn
    from tests.test_gpu_models import _World, _model, _prepare
    world = _World()
    losses = {}
    for fused in (False, True):
        model, kw = _model("tgat", dropout=0.0, att_dropout=0.0)
        model.train()
        opt = torch.optim.SGD(model.parameters(), lr=0.05)
        crit = nn.LinkLoss()
        got = []
        for step in range(2):
            mfgs = world.mfgs(kw, 1 + step)
            _prepare(model, mfgs)
            opt.zero_grad()
            pos, neg = model(mfgs)
            if fused:
                loss = crit(pos, neg)
            else:
                loss = F.binary_cross_entropy_with_logits(pos, torch.ones_like(pos)) + \
                    F.binary_cross_entropy_with_logits(neg, torch.zeros_like(neg))
            loss.backward()
            assert all(torch.isfinite(p.grad).all() for p in model.parameters()
                       if p.grad is not None)
            opt.step()
            got.append(loss.detach())
        losses[fused] = torch.stack(got)
        if fused:
            out = crit.compute()
            assert out["batches"] == 2 and out["nonfinite"] == 0
            assert out["mean_loss"] == (float(got[0]) + float(got[1])) / 2
    print("\n[link_loss] DGNN losses: torch {}, fused {}".format(
        losses[False].tolist(), losses[True].tolist()))
    assert losses[True][0] != losses[True][1]      # the step moved the model
    torch.testing.assert_close(losses[True], losses[False])


def test_example_runs_with_the_fused_loss():
    spec = importlib.util.spec_from_file_location(
        "train_edge_prediction", os.path.join(ROOT, "examples", "train_edge_prediction.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    losses = mod.main(num_batches=3, verbose=False, fused_loss=True)
    assert isinstance(losses, list) and len(losses) == 3
    assert all(isinstance(l, float) and np.isfinite(l) for l in losses)
