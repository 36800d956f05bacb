"""The float64 reference and error bounds of tests/time_encode_ref.py, checked on the CPU before
any GPU run: the reference agrees with float64 autograd on the plain expression, an fp32
emulation of the kernels stays within every bound on the inputs that
tests/test_gpu_time_encode.py feeds them, and seeded mistakes break a bound.  Also what needs no
GPU of nn.GRUMemoryUpdater and of ops.time_encode_cat's argument checks."""
import numpy as np
import pytest

from tests import time_encode_ref as TE

SMALL = [c for c in TE.CASES if c[0] <= 257]


@pytest.mark.parametrize("case", SMALL, ids=TE.case_id)
def test_reference_agrees_with_float64_autograd(case):
    import torch
    c = TE.make_inputs(case)
    r = TE.reference(c)
    parts = [torch.from_numpy(p).double().requires_grad_(True) for p in c["parts"]]
    w = torch.from_numpy(c["w"]).double().reshape(-1, 1).requires_grad_(True)
    bias = torch.from_numpy(c["bias"]).double().requires_grad_(True)
    t = torch.from_numpy(c["t"]).double()
    out = torch.cat(parts + [torch.cos(t[:, None] @ w.T + bias)], 1)
    out.backward(torch.from_numpy(c["gout"]).double())

    def close(got, want):
        scale = max(1.0, float(np.abs(want).max(initial=0)))
        return np.abs(got - want).max(initial=0) <= 1e-12 * scale * max(len(c["t"]), 1)

    assert close(out.detach().numpy(), r.out)
    assert close(w.grad.numpy().ravel(), r.gw)
    assert close(bias.grad.numpy(), r.gbias)
    for p, gp in zip(parts, r.gparts):
        assert np.array_equal(p.grad.numpy(), gp)


@pytest.mark.parametrize("case", TE.CASES, ids=TE.case_id)
def test_fp32_emulation_stays_within_the_bounds(case):
    c = TE.make_inputs(case)
    r = TE.reference(c)
    out, gw, gbias = TE.emulate_fp32(c)
    assert r.copied_equal(out)
    ratios = r.ratios(out=out, gw=gw, gbias=gbias)
    print("\n[error / bound] {}: {}".format(
        TE.case_id(case), ", ".join("{} {:.3g}".format(k, v) for k, v in ratios.items())))
    assert max(ratios.values()) <= 1.0, ratios


@pytest.mark.parametrize("case", [c for c in SMALL if c[0] > 1], ids=TE.case_id)
def test_seeded_mistakes_break_a_bound(case):
    n, T, widths, kind = case
    c = TE.make_inputs(case)
    r = TE.reference(c)
    out, gw, gbias = TE.emulate_fp32(c)
    # a wrong sign of either gradient
    assert r.ratios(gbias=-gbias)["gbias"] > 1.0
    if kind != "zero":      # t = 0: gw is exactly 0 either way
        assert np.abs(r.gw).max() > 0 and r.ratios(gw=-gw)["gw"] > 1.0
    # the time encoding's sign
    flipped = out.copy()
    flipped[:, r.offset:] *= -1
    assert r.ratios(out=flipped)["enc"] > 1.0
    # a swapped column: among the time columns, and among the copied ones
    if T > 1:
        swapped = out.copy()
        swapped[:, [r.offset, r.offset + 1]] = swapped[:, [r.offset + 1, r.offset]]
        assert r.ratios(out=swapped)["enc"] > 1.0
        assert r.ratios(gw=np.roll(gw, 1), gbias=np.roll(gbias, 1))["gbias"] > 1.0
    if r.offset > 1:
        swapped = out.copy()
        swapped[:, [0, r.offset - 1]] = swapped[:, [r.offset - 1, 0]]
        assert not r.copied_equal(swapped)
    if r.offset:            # the parts in the wrong place: shifted by one column
        assert not r.copied_equal(np.roll(out, 1, axis=1))
    # a dropped row: the last row left out of the sums, and a row of the output shifted
    short = dict(c, parts=[p[:-1] for p in c["parts"]], t=c["t"][:-1], gout=c["gout"][:-1])
    _, gw1, gbias1 = TE.emulate_fp32(short)
    assert r.ratios(gbias=gbias1)["gbias"] > 1.0
    shifted = np.roll(out, 1, axis=0)
    if kind != "zero":      # t = 0: every row has the same time columns
        assert r.ratios(out=shifted)["enc"] > 1.0
    if r.offset:
        assert not r.copied_equal(shifted)


UPDATER_CONFIGS = [(0, 0, 100, 100, 100), (32, 16, 20, 24, 24), (24, 16, 20, 24, 24),
                   (32, 0, 0, 24, 24)]


@pytest.mark.parametrize("cfg", UPDATER_CONFIGS, ids=lambda c: "_".join(map(str, c)))
def test_gru_memory_updater_state_dict(cfg):
    from gnnflow_amd import nn as gnn
    dn, de, dt, demb, dm = cfg
    m = gnn.GRUMemoryUpdater(*cfg)
    want = {"updater.weight_ih": [3 * dm, 2 * dm + de + dt], "updater.weight_hh": [3 * dm, dm],
            "updater.bias_ih": [3 * dm], "updater.bias_hh": [3 * dm]}
    if dt > 0:
        want.update({"time_enc.w.weight": [dt, 1], "time_enc.w.bias": [dt]})
    if dn > 0 and dn != dm:
        want.update({"node_feat_proj.weight": [dm, dn], "node_feat_proj.bias": [dm]})
    assert {k: list(v.shape) for k, v in m.state_dict().items()} == want
    assert isinstance(m.fused_time_encode, bool)
    assert "fused_time_encode" not in m.state_dict()
    if dt > 0:
        assert np.array_equal(m.time_enc.w.weight.detach().numpy().ravel(),
                              TE.tgat_frequencies(dt))


def test_package_exports_both_spellings():
    import gnnflow_amd
    from gnnflow_amd import nn as gnn
    assert gnnflow_amd.GRUMemoryUpdater is gnn.GRUMemoryUpdater
    assert gnnflow_amd.GRUMemeoryUpdater is gnn.GRUMemoryUpdater
    assert gnn.GRUMemeoryUpdater is gnn.GRUMemoryUpdater
    assert {"GRUMemoryUpdater", "GRUMemeoryUpdater"} <= set(gnnflow_amd.__all__)


def test_layers_carry_the_switch_outside_their_state():
    from gnnflow_amd import nn as gnn
    layer = gnn.TemporalAttentionLayer(32, 16, 20, 24, 2, 0.1, 0.1)
    assert layer.fused_time_encode is gnn.FUSED_TIME_ENCODE_DEFAULT
    assert layer.fused_time_encode == gnn.GRUMemoryUpdater(32, 16, 20, 24, 24).fused_time_encode
    assert "fused_time_encode" not in layer.state_dict()


def test_argument_errors_raise_before_any_native_call(monkeypatch):
    import torch
    from gnnflow_amd import _capi, ops

    def no_native(*a, **k):
        raise AssertionError("native library touched")
    monkeypatch.setattr(_capi, "load", no_native)
    n, T = 5, 4
    t, w, b = torch.zeros(n), torch.ones(T, 1), torch.zeros(T)
    part = torch.zeros(n, 3)
    with pytest.raises(ValueError, match="at most two parts"):
        ops.time_encode_cat((part, part, part), t, w, b)
    for bad in ((part.double(), t, w, b), (part, t.double(), w, b), (part, t, w.double(), b),
                (part, t, w, b.double()), (part.long(), t, w, b)):
        with pytest.raises(TypeError, match="float32"):
            ops.time_encode_cat((bad[0],), *bad[1:])
    with pytest.raises(ValueError, match="rows"):
        ops.time_encode_cat((torch.zeros(n + 1, 3),), t, w, b)
    with pytest.raises(ValueError, match="rows"):
        ops.time_encode_cat((part, torch.zeros(n - 1, 2)), t, w, b)
    with pytest.raises(ValueError, match="T >= 1"):
        ops.time_encode_cat((part,), t, torch.ones(0, 1), torch.zeros(0))
    with pytest.raises(ValueError, match="T >= 1"):
        ops.time_encode(t, torch.ones(0), torch.zeros(0))
    with pytest.raises(ValueError, match="weight must be"):
        ops.time_encode_cat((part,), t, torch.ones(T + 1, 1), b)
    with pytest.raises(ValueError, match="weight must be"):
        ops.time_encode_cat((part,), t, torch.ones(1, T), b)
    with pytest.raises(ValueError, match=r"t must be \[n\]"):
        ops.time_encode_cat((part,), torch.zeros(n, 2), w, b)
    with pytest.raises(ValueError, match=r"parts\[0\] must be \[n, W\]"):
        ops.time_encode_cat((torch.zeros(n),), t, w, b)
    with pytest.raises(ValueError, match="bias must be"):
        ops.time_encode_cat((part,), t, w, torch.zeros(T, 1))
    with pytest.raises(ValueError, match="runs on the GPU"):      # well-formed, but on the CPU
        ops.time_encode_cat((part,), t, w, b)
    with pytest.raises(ValueError, match="runs on the GPU"):
        ops.time_encode(t.reshape(n, 1), w.reshape(T), b)
