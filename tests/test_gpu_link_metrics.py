"""ops.link_metrics and metrics.LinkMetrics on the GPU against tests/link_metrics_ref.py.

AUC equals the restatement bit for bit; AP and MRR sit within (P + 2) * 2**-53 of it (the
derivations are in link_metrics_ref.py).  The shapes cover the workgroup edge (255, 256, 257
positives), the LDS tile edge (P + N = TILE, TILE + 1, 2 * TILE + 6), r = 1 .. 3 and a ragged
N, where MRR is NaN."""
import importlib.util
import math
import os
import re

import numpy as np
import pytest

from tests import link_metrics_ref as R
from tests.test_link_metrics_ref import golden_cases

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = 2048


def _shapes():
    return [(1, 1), (1, 3), (255, 255), (256, 512), (257, 514), (300, 301), (3, TILE - 3),
            (3, TILE - 2), (5, 2 * TILE + 1)]


def _run(pos, neg, acc=None):
    import torch
    from gnnflow_amd import ops
    out = ops.link_metrics(torch.from_numpy(pos).cuda(), torch.from_numpy(neg).cuda(), acc)
    assert out.dtype == torch.float64 and tuple(out.shape) == (3,) and out.is_cuda
    return out.cpu().numpy()


def _bits(x):
    return np.asarray(x, dtype=np.float64).view(np.int64)


def _check(got, want, P, name=""):
    """got: float64 [3] from the kernel; want: the restatement's dict."""
    bound = R.kernel_bound(P)
    err_ap = abs(got[0] - want["ap"])
    print("\n{} AP {!r} (off by {:.3g}), AUC {!r}, MRR {!r}; bound {:.3g}".format(
        name, got[0], err_ap, got[1], got[2], bound))
    assert err_ap <= bound
    assert _bits(got[1]) == _bits(want["auc"])
    if math.isnan(want["mrr"]):
        assert math.isnan(got[2])
    else:
        print("MRR off by {:.3g}".format(abs(got[2] - want["mrr"])))
        assert abs(got[2] - want["mrr"]) <= bound


def test_tile_constant_is_the_library_s():
    from gnnflow_amd import ops
    assert ops.LINK_METRICS_TILE == TILE and ops.LINK_METRICS_MAX_SCORES == 65536


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("shape", _shapes(), ids=lambda s: "{}x{}".format(*s))
def test_matches_the_restatement(shape, kind):
    P, N = shape
    pos, neg = R.make_scores(kind, P, N, seed=7 * P + N)
    want = R.reference(pos, neg)
    assert math.isnan(want["mrr"]) == (N % P != 0)
    _check(_run(pos, neg), want, P, "{} {}x{}".format(kind, P, N))


@pytest.mark.parametrize("P,r", [(1, 1), (255, 1), (257, 2), (64, 9)])
def test_closed_forms_with_all_scores_equal(P, r):
    N = r * P
    pos, neg = R.make_scores("equal", P, N, seed=0)
    got = _run(pos, neg)
    assert abs(got[0] - P / (P + N)) <= R.kernel_bound(P)
    assert got[1] == 0.5
    assert abs(got[2] - 1 / (1 + r / 2)) <= R.kernel_bound(P)


@pytest.mark.parametrize("case", golden_cases(), ids=lambda c: c[0])
def test_matches_recorded_scikit_learn(case):
    name, pos, neg, ap, auc = case
    got = _run(np.ascontiguousarray(pos), np.ascontiguousarray(neg))
    bound = R.sklearn_bound(len(pos), len(neg))
    print("\n{}: |ap - sklearn| = {:.3g}, |auc - sklearn| = {:.3g}, bound {:.3g}".format(
        name, abs(got[0] - ap), abs(got[1] - auc), bound))
    assert abs(got[0] - ap) <= bound and abs(got[1] - auc) <= bound


@pytest.mark.parametrize("side,value", [("pos", np.nan), ("neg", np.inf), ("pos", -np.inf)])
@pytest.mark.parametrize("shape", [(5, 10), (300, 2 * TILE)], ids=["5x10", "300x4096"])
def test_non_finite_scores_give_nan_and_touch_only_their_counter(shape, side, value):
    import torch
    P, N = shape
    pos, neg = R.make_scores("normal", P, N, seed=3)
    acc = torch.zeros(8, dtype=torch.float64, device="cuda")
    _run(pos, neg, acc)                      # a finite batch first: the fields are not zero
    before = acc.cpu().numpy().copy()
    assert before[3] == 1 and before[0] > 0
    bad = {"pos": pos, "neg": neg}[side]
    bad[len(bad) - 1] = value                # the last element: the last tile, the last lane
    got = _run(pos, neg, acc)
    assert np.isnan(got).all()
    after = acc.cpu().numpy()
    assert after[5] == before[5] + 1 == 1
    keep = [0, 1, 2, 3, 4, 6, 7]
    assert np.array_equal(_bits(after[keep]), _bits(before[keep]))
    # without an accumulator the outputs are NaN all the same
    assert np.isnan(_run(pos, neg)).all()


def test_five_batches_through_one_accumulator():
    import torch
    acc = torch.zeros(8, dtype=torch.float64, device="cuda")
    ref = R.Accumulator()
    batches = [("normal", 7, 14), ("four", 64, 64), ("normal", 300, 301), ("zeros", 257, 514),
               ("normal", 5, 2 * TILE + 1)]
    outs = []
    for i, (kind, P, N) in enumerate(batches):
        pos, neg = R.make_scores(kind, P, N, seed=50 + i)
        ref.add(pos, neg)
        outs.append(_run(pos, neg, acc))
    got = acc.cpu().numpy()
    print("\nsums {!r}\nwant {!r}\nbounds ap {:.3g} mrr {:.3g}".format(got, ref.state, ref.bound_ap,
                                                                      ref.bound_mrr))
    assert got[3] == 5 and got[4] == 3 and got[5] == 0 and got[6] == 0 and got[7] == 0
    assert abs(got[0] - ref.state[0]) <= ref.bound_ap
    assert _bits(got[1]) == _bits(ref.state[1])      # every AUC is exact, and so is their order
    assert abs(got[2] - ref.state[2]) <= ref.bound_mrr
    # the accumulator holds the sums of what the calls returned
    assert got[0] == sum(o[0] for o in outs) and got[2] == outs[0][2] + outs[1][2] + outs[3][2]


def test_two_runs_give_identical_bits():
    import torch
    for kind, P, N in (("normal", 300, 900), ("four", 257, 2 * TILE + 1)):
        pos, neg = R.make_scores(kind, P, N, seed=9)
        a, b = _run(pos, neg), _run(pos, neg)
        assert np.array_equal(_bits(a), _bits(b))
        accs = []
        for _ in range(2):
            acc = torch.zeros(8, dtype=torch.float64, device="cuda")
            _run(pos, neg, acc)
            _run(neg[:P], pos, acc)
            accs.append(acc.cpu().numpy())
        assert np.array_equal(_bits(accs[0]), _bits(accs[1]))


def test_column_inputs_grad_inputs_strided_input_and_a_side_stream():
    import torch
    from gnnflow_amd import ops
    P, N = 130, 390
    pos_np, neg_np = R.make_scores("normal", P, N, seed=21)
    want = _run(pos_np, neg_np)
    pos, neg = torch.from_numpy(pos_np).cuda(), torch.from_numpy(neg_np).cuda()
    # [P, 1] and [N, 1], as EdgePredictor returns them
    col = ops.link_metrics(pos.reshape(P, 1), neg.reshape(N, 1))
    assert np.array_equal(_bits(col.cpu().numpy()), _bits(want))
    # inputs that require grad: detached, nothing recorded
    pg, ng = pos.clone().requires_grad_(True), neg.clone().requires_grad_(True)
    out = ops.link_metrics(pg * 1.0, ng.reshape(N, 1))
    assert not out.requires_grad and out.grad_fn is None
    assert np.array_equal(_bits(out.cpu().numpy()), _bits(want))
    # a strided neg: every other element of a buffer twice as long, the rest poisoned with NaN
    wide = torch.full((2 * N,), float("nan"), device="cuda")
    wide[::2] = neg
    assert not wide[::2].is_contiguous()
    got = ops.link_metrics(pos, wide[::2])
    assert np.array_equal(_bits(got.cpu().numpy()), _bits(want))
    # a side stream
    side = torch.cuda.Stream()
    acc = torch.zeros(8, dtype=torch.float64, device="cuda")
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        s_out = ops.link_metrics(pos, neg, acc)
    side.synchronize()
    assert np.array_equal(_bits(s_out.cpu().numpy()), _bits(want))
    assert acc.cpu().numpy()[3] == 1


def test_link_metrics_class_update_compute_reset():
    import torch
    import gnnflow_amd
    from gnnflow_amd import metrics
    assert gnnflow_amd.LinkMetrics is metrics.LinkMetrics
    m = gnnflow_amd.LinkMetrics("cuda")
    batches = [("normal", 40, 40), ("normal", 33, 99), ("four", 20, 30)]
    ref = R.Accumulator()
    sig = []
    for i, (kind, P, N) in enumerate(batches):
        pos, neg = R.make_scores(kind, P, N, seed=70 + i)
        pos, neg = (pos * 6).astype(np.float32), (neg * 6).astype(np.float32)      # logits
        tp, tn = torch.from_numpy(pos).cuda().reshape(P, 1), torch.from_numpy(neg).cuda().reshape(N, 1)
        m.update(tp, tn)
        sp, sn = torch.sigmoid(tp), torch.sigmoid(tn)
        sig.append((sp, sn))
        ref.add(sp.cpu().numpy(), sn.cpu().numpy())
    got = m.compute()
    assert set(got) == {"ap", "auc", "mrr", "batches", "mrr_batches", "nonfinite"}
    assert (got["batches"], got["mrr_batches"], got["nonfinite"]) == (3, 2, 0)
    assert abs(got["ap"] - ref.state[0] / 3) <= ref.bound_ap / 3 + R.U      # + the division
    assert got["auc"] == ref.state[1] / 3
    assert abs(got["mrr"] - ref.state[2] / 2) <= ref.bound_mrr / 2 + R.U
    # sigmoid=True is sigmoid=False on torch.sigmoid of the scores
    m2 = gnnflow_amd.LinkMetrics(torch.device("cuda", 0))
    for sp, sn in sig:
        m2.update(sp, sn, sigmoid=False)
    assert np.array_equal(_bits(m2.state.cpu().numpy()), _bits(m.state.cpu().numpy()))
    assert m2.compute() == got
    m.reset()
    assert m.state.cpu().tolist() == [0.0] * 8
    empty = m.compute()
    assert (empty["batches"], empty["mrr_batches"], empty["nonfinite"]) == (0, 0, 0)
    assert all(math.isnan(empty[k]) for k in ("ap", "auc", "mrr"))


def test_evaluation_example_runs_and_prints_ap_and_auc(capsys):
    spec = importlib.util.spec_from_file_location(
        "evaluate_edge_prediction", os.path.join(ROOT, "examples", "evaluate_edge_prediction.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    result = mod.main(num_batches=4)
    line = [l for l in capsys.readouterr().out.splitlines() if l.startswith("ap ")][-1]
    ap, auc = (float(x) for x in re.match(r"ap (\S+) auc (\S+) ", line).groups())
    assert math.isfinite(ap) and math.isfinite(auc) and 0 <= ap <= 1 and 0 <= auc <= 1
    assert result["batches"] == 4 and result["mrr_batches"] == 4 and result["nonfinite"] == 0
    assert abs(result["ap"] - ap) < 1e-4 and abs(result["auc"] - auc) < 1e-4
