"""CPU checks of tests/link_metrics_ref.py, the restatement ops.link_metrics is tested against:
scikit-learn's recorded average_precision_score / roc_auc_score
(tests/golden/link_metrics_reference.npz), the closed forms with all scores equal, the MRR on
hand-made ranks, and that the Python constants are those of include/gnnflow_hip.h."""
import math
import os
import re

import numpy as np
import pytest

from tests import link_metrics_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "link_metrics_reference.npz")


def golden_cases():
    """[(id, pos, neg, ap, auc)] of the recorded scikit-learn run."""
    z = np.load(GOLDEN)
    names = sorted({k.split(".")[0] for k in z.files if k.startswith("c")})
    out = []
    for c in names:
        s, y = z[c + ".scores"], z[c + ".labels"]
        pos, neg = s[y == 1], s[y == 0]
        out.append(("{}-{}-{}x{}".format(c, str(z[c + ".kind"]), len(pos), len(neg)), pos, neg,
                    float(z[c + ".ap"]), float(z[c + ".auc"])))
    return out


def test_golden_file_covers_the_families():
    cases = golden_cases()
    assert len(cases) >= 36
    kinds = {c[0].split("-")[1] for c in cases}
    assert kinds >= {"normal", "four", "equal", "zeros", "denormal", "heavy_ties"}
    assert any(len(c[1]) == 1 for c in cases) and any(len(c[2]) == 1 for c in cases)
    # +-0 really are mixed, and denormals really are denormal
    z = [np.concatenate([c[1], c[2]]) for c in cases if "-zeros-" in c[0]]
    assert any((np.signbit(s) & (s == 0)).any() and (~np.signbit(s) & (s == 0)).any() for s in z)
    d = [np.concatenate([c[1], c[2]]) for c in cases if "-denormal-" in c[0]]
    assert all((np.abs(s[s != 0]) < np.finfo(np.float32).tiny).all() for s in d)


@pytest.mark.parametrize("case", golden_cases(), ids=lambda c: c[0])
def test_restatement_matches_scikit_learn(case):
    name, pos, neg, ap, auc = case
    r = R.reference(pos, neg)
    bound = R.sklearn_bound(len(pos), len(neg))
    print("\n{}: |ap - sklearn| = {:.3g}, |auc - sklearn| = {:.3g}, bound {:.3g}".format(
        name, abs(r["ap"] - ap), abs(r["auc"] - auc), bound))
    assert abs(r["ap"] - ap) <= bound
    assert abs(r["auc"] - auc) <= bound


@pytest.mark.parametrize("P,r", [(1, 1), (1, 4), (7, 1), (7, 3), (64, 2), (100, 9)])
def test_closed_forms_with_all_scores_equal(P, r):
    N = r * P
    pos, neg = R.make_scores("equal", P, N, seed=0)
    got = R.reference(pos, neg)
    assert abs(got["ap"] - P / (P + N)) <= R.kernel_bound(P)
    assert got["auc"] == 0.5
    assert abs(got["mrr"] - 1 / (1 + r / 2)) <= R.kernel_bound(P)


def test_mrr_uses_each_positive_s_own_negatives():
    # P = 2, r = 3: negatives of positive 0 are neg[0], neg[2], neg[4]
    pos = np.array([1.0, 5.0], dtype=np.float32)
    neg = np.array([2.0, 9.0, 1.0, 5.0, 0.0, 5.0], dtype=np.float32)
    # positive 0: one greater, one equal -> rank 2.5; positive 1: one greater, two equal -> rank 3
    got = R.reference(pos, neg)
    assert got["mrr"] == (1 / 2.5 + 1 / 3) / 2
    assert math.isnan(R.reference(pos, neg[:5])["mrr"])
    assert not math.isnan(R.reference(pos, neg[:5])["ap"])


def test_signed_zeros_tie_and_non_finite_scores_give_nan():
    pos = np.array([0.0, -0.0], dtype=np.float32)
    neg = np.array([-0.0, 0.0], dtype=np.float32)
    got = R.reference(pos, neg)
    assert got == {"ap": 0.5, "auc": 0.5, "mrr": 1 / 1.5}
    for bad in (np.nan, np.inf, -np.inf):
        p = pos.copy()
        p[1] = bad
        assert all(math.isnan(v) for v in R.reference(p, neg).values())
        assert all(math.isnan(v) for v in R.reference(neg, p).values())


def test_accumulator_counts_batches_mrr_batches_and_non_finite():
    acc = R.Accumulator()
    a = acc.add(*R.make_scores("normal", 5, 10, 1))
    b = acc.add(*R.make_scores("normal", 5, 11, 2))
    pos, neg = R.make_scores("normal", 5, 5, 3)
    pos[0] = np.nan
    before = acc.state.copy()
    acc.add(pos, neg)
    assert acc.state[5] == 1 and np.array_equal(acc.state[:5], before[:5])
    assert acc.state[3] == 2 and acc.state[4] == 1 and acc.state[2] == a["mrr"]
    assert acc.state[0] == a["ap"] + b["ap"] and acc.state[1] == a["auc"] + b["auc"]
    assert acc.bound_ap == 2 * R.kernel_bound(5) and acc.bound_mrr == R.kernel_bound(5)


def test_python_constants_are_the_header_s():
    text = open(os.path.join(ROOT, "include", "gnnflow_hip.h")).read()
    macro = {k: int(v) for k, v in re.findall(r"#define (GF_LINK_METRICS_[A-Z_]+) (\d+)", text)}
    from gnnflow_amd import ops
    const = {k: getattr(ops, k) for k in ("LINK_METRICS_MAX_SCORES", "LINK_METRICS_TILE",
                                          "_LINK_METRICS_PARTIAL_WORDS")}
    assert macro == {"GF_LINK_METRICS_MAX_SCORES": 65536, "GF_LINK_METRICS_TILE": const["LINK_METRICS_TILE"],
                     "GF_LINK_METRICS_PARTIAL_WORDS": const["_LINK_METRICS_PARTIAL_WORDS"]}
    assert const["LINK_METRICS_MAX_SCORES"] == 65536
    assert const["LINK_METRICS_TILE"] >= 256 and const["LINK_METRICS_TILE"] % 256 == 0
