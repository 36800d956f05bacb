"""Writes tests/golden/link_metrics_reference.npz: what scikit-learn's average_precision_score
and roc_auc_score give for small score vectors, the two calls the reference's evaluate() makes
per batch (scripts/offline_edge_prediction.py:141-146).  Per case cNN:

    cNN.scores   float32 [P + N], the positives first
    cNN.labels   int8 [P + N], 1 for a positive
    cNN.ap       float64, average_precision_score(labels, scores)
    cNN.auc      float64, roc_auc_score(labels, scores)
    cNN.kind     the family of the scores (tests/link_metrics_ref.py make_scores, plus 'heavy_ties')

and `sklearn`, the version that computed them.  Needs scikit-learn; the tests do not.

    python tests/golden/make_link_metrics_fixture.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

# (kind, P, N): random, four-valued, all equal, +-0 mixed, denormal, P = 1, N = 1, N = r P
CASES = [
    ("normal", 1, 1), ("normal", 1, 7), ("normal", 9, 1), ("normal", 2, 2), ("normal", 5, 5),
    ("normal", 13, 39), ("normal", 31, 17), ("normal", 64, 64), ("normal", 69, 139),
    ("normal", 50, 100), ("normal", 7, 130),
    ("four", 1, 1), ("four", 1, 12), ("four", 11, 1), ("four", 6, 6), ("four", 20, 40),
    ("four", 33, 47), ("four", 69, 138), ("four", 3, 100),
    ("equal", 1, 1), ("equal", 1, 5), ("equal", 5, 1), ("equal", 8, 8), ("equal", 10, 30),
    ("equal", 17, 23),
    ("zeros", 1, 1), ("zeros", 1, 9), ("zeros", 9, 1), ("zeros", 12, 12), ("zeros", 21, 63),
    ("zeros", 40, 27),
    ("denormal", 1, 4), ("denormal", 4, 1), ("denormal", 16, 16), ("denormal", 25, 75),
    ("denormal", 38, 51),
    ("heavy_ties", 30, 30), ("heavy_ties", 45, 90), ("heavy_ties", 60, 7), ("heavy_ties", 2, 120),
]


def scores(kind, P, N, seed):
    from tests import link_metrics_ref as R
    if kind != "heavy_ties":      # a coarse grid: most values occur on both sides
        return R.make_scores(kind, P, N, seed)
    rng = np.random.RandomState(seed)
    x = (rng.randint(0, 6, size=P + N) / 8.0).astype(np.float32)
    return x[:P].copy(), x[P:].copy()


def main():
    import sklearn
    from sklearn.metrics import average_precision_score, roc_auc_score
    out = {"sklearn": np.array(sklearn.__version__)}
    for i, (kind, P, N) in enumerate(CASES):
        pos, neg = scores(kind, P, N, seed=1000 + i)
        s = np.concatenate([pos, neg])
        y = np.concatenate([np.ones(P, np.int8), np.zeros(N, np.int8)])
        key = "c{:02d}.".format(i)
        out[key + "scores"], out[key + "labels"] = s, y
        out[key + "ap"] = np.float64(average_precision_score(y, s))
        out[key + "auc"] = np.float64(roc_auc_score(y, s))
        out[key + "kind"] = np.array(kind)
    np.savez(os.path.join(HERE, "link_metrics_reference.npz"), **out)
    print("wrote {} cases, scikit-learn {}".format(len(CASES), sklearn.__version__))


if __name__ == "__main__":
    main()
