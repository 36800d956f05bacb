"""Numpy restatement of ops.link_metrics (csrc/link_metrics.hip): average precision, ROC-AUC and
MRR of a batch from exact integer counts per positive.

    pge_i = #{j : pos[j] >= pos[i]}      nge_i = #{k : neg[k] >= pos[i]}
    nlt_i = #{k : neg[k] <  pos[i]}      neq_i = #{k : neg[k] == pos[i]}
    AP  = (1/P) sum_i pge_i / (pge_i + nge_i)
    AUC = (sum_i (2 nlt_i + neq_i)) / (2 P N)
    MRR = (1/P) sum_i 1 / (1 + gt_i + eq_i / 2)      N = r P; gt_i / eq_i over neg[k P + i], k < r

The comparisons are numpy's on float32 (IEEE: -0 == +0).  The counts are Python / int64
integers, every quotient one correctly rounded float64 division, the sums of quotients
math.fsum (correctly rounded), the AUC one division of two integers.

Bounds (u = 2**-53, the unit roundoff of float64):
  * against the kernel, AUC: 0.  Its numerator is an integer below 2**53 and 2 P N <= 2**31
    converts exactly; one correctly rounded division on either side.
  * against the kernel, AP and MRR: (P + 2) u.  P quotients of relative error u, each at most
    1; a sum of non-negative terms totalling at most P, in any order; one division by P.
  * against scikit-learn, AP and AUC: (P + N + 2) * 2u.  scikit-learn sums up to P + N terms in
    its own order (cumulative sums over the distinct thresholds, a trapezoid rule for the AUC).
"""
import math

import numpy as np

U = 2.0 ** -53
KINDS = ("normal", "four", "equal", "zeros", "denormal")


def kernel_bound(P):
    return (P + 2) * U


def sklearn_bound(P, N):
    return (P + N + 2) * 2.0 ** -52


def _f32(x):
    x = np.asarray(x)
    assert x.dtype == np.float32, x.dtype
    return x.reshape(-1)


def counts(pos, neg):
    """pge, nge, nlt, neq per positive, int64."""
    pos, neg = _f32(pos), _f32(neg)
    p = pos[:, None]
    pge = (pos[None, :] >= p).sum(1, dtype=np.int64)
    nge = (neg[None, :] >= p).sum(1, dtype=np.int64)
    nlt = (neg[None, :] < p).sum(1, dtype=np.int64)
    neq = (neg[None, :] == p).sum(1, dtype=np.int64)
    return pge, nge, nlt, neq


def reference(pos, neg):
    """{'ap', 'auc', 'mrr'} as Python floats; all NaN when a score is NaN or infinite, 'mrr' NaN
    when N is not a multiple of P."""
    pos, neg = _f32(pos), _f32(neg)
    P, N = len(pos), len(neg)
    assert P >= 1 and N >= 1
    nan = float("nan")
    if not (np.isfinite(pos).all() and np.isfinite(neg).all()):
        return {"ap": nan, "auc": nan, "mrr": nan}
    pge, nge, nlt, neq = counts(pos, neg)
    assert ((nge + nlt) == N).all() and (pge >= 1).all()
    ap = math.fsum(int(a) / int(a + b) for a, b in zip(pge, nge)) / P
    auc = int((2 * nlt + neq).sum()) / (2 * P * N)
    mrr = nan
    if N % P == 0:
        own = neg.reshape(N // P, P)
        gt = (own > pos[None, :]).sum(0, dtype=np.int64)
        eq = (own == pos[None, :]).sum(0, dtype=np.int64)
        mrr = math.fsum(1.0 / (1.0 + int(g) + int(e) / 2.0) for g, e in zip(gt, eq)) / P
    return {"ap": ap, "auc": auc, "mrr": mrr}


class Accumulator:
    """The eight-field running sum of gf_link_metrics, batch after batch in float64."""
    FIELDS = ("sum_ap", "sum_auc", "sum_mrr", "batches", "mrr_batches", "nonfinite")

    def __init__(self):
        self.state = np.zeros(8, dtype=np.float64)
        self.bound_ap = 0.0       # the per-batch bounds against the kernel, added together
        self.bound_mrr = 0.0

    def add(self, pos, neg):
        r = reference(pos, neg)
        if math.isnan(r["ap"]):
            self.state[5] += 1
            return r
        self.state[0] += r["ap"]
        self.state[1] += r["auc"]
        self.state[3] += 1
        self.bound_ap += kernel_bound(len(_f32(pos)))
        if not math.isnan(r["mrr"]):
            self.state[2] += r["mrr"]
            self.state[4] += 1
            self.bound_mrr += kernel_bound(len(_f32(pos)))
        return r


def make_scores(kind, P, N, seed):
    """(pos [P], neg [N]) float32.  normal: N(0, 1), the positives shifted up; four: four
    distinct values; equal: one value; zeros: -0.0 and +0.0 mixed with a few other values;
    denormal: small multiples of 2**-149 of either sign."""
    rng = np.random.RandomState(seed)
    n = P + N
    if kind == "normal":
        x = rng.randn(n).astype(np.float32)
        x[:P] += np.float32(0.5)
    elif kind == "four":
        x = rng.choice(np.array([-1.5, 0.25, 0.75, 3.0], dtype=np.float32), size=n)
    elif kind == "equal":
        x = np.full(n, 0.625, dtype=np.float32)
    elif kind == "zeros":
        x = rng.choice(np.array([-0.0, 0.0, -0.0, 0.0, -1.0, 2.0], dtype=np.float32), size=n)
    elif kind == "denormal":
        x = (rng.randint(-40, 41, size=n) * 2.0 ** -149).astype(np.float32)
        assert (np.abs(x[x != 0]) < np.finfo(np.float32).tiny).all()
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(x[:P]), np.ascontiguousarray(x[P:])
