"""Numpy float64 restatement of ops.link_loss (csrc/link_loss.hip): the reference's training loss
criterion(pred_pos, ones) + criterion(pred_neg, zeros) with BCEWithLogitsLoss, its gradients and
the running sums of an epoch.

    t(x)   = log1p(exp(-|x|))
    l_pos  = max(-x, 0) + t(x)            softplus(-x)
    l_neg  = max( y, 0) + t(y)            softplus( y)
    loss   = (1/P) sum_i l_pos(x_i) + (1/N) sum_j l_neg(y_j)
    dloss/dx_i = -s(-x_i) / P        dloss/dy_j = s(y_j) / N
    s(t)   = 1 / (1 + exp(-t)) for t >= 0,   exp(t) / (1 + exp(t)) for t < 0

Everything is float64 on the logits as given (float32, or bfloat16 values held in float32); the
sums are math.fsum.  No expression subtracts nearly equal numbers, so each term, each gradient
and the loss carry a few units of 2**-53 of relative error.

Bounds for the kernels against this file (u = 2**-24, float32's unit roundoff; a function
"within k ulp" has relative error at most 2 k u):
  * loss: 16 u relative.  A term is expf (1 ulp in the device library, 2 allowed for), log1pf
    (2 ulp; the relative error of its argument passes through with a factor below 1) and one
    add: at most 4 u + 4 u + u; every term is non-negative, so the means inherit the bound; the
    float64 sums add nothing visible; the rounding to float32 adds u.
  * gradients: 8 u relative where the result is a normal float32, 2**-126 absolute below.  expf
    (2 u), the add, the division, g / P and the product (u each): 6 u.
"""
import math

import numpy as np

U32 = 2.0 ** -24
LOSS_RTOL = 16 * U32
GRAD_RTOL = 8 * U32
GRAD_ATOL = 2.0 ** -126
ACC_FIELDS = ("sum_loss", "sum_loss_times_P", "batches", "nonfinite", "sum_P")
FIXED = (0.0, 1e-8, -1e-8, 20.0, -20.0, 80.0, -80.0)


def _f64(x):
    x = np.asarray(x)
    assert x.dtype == np.float32, x.dtype
    return x.reshape(-1).astype(np.float64)


def sigmoid(t):
    t = np.asarray(t, dtype=np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        e = np.exp(-np.abs(t))      # <= 1
        return np.where(t >= 0, 1.0 / (1.0 + e), e / (1.0 + e))      # e is NaN where t is


def terms(pos, neg):
    """(l_pos [P], l_neg [N]) in float64."""
    x, y = _f64(pos), _f64(neg)
    with np.errstate(invalid="ignore"):
        lp = np.fmax(-x, 0.0) + np.log1p(np.exp(-np.abs(x)))
        ln = np.fmax(y, 0.0) + np.log1p(np.exp(-np.abs(y)))
    return lp, ln


def _sum(a):
    return math.fsum(a) if np.isfinite(a).all() else float(np.sum(a))


def reference(pos, neg, upstream=1.0):
    """{'loss': float, 'grad_pos': float64 [P], 'grad_neg': float64 [N]}; the gradients are those
    of upstream * loss."""
    x, y = _f64(pos), _f64(neg)
    P, N = len(x), len(y)
    assert P >= 1 and N >= 1
    lp, ln = terms(pos, neg)
    loss = _sum(lp) / P + _sum(ln) / N
    return {"loss": loss,
            "grad_pos": -sigmoid(-x) / P * upstream,
            "grad_neg": sigmoid(y) / N * upstream}


def round_bf16(a):
    """fp32 -> the nearest bfloat16 (ties to even) as fp32: the kernels' narrow() of bf16.hpp on
    finite values (tests/layer_epilogue_ref.py has the same helper)."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    b = a.view(np.uint32).astype(np.uint64)
    b = ((b + np.uint64(0x7FFF) + ((b >> np.uint64(16)) & np.uint64(1))) >> np.uint64(16)) \
        << np.uint64(16)
    return b.astype(np.uint32).view(np.float32).reshape(a.shape)


def bf16_gradients(pos, neg, upstream=1.0):
    """The gradients rounded to float32 and then to bfloat16, as float32 arrays.  The kernels
    round their own float32 gradient, which may sit one float32 ulp from this file's, so a
    comparison allows one bfloat16 ulp where the two straddle a rounding boundary."""
    r = reference(pos, neg, upstream)
    return (round_bf16(r["grad_pos"].astype(np.float32)),
            round_bf16(r["grad_neg"].astype(np.float32)))


class Accumulator:
    """The five-field running sum of gf_link_loss, batch after batch in float64.  The kernel
    adds its float32 loss; add() takes that loss, or rounds this file's own."""

    def __init__(self):
        self.state = np.zeros(len(ACC_FIELDS), dtype=np.float64)

    def add(self, pos, neg, loss=None):
        if loss is None:
            with np.errstate(over="ignore"):
                loss = np.float32(reference(pos, neg)["loss"])
        loss = float(np.float32(loss))
        if not math.isfinite(loss):
            self.state[3] += 1
            return loss
        P = len(_f64(pos))
        self.state[0] += loss
        self.state[1] += loss * P
        self.state[2] += 1
        self.state[4] += P
        return loss

    def compute(self):
        s = dict(zip(ACC_FIELDS, self.state.tolist()))
        nan = float("nan")
        return {"mean_loss": s["sum_loss"] / s["batches"] if s["batches"] else nan,
                "edge_weighted_loss": s["sum_loss_times_P"] / s["sum_P"] if s["sum_P"] else nan,
                "batches": int(s["batches"]), "nonfinite": int(s["nonfinite"])}


def make_logits(P, N, seed, fixed=True):
    """(pos [P], neg [N]) float32 drawn from N(0, 3); with `fixed`, a side of at least
    len(FIXED) logits starts with the values FIXED (0, +-1e-8, +-20, +-80)."""
    rng = np.random.RandomState(seed)
    pos = (3.0 * rng.randn(P)).astype(np.float32)
    neg = (3.0 * rng.randn(N)).astype(np.float32)
    if fixed:
        for side in (pos, neg):
            if len(side) >= len(FIXED):
                side[:len(FIXED)] = FIXED
    return pos, neg
