"""link_loss (csrc/link_loss.hip) and link_metrics (csrc/link_metrics.hip): the training loss and
the evaluation metrics of a batch of link scores, with running sums on the device."""
from typing import Optional

import torch

from .. import _capi
from ._common import (_bwd, _check_accumulator, _check_on_gpu, _check_same_device, _check_tensors,
                      _fwd, _grad_as, _grads_like, _launch, _partial_rows, _ptr)

LINK_METRICS_MAX_SCORES = 65536      # GF_LINK_METRICS_MAX_SCORES: the limit on P + N
LINK_METRICS_TILE = 2048             # GF_LINK_METRICS_TILE: scores per LDS tile of the kernel
_LINK_METRICS_PARTIAL_WORDS = 4      # GF_LINK_METRICS_PARTIAL_WORDS


def link_metrics(pos: torch.Tensor, neg: torch.Tensor,
                 accumulator: Optional[torch.Tensor] = None) -> torch.Tensor:
    """[AP, AUC, MRR] of one batch as a float64 tensor [3] on the GPU: sklearn's
    average_precision_score and roc_auc_score of torch.cat([pos, neg]) against the labels
    [1] * P + [0] * N, as the reference's evaluate() computes them per batch, and the mean
    reciprocal rank of each positive among its own negatives.

    pos: [P] or [P, 1], the scores of the true edges; neg: [N] or [N, 1], those of the negative
    ones, as EdgePredictor returns them; float32 on one GPU, P >= 1, N >= 1 and
    P + N <= LINK_METRICS_MAX_SCORES.  Both are detached; a non-contiguous input is copied.
    MRR needs N = r * P with positive i's negatives at neg[k * P + i] (the block layout of
    edge_score); its rank is 1 + #greater + #equal / 2, the mean of the optimistic and the
    pessimistic rank.  When N is not a multiple of P it is NaN.

    accumulator: a float64 [8] tensor on the same GPU, the running sums of a validation pass
    (sum_ap, sum_auc, sum_mrr, batches, mrr_batches, nonfinite, 2 reserved), updated on the
    device; metrics.LinkMetrics wraps it.  A NaN or an infinity among the scores (scikit-learn
    raises) gives three NaNs and adds 1 to `nonfinite` alone.

    Runs on the current stream and never synchronises.  Ties are counted, not broken, and the
    sums run in a fixed order: the same inputs give the same bits.

    The scores are ranked as given.  sigmoid is increasing, so ranking logits is ranking their
    exact sigmoids; float32 torch.sigmoid saturates (to 1.0 from about 17 on, to 0 below about
    -104) and rounds neighbouring logits to one value, so sigmoid(logits) has ties that the logits
    do not have, and its metrics can differ from those of the logits.  Pass what you want ranked."""
    for name, x in (("pos", pos), ("neg", neg)):
        _check_tensors((name, x))      # everything about pos before anything about neg
        if x.dtype != torch.float32:
            raise TypeError("link_metrics ranks float32 scores, {} is {}".format(name, x.dtype))
        if not (x.dim() == 1 or (x.dim() == 2 and x.shape[1] == 1)):
            raise ValueError("{} must be [n] or [n, 1], got {}".format(name, tuple(x.shape)))
    P, N = int(pos.shape[0]), int(neg.shape[0])
    if P == 0 or N == 0:
        raise ValueError("link_metrics needs at least one positive and one negative score, got "
                         "{} and {}".format(P, N))
    if P + N > LINK_METRICS_MAX_SCORES:
        raise ValueError("link_metrics takes at most {} scores per call, got {} + {}".format(
            LINK_METRICS_MAX_SCORES, P, N))
    # the devices of the scores before the accumulator: link_loss has it the other way round
    _check_same_device("pos", pos, ("neg", neg))
    _check_on_gpu("link_metrics", pos.device)
    acc = accumulator
    if acc is not None:
        _check_accumulator(acc, 8)
        _check_same_device("pos", pos, ("accumulator", acc))
    p = pos.detach().reshape(P).contiguous()
    n = neg.detach().reshape(N).contiguous()
    rows = _partial_rows(_capi.load().gf_link_metrics_partial_rows, P)
    f64 = dict(dtype=torch.float64, device=p.device)
    partials = torch.empty((rows, _LINK_METRICS_PARTIAL_WORDS), **f64)
    out = torch.empty(3, **f64)
    _launch(p.device, "gf_link_metrics", None, None,
            (p.data_ptr(), n.data_ptr(), P, N, partials.data_ptr(), rows, out.data_ptr(),
             _ptr(acc)))
    return out


LINK_LOSS_TILE = 1024                # GF_LINK_LOSS_TILE: logits per workgroup pass of the kernel
LINK_LOSS_SINGLE_TILES = 8           # GF_LINK_LOSS_SINGLE_TILES: up to here the forward is one launch
LINK_LOSS_MAX_PARTIAL_ROWS = 256     # GF_LINK_LOSS_MAX_PARTIAL_ROWS: half of them for each side
LINK_LOSS_ACC_FIELDS = 5             # GF_LINK_LOSS_ACC_FIELDS


class _LinkLoss(torch.autograd.Function):
    @staticmethod
    @_fwd
    def forward(ctx, pos, neg, acc):
        # pos [P], neg [N] contiguous, both fp32 or both bf16; acc None or float64 [5]
        P, N = pos.shape[0], neg.shape[0]
        rows = _partial_rows(_capi.load().gf_link_loss_partial_rows, P, N)
        partials = torch.empty(rows, dtype=torch.float64, device=pos.device) if rows else None
        out = torch.empty((), dtype=torch.float32, device=pos.device)
        _launch(pos.device, "gf_link_loss", "gf_link_loss_bf16", pos.dtype,
                (pos.data_ptr(), neg.data_ptr(), P, N, _ptr(partials), rows, out.data_ptr(),
                 _ptr(acc)))
        ctx.save_for_backward(pos, neg)
        return out

    @staticmethod
    @_bwd
    def backward(ctx, grad):
        pos, neg = ctx.saved_tensors
        needs = ctx.needs_input_grad[:2]
        if not any(needs):
            return None, None, None
        g = _grad_as(grad, torch.float32)
        gp, gn = _grads_like((pos, neg), needs)
        _launch(pos.device, "gf_link_loss_backward", "gf_link_loss_backward_bf16", pos.dtype,
                (pos.data_ptr(), neg.data_ptr(), pos.shape[0], neg.shape[0], g.data_ptr(),
                 _ptr(gp), _ptr(gn)))
        return gp, gn, None


def link_loss(pos: torch.Tensor, neg: torch.Tensor,
              accumulator: Optional[torch.Tensor] = None) -> torch.Tensor:
    """mean(softplus(-pos)) + mean(softplus(neg)) as a float32 scalar tensor (shape []) on the
    GPU: the reference's training loss, criterion(pred_pos, ones) + criterion(pred_neg, zeros)
    with BCEWithLogitsLoss, in one launch (two beyond LINK_LOSS_SINGLE_TILES tiles of
    LINK_LOSS_TILE logits in all) and one more for the backward.

    pos: [P] or [P, 1], the logits of the true edges; neg: [N] or [N, 1], those of the negative
    ones, as EdgePredictor returns them; N need not be a multiple of P.  Both float32 or both
    bfloat16 on one GPU, P >= 1, N >= 1; any other dtype or a mixture raises TypeError.  Row
    slices of one buffer (out[:B], out[B:] of edge_score) are taken as they are; a non-contiguous
    input is copied.  Differentiable in pos and neg; only the logits are saved.

    Every term is float32 arithmetic, the sums are float64 in a fixed order and the loss is
    rounded to float32 once: the same inputs give the same bits.  bfloat16 logits follow the
    module's rule: the loss is float32 and equals link_loss(pos.float(), neg.float()) bit for
    bit, the gradients are bfloat16, the float32 gradients rounded once.

    accumulator: a float64 contiguous [LINK_LOSS_ACC_FIELDS] = [5] tensor on the same GPU, the
    running sums of an epoch (sum_loss, sum_loss_times_P, batches, nonfinite, sum_P), updated on
    the device in the forward from the float32 loss; nn.LinkLoss wraps it.  A NaN logit gives a
    NaN loss, infinities follow the formulas; a loss that is not finite adds 1 to `nonfinite`
    alone.

    Runs on the current stream and never synchronises."""
    _check_tensors(("pos", pos), ("neg", neg))
    if (pos.dtype, neg.dtype) not in ((torch.float32,) * 2, (torch.bfloat16,) * 2):
        raise TypeError("link_loss computes in float32 and takes pos and neg both float32 or both "
                        "bfloat16, pos is {} and neg is {}".format(pos.dtype, neg.dtype))
    for name, x in (("pos", pos), ("neg", neg)):
        if not (x.dim() == 1 or (x.dim() == 2 and x.shape[1] == 1)):
            raise ValueError("{} must be [n] or [n, 1], got {}".format(name, tuple(x.shape)))
    P, N = int(pos.shape[0]), int(neg.shape[0])
    if P == 0 or N == 0:
        raise ValueError("link_loss needs at least one positive and one negative logit, got "
                         "{} and {}".format(P, N))
    if P >= 1 << 31 or N >= 1 << 31:
        raise ValueError("link_loss takes fewer than 2^31 logits on a side, got {} and {}".format(
            P, N))
    acc = accumulator
    if acc is not None:
        _check_accumulator(acc, LINK_LOSS_ACC_FIELDS)
    # the accumulator's type and shape before any device: link_metrics has it the other way round
    _check_same_device("pos", pos, ("neg", neg), ("accumulator", acc))
    _check_on_gpu("link_loss", pos.device)
    return _LinkLoss.apply(pos.reshape(P).contiguous(), neg.reshape(N).contiguous(),
                           None if acc is None else acc.detach())
