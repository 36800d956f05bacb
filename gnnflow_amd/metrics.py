"""Validation metrics of link prediction, accumulated in HBM.

The reference's evaluate() (scripts/offline_edge_prediction.py:102-152) ends every batch with
`torch.cat([pred_pos, pred_neg]).sigmoid().cpu()`, scikit-learn's roc_auc_score and
average_precision_score on the host, and reports the mean over the batches.  LinkMetrics gives
the same means from ops.link_metrics: one kernel chain per batch on the current stream, the sums
kept on the device, one synchronisation per pass in compute().

    metrics = LinkMetrics(device)
    for ...:                                   # the validation batches
        pred_pos, pred_neg = model(mfgs)
        metrics.update(pred_pos, pred_neg)     # no sync
    result = metrics.compute()                 # {'ap', 'auc', 'mrr', ...}, one sync
"""
import torch

from . import ops
from .nn import LinkLoss  # noqa: F401  (the training loss kept the same way: nn.LinkLoss)

_FIELDS = ("sum_ap", "sum_auc", "sum_mrr", "batches", "mrr_batches", "nonfinite")


class LinkMetrics:
    """Running mean over batches of average precision, ROC-AUC and MRR."""

    def __init__(self, device="cuda"):
        device = torch.device(device)
        if device.type != "cuda":
            raise ValueError("LinkMetrics accumulates on the GPU, got {}".format(device))
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        self.device = device
        # the accumulator of ops.link_metrics: _FIELDS and two reserved fields
        self.state = torch.zeros(8, dtype=torch.float64, device=device)

    def update(self, pred_pos: torch.Tensor, pred_neg: torch.Tensor,
               sigmoid: bool = True) -> torch.Tensor:
        """Adds one batch and returns its [AP, AUC, MRR] (float64, on the device) without
        synchronising.  pred_pos / pred_neg: what EdgePredictor returns, [P, 1] and [r * P, 1].
        sigmoid=True ranks torch.sigmoid of the scores, as the reference's evaluate() does, ties
        of the saturated float32 sigmoid included; sigmoid=False ranks the scores as they are
        (ops.link_metrics says how the two differ)."""
        if sigmoid:
            pred_pos, pred_neg = torch.sigmoid(pred_pos.detach()), torch.sigmoid(pred_neg.detach())
        return ops.link_metrics(pred_pos, pred_neg, accumulator=self.state)

    def compute(self) -> dict:
        """The means over the batches counted so far (one device-to-host copy, which waits for
        the updates): 'ap' and 'auc' over 'batches', 'mrr' over 'mrr_batches' (the batches whose
        negatives were a whole number of blocks), NaN where the count is 0; 'nonfinite' counts
        the batches left out because a score was NaN or infinite."""
        s = dict(zip(_FIELDS, self.state.tolist()))
        nan = float("nan")
        b, mb = int(s["batches"]), int(s["mrr_batches"])
        return {"ap": s["sum_ap"] / b if b else nan,
                "auc": s["sum_auc"] / b if b else nan,
                "mrr": s["sum_mrr"] / mb if mb else nan,
                "batches": b, "mrr_batches": mb, "nonfinite": int(s["nonfinite"])}

    def reset(self) -> None:
        self.state.zero_()
