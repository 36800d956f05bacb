"""Baselines that need no parameters.  EdgeBank, the memorisation baseline of the temporal
link-prediction protocols (Poursafaei et al., "Towards Better Evaluation for Dynamic Link
Prediction", NeurIPS 2022; the TGB protocol), over DynamicGraph.pair_history."""
import math

import numpy as np
import torch

_MODES = ("unlimited", "time_window")
_SCORES = ("seen", "count")


class EdgeBank:
    """Predicts that an edge exists if the pair has been seen before: a plain class, nothing to
    train.

        bank = EdgeBank(graph)                                   # unlimited memory
        bank = EdgeBank(graph, "time_window", window=86400.0)    # only the last day counts
        bank = EdgeBank(graph, min_count=3)                      # the repeat-count threshold
        pos, neg = bank.predict(roots, ts, neg_sample_ratio=K)   # EdgePredictor's shapes
        metrics.update(pos, neg, sigmoid=False)                  # LinkMetrics, as they are

    The memory is the graph's temporal edge store itself, read by graph.pair_history (one kernel
    per call on the current stream, no synchronisation):

    - mode="unlimited": every live edge of the source strictly before the row's time.
    - mode="time_window": those not older than `window`, since = ts - window (one float32
      subtraction on the device), lower end inclusive; `window` is a positive finite float.
    - max_history > 0 keeps only the newest max_history edges of the source in that window,
      which also bounds the cost for hubs (pair_history's cost note).
    - score="seen": (count >= min_count) as 0.0 / 1.0; score="count": the count itself as
      float32.  Both are finite.

    Because only edges strictly before each row's own time count, the whole stream can be
    ingested into the graph once and any split of it evaluated afterwards: a row never sees
    itself or anything later, so there is no leakage and no incremental "memory update" between
    batches.  On a graph built with reverse edges (add_reverse=True, undirected=True) the bank is
    symmetric: (u, v) has been seen when either direction was; on a directed graph only the
    source's own edges count."""

    def __init__(self, graph, mode: str = "unlimited", window=None, min_count: int = 1,
                 max_history: int = 0, score: str = "seen"):
        if mode not in _MODES:
            raise ValueError("mode must be one of {}, got {!r}".format(_MODES, mode))
        if score not in _SCORES:
            raise ValueError("score must be one of {}, got {!r}".format(_SCORES, score))
        if mode == "time_window":
            if isinstance(window, bool) or not isinstance(window, (int, float)) or \
                    not math.isfinite(window) or window <= 0:
                raise ValueError("mode 'time_window' needs a positive finite window, got "
                                 "{!r}".format(window))
            window = float(window)
        elif window is not None:
            raise ValueError("window is only for mode 'time_window', got {!r}".format(window))
        if isinstance(min_count, bool) or not isinstance(min_count, int) or min_count < 1:
            raise ValueError("min_count must be an int >= 1, got {!r}".format(min_count))
        if isinstance(max_history, bool) or not isinstance(max_history, int) or max_history < 0:
            raise ValueError("max_history must be an int >= 0, got {!r}".format(max_history))
        self.graph, self.mode, self.window = graph, mode, window
        self.min_count, self.max_history, self.score = min_count, max_history, score

    def score_pairs(self, src: torch.Tensor, dst: torch.Tensor, ts: torch.Tensor) -> torch.Tensor:
        """float32 [N]: the score of every (src[i], dst[i]) at time ts[i]; tensors on the
        graph's device, as for graph.pair_history."""
        since = ts - self.window if self.mode == "time_window" else None
        count = self.graph.pair_history(src, dst, ts, since=since,
                                        max_history=self.max_history).count
        if self.score == "seen":
            return (count >= self.min_count).float()
        return count.float()

    def _on_device(self, x, dtype):
        if isinstance(x, np.ndarray):
            x = torch.from_numpy(np.ascontiguousarray(x))
        if not isinstance(x, torch.Tensor):
            raise TypeError("roots and ts must be tensors or arrays, got {}".format(
                type(x).__name__))
        return x.to(device=torch.device("cuda", self.graph.device), dtype=dtype)

    def predict(self, roots, ts, neg_sample_ratio: int = 1):
        """(pred_pos [B, 1], pred_neg [K * B, 1]) for one batch in get_batch's /
        DeviceBatchStream's layout: roots = [src | dst | K blocks of B negatives] (k-major) and
        ts with at least B entries, the edges' times first.  src is paired with dst and with each
        negative block at the edge's time; one pair_history call for all (1 + K) * B pairs."""
        K = neg_sample_ratio
        if isinstance(K, bool) or not isinstance(K, int) or K < 0:
            raise ValueError("neg_sample_ratio must be an int >= 0, got {!r}".format(K))
        roots = self._on_device(roots, torch.int64)
        ts = self._on_device(ts, torch.float32)
        if roots.dim() != 1 or roots.shape[0] % (2 + K):
            raise ValueError("roots must be [src | dst | {} negative blocks], {} rows are not a "
                             "multiple of {}".format(K, tuple(roots.shape), 2 + K))
        B = roots.shape[0] // (2 + K)
        if ts.dim() != 1 or ts.shape[0] < B:
            raise ValueError("ts must hold the {} edge times first, got shape {}".format(
                B, tuple(ts.shape)))
        out = self.score_pairs(roots[:B].repeat(1 + K), roots[B:], ts[:B].repeat(1 + K))
        return out[:B].reshape(B, 1), out[B:].reshape(K * B, 1)
