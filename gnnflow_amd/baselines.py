"""Baselines that need no parameters.  EdgeBank, the memorisation baseline of the temporal
link-prediction protocols (Poursafaei et al., "Towards Better Evaluation for Dynamic Link
Prediction", NeurIPS 2022; the TGB protocol), over DynamicGraph.pair_history; NeighborOverlap,
the neighbour-overlap heuristics (common neighbours, Jaccard, Adamic-Adar, resource allocation,
preferential attachment), over DynamicGraph.common_neighbors."""
import math

import numpy as np
import torch

_MODES = ("unlimited", "time_window")
_SCORES = ("seen", "count")


class _PairScorer:
    """predict() in EdgePredictor's shapes over a subclass's score_pairs(src, dst, ts)."""

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
        negative block at the edge's time; one score_pairs call for all (1 + K) * B pairs."""
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


class EdgeBank(_PairScorer):
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


_OVERLAP_SCORES = ("cn", "jaccard", "aa", "ra", "pa")


class NeighborOverlap(_PairScorer):
    """The neighbour-overlap heuristics that stand beside EdgeBank in link-prediction tables:
    common neighbours, Jaccard, Adamic-Adar, resource allocation and preferential attachment,
    over the temporal neighbourhoods of DynamicGraph.common_neighbors.  A plain class, nothing to
    train.

        base = NeighborOverlap(graph, "aa")                       # Adamic-Adar
        base = NeighborOverlap(graph, "jaccard", window=86400.0)  # only the last day counts
        pos, neg = base.predict(roots, ts, neg_sample_ratio=K)    # EdgePredictor's shapes
        metrics.update(pos, neg, sigmoid=False)                   # LinkMetrics, as they are

    The neighbourhood of a node at a row's time is the set of destinations of its newest
    max_history (1 .. 512) live edges strictly before that time and, with `window` (a positive
    finite float), not older than it: since = ts - window, one float32 subtraction on the device,
    lower end inclusive, as for EdgeBank.  With cn = the common neighbours of the two ends,
    u_src / u_dst their distinct neighbours and n_src / n_dst their edges in that window
    (CommonNeighbors' fields):

    - "cn":      cn
    - "jaccard": cn / (u_src + u_dst - cn), 0 where the union is empty
    - "pa":      n_src * n_dst
    - "aa":      the sum over the common neighbours z of 1 / ln(deg z), for deg z >= 2
    - "ra":      the sum over the common neighbours z of 1 / deg z, for deg z >= 1

    deg z = graph.temporal_degree(z, ts, since): all of z's edges in the row's window, not capped
    by max_history.  "aa" and "ra" sum over the nodes common_neighbors RETURNS, the max_common
    (0 .. 512) that the source met most recently: where a pair has more common neighbours than
    max_common, the rest do not contribute.  The other three scores do not depend on max_common.
    All scores are computed in float64 by torch and rounded once to float32; they are finite.

    As for EdgeBank the whole stream can be ingested once and any split evaluated afterwards: a
    row sees only edges strictly before its own time.  The two ends themselves are not removed
    from the neighbourhoods (common_neighbors' note on graphs with reverse edges)."""

    def __init__(self, graph, score: str = "cn", max_history: int = 64, max_common: int = 64,
                 window=None):
        from .dynamic_graph import CN_MAX_HISTORY
        if score not in _OVERLAP_SCORES:
            raise ValueError("score must be one of {}, got {!r}".format(_OVERLAP_SCORES, score))
        for name, v, lo in (("max_history", max_history, 1), ("max_common", max_common, 0)):
            if isinstance(v, bool) or not isinstance(v, int) or not lo <= v <= CN_MAX_HISTORY:
                raise ValueError("{} must be an int in [{}, {}], got {!r}".format(
                    name, lo, CN_MAX_HISTORY, v))
        if window is not None:
            if isinstance(window, bool) or not isinstance(window, (int, float)) or \
                    not math.isfinite(window) or window <= 0:
                raise ValueError("window must be None or a positive finite float, got "
                                 "{!r}".format(window))
            window = float(window)
        self.graph, self.score, self.window = graph, score, window
        self.max_history, self.max_common = max_history, max_common

    def score_pairs(self, src: torch.Tensor, dst: torch.Tensor, ts: torch.Tensor) -> torch.Tensor:
        """float32 [N]: the score of every (src[i], dst[i]) at time ts[i]; tensors on the
        graph's device, as for graph.common_neighbors."""
        return self.scores_float64(src, dst, ts).float()

    def scores_float64(self, src: torch.Tensor, dst: torch.Tensor,
                       ts: torch.Tensor) -> torch.Tensor:
        """float64 [N]: score_pairs before its one rounding to float32."""
        since = ts - self.window if self.window is not None else None
        by_node = self.score in ("aa", "ra")
        cn = self.graph.common_neighbors(src, dst, ts, since=since, max_history=self.max_history,
                                         max_common=self.max_common if by_node else 0)
        if self.score == "cn":
            out = cn.common.double()
        elif self.score == "pa":
            out = cn.n_src.double() * cn.n_dst.double()
        elif self.score == "jaccard":
            union = (cn.u_src + cn.u_dst - cn.common).double()
            out = torch.where(union > 0, cn.common.double() / union.clamp(min=1.0),
                              torch.zeros_like(union))
        else:
            K = cn.nodes.shape[1]
            deg = self.graph.temporal_degree(
                cn.nodes, ts.reshape(-1, 1).expand(-1, K),
                since=None if since is None else since.reshape(-1, 1).expand(-1, K)).double()
            if self.score == "aa":
                term = torch.where(deg >= 2, 1.0 / torch.log(deg.clamp(min=2.0)),
                                   torch.zeros_like(deg))
            else:
                term = torch.where(deg >= 1, 1.0 / deg.clamp(min=1.0), torch.zeros_like(deg))
            out = term.sum(dim=1)
        return out
