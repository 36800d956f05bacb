"""The neighbour-overlap heuristics that stand beside EdgeBank in temporal link-prediction
tables, on this package only: common neighbours, Jaccard, Adamic-Adar, resource allocation and
preferential attachment of the two ends' temporal neighbourhoods as the prediction.

The whole stream is ingested into the graph once.  `gnnflow_amd.NeighborOverlap` then asks the
temporal edge store, for every (src, dst, t) of a batch, which nodes both ends met STRICTLY BEFORE
t among their newest `--max-history` edges (`graph.common_neighbors`, one kernel per batch on the
GPU, and `graph.temporal_degree` for the two scores that weigh a common neighbour by its degree):
a row never sees itself or anything later, so any part of the stream is evaluated without leakage.
The batches come from a `gnnflow_amd.DeviceBatchStream` over the last rows of the stream, the
metrics from `gnnflow_amd.LinkMetrics` on the scores as they are (`sigmoid=False`); nothing waits
for the GPU until the one `compute()` at the end of each pass.  The graph is built with reverse
edges; on the bipartite REDDIT-shaped stream a user and a community then share no neighbour (a
user's neighbours are communities), so the overlap scores sit at chance while preferential
attachment does not: what a table with these baselines is there to show.  Synthetic data; a usage
example, not a benchmark.

    python examples/neighbor_baselines.py [--batches 20] [--batch-size 600] [--neg-ratio 1]
                                          [--scores cn,jaccard,aa,ra,pa] [--max-history 64]
                                          [--max-common 64] [--window W] [--hist-negatives N]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

import gnnflow_amd
from gnnflow_amd import synthetic
from gnnflow_amd.utils import build_dynamic_graph

SCORES = ("cn", "jaccard", "aa", "ra", "pa")


def main(num_batches=20, batch_size=600, neg_ratio=1, scores=SCORES, max_history=64,
         max_common=64, window=None, seed=0, verbose=True, hist_negatives=0, num_edges=60000):
    import pandas as pd
    dev = torch.device("cuda", 0)
    g = synthetic.reddit_like(seed=42, num_edges=num_edges)
    df = pd.DataFrame({"src": g["src"], "dst": g["dst"], "time": g["ts"], "eid": g["eid"]})
    graph = build_dynamic_graph(20 << 20, 1000 << 20, "cuda", 62, 1024, "insert",
                                undirected=True, device=0, dataset_df=df)
    # the last rows of the stream are the test split; their history is everything before them
    rows = min(num_batches * batch_size, len(df))
    dst_set = gnnflow_amd.DeviceDstSet(g["num_nodes"], dev, df["dst"].to_numpy())
    stream = gnnflow_amd.DeviceBatchStream.from_dataframe(
        df.iloc[len(df) - rows:].reset_index(drop=True), batch_size, dst_set,
        neg_ratio=neg_ratio, seed=seed, graph=graph if hist_negatives else None,
        hist_ratio=hist_negatives)
    results = {}
    for score in scores:
        base = gnnflow_amd.NeighborOverlap(graph, score, max_history=max_history,
                                           max_common=max_common, window=window)
        metrics = gnnflow_amd.LinkMetrics(dev)
        for roots, ts, _ in stream:
            pred_pos, pred_neg = base.predict(roots, ts, neg_ratio)
            metrics.update(pred_pos, pred_neg, sigmoid=False)      # scores as they are; no sync
        results[score] = r = metrics.compute()                      # the one sync of the pass
        if verbose:
            print("NeighborOverlap {:<7} max_history {}{}: ap {:.4f} auc {:.4f} mrr {:.4f} over "
                  "{} batches of {} edges, {} negative(s) each ({} historical)".format(
                      score, max_history, "" if window is None else " window {:g}".format(window),
                      r["ap"], r["auc"], r["mrr"], r["batches"], batch_size, neg_ratio,
                      hist_negatives))
    return results


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=20)
    ap.add_argument("--batch-size", type=int, default=600)
    ap.add_argument("--neg-ratio", type=int, default=1)
    ap.add_argument("--scores", default=",".join(SCORES))
    ap.add_argument("--max-history", type=int, default=64)
    ap.add_argument("--max-common", type=int, default=64)
    ap.add_argument("--window", type=float, default=None)
    ap.add_argument("--hist-negatives", type=int, default=0)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    main(a.batches, a.batch_size, a.neg_ratio, tuple(a.scores.split(",")), a.max_history,
         a.max_common, a.window, a.seed, hist_negatives=a.hist_negatives)
