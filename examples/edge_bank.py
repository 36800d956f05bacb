"""EdgeBank, the memorisation baseline of the temporal link-prediction protocols, on this package
only: "this pair has interacted before" as the prediction.  A model's AP / AUC / MRR on a temporal
graph means little without it.

The whole stream is ingested into the graph once.  `gnnflow_amd.EdgeBank` then asks the temporal
edge store, for every (src, dst, t) of a batch, whether src met dst STRICTLY BEFORE t
(`graph.pair_history`, one kernel per batch on the GPU): a row never sees itself or anything
later, so any part of the stream is evaluated without leakage and without "memory updates"
between batches.  The batches come from a `gnnflow_amd.DeviceBatchStream` over the last rows of
the stream, the metrics from `gnnflow_amd.LinkMetrics` on the scores as they are
(`sigmoid=False`); nothing waits for the GPU until the one `compute()` at the end of the pass.
The graph is built with reverse edges, so the bank is symmetric.  Synthetic REDDIT-shaped data;
a usage example, not a benchmark.

    python examples/edge_bank.py [--batches 20] [--batch-size 600] [--neg-ratio 1]
                                 [--mode unlimited|time_window] [--window W] [--score seen|count]
                                 [--min-count 1] [--hist-negatives N]

--hist-negatives N makes the first N negatives of every edge destinations the source has met
before: the setting in which a memorisation baseline stops looking good.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

import gnnflow_amd
from gnnflow_amd import synthetic
from gnnflow_amd.utils import build_dynamic_graph


def main(num_batches=20, batch_size=600, neg_ratio=1, mode="unlimited", window=None, seed=0,
         verbose=True, score="seen", min_count=1, max_history=0, hist_negatives=0,
         num_edges=60000):
    import pandas as pd
    dev = torch.device("cuda", 0)
    g = synthetic.reddit_like(seed=42, num_edges=num_edges)
    df = pd.DataFrame({"src": g["src"], "dst": g["dst"], "time": g["ts"], "eid": g["eid"]})
    graph = build_dynamic_graph(20 << 20, 1000 << 20, "cuda", 62, 1024, "insert",
                                undirected=True, device=0, dataset_df=df)
    if mode == "time_window" and window is None:
        window = float(df["time"].max() - df["time"].min()) / 10      # a tenth of the span
    bank = gnnflow_amd.EdgeBank(graph, mode, window=window if mode == "time_window" else None,
                                min_count=min_count, max_history=max_history, score=score)

    # the last rows of the stream are the test split; their history is everything before them
    rows = min(num_batches * batch_size, len(df))
    dst_set = gnnflow_amd.DeviceDstSet(g["num_nodes"], dev, df["dst"].to_numpy())
    stream = gnnflow_amd.DeviceBatchStream.from_dataframe(
        df.iloc[len(df) - rows:].reset_index(drop=True), batch_size, dst_set,
        neg_ratio=neg_ratio, seed=seed, graph=graph if hist_negatives else None,
        hist_ratio=hist_negatives)
    metrics = gnnflow_amd.LinkMetrics(dev)
    for roots, ts, _ in stream:
        pred_pos, pred_neg = bank.predict(roots, ts, neg_ratio)
        metrics.update(pred_pos, pred_neg, sigmoid=False)      # scores as they are; no sync
    result = metrics.compute()                                  # the one sync of the pass
    if verbose:
        print("EdgeBank {}{} score={} min_count={}: ap {:.4f} auc {:.4f} mrr {:.4f} over {} "
              "batches of {} edges, {} negative(s) each ({} historical)".format(
                  mode, " window {:g}".format(window) if mode == "time_window" else "", score,
                  min_count, result["ap"], result["auc"], result["mrr"], result["batches"],
                  batch_size, neg_ratio, hist_negatives))
    return result


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=20)
    ap.add_argument("--batch-size", type=int, default=600)
    ap.add_argument("--neg-ratio", type=int, default=1)
    ap.add_argument("--mode", default="unlimited", choices=["unlimited", "time_window"])
    ap.add_argument("--window", type=float, default=None,
                    help="time_window's width (default: a tenth of the stream's time span)")
    ap.add_argument("--score", default="seen", choices=["seen", "count"])
    ap.add_argument("--min-count", type=int, default=1)
    ap.add_argument("--max-history", type=int, default=0)
    ap.add_argument("--hist-negatives", type=int, default=0)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    main(a.batches, a.batch_size, a.neg_ratio, a.mode, a.window, a.seed, score=a.score,
         min_count=a.min_count, max_history=a.max_history, hist_negatives=a.hist_negatives)
