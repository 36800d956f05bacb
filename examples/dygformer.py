"""DyGFormer on this package only: a few optimiser steps of `gnnflow_amd.models.DyGFormer` on a
stream whose every input is read from the temporal edge store by one launch per batch, then its
metrics on the held-out tail of the stream.

The whole stream is ingested into the graph once.  Per batch of B edges the pairs are the B
positive ones and `--negatives` random destinations per source, (1 + K) * B rows laid out
[src | src .. ] against [dst | neg_1 | .. | neg_K], all at the edge's time.
`model.forward_graph(graph, src, dst, ts, node_feats, edge_feats)` calls
`graph.pair_sequence(..., length=L, node_feats=, edge_feats=, time_encoder=model.time_enc)`, which
returns for both ends of every pair the node itself and its newest L - 1 interactions STRICTLY
BEFORE t as finished node-feature, edge-feature and time-encoding channels and the neighbour
co-occurrence counts, padded slots zero, and runs the model on them.  examples/dygformer_inputs.py
shows the same inputs built step by step from `neighbor_cooccurrence`.

A row never sees itself or anything later, so there is nothing to update between batches.  The
loss is `nn.LinkLoss`, the metrics `LinkMetrics` on the last `--eval-batches` batches, which are
not trained on; nothing waits for the GPU until the `compute()` calls at the end.  Synthetic
REDDIT-shaped data; a usage example, not a benchmark.

    python examples/dygformer.py [--batches 5] [--eval-batches 2] [--batch-size 200]
                                 [--negatives 1] [--length 32] [--patch 1] [--dim 16]
                                 [--edges 20000]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

import gnnflow_amd
from gnnflow_amd import synthetic
from gnnflow_amd.models import DyGFormer
from gnnflow_amd.utils import build_dynamic_graph


def main(num_batches=5, eval_batches=2, batch_size=200, negatives=1, length=32, patch_size=1,
         dim=16, num_edges=20000, seed=0, lr=1e-3, verbose=True):
    import pandas as pd
    dev = torch.device("cuda", 0)
    g = synthetic.reddit_like(seed=42, num_edges=num_edges)
    df = pd.DataFrame({"src": g["src"], "dst": g["dst"], "time": g["ts"], "eid": g["eid"]})
    graph = build_dynamic_graph(20 << 20, 1000 << 20, "cuda", 62, 1024, "insert",
                                undirected=True, device=0, dataset_df=df)
    torch.manual_seed(seed)
    node_feats = torch.randn(g["num_nodes"], dim).to(dev)
    edge_feats = torch.randn(g["num_edges"], dim).to(dev)
    dsts = torch.from_numpy(np.unique(df["dst"].to_numpy()).astype(np.int64)).to(dev)
    model = DyGFormer(dim, dim, dim_time=dim, channel_dim=dim, patch_size=patch_size,
                      max_length=length, dim_embed=dim).to(dev)
    optimizer = torch.optim.Adam(model.parameters(), lr=lr)
    criterion = gnnflow_amd.LinkLoss()
    metrics = gnnflow_amd.LinkMetrics(dev)

    rows = min((num_batches + eval_batches) * batch_size, len(df))
    first = len(df) - rows      # the last rows of the stream; their history is what came before
    starts = list(range(first, len(df), batch_size))
    batches = []
    for i, lo in enumerate(starts):
        train = i < len(starts) - eval_batches
        part = df.iloc[lo:lo + batch_size]
        src = torch.from_numpy(part["src"].to_numpy().astype(np.int64)).to(dev)
        dst = torch.from_numpy(part["dst"].to_numpy().astype(np.int64)).to(dev)
        t = torch.from_numpy(part["time"].to_numpy().astype(np.float32)).to(dev)
        B = len(src)
        neg = dsts[torch.randint(0, len(dsts), (negatives * B,), device=dev)]
        pair_src, pair_dst = src.repeat(1 + negatives), torch.cat([dst, neg])
        pair_ts = t.repeat(1 + negatives)

        model.train(train)
        with torch.set_grad_enabled(train):
            score = model.forward_graph(graph, pair_src, pair_dst, pair_ts, node_feats,
                                        edge_feats)
        pred_pos, pred_neg = score[:B], score[B:]
        entry = {"train": train, "score": tuple(score.shape), "pred_pos": tuple(pred_pos.shape),
                 "pred_neg": tuple(pred_neg.shape)}
        if train:
            loss = criterion(pred_pos, pred_neg)
            optimizer.zero_grad()
            loss.backward()
            optimizer.step()
            entry["loss"] = loss.detach()
        else:
            metrics.update(pred_pos, pred_neg)
        batches.append(entry)
    result = {"loss": criterion.compute(), "metrics": metrics.compute(), "batches": batches}
    for b in batches:                                              # after the syncs above
        if "loss" in b:
            b["loss"] = float(b["loss"])
    if verbose:
        for i, b in enumerate(batches):
            if b["train"]:
                print("batch {}: loss {:.4f} over {} pairs".format(i, b["loss"], b["score"][0]))
        m = result["metrics"]
        print("DyGFormer, {} steps: mean loss {:.4f}; held-out {} batches: ap {:.4f} auc {:.4f} "
              "mrr {:.4f}".format(result["loss"]["batches"], result["loss"]["mean_loss"],
                                  m["batches"], m["ap"], m["auc"], m["mrr"]))
    return result


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=5)
    ap.add_argument("--eval-batches", type=int, default=2)
    ap.add_argument("--batch-size", type=int, default=200)
    ap.add_argument("--negatives", type=int, default=1)
    ap.add_argument("--length", type=int, default=32)
    ap.add_argument("--patch", type=int, default=1)
    ap.add_argument("--dim", type=int, default=16)
    ap.add_argument("--edges", type=int, default=20000)
    a = ap.parse_args()
    main(a.batches, a.eval_batches, a.batch_size, a.negatives, a.length, a.patch, a.dim, a.edges)
