"""GraphMixer on this package only: a few optimiser steps of `gnnflow_amd.models.GraphMixer` on the
last batches of a stream, with both of its inputs read from the temporal edge store.

The whole stream is ingested into the graph once.  Per batch the roots are [src | dst | neg] (one
random destination per edge as the negative), all at the edge's time, and for every root

- the link encoder's tokens are its newest `--tokens` interactions STRICTLY BEFORE t:
  `graph.neighbor_sequence(roots, ts, length=K, edge_feats=..., time_encoder=model.time_enc)`
  returns them finished, [edge features | time encoding of t minus the edge's time] with the
  padded slots zero, from one kernel, and `model.forward_tokens` takes them as they are;
- the node encoder's `nbr_mean` is `graph.neighbor_aggregate(roots, ts, node_feats=...,
  max_history=H).node`: the mean of the features of the nodes met over the newest `--history`
  edges, one kernel, no [N, H, d] intermediate.

A row never sees itself or anything later, so there is nothing to update between batches.  The
loss is `nn.LinkLoss`, the metrics `LinkMetrics`; nothing waits for the GPU until the two
`compute()` calls at the end.  Synthetic REDDIT-shaped data; a usage example, not a benchmark.

    python examples/graphmixer.py [--batches 5] [--batch-size 200] [--tokens 32] [--history 64]
                                  [--dim 16] [--edges 20000]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

import gnnflow_amd
from gnnflow_amd import synthetic
from gnnflow_amd.models import GraphMixer
from gnnflow_amd.utils import build_dynamic_graph


def main(num_batches=5, batch_size=200, num_tokens=32, max_history=64, dim=16, num_edges=20000,
         seed=0, lr=1e-3, verbose=True):
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
    K = num_tokens
    model = GraphMixer(dim, dim, dim_time=dim, dim_embed=dim, num_tokens=K).to(dev)
    optimizer = torch.optim.Adam(model.parameters(), lr=lr)
    criterion = gnnflow_amd.LinkLoss()
    metrics = gnnflow_amd.LinkMetrics(dev)

    rows = min(num_batches * batch_size, len(df))
    first = len(df) - rows      # the last rows of the stream; their history is what came before
    batches = []
    for lo in range(first, len(df), batch_size):
        part = df.iloc[lo:lo + batch_size]
        src = torch.from_numpy(part["src"].to_numpy().astype(np.int64)).to(dev)
        dst = torch.from_numpy(part["dst"].to_numpy().astype(np.int64)).to(dev)
        t = torch.from_numpy(part["time"].to_numpy().astype(np.float32)).to(dev)
        neg = dsts[torch.randint(0, len(dsts), (len(src),), device=dev)]
        roots, ts = torch.cat([src, dst, neg]), t.repeat(3)

        seq = graph.neighbor_sequence(roots, ts, length=K, edge_feats=edge_feats,
                                      time_encoder=model.time_enc)
        lengths, delta_t = seq.lengths, seq.delta_t
        edge_x = seq.tokens[..., :dim]                            # a view: the tokens' edge part
        agg = graph.neighbor_aggregate(roots, ts, node_feats=node_feats, max_history=max_history)

        pred_pos, pred_neg = model.forward_tokens(seq.tokens, node_feats[roots], agg.node)
        loss = criterion(pred_pos, pred_neg)
        optimizer.zero_grad()
        loss.backward()
        optimizer.step()
        metrics.update(pred_pos, pred_neg)
        batches.append({"edge_x": tuple(edge_x.shape), "delta_t": tuple(delta_t.shape),
                        "nbr_mean": tuple(agg.node.shape), "pred_pos": tuple(pred_pos.shape),
                        "pred_neg": tuple(pred_neg.shape), "loss": loss.detach(),
                        "mean_tokens": lengths.double().mean(),
                        "mean_history": agg.count.double().mean()})
    result = {"loss": criterion.compute(), "metrics": metrics.compute(), "batches": batches}
    for b in batches:                                              # after the syncs above
        for key in ("loss", "mean_tokens", "mean_history"):
            b[key] = float(b[key])
    if verbose:
        for i, b in enumerate(batches):
            print("batch {}: loss {:.4f}; {:.1f} of {} tokens, {:.1f} of {} history edges per "
                  "root".format(i, b["loss"], b["mean_tokens"], K, b["mean_history"],
                                max_history))
        m = result["metrics"]
        print("GraphMixer, {} steps: mean loss {:.4f}, ap {:.4f} auc {:.4f} mrr {:.4f}".format(
            len(batches), result["loss"]["mean_loss"], m["ap"], m["auc"], m["mrr"]))
    return result


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=5)
    ap.add_argument("--batch-size", type=int, default=200)
    ap.add_argument("--tokens", type=int, default=32)
    ap.add_argument("--history", type=int, default=64)
    ap.add_argument("--dim", type=int, default=16)
    ap.add_argument("--edges", type=int, default=20000)
    a = ap.parse_args()
    main(a.batches, a.batch_size, a.tokens, a.history, a.dim, a.edges)
