"""The reference's evaluate() loop (scripts/offline_edge_prediction.py:102-152) on this package
only: batches from `gnnflow_amd.data`, neighbourhoods from `TemporalSampler`, features through
`LRUCache`, the model `gnnflow_amd.models.DGNN` in its TGAT configuration, and the metrics from
`gnnflow_amd.LinkMetrics` instead of `.sigmoid().cpu()` plus scikit-learn: nothing waits for the
GPU until the one `compute()` at the end.  Synthetic REDDIT-shaped data and an untrained model
by default; a usage example, not a benchmark.

    python examples/evaluate_edge_prediction.py [--batches 20] [--train-batches 0]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch
import torch.nn.functional as F
from torch.utils.data import DataLoader, SequentialSampler

import gnnflow_amd
from gnnflow_amd import synthetic
from gnnflow_amd.cache import LRUCache
from gnnflow_amd.data import (EdgePredictionDataset, RandomStartBatchSampler,
                              default_collate_ndarray)
from gnnflow_amd.models import DGNN
from gnnflow_amd.utils import DstRandEdgeSampler, build_dynamic_graph


def evaluate(loader, sampler, model, cache, metrics, num_batches):
    """One validation pass: returns (ap, auc) as the reference does, and leaves the other
    fields in `metrics`."""
    model.eval()
    metrics.reset()
    with torch.no_grad():
        for i, (roots, ts, eid) in enumerate(loader):
            if i >= num_batches:
                break
            mfgs = sampler.sample(roots, ts)
            cache.fetch_feature(mfgs, eid)
            pred_pos, pred_neg = model(mfgs)
            metrics.update(pred_pos, pred_neg)      # sigmoid, then AP / AUC / MRR; no sync
    result = metrics.compute()                      # the one sync of the pass
    return result["ap"], result["auc"]


def main(num_batches=20, batch_size=600, train_batches=0, seed=0, verbose=True):
    import pandas as pd
    torch.manual_seed(seed)
    dev = torch.device("cuda", 0)
    g = synthetic.reddit_like(seed=42, num_edges=60000)
    df = pd.DataFrame({"src": g["src"], "dst": g["dst"], "time": g["ts"], "eid": g["eid"]})
    graph = build_dynamic_graph(20 << 20, 1000 << 20, "cuda", 62, 1024, "insert",
                                undirected=True, device=0, dataset_df=df)
    sampler = gnnflow_amd.TemporalSampler(graph, fanouts=[10, 10], sample_strategy="recent")
    dim_node, dim_edge = 32, 16
    node_feats = torch.randn(g["num_nodes"], dim_node)
    edge_feats = torch.randn(g["num_edges"], dim_edge)
    cache = LRUCache(0.2, 0.2, g["num_nodes"], g["num_edges"], dev, node_feats, edge_feats,
                     dim_node, dim_edge)
    cache.init_cache()

    ds = EdgePredictionDataset(df, DstRandEdgeSampler(df["dst"].to_numpy(), seed=seed))
    loader = DataLoader(ds, sampler=RandomStartBatchSampler(SequentialSampler(ds), batch_size, False),
                        collate_fn=default_collate_ndarray, num_workers=0)
    model = DGNN(dim_node, dim_edge, 16, 32, 2, 1, 2, 0.1, 0.1, False).to(dev)

    if train_batches:
        model.train()
        opt = torch.optim.Adam(model.parameters(), lr=1e-3)
        for i, (roots, ts, eid) in enumerate(loader):
            if i >= train_batches:
                break
            mfgs = sampler.sample(roots, ts)
            cache.fetch_feature(mfgs, eid)
            pos, neg = model(mfgs)
            loss = F.binary_cross_entropy_with_logits(pos, torch.ones_like(pos)) + \
                F.binary_cross_entropy_with_logits(neg, torch.zeros_like(neg))
            opt.zero_grad()
            loss.backward()
            opt.step()

    metrics = gnnflow_amd.LinkMetrics(dev)
    ap, auc = evaluate(loader, sampler, model, cache, metrics, num_batches)
    result = metrics.compute()
    if verbose:
        print("ap {:.4f} auc {:.4f} mrr {:.4f} over {} batches ({} left out as non-finite)".format(
            ap, auc, result["mrr"], result["batches"], result["nonfinite"]))
    return result


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=20)
    ap.add_argument("--train-batches", type=int, default=0)
    a = ap.parse_args()
    main(a.batches, train_batches=a.train_batches)
