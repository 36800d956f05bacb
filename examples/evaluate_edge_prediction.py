"""The reference's evaluate() loop (scripts/offline_edge_prediction.py:102-152) on this package
only: batches from `gnnflow_amd.data`, neighbourhoods from `TemporalSampler`, features through
`LRUCache`, the model `gnnflow_amd.models.DGNN` in its TGAT configuration, and the metrics from
`gnnflow_amd.LinkMetrics` instead of `.sigmoid().cpu()` plus scikit-learn: nothing waits for the
GPU until the one `compute()` at the end.  Synthetic REDDIT-shaped data and an untrained model
by default; a usage example, not a benchmark.

    python examples/evaluate_edge_prediction.py [--batches 20] [--train-batches 0]
                                                [--hist-negatives N] [--edge-bank]
                                                [--neighbor-overlap SCORE]

--hist-negatives N takes the validation batches from a `gnnflow_amd.DeviceBatchStream` with N
negatives per edge, all of them historical where the source has a history (`hist_ratio=N`:
destinations the source interacted with before the edge's time, drawn on the GPU from the
graph's edge store), and prints the share of negative slots that hold one.  The graph is built
with reverse edges, so a source's history includes the nodes that pointed at it.

--edge-bank scores the same batches, negatives included, with `gnnflow_amd.EdgeBank` as well
("the pair has interacted strictly before the edge's time", read from the graph's edge store by
`graph.pair_history`) and prints the baseline's AP / AUC / MRR beside the model's.

--neighbor-overlap SCORE (cn, jaccard, aa, ra or pa) does the same with
`gnnflow_amd.NeighborOverlap`: the overlap of the two ends' temporal neighbourhoods strictly
before the edge's time, read by `graph.common_neighbors`.
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


def scores(model, mfgs, neg_ratio):
    """(pred_pos [B, 1], pred_neg [K * B, 1], k-major) of roots laid out [src | dst | K negative
    planes].  The model's edge predictor takes one negative per edge: with K > 1 it scores the
    embeddings once per negative plane."""
    if neg_ratio == 1:
        return model(mfgs)
    h = model(mfgs, return_embed=True)
    B = h.shape[0] // (2 + neg_ratio)
    planes = [model.edge_predictor(torch.cat([h[:2 * B], h[(2 + k) * B:(3 + k) * B]]))
              for k in range(neg_ratio)]
    return planes[0][0], torch.cat([neg for _, neg in planes])


def evaluate(loader, sampler, model, cache, metrics, num_batches, neg_ratio=1, bank=None,
             bank_metrics=None, overlap=None, overlap_metrics=None):
    """One validation pass: returns (ap, auc) as the reference does, and leaves the other
    fields in `metrics`.  With `bank` (an EdgeBank) every batch is scored by it too, into
    `bank_metrics`; with `overlap` (a NeighborOverlap) likewise into `overlap_metrics`."""
    model.eval()
    metrics.reset()
    with torch.no_grad():
        for i, (roots, ts, eid) in enumerate(loader):
            if i >= num_batches:
                break
            mfgs = sampler.sample(roots, ts)
            cache.fetch_feature(mfgs, eid)
            pred_pos, pred_neg = scores(model, mfgs, neg_ratio)
            metrics.update(pred_pos, pred_neg)      # sigmoid, then AP / AUC / MRR; no sync
            if bank is not None:
                bank_metrics.update(*bank.predict(roots, ts, neg_ratio), sigmoid=False)
            if overlap is not None:
                overlap_metrics.update(*overlap.predict(roots, ts, neg_ratio), sigmoid=False)
    result = metrics.compute()                      # the one sync of the pass
    return result["ap"], result["auc"]


def main(num_batches=20, batch_size=600, train_batches=0, seed=0, verbose=True,
         hist_negatives=0, edge_bank=False, neighbor_overlap=None):
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
    if hist_negatives:
        dst_set = gnnflow_amd.DeviceDstSet(g["num_nodes"], dev, df["dst"].to_numpy())
        # the rows of the pass only, so that the counter below is over exactly its batches
        loader = gnnflow_amd.DeviceBatchStream.from_dataframe(
            df.iloc[:num_batches * batch_size], batch_size, dst_set, neg_ratio=hist_negatives,
            seed=seed, graph=graph, hist_ratio=hist_negatives)
    bank = gnnflow_amd.EdgeBank(graph) if edge_bank else None
    bank_metrics = gnnflow_amd.LinkMetrics(dev) if edge_bank else None
    overlap = gnnflow_amd.NeighborOverlap(graph, neighbor_overlap) if neighbor_overlap else None
    overlap_metrics = gnnflow_amd.LinkMetrics(dev) if neighbor_overlap else None
    ap, auc = evaluate(loader, sampler, model, cache, metrics, num_batches,
                       neg_ratio=hist_negatives or 1, bank=bank, bank_metrics=bank_metrics,
                       overlap=overlap, overlap_metrics=overlap_metrics)
    result = metrics.compute()
    if edge_bank:
        result["edge_bank"] = bank_metrics.compute()
    if neighbor_overlap:
        result["neighbor_overlap"] = overlap_metrics.compute()
    if hist_negatives:
        # read once per pass, like the metrics
        slots = int(loader.borders[-1] - loader.borders[0]) * hist_negatives
        result["hist_share"] = int(loader.hist_filled.item()) / max(slots, 1)
    if verbose:
        print("ap {:.4f} auc {:.4f} mrr {:.4f} over {} batches ({} left out as non-finite)".format(
            ap, auc, result["mrr"], result["batches"], result["nonfinite"]) +
            (" historical negatives {:.1%} of {} per edge".format(
                result["hist_share"], hist_negatives) if hist_negatives else ""))
        if edge_bank:
            print("EdgeBank (unlimited memory) on the same batches: ap {:.4f} auc {:.4f} "
                  "mrr {:.4f}".format(result["edge_bank"]["ap"], result["edge_bank"]["auc"],
                                      result["edge_bank"]["mrr"]))
        if neighbor_overlap:
            r = result["neighbor_overlap"]
            print("NeighborOverlap ({}, the newest {} edges of each end) on the same batches: "
                  "ap {:.4f} auc {:.4f} mrr {:.4f}".format(neighbor_overlap, overlap.max_history,
                                                           r["ap"], r["auc"], r["mrr"]))
    return result


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=20)
    ap.add_argument("--train-batches", type=int, default=0)
    ap.add_argument("--hist-negatives", type=int, default=0,
                    help="N historical negatives per edge from a DeviceBatchStream (0: the "
                         "host loader's one random negative)")
    ap.add_argument("--edge-bank", action="store_true",
                    help="print the EdgeBank baseline's metrics on the same batches as well")
    ap.add_argument("--neighbor-overlap", default=None, metavar="SCORE",
                    choices=["cn", "jaccard", "aa", "ra", "pa"],
                    help="print a NeighborOverlap baseline's metrics on the same batches as well")
    a = ap.parse_args()
    main(a.batches, train_batches=a.train_batches, hist_negatives=a.hist_negatives,
         edge_bank=a.edge_bank, neighbor_overlap=a.neighbor_overlap)
