"""Full ranking with `EdgePredictor.rank`: for a batch of sources, which of C candidate nodes is
each most likely to connect to next, and where does its true destination rank among all of them
(filtered MRR and Hits@10, the protocol of the temporal link-prediction benchmarks)?

The embeddings of the batch's sources and of the candidate set come from one forward of an
untrained TGAT-shaped `models.DGNN` with `return_embed=True`; `edge_predictor.rank` then scores
every source against every candidate in one streaming kernel (ops.edge_rank) without the
[B * C, D] rows a paired edge_score would need.  Synthetic data; a usage example, not a
benchmark.

With --filter-seen the nodes a source has already interacted with before its query time are left
out of its ranking: `graph.seen_mask(src, ts, cand)` reads them from the temporal edge store on the
GPU as one bit per (source, candidate), and `rank(..., exclude=mask)` skips them in the same
kernel.  The target is then ranked among the candidates that are not known positives of its source
(the filtered setting), and the top 5 holds only nodes that would be new to the source.

    python examples/recommend_edges.py [--batch 200] [--candidates 2000] [--filter-seen]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

import gnnflow_amd
from gnnflow_amd import synthetic
from gnnflow_amd.cache import LRUCache
from gnnflow_amd.models import DGNN
from gnnflow_amd.utils import build_dynamic_graph


def main(batch_size=200, num_candidates=2000, num_edges=20000, seed=0, verbose=True,
         filter_seen=False):
    import pandas as pd
    torch.manual_seed(seed)
    dev = torch.device("cuda", 0)
    g = synthetic.reddit_like(seed=42, num_edges=num_edges)
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
    model = DGNN(dim_node, dim_edge, 16, 32, 2, 1, 2, 0.1, 0.1, False).to(dev).eval()

    # the last edges of the stream are the queries; the candidates are their true destinations
    # and other destination nodes, embedded at the time of the latest query
    B = min(batch_size, len(df))
    src = df["src"].to_numpy()[-B:]
    dst = df["dst"].to_numpy()[-B:]
    ts = df["time"].to_numpy()[-B:].astype(np.float32)
    pool = np.unique(df["dst"].to_numpy())
    rng = np.random.RandomState(seed)
    extra = rng.choice(pool, size=min(len(pool), max(num_candidates - len(np.unique(dst)), 0)),
                       replace=False)
    cand = np.unique(np.concatenate([dst, extra]))      # sorted
    target = torch.from_numpy(np.searchsorted(cand, dst)).to(dev)
    roots = np.concatenate([src, cand])
    times = np.concatenate([ts, np.full(len(cand), ts.max(), np.float32)])

    with torch.no_grad():
        mfgs = sampler.sample(roots, times)
        cache.fetch_feature(mfgs)
        embed = model(mfgs, return_embed=True)
        k = min(10, len(cand))
        out = model.edge_predictor.rank(embed[:B], embed[B:], k=k, target=target)
        if filter_seen:
            mask = graph.seen_mask(torch.from_numpy(src.astype(np.int64)).to(dev),
                                   torch.from_numpy(ts).to(dev),
                                   torch.from_numpy(cand.astype(np.int64)).to(dev))
            unfiltered = out
            out = model.edge_predictor.rank(embed[:B], embed[B:], k=k, target=target,
                                            exclude=mask)
    rank = out.rank
    result = {
        "mrr": float((1.0 / rank).mean()),
        "hits@10": float((rank <= 10).double().mean()),
        "top5": [int(cand[i]) for i in out.indices[0, :5].tolist() if i >= 0],
        "top5_index": [i for i in out.indices[0, :5].tolist() if i >= 0],
        "num_candidates": int(len(cand)),
    }
    if filter_seen:
        result["source"], result["time"] = int(src[0]), float(ts[0])
        result["unfiltered_mrr"] = float((1.0 / unfiltered.rank).mean())
        result["unfiltered_hits@10"] = float((unfiltered.rank <= 10).double().mean())
        ids = torch.arange(len(cand), device=dev)
        result["seen_share"] = float(((mask[:, ids >> 6] >> (ids & 63)) & 1).double().mean())
    if verbose:
        if filter_seen:
            print("{} sources against {} candidates, unfiltered: MRR {:.4f}  Hits@10 {:.4f}".format(
                B, len(cand), result["unfiltered_mrr"], result["unfiltered_hits@10"]))
            print("without the {:.1%} of the pairs that have already interacted:".format(
                result["seen_share"]))
        print("{} sources against {} candidates: MRR {:.4f}  Hits@10 {:.4f}".format(
            B, len(cand), result["mrr"], result["hits@10"]))
        print("source {}: top 5 nodes {} (true destination {} left out, rank {:.1f})".format(
            int(src[0]), result["top5"], int(dst[0]), float(rank[0])))
    return result


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=200)
    ap.add_argument("--candidates", type=int, default=2000)
    ap.add_argument("--filter-seen", action="store_true",
                    help="leave the nodes a source has already met out of its ranking")
    a = ap.parse_args()
    main(a.batch, a.candidates, filter_seen=a.filter_seen)
