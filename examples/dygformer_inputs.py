"""The inputs of a sequence-based temporal link predictor (DyGFormer, GraphMixer) for the batches
of a stream, on this package only.

The whole stream is ingested into the graph once.  For every (src, dst, t) of a batch,
`graph.neighbor_cooccurrence` returns the most recent `--length` interactions of both ends
STRICTLY BEFORE t as two padded sequences (node id, edge id, time; the end itself at position 0)
and, for every element, how often its node occurs in src's sequence and in dst's: one kernel per
batch on the GPU, nothing sampled, nothing deduplicated.  The sequences' node and edge features
come through the LRU feature cache as one block of ids (padding slots fetch row 0 and are zeroed
by `lengths`), the time deltas are t - times, and `nn.NeighborCooccurrenceEncoder` turns the counts
into features: the four tensors DyGFormer concatenates before patching.  The REDDIT-shaped stream
is bipartite, so a user and a community share no neighbour: an element is counted on both sides
there only through the self slots, where the pair itself has interacted before.  `--pair
previous` pairs every source with the row before's instead, two users, which do share
communities.  Synthetic data; a usage example, not a benchmark.

    python examples/dygformer_inputs.py [--batches 5] [--batch-size 200] [--length 32]
                                        [--dim 16] [--pair stream|previous]
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
from gnnflow_amd.utils import build_dynamic_graph


def main(num_batches=5, batch_size=200, length=32, dim=16, pair="stream", num_edges=20000,
         seed=0, verbose=True):
    import pandas as pd
    assert pair in ("stream", "previous")
    dev = torch.device("cuda", 0)
    g = synthetic.reddit_like(seed=42, num_edges=num_edges)
    df = pd.DataFrame({"src": g["src"], "dst": g["dst"], "time": g["ts"], "eid": g["eid"]})
    graph = build_dynamic_graph(20 << 20, 1000 << 20, "cuda", 62, 1024, "insert",
                                undirected=True, device=0, dataset_df=df)
    torch.manual_seed(seed)
    node_feats = torch.randn(g["num_nodes"], dim)
    edge_feats = torch.randn(g["num_edges"], dim)
    cache = LRUCache(0.5, 0.5, g["num_nodes"], g["num_edges"], dev, node_feats, edge_feats, dim,
                     dim)
    cache.init_cache()
    encoder = gnnflow_amd.NeighborCooccurrenceEncoder(dim, max_count=length).to(dev)

    rows = min(num_batches * batch_size, len(df))
    first = len(df) - rows      # the last rows of the stream; their history is what came before
    results = []
    for lo in range(first, len(df), batch_size):
        part = df.iloc[lo:lo + batch_size]
        src = torch.from_numpy(part["src"].to_numpy().astype(np.int64)).to(dev)
        dst = torch.from_numpy(part["dst"].to_numpy().astype(np.int64)).to(dev)
        ts = torch.from_numpy(part["time"].to_numpy().astype(np.float32)).to(dev)
        if pair == "previous":
            dst = src.roll(1)
        seq = graph.neighbor_cooccurrence(src, dst, ts, length=length)
        B, L = len(src), length
        filled = torch.arange(L, device=dev) < seq.lengths.unsqueeze(2)          # [B, 2, L]
        has_edge = seq.eids >= 0                                                 # not the self slot

        # one block of ids through the cache; the -1 slots fetch row 0 and are zeroed below
        block = gnnflow_amd.MFGBlock(2 * B * L, 2 * B * L,
                                     col=torch.empty(0, dtype=torch.int64, device=dev),
                                     row=torch.empty(0, dtype=torch.int64, device=dev),
                                     num_edges=2 * B * L, device=dev)
        block.srcdata["ID"] = seq.nodes.clamp(min=0).reshape(-1)
        block.edata["ID"] = seq.eids.clamp(min=0).reshape(-1)
        cache.fetch_feature([[block]], update_cache=True, target_edge_features=False)
        node_x = block.srcdata["h"].reshape(B, 2, L, dim) * filled.unsqueeze(3)
        edge_x = block.edata["f"].reshape(B, 2, L, dim) * has_edge.unsqueeze(3)
        delta_t = (ts[:, None, None] - seq.times) * filled
        cooc_x = encoder(seq.counts, seq.lengths)

        both = (seq.nodes >= 0) & has_edge & (seq.counts[..., 0] > 0) & (seq.counts[..., 1] > 0)
        r = {"node_x": tuple(node_x.shape), "edge_x": tuple(edge_x.shape),
             "delta_t": tuple(delta_t.shape), "cooc_x": tuple(cooc_x.shape),
             "mean_length": float(seq.lengths.double().mean()),
             "cooccurrence_share": float(both.reshape(B, -1).any(1).double().mean()),
             "finite": bool(torch.isfinite(node_x).all() and torch.isfinite(edge_x).all() and
                            torch.isfinite(cooc_x).all() and torch.isfinite(delta_t).all()),
             "min_delta_t": float(delta_t.min())}
        results.append(r)
        if verbose:
            print("rows {}..{}: node {} edge {} dt {} co-occurrence {}; {:.1f} of {} slots "
                  "filled, {:.1%} of rows have a history element counted on both sides".format(
                      lo, lo + B, r["node_x"], r["edge_x"], r["delta_t"], r["cooc_x"],
                      r["mean_length"], L, r["cooccurrence_share"]))
    return results


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=5)
    ap.add_argument("--batch-size", type=int, default=200)
    ap.add_argument("--length", type=int, default=32)
    ap.add_argument("--dim", type=int, default=16)
    ap.add_argument("--pair", default="stream", choices=("stream", "previous"))
    ap.add_argument("--edges", type=int, default=20000)
    a = ap.parse_args()
    main(a.batches, a.batch_size, a.length, a.dim, a.pair, a.edges)
