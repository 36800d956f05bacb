"""Temporal random walks and their anonymous encoding for the (src, dst) pairs of one batch: what
a CAWN-style link predictor feeds to its networks.

For every edge (u, v, t) of the batch, `graph.temporal_random_walk` walks W times L steps
backward in time from u and from v, starting at t (one kernel, a lane per walk, on the temporal
edge store).  `ops.walk_position_counts` then encodes every node met on the way by how often it
stands at each position of the walks of its own side and of the partner's side: two calls per
side, four small integer tensors per pair, and no node id reaches the model.  Synthetic data; a
usage example, not a benchmark.

    python examples/temporal_walks.py [--batch 200] [--walks 16] [--length 3] [--recency 2]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

from gnnflow_amd import ops, synthetic
from gnnflow_amd.utils import build_dynamic_graph


def main(batch_size=200, num_walks=16, length=3, recency=2, max_history=0, num_edges=20000,
         seed=0, verbose=True):
    import pandas as pd
    dev = torch.device("cuda", 0)
    g = synthetic.reddit_like(seed=42, num_edges=num_edges)
    df = pd.DataFrame({"src": g["src"], "dst": g["dst"], "time": g["ts"], "eid": g["eid"]})
    graph = build_dynamic_graph(20 << 20, 1000 << 20, "cuda", 62, 1024, "insert",
                                undirected=True, device=0, dataset_df=df)

    # the last edges of the stream are the batch
    B = min(batch_size, len(df))
    first_row = len(df) - B
    src = torch.from_numpy(df["src"].to_numpy()[-B:].astype(np.int64)).to(dev)
    dst = torch.from_numpy(df["dst"].to_numpy()[-B:].astype(np.int64)).to(dev)
    ts = torch.from_numpy(df["time"].to_numpy()[-B:].astype(np.float32)).to(dev)

    # the two sides draw under seeds of their own; the key is the edge's row in the stream, so
    # another batching of the same stream walks the same walks
    kw = dict(recency=recency, max_history=max_history, first_row=first_row)
    wu = graph.temporal_random_walk(src, ts, length, num_walks, seed=2 * seed, **kw)
    wv = graph.temporal_random_walk(dst, ts, length, num_walks, seed=2 * seed + 1, **kw)
    enc = {"u|u": ops.walk_position_counts(wu.nodes),
           "u|v": ops.walk_position_counts(wu.nodes, wv.nodes),
           "v|v": ops.walk_position_counts(wv.nodes),
           "v|u": ops.walk_position_counts(wv.nodes, wu.nodes)}
    steps = (wu.eids >= 0).sum(-1)
    result = {"nodes": tuple(wu.nodes.shape), "eids": tuple(wu.eids.shape),
              "times": tuple(wu.times.shape), "encoding": tuple(enc["u|v"].shape),
              "mean_steps": float(steps.double().mean()),
              "full_length_share": float((steps == length).double().mean()),
              "common_share": float((enc["u|v"].sum(-1) > 0).double().mean())}
    if verbose:
        print("{} edges, {} walks of {} steps from each end (recency {}):".format(
            B, num_walks, length, recency))
        print("  nodes {}  eids {}  times {}  encoding {} x 4".format(
            result["nodes"], result["eids"], result["times"], result["encoding"]))
        print("  {:.2f} steps per walk, {:.1%} reach full length; {:.1%} of u's walk entries are "
              "nodes v's walks meet too".format(result["mean_steps"], result["full_length_share"],
                                                 result["common_share"]))
        i, w = (int(x) for x in (steps == steps.max()).nonzero()[0])      # the first longest walk
        print("  edge ({}, {}) at t = {:.1f}, walk {} from its source:".format(
            int(src[i]), int(dst[i]), float(ts[i]), w))
        t = float(ts[i])
        for j in range(length + 1):
            node = int(wu.nodes[i, w, j])
            if node < 0:
                print("    step {}: the walk has ended".format(j))
                break
            if j:
                t = float(wu.times[i, w, j - 1])
            print("    {} node {:6d}  t = {:10.1f}{}  own counts {}  partner's counts {}".format(
                "root" if j == 0 else "step", node, t,
                "" if j == 0 else "  edge {:6d}".format(int(wu.eids[i, w, j - 1])),
                enc["u|u"][i, w, j].tolist(), enc["u|v"][i, w, j].tolist()))
    return result, wu, wv, enc


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=200)
    ap.add_argument("--walks", type=int, default=16)
    ap.add_argument("--length", type=int, default=3)
    ap.add_argument("--recency", type=int, default=2)
    ap.add_argument("--max-history", type=int, default=0)
    a = ap.parse_args()
    main(a.batch, a.walks, a.length, a.recency, a.max_history)
