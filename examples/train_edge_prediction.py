"""Minimal offline edge-prediction loop in the shape of the reference's
scripts/offline_edge_prediction.py, on this package only: batches from
`gnnflow_amd.data`, neighbourhoods from `TemporalSampler`, features through `LRUCache`, and one
of the reference's static models, the 2-layer `gnnflow_amd.models.SAGE` (GraphSAGE) or
`gnnflow_amd.models.GAT`.  Synthetic REDDIT-shaped data; a usage example, not a benchmark.

    python examples/train_edge_prediction.py [--batches 50] [--model {sage,gat}] [--amp]
                                             [--fused-loss] [--device-batches]

--amp runs the forward and the loss under torch.autocast('cuda', dtype=torch.bfloat16).  No
GradScaler: bfloat16 has float32's range.  The models need no cast for it: the block ops take
the bfloat16 rows autocast produces (as models.DGNN does, examples/tgn_epoch.py --amp).

--fused-loss takes gnnflow_amd.nn.LinkLoss as the criterion: one ops.link_loss launch each way
instead of torch's two BCE-with-logits expressions, the epoch's sums kept on the device, and no
float(loss) per batch -- the losses are read once, after the loop.

--device-batches takes the batches from a gnnflow_amd.DeviceBatchStream instead of the
DataLoader: the edge stream and the destination set live in HBM, every batch is one kernel
launch, and no numpy array reaches the sampler.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch
import torch.nn.functional as F
from torch.utils.data import DataLoader, SequentialSampler

import gnnflow_amd
from gnnflow_amd import models, synthetic
from gnnflow_amd.cache import LRUCache
from gnnflow_amd.data import (EdgePredictionDataset, RandomStartBatchSampler,
                              default_collate_ndarray)
from gnnflow_amd.utils import DstRandEdgeSampler, build_dynamic_graph


def build_model(name, dim_in, dim_hidden):
    if name == 'sage':
        return models.SAGE(dim_in, dim_hidden, num_layers=2, aggregator='mean')
    if name == 'gat':
        return models.GAT(dim_in, dim_hidden, num_layers=2, attn_head=[2, 1])
    raise ValueError("model must be 'sage' or 'gat', got {!r}".format(name))


def main(num_batches=50, batch_size=600, seed=0, verbose=True, amp=False, model='sage',
         fused_loss=False, device_batches=False):
    import pandas as pd
    torch.manual_seed(seed)
    dev = torch.device("cuda", 0)
    g = synthetic.reddit_like(seed=42, num_edges=60000)
    df = pd.DataFrame({"src": g["src"], "dst": g["dst"], "time": g["ts"], "eid": g["eid"]})
    graph = build_dynamic_graph(20 << 20, 1000 << 20, "cuda", 62, 1024, "insert",
                                undirected=True, device=0, dataset_df=df)
    sampler = gnnflow_amd.TemporalSampler(graph, fanouts=[10, 10], sample_strategy="recent")
    d = 32
    node_feats = torch.randn(g["num_nodes"], d)
    cache = LRUCache(0.0, 0.2, g["num_nodes"], g["num_edges"], dev, node_feats, None, d, 0)
    cache.init_cache()

    if device_batches:
        dst_set = gnnflow_amd.DeviceDstSet(g["num_nodes"], dev, df["dst"].to_numpy())
        loader = gnnflow_amd.DeviceBatchStream.from_dataframe(df, batch_size, dst_set, seed=seed)
    else:
        ds = EdgePredictionDataset(df, DstRandEdgeSampler(df["dst"].to_numpy(), seed=seed))
        loader = DataLoader(ds, sampler=RandomStartBatchSampler(SequentialSampler(ds), batch_size,
                                                                False),
                            collate_fn=default_collate_ndarray, num_workers=0)
    model = build_model(model, d, 64).to(dev)
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    criterion = gnnflow_amd.nn.LinkLoss() if fused_loss else None
    losses = []      # floats; with fused_loss detached device scalars, read once after the loop
    for i, (roots, ts, eid) in enumerate(loader):
        if i >= num_batches:
            break
        mfgs = sampler.sample(roots, ts)
        cache.fetch_feature(mfgs, eid)
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=amp):
            pos, neg = model(mfgs)
            if fused_loss:
                loss = criterion(pos, neg)
            else:
                loss = F.binary_cross_entropy_with_logits(pos, torch.ones_like(pos)) + \
                    F.binary_cross_entropy_with_logits(neg, torch.zeros_like(neg))
        opt.zero_grad()
        loss.backward()
        opt.step()
        if fused_loss:
            losses.append(loss.detach())      # no sync
            continue
        losses.append(float(loss.detach()))
        if verbose and i % 10 == 0:
            print("batch {:4d} loss {:.4f} node-cache hit ratio {:.3f}".format(
                i, losses[-1], float(cache.cache_node_ratio)))
    if fused_loss and losses:
        epoch = criterion.compute()      # the loop's one sync for the loss
        losses = torch.stack(losses).tolist()
        if verbose:
            print("{} batches: mean loss {:.4f}, edge-weighted {:.4f}, {} non-finite".format(
                epoch["batches"], epoch["mean_loss"], epoch["edge_weighted_loss"],
                epoch["nonfinite"]))
    return losses


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=50)
    ap.add_argument("--amp", action="store_true", help="bfloat16 autocast around forward and loss")
    ap.add_argument("--model", choices=["sage", "gat"], default="sage")
    ap.add_argument("--fused-loss", action="store_true",
                    help="nn.LinkLoss as the criterion, the losses read once after the loop")
    ap.add_argument("--device-batches", action="store_true",
                    help="batches from a DeviceBatchStream: assembled on the GPU, one launch each")
    args = ap.parse_args()
    main(args.batches, amp=args.amp, model=args.model, fused_loss=args.fused_loss,
         device_batches=args.device_batches)
