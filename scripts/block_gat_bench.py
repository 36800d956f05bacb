#!/usr/bin/env python3
"""Fused ops.block_gat against the composed chain of nn.GATConv.forward (el[col] + er[row],
leaky_relu, ops.edge_softmax, attn_drop, ops.block_reduce), forward + backward, interleaved in
one process and timed with device events.

    python scripts/block_gat_bench.py                   # heads 8 and 1, head width 100
    python scripts/block_gat_bench.py --dropout 0.2

The blocks are the sampler's own: both layers' blocks of one late batch (600 positive edges: 1800
roots) of the REDDIT-shaped replay, fanout [10, 10], most recent.  Per (layer, heads) shape, the
variants are timed in `--rounds` rounds that alternate between them; a round runs enough
iterations for at least `--min-seconds / --rounds` of device time.  With --dropout P > 0 the
fused variant passes dropout_p=P and a fresh seed per call and the composed one puts
F.dropout(att, P) between edge_softmax and block_reduce.  Prints one JSON line per shape and
appends it to profiles/block_gat_bench.jsonl: the median round of each variant in microseconds
per iteration, the composed chain's own round-to-round spread (max - min), and whether the fused
side wins by more than that spread -- the rule for the defaults of nn.GATConv.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def sampler_blocks(batch):
    import torch
    import gnnflow_amd
    from gnnflow_amd import synthetic
    g = synthetic.reddit_like(seed=42)
    MiB = 1 << 20
    graph = gnnflow_amd.DynamicGraph(20 * MiB, 1000 * MiB, "cuda", 62, 1024, "insert")
    for lo in range(0, g["num_edges"], 100000):
        hi = lo + 100000
        graph.add_edges(g["src"][lo:hi], g["dst"][lo:hi], g["ts"][lo:hi], g["eid"][lo:hi])
    sampler = gnnflow_amd.TemporalSampler(graph, [10, 10], "recent", seed=1234)
    batches = list(synthetic.replay_batches(g, batch, seed=42))
    r, t, _ = batches[-2]                       # a late, full batch: long histories
    dev = torch.device("cuda", 0)
    mfgs = sampler.sample(torch.from_numpy(r).to(dev), torch.from_numpy(t).to(dev))
    return [(li, b) for li, layer in enumerate(mfgs) for b in layer], graph, sampler, mfgs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=600)
    ap.add_argument("--heads", type=int, nargs="+", default=[8, 1])
    ap.add_argument("--head-dim", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--min-seconds", type=float, default=0.5)
    ap.add_argument("--dropout", type=float, default=0.0,
                    help="attention dropout probability (0: none)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "block_gat_bench.jsonl"))
    a = ap.parse_args()
    import torch
    import torch.nn.functional as F
    from gnnflow_amd import ops

    blocks, *keep = sampler_blocks(a.batch)
    dev = torch.device("cuda", 0)
    P, D = a.dropout, a.head_dim
    seeds = iter(range(1, 1 << 62))

    def timed(fn, iters):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(iters):
            fn()
        stop.record()
        stop.synchronize()
        return start.elapsed_time(stop) * 1e-3

    for li, b in blocks:
        assert b.segments()[1] is None and b.segments()[2] is None      # the sampler's layout
        nd, ns, E = b.num_dst_nodes(), b.num_src_nodes(), b.num_edges()
        col, row = b.edges()
        for H in a.heads:
            feat = torch.randn(ns, H, D, device=dev, requires_grad=True)
            el = torch.randn(ns, H, device=dev, requires_grad=True)
            er = torch.randn(nd, H, device=dev, requires_grad=True)
            gout = torch.randn(nd, H, D, device=dev)

            def fused():
                if P > 0:
                    return ops.block_gat(b, feat, el, er, dropout_p=P, dropout_seed=next(seeds))
                return ops.block_gat(b, feat, el, er)

            def composed():
                att = ops.edge_softmax(b, F.leaky_relu(el[col] + er[row], 0.2))
                if P > 0:
                    att = F.dropout(att, P)
                return ops.block_reduce(b, feat, att)

            def fwd_bwd(fn):
                feat.grad = el.grad = er.grad = None
                fn().backward(gout)

            variants = {"fused_fwd_bwd": lambda: fwd_bwd(fused),
                        "composed_fwd_bwd": lambda: fwd_bwd(composed)}
            iters = {}
            for name, fn in variants.items():          # warm-up, then size a round
                timed(fn, 20)
                per = timed(fn, 50) / 50
                iters[name] = max(50, int(np.ceil(1.3 * a.min_seconds / a.rounds / per)))
            rounds = {name: [] for name in variants}
            for _ in range(a.rounds):
                for name, fn in variants.items():
                    rounds[name].append(timed(fn, iters[name]) / iters[name])
            us = {name: float(np.median(r)) * 1e6 for name, r in rounds.items()}
            spread = (max(rounds["composed_fwd_bwd"]) - min(rounds["composed_fwd_bwd"])) * 1e6
            margin = us["composed_fwd_bwd"] - us["fused_fwd_bwd"]
            # what the two fused kernels must move (fp32): forward reads feat, el, er, writes out
            # and att; backward reads feat, el, er, att, out, gout, writes gfeat, gel, ger
            nbytes = 4 * (3 * ns * H * D + 3 * nd * H * D + 4 * ns * H + 3 * nd * H + 3 * E * H)
            out = {"bench": "block_gat", "layer": li, "num_dst": nd, "num_src": ns,
                   "num_edges": E, "heads": H, "head_dim": D, "dropout": P, "batch": a.batch,
                   "rounds": a.rounds, "iters_per_round": iters,
                   "timed_seconds": {n: float(np.sum(r)) * iters[n] for n, r in rounds.items()},
                   "us_per_iter_median": {n: round(x, 2) for n, x in us.items()},
                   "us_per_iter_min_max": {n: [round(min(r) * 1e6, 2), round(max(r) * 1e6, 2)]
                                           for n, r in rounds.items()},
                   "speedup_fwd_bwd": round(us["composed_fwd_bwd"] / us["fused_fwd_bwd"], 3),
                   "composed_fwd_bwd_spread_us": round(spread, 2),
                   "fused_fwd_bwd_margin_us": round(margin, 2),
                   "fused_beats_composed_by_more_than_spread": bool(margin > spread),
                   "fused_fwd_bwd_GBps": round(nbytes / us["fused_fwd_bwd"] * 1e-3, 1),
                   "note": "us_per_iter includes host launch overhead of each path (wall time "
                           "between device events); GB/s = mandatory bytes / that time",
                   "device": torch.cuda.get_device_name(0)}
            line = json.dumps(out)
            print(line, flush=True)
            with open(a.out, "a") as f:
                f.write(line + "\n")
    del keep


if __name__ == "__main__":
    main()
