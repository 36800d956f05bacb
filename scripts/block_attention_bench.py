#!/usr/bin/env python3
"""Fused ops.block_attention against the composed chain of existing ops (q[row], mul-sum,
leaky_relu, ops.edge_softmax, multiply, zero-pad, ops.block_reduce), forward and
forward + backward, interleaved in one process and timed with device events.

    python scripts/block_attention_bench.py --shape epoch    # 12 000 destinations, ~29 k edges
    python scripts/block_attention_bench.py --shape dense    # 6 600 destinations, fanout 10

Each of the four variants is timed in `--rounds` rounds that alternate between the variants;
a round runs enough iterations for at least `--min-seconds / --rounds` of device time, so every
variant's timed region is at least --min-seconds.  Prints one JSON line: the median round of
each variant in microseconds per iteration, and the fused kernels' mandatory bytes / time.

    python scripts/block_attention_bench.py --shape epoch --dropout 0.2

With --dropout P > 0 the fused variants pass dropout_p=P and a fresh seed per call, the composed
variants put F.dropout(att, P) between edge_softmax and the multiply, and two more variants time
the fused op WITHOUT dropout in the same interleaved rounds, so that the line also carries the
dropout kernels' time as a fraction of the plain kernels' time and the composed chain's own
round-to-round spread (max - min), the margin a change of the layer's default has to beat.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=["epoch", "dense"], default="epoch")
    ap.add_argument("--heads", type=int, default=2)
    ap.add_argument("--head-dim", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--min-seconds", type=float, default=0.5)
    ap.add_argument("--dropout", type=float, default=0.0,
                    help="attention dropout probability (0: none, the original four variants)")
    a = ap.parse_args()
    import torch
    import torch.nn.functional as F
    from gnnflow_amd import MFGBlock, ops

    rng = np.random.RandomState(0)
    if a.shape == "epoch":      # 12 000 roots, fanout 10, mostly short histories
        nd = 12000
        degs = np.minimum(rng.geometric(1 / 3.4, nd) - 1, 10)
    else:
        nd = 6600
        degs = np.full(nd, 10)
    row = np.repeat(np.arange(nd), degs).astype(np.int64)
    E, H, D = len(row), a.heads, a.head_dim
    dev = torch.device("cuda")
    b = MFGBlock(nd + E, nd, torch.arange(nd, nd + E, device=dev), torch.from_numpy(row).to(dev))
    offsets, _, perm = b.segments()
    assert perm is None
    b._segments = (offsets, None, None)        # the sampler's col-less layout, as its blocks have
    q = torch.randn(nd, H, D, device=dev, requires_grad=True)
    k = torch.randn(E, H, D, device=dev, requires_grad=True)
    v = torch.randn(E, H, D, device=dev, requires_grad=True)
    gout = torch.randn(nd, H, D, device=dev)
    row_t = b.edges()[1]

    P = a.dropout
    seeds = iter(range(1, 1 << 62))

    def plain():
        return ops.block_attention(b, q, k, v)

    def fused():
        if P > 0:
            return ops.block_attention(b, q, k, v, dropout_p=P, dropout_seed=next(seeds))
        return ops.block_attention(b, q, k, v)

    def composed():
        att = ops.edge_softmax(b, F.leaky_relu((q[row_t] * k).sum(2), 0.2))
        if P > 0:
            att = F.dropout(att, P)
        msg = (v * att[:, :, None]).reshape(E, -1)
        pad = torch.cat([torch.zeros((nd, H * D), device=dev), msg])
        return ops.block_reduce(b, pad).view(nd, H, D)

    def fwd(fn):
        with torch.no_grad():
            fn()

    def fwd_bwd(fn):
        q.grad = k.grad = v.grad = None
        fn().backward(gout)

    variants = {"fused_fwd": lambda: fwd(fused), "composed_fwd": lambda: fwd(composed),
                "fused_fwd_bwd": lambda: fwd_bwd(fused), "composed_fwd_bwd": lambda: fwd_bwd(composed)}
    if P > 0:
        variants["plain_fwd"] = lambda: fwd(plain)
        variants["plain_fwd_bwd"] = lambda: fwd_bwd(plain)

    def timed(fn, iters):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(iters):
            fn()
        stop.record()
        stop.synchronize()
        return start.elapsed_time(stop) * 1e-3

    iters = {}
    for name, fn in variants.items():          # warm-up, then size a round
        timed(fn, 20)
        per = timed(fn, 50) / 50
        iters[name] = max(50, int(np.ceil(1.3 * a.min_seconds / a.rounds / per)))   # 30 % margin
    rounds = {name: [] for name in variants}
    for _ in range(a.rounds):
        for name, fn in variants.items():
            rounds[name].append(timed(fn, iters[name]) / iters[name])
    us = {name: float(np.median(r)) * 1e6 for name, r in rounds.items()}
    # mandatory traffic of the fused kernels (fp32): forward reads q, k, v and writes out, att;
    # backward reads q, k, v (v twice), att, gout and writes gq, gk, gv
    fwd_bytes = 4 * (2 * nd * H * D + 2 * E * H * D + E * H)
    bwd_bytes = 4 * (3 * nd * H * D + 5 * E * H * D + E * H)
    out = {"bench": "block_attention", "shape": a.shape, "num_dst": nd, "num_edges": E,
           "heads": H, "head_dim": D, "rounds": a.rounds, "iters_per_round": iters,
           "timed_seconds": {n: float(np.sum(r)) * iters[n] for n, r in rounds.items()},
           "us_per_iter_median": {n: round(x, 2) for n, x in us.items()},
           "us_per_iter_min_max": {n: [round(min(r) * 1e6, 2), round(max(r) * 1e6, 2)]
                                   for n, r in rounds.items()},
           "speedup_fwd": round(us["composed_fwd"] / us["fused_fwd"], 3),
           "speedup_fwd_bwd": round(us["composed_fwd_bwd"] / us["fused_fwd_bwd"], 3),
           "fused_fwd_GBps": round(fwd_bytes / us["fused_fwd"] * 1e-3, 1),
           "fused_fwd_bwd_GBps": round((fwd_bytes + bwd_bytes) / us["fused_fwd_bwd"] * 1e-3, 1),
           "note": "us_per_iter includes host launch overhead of each path (wall time between "
                   "device events); GB/s = mandatory bytes / that time",
           "device": torch.cuda.get_device_name(0)}
    if P > 0:
        spread = (max(rounds["composed_fwd_bwd"]) - min(rounds["composed_fwd_bwd"])) * 1e6
        out.update({
            "dropout": P,
            "composed_fwd_bwd_spread_us": round(spread, 2),
            "fused_fwd_bwd_margin_us": round(us["composed_fwd_bwd"] - us["fused_fwd_bwd"], 2),
            "fused_beats_composed_by_more_than_spread":
                bool(us["composed_fwd_bwd"] - us["fused_fwd_bwd"] > spread),
            "dropout_over_plain_fwd": round(us["fused_fwd"] / us["plain_fwd"], 3),
            "dropout_over_plain_fwd_bwd": round(us["fused_fwd_bwd"] / us["plain_fwd_bwd"], 3)})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
