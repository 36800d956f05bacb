#!/usr/bin/env python3
"""What DyGFormer's node, edge and time channels cost up to their projections, forward and
backward, for a batch of pairs, one GPU and one process:

  (a) parts:  graph.pair_sequence(src, dst, ts, length=L, node_feats=, edge_feats=,
              time_encoder=enc) -> F.linear(part.reshape(N, 2, L // P, P * d), w, b) for the three
              parts -> backward to the three (w, b)            models.DyGFormer's default route
  (b) fused:  graph.pair_sequence(src, dst, ts, length=L) (planes only) -> ops.patch_project on
              nodes and eids, ops.patch_project_time on delta_t -> the same backward
                                                                DyGFormer(fused_patches=True)'s

for N = (1 + K) * B pairs per call, B = 600 and 4000 edges with K = 1 and 9, L = 32 and 128,
P = 1 and 4, float32 tables of 172 columns, dT = 100, C = 50.

    python scripts/patch_project_bench.py [--edges 240000] [--rounds 7]

scripts/pair_sequence_bench.py's graph, pairs and protocol: (a) and (b) alternate inside every
round; a round of a route is one pass over --batches consecutive batches and ends in
torch.cuda.synchronize().  On the first call of every line the three outputs and the three weight
gradients of (b) are asserted to agree with (a)'s within the sum of both routes' a priori bounds,
2 (n + 2) 2^-24 (|x| |w|^T + |b|) per element (tests/test_gpu_patch_project.py's bound, the
magnitudes from (a)'s parts).  (a) is skipped, and the line says so, where its three parts exceed
--max-intermediate-gb.  One JSON line per (B, K, L, P), appended to
profiles/patch_project_bench.jsonl: the median round in microseconds per call, its min and max,
each route's peak allocated memory over its first call, how (a) compares with (b), and whether
the difference exceeds the rounds' spread.  Host wall time only.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--edges", type=int, default=240000)
    ap.add_argument("--batch", type=int, nargs="+", default=[600, 4000])
    ap.add_argument("--neg-ratio", type=int, nargs="+", default=[1, 9])
    ap.add_argument("--batches", type=int, default=20, help="calls per round")
    ap.add_argument("--length", type=int, nargs="+", default=[32, 128])
    ap.add_argument("--patch", type=int, nargs="+", default=[1, 4])
    ap.add_argument("--dim-node", type=int, default=172)
    ap.add_argument("--dim-edge", type=int, default=172)
    ap.add_argument("--dim-time", type=int, default=100)
    ap.add_argument("--channel-dim", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--max-intermediate-gb", type=float, default=8.0,
                    help="(a) is skipped where its parts exceed this")
    ap.add_argument("--label", default="", help="a name for this run, for the record")
    ap.add_argument("--measured-by", default="", help="who ran this, for the record")
    ap.add_argument("--out",
                    default=os.path.join(ROOT, "profiles", "patch_project_bench.jsonl"))
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import pandas as pd
    import torch
    import torch.nn.functional as F
    if not torch.cuda.is_available():
        sys.exit("patch_project_bench.py needs a GPU")
    from gnnflow_amd import ops, synthetic
    from gnnflow_amd import utils
    from gnnflow_amd.nn import FixedTimeEncode

    dev = torch.device("cuda", 0)
    g = synthetic.reddit_like(seed=42, num_edges=a.edges)
    df = pd.DataFrame({"src": g["src"], "dst": g["dst"], "time": g["ts"], "eid": g["eid"]})
    graph = utils.build_dynamic_graph(20 << 20, 1000 << 20, "cuda", 62, 1024, "insert",
                                      undirected=True, device=0, dataset_df=df)
    torch.manual_seed(0)
    widths = (a.dim_node, a.dim_edge, a.dim_time)
    C = a.channel_dim
    node_table = torch.randn(g["num_nodes"], widths[0], device=dev)
    edge_table = torch.randn(g["num_edges"], widths[1], device=dev)
    enc = FixedTimeEncode(widths[2]).to(dev)
    items = np.unique(df["dst"].to_numpy())
    nb = a.batches

    for B in a.batch:
        rows = slice(len(df) - B * nb, len(df))
        e_src = df["src"].to_numpy()[rows].astype(np.int64)
        e_dst = df["dst"].to_numpy()[rows].astype(np.int64)
        e_ts = df["time"].to_numpy()[rows].astype(np.float32)
        for K in a.neg_ratio:
            rng = np.random.RandomState(1000 * K + B % 1000)
            N = (1 + K) * B
            src = np.concatenate([np.tile(e_src[b * B:(b + 1) * B], 1 + K) for b in range(nb)])
            dst = np.concatenate([np.concatenate([e_dst[b * B:(b + 1) * B],
                                                  rng.choice(items, K * B)]) for b in range(nb)])
            ts = np.concatenate([np.tile(e_ts[b * B:(b + 1) * B], 1 + K) for b in range(nb)])
            d_src, d_dst = torch.from_numpy(src).to(dev), torch.from_numpy(dst).to(dev)
            d_ts = torch.from_numpy(ts).to(dev)
            for L in a.length:
                for P in a.patch:
                    params = [(torch.randn(C, P * d, device=dev).div_((P * d) ** 0.5)
                               .requires_grad_(), torch.randn(C, device=dev).requires_grad_())
                              for d in widths]
                    douts = [torch.randn(N, 2, L // P, C, device=dev) for _ in widths]

                    def parts_call(s, keep=False):
                        seq = graph.pair_sequence(d_src[s], d_dst[s], d_ts[s], length=L,
                                                  node_feats=node_table, edge_feats=edge_table,
                                                  time_encoder=enc)
                        xs = [x.reshape(N, 2, L // P, P * x.shape[3])
                              for x in (seq.node, seq.edge, seq.time)]
                        outs = [F.linear(x, w, b) for x, (w, b) in zip(xs, params)]
                        torch.autograd.backward(outs, douts)
                        return (outs, xs) if keep else None

                    def fused_call(s, keep=False):
                        seq = graph.pair_sequence(d_src[s], d_dst[s], d_ts[s], length=L)
                        (wn, bn), (we, be), (wt, bt) = params
                        outs = [ops.patch_project(seq.nodes, seq.lengths, node_table, wn, bn, P),
                                ops.patch_project(seq.eids, seq.lengths, edge_table, we, be, P),
                                ops.patch_project_time(seq.delta_t, seq.lengths, enc.weight,
                                                       enc.bias, wt, bt, P)]
                        torch.autograd.backward(outs, douts)
                        return outs if keep else None

                    def grads():      # the weight gradients, taken and cleared
                        got = [w.grad for w, _ in params]
                        for w, b in params:
                            w.grad = b.grad = None
                        return got

                    def one_pass(call):
                        for b in range(nb):
                            call(slice(b * N, (b + 1) * N))
                        grads()

                    def timed(fn):
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        fn()
                        torch.cuda.synchronize()
                        return (time.perf_counter() - t0) / nb

                    def peak(call, keep=False):      # (result, peak bytes above what is held)
                        torch.cuda.synchronize()
                        held = torch.cuda.memory_allocated()
                        torch.cuda.reset_peak_memory_stats()
                        got = call(slice(0, N), keep)
                        torch.cuda.synchronize()
                        return got, torch.cuda.max_memory_allocated() - held

                    parts_bytes = N * 2 * L * sum(widths) * 4
                    fits = parts_bytes <= a.max_intermediate_gb * 2 ** 30
                    fused_outs, fused_peak = peak(fused_call, keep=True)
                    fused_grads = grads()
                    parts_peak = None
                    if fits:      # the two routes agree
                        (outs, xs), parts_peak = peak(parts_call, keep=True)
                        M = N * 2 * (L // P)
                        for o, fo, x, (w, b), gw, fgw, dout in zip(outs, fused_outs, xs, params,
                                                                  grads(), fused_grads, douts):
                            n = x.shape[3]
                            with torch.no_grad():
                                bound = F.linear(x.abs(), w.abs(), b.abs()) * (2 * (n + 2) * U)
                                assert ((o - fo).abs() <= bound * 1.001).all()
                                gbound = dout.reshape(M, C).abs().t() @ x.reshape(M, n).abs()
                                gbound *= 2 * (M + 2) * U
                                assert ((gw - fgw).abs() <= gbound * 1.001).all()
                        del outs, xs, bound, gbound
                        timed(lambda: one_pass(parts_call))
                    del fused_outs, fused_grads
                    timed(lambda: one_pass(fused_call))
                    fr, pr = [], []
                    for r in range(a.rounds):
                        fr.append(timed(lambda: one_pass(fused_call)))
                        if fits:
                            pr.append(timed(lambda: one_pass(parts_call)))
                    f_us = float(np.median(fr)) * 1e6
                    f_spread = (max(fr) - min(fr)) * 1e6
                    out = {"bench": "patch_project", "label": a.label, "B": B, "K": K, "N": N,
                           "length": L, "patch": P, "dim_node": widths[0], "dim_edge": widths[1],
                           "dim_time": widths[2], "channel_dim": C, "edges": a.edges,
                           "calls_per_round": nb, "rounds": len(fr),
                           "fused_us_per_call_median": round(f_us, 2),
                           "fused_us_per_call_min_max": [round(min(fr) * 1e6, 2),
                                                         round(max(fr) * 1e6, 2)],
                           "fused_spread_us": round(f_spread, 2),
                           "fused_peak_gb": round(fused_peak / 2 ** 30, 3),
                           "parts_gb": round(parts_bytes / 2 ** 30, 3),
                           "note": "host wall time over one pass of all calls (reader, the three "
                                   "projections, their backward), ending in a device synchronise, "
                                   "divided by the calls; the two routes alternate inside every "
                                   "round; peak memory is the first call's, above what was held",
                           "measured_by": a.measured_by,
                           "device": torch.cuda.get_device_name(0)}
                    if pr:
                        p_us = float(np.median(pr)) * 1e6
                        p_spread = (max(pr) - min(pr)) * 1e6
                        out["parts_us_per_call_median"] = round(p_us, 2)
                        out["parts_us_per_call_min_max"] = [round(min(pr) * 1e6, 2),
                                                            round(max(pr) * 1e6, 2)]
                        out["parts_spread_us"] = round(p_spread, 2)
                        out["parts_peak_gb"] = round(parts_peak / 2 ** 30, 3)
                        out["parts_over_fused"] = round(p_us / f_us, 2)
                        out["difference_exceeds_spread"] = bool(
                            abs(p_us - f_us) > max(p_spread, f_spread))
                    else:
                        out["parts_route"] = "skipped: its parts exceed {:g} GiB".format(
                            a.max_intermediate_gb)
                    line = json.dumps(out)
                    print(line, flush=True)
                    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                    with open(a.out, "a") as f:
                        f.write(line + "\n")
                    del params, douts


if __name__ == "__main__":
    main()
