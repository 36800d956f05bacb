#!/usr/bin/env python3
"""What the windowed mean of neighbour features costs for a batch of nodes, one GPU and one
process:

  (a) reader:  graph.neighbor_aggregate(nodes, ts, node_feats=table, max_history=H)   one kernel
  (b) torch:   the route that existed before it, on the same build:
               graph.neighbor_cooccurrence(nodes, nodes, ts, length=H, include_self=False), side 0
               -> table[ids.clamp(0)] -> mask -> sum over H / count, with its [N, H, d] intermediate

for N = (1 + K) * B nodes per call, B = 600 and 4000 edges with K = 1 and 9 (the sources of a batch
and K random destinations each, at the edge's time), H = 32, 128 and 512, and a float32 table of
d = 172 columns over the graph's nodes.

    python scripts/neighbor_aggregate_bench.py [--edges 240000] [--rounds 7]

pair_history_bench.py's protocol: (a) and (b) alternate inside every round; a round of a variant
is one pass over --batches consecutive batches of the stream's last rows and ends in
torch.cuda.synchronize().  On the first call of every line (b)'s result is asserted allclose to
(a)'s -- not bit-equal: torch's reduction order differs.  (b) is skipped, and the line says so,
where its [N, H, d] intermediate would exceed --max-intermediate-gb.  One JSON line per (B, K, H),
appended to profiles/neighbor_aggregate_bench.jsonl: the median round in microseconds per call,
its min and max, how (b) compares with (a), and whether the difference exceeds the rounds'
spread.  Host wall time only: the kernel alone is not traced here.  Synthetic REDDIT-shaped graph
with reverse edges, as scripts/pair_history_bench.py builds it.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def torch_route(graph, nodes, ts, table, H):
    """(b): (count, mean) through the padded id matrix."""
    seq = graph.neighbor_cooccurrence(nodes, nodes, ts, length=H, include_self=False)
    ids = seq.nodes[:, 0]                                           # [N, H], -1 in the padding
    known = (ids >= 0) & (ids < table.shape[0])
    rows = table[ids.clamp(0, table.shape[0] - 1)]                  # [N, H, d]
    total = (rows * known.unsqueeze(2)).sum(1)
    count = seq.lengths[:, 0].long()
    return count, total / count.clamp(min=1).unsqueeze(1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--edges", type=int, default=240000)
    ap.add_argument("--batch", type=int, nargs="+", default=[600, 4000])
    ap.add_argument("--neg-ratio", type=int, nargs="+", default=[1, 9])
    ap.add_argument("--batches", type=int, default=20, help="calls per round")
    ap.add_argument("--max-history", type=int, nargs="+", default=[32, 128, 512])
    ap.add_argument("--dim", type=int, default=172)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--max-intermediate-gb", type=float, default=8.0,
                    help="(b) is skipped where N * H * d * 4 bytes exceeds this")
    ap.add_argument("--label", default="", help="a name for this run, for the record")
    ap.add_argument("--measured-by", default="", help="who ran this, for the record")
    ap.add_argument("--out",
                    default=os.path.join(ROOT, "profiles", "neighbor_aggregate_bench.jsonl"))
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import pandas as pd
    import torch
    if not torch.cuda.is_available():
        sys.exit("neighbor_aggregate_bench.py needs a GPU")
    from gnnflow_amd import synthetic
    from gnnflow_amd import utils as U

    dev = torch.device("cuda", 0)
    g = synthetic.reddit_like(seed=42, num_edges=a.edges)
    df = pd.DataFrame({"src": g["src"], "dst": g["dst"], "time": g["ts"], "eid": g["eid"]})
    graph = U.build_dynamic_graph(20 << 20, 1000 << 20, "cuda", 62, 1024, "insert",
                                  undirected=True, device=0, dataset_df=df)
    torch.manual_seed(0)
    table = torch.randn(g["num_nodes"], a.dim, device=dev)
    items = np.unique(df["dst"].to_numpy())
    nb, d = a.batches, a.dim

    for B in a.batch:
        rows = slice(len(df) - B * nb, len(df))
        e_src = df["src"].to_numpy()[rows].astype(np.int64)
        e_ts = df["time"].to_numpy()[rows].astype(np.float32)
        for K in a.neg_ratio:
            rng = np.random.RandomState(1000 * K + B % 1000)
            N = (1 + K) * B
            # call b: [the batch's sources | K blocks of random destinations], at the edges' times
            nodes = np.concatenate([np.concatenate([e_src[b * B:(b + 1) * B],
                                                    rng.choice(items, K * B)]) for b in range(nb)])
            ts = np.concatenate([np.tile(e_ts[b * B:(b + 1) * B], 1 + K) for b in range(nb)])
            d_nodes, d_ts = torch.from_numpy(nodes).to(dev), torch.from_numpy(ts).to(dev)

            def reader_pass(H):
                for b in range(nb):
                    s = slice(b * N, (b + 1) * N)
                    graph.neighbor_aggregate(d_nodes[s], d_ts[s], node_feats=table,
                                             max_history=H)

            def torch_pass(H):
                for b in range(nb):
                    s = slice(b * N, (b + 1) * N)
                    torch_route(graph, d_nodes[s], d_ts[s], table, H)

            def timed(fn):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                return (time.perf_counter() - t0) / nb

            fits, mean_count = {}, {}
            for H in a.max_history:      # (a) and (b) agree; and the warm-up of both
                s = slice(0, N)
                got = graph.neighbor_aggregate(d_nodes[s], d_ts[s], node_feats=table,
                                               max_history=H)
                mean_count[H] = float(got.count.double().mean())
                fits[H] = N * H * d * 4 <= a.max_intermediate_gb * 2 ** 30
                if fits[H]:
                    count, mean = torch_route(graph, d_nodes[s], d_ts[s], table, H)
                    assert torch.equal(got.count, count)
                    assert torch.allclose(got.node, mean, rtol=1e-4, atol=1e-4)
                    del count, mean
                    timed(lambda: torch_pass(H))
                timed(lambda: reader_pass(H))
            reader_rounds = {H: [] for H in a.max_history}
            torch_rounds = {H: [] for H in a.max_history}
            for r in range(a.rounds):
                for H in a.max_history:
                    reader_rounds[H].append(timed(lambda: reader_pass(H)))
                    if fits[H]:
                        torch_rounds[H].append(timed(lambda: torch_pass(H)))
            for H in a.max_history:
                rr, tr = reader_rounds[H], torch_rounds[H]
                r_us = float(np.median(rr)) * 1e6
                r_spread = (max(rr) - min(rr)) * 1e6
                out = {"bench": "neighbor_aggregate", "label": a.label, "B": B, "K": K, "N": N,
                       "max_history": H, "dim": d, "edges": a.edges, "calls_per_round": nb,
                       "rounds": len(rr), "mean_count_first_call": round(mean_count[H], 2),
                       "reader_us_per_call_median": round(r_us, 2),
                       "reader_us_per_call_min_max": [round(min(rr) * 1e6, 2),
                                                      round(max(rr) * 1e6, 2)],
                       "reader_spread_us": round(r_spread, 2),
                       "intermediate_gb": round(N * H * d * 4 / 2 ** 30, 3),
                       "note": "host wall time over one pass of all calls, ending in a device "
                               "synchronise, divided by the calls; the reader and the torch "
                               "route alternate inside every round; the kernel alone was not "
                               "traced",
                       "measured_by": a.measured_by, "device": torch.cuda.get_device_name(0)}
                if tr:
                    t_us = float(np.median(tr)) * 1e6
                    t_spread = (max(tr) - min(tr)) * 1e6
                    out["torch_us_per_call_median"] = round(t_us, 2)
                    out["torch_us_per_call_min_max"] = [round(min(tr) * 1e6, 2),
                                                        round(max(tr) * 1e6, 2)]
                    out["torch_spread_us"] = round(t_spread, 2)
                    out["torch_over_reader"] = round(t_us / r_us, 2)
                    out["torch_minus_reader_exceeds_spread"] = bool(
                        abs(t_us - r_us) > max(t_spread, r_spread))
                else:
                    out["torch_route"] = "skipped: its [N, H, d] intermediate exceeds " \
                                         "{:g} GiB".format(a.max_intermediate_gb)
                line = json.dumps(out)
                print(line, flush=True)
                os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                with open(a.out, "a") as f:
                    f.write(line + "\n")


if __name__ == "__main__":
    main()
