#!/usr/bin/env python3
"""What a batch of common-neighbour queries costs, one GPU and one process:

  (a) device:  graph.common_neighbors(src, dst, ts, max_history=H, max_common=32)
               one kernel per call
  (b) host:    the same eight arrays made on the host: per distinct node of the call one
               graph.get_temporal_neighbors call, then numpy per row (a searchsorted per end for
               the window, np.unique per end, np.intersect1d, an argsort by the last position),
               uploaded -- what (a) replaces

for N = (1 + K) * B pairs per call, B = 600 and 4000 edges with K = 1 and 9 negatives each (an
evaluation batch: every source paired with its true destination and K random destinations),
max_history H = 32, 128 and 512: the kernel's three instantiations.

    python scripts/common_neighbors_bench.py [--edges 240000] [--rounds 7]

The H variants of (a) alternate inside every round; a round of a variant is one pass over
--batches consecutive batches of the stream's last rows and ends in torch.cuda.synchronize().
(b) runs in the first --host-rounds rounds over --host-batches batches (a call of it takes up to
seconds), and its outputs are asserted equal to (a)'s.  One JSON line per (B, K, H), appended to
profiles/common_neighbors_bench.jsonl: the median round in microseconds per call, its min and
max, how (b) compares with (a), and whether the difference exceeds the rounds' spread; and one
line per (B, K, H > the first) on whether the bucket changes the device's time by more than the
spread.  Host wall time only: the kernel alone is not traced here, and NeighborOverlap inside an
evaluation pass is not measured.  Synthetic REDDIT-shaped graph with reverse edges, as
scripts/pair_history_bench.py builds it.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_COMMON = 32


def host_common_neighbors(graph, src, dst, ts, H, K, device):
    """(b): the eight outputs on `device`, from the host's view of the store."""
    import torch
    N = len(src)
    scalars = np.zeros((5, N), np.int32)
    nodes = np.full((N, K), -1, np.int64)
    cnt = np.zeros((2, N, K), np.int32)
    hist = {}
    for v in np.unique(np.concatenate([src, dst])):
        h_dst, h_ts, _ = graph.get_temporal_neighbors(int(v))
        hist[int(v)] = (h_dst[::-1], h_ts[::-1])                          # oldest first
    for i in range(N):
        sides = []
        for v in (src[i], dst[i]):
            h_dst, h_ts = hist[int(v)]
            c = int(np.searchsorted(h_ts, ts[i], side="left"))
            sides.append(h_dst[c - min(c, H):c])
        A, B = sides
        # the first occurrence in the reversed window is the last position in the window
        ua, first, ca = np.unique(A[A >= 0][::-1], return_index=True, return_counts=True)
        ub, cb = np.unique(B[B >= 0], return_counts=True)
        both, xa, xb = np.intersect1d(ua, ub, assume_unique=True, return_indices=True)
        scalars[:, i] = len(A), len(B), len(ua), len(ub), len(both)
        order = np.argsort(first[xa], kind="stable")[:K]                   # newest first
        nodes[i, :len(order)] = both[order]
        cnt[0, i, :len(order)], cnt[1, i, :len(order)] = ca[xa][order], cb[xb][order]
    return tuple(torch.from_numpy(x).to(device) for x in (*scalars, nodes, cnt[0], cnt[1]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--edges", type=int, default=240000)
    ap.add_argument("--batch", type=int, nargs="+", default=[600, 4000])
    ap.add_argument("--neg-ratio", type=int, nargs="+", default=[1, 9])
    ap.add_argument("--batches", type=int, default=20, help="calls per round")
    ap.add_argument("--max-history", type=int, nargs="+", default=[32, 128, 512])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--host-rounds", type=int, default=3, help="rounds in which (b) runs too")
    ap.add_argument("--host-batches", type=int, default=1,
                    help="calls per round of (b): a call of it takes up to seconds")
    ap.add_argument("--label", default="", help="a name for this run, for the record")
    ap.add_argument("--measured-by", default="", help="who ran this, for the record")
    ap.add_argument("--out",
                    default=os.path.join(ROOT, "profiles", "common_neighbors_bench.jsonl"))
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import pandas as pd
    import torch
    if not torch.cuda.is_available():
        sys.exit("common_neighbors_bench.py needs a GPU")
    from gnnflow_amd import synthetic
    from gnnflow_amd import utils as U

    dev = torch.device("cuda", 0)
    g = synthetic.reddit_like(seed=42, num_edges=a.edges)
    df = pd.DataFrame({"src": g["src"], "dst": g["dst"], "time": g["ts"], "eid": g["eid"]})
    graph = U.build_dynamic_graph(20 << 20, 1000 << 20, "cuda", 62, 1024, "insert",
                                  undirected=True, device=0, dataset_df=df)
    items = np.unique(df["dst"].to_numpy())
    nb = a.batches

    def emit(record):
        line = json.dumps(record)
        print(line, flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")

    for B in a.batch:
        rows = slice(len(df) - B * nb, len(df))
        e_src = df["src"].to_numpy()[rows].astype(np.int64)
        e_dst = df["dst"].to_numpy()[rows].astype(np.int64)
        e_ts = df["time"].to_numpy()[rows].astype(np.float32)
        for K in a.neg_ratio:
            rng = np.random.RandomState(1000 * K + B % 1000)
            N = (1 + K) * B
            # call b: [src | K more copies] against [dst | K blocks of random destinations]
            src = np.concatenate([np.tile(e_src[b * B:(b + 1) * B], 1 + K) for b in range(nb)])
            ts = np.concatenate([np.tile(e_ts[b * B:(b + 1) * B], 1 + K) for b in range(nb)])
            dst = np.concatenate([np.concatenate([e_dst[b * B:(b + 1) * B],
                                                  rng.choice(items, K * B)]) for b in range(nb)])
            d_src, d_dst = torch.from_numpy(src).to(dev), torch.from_numpy(dst).to(dev)
            d_ts = torch.from_numpy(ts).to(dev)

            def device_pass(H, calls=nb):
                out = None
                for b in range(calls):
                    s = slice(b * N, (b + 1) * N)
                    out = graph.common_neighbors(d_src[s], d_dst[s], d_ts[s], max_history=H,
                                                 max_common=MAX_COMMON)
                return out

            def host_pass(H):
                for b in range(a.host_batches):
                    s = slice(b * N, (b + 1) * N)
                    host_common_neighbors(graph, src[s], dst[s], ts[s], H, MAX_COMMON, dev)

            def timed(fn, calls):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                return (time.perf_counter() - t0) / calls

            share = {}
            for H in a.max_history:          # (a) and (b) agree; and the warm-up of both
                s = slice(0, N)
                got = graph.common_neighbors(d_src[s], d_dst[s], d_ts[s], max_history=H,
                                             max_common=MAX_COMMON)
                want = host_common_neighbors(graph, src[s], dst[s], ts[s], H, MAX_COMMON, dev)
                for name, x, y in zip(got._fields, got, want):
                    assert torch.equal(x, y), name
                share[H] = (float((got.common > 0).double().mean()),
                            float(got.n_src.double().mean()), float(got.n_dst.double().mean()))
                timed(lambda: device_pass(H), nb)
            dev_rounds = {H: [] for H in a.max_history}
            host_rounds = {H: [] for H in a.max_history}
            for r in range(a.rounds):
                for H in a.max_history:
                    dev_rounds[H].append(timed(lambda: device_pass(H), nb))
                if r < a.host_rounds:
                    for H in a.max_history:
                        host_rounds[H].append(timed(lambda: host_pass(H), a.host_batches))
            for H in a.max_history:
                dr, hr = dev_rounds[H], host_rounds[H]
                d_us = float(np.median(dr)) * 1e6
                d_spread = (max(dr) - min(dr)) * 1e6
                out = {"bench": "common_neighbors", "label": a.label, "B": B, "K": K, "N": N,
                       "max_history": H, "max_common": MAX_COMMON, "edges": a.edges,
                       "calls_per_round": {"device": nb, "host": a.host_batches},
                       "rounds": {"device": len(dr), "host": len(hr)},
                       "device_us_per_call_median": round(d_us, 2),
                       "device_us_per_call_min_max": [round(min(dr) * 1e6, 2),
                                                      round(max(dr) * 1e6, 2)],
                       "device_spread_us": round(d_spread, 2),
                       "common_share_first_call": round(share[H][0], 5),
                       "mean_n_src_n_dst_first_call": [round(share[H][1], 2),
                                                       round(share[H][2], 2)],
                       "note": "host wall time over one pass of all calls, ending in a device "
                               "synchronise, divided by the calls; the max_history variants "
                               "alternate inside every round; the kernel alone was not traced",
                       "measured_by": a.measured_by, "device": torch.cuda.get_device_name(0)}
                if hr:
                    h_us = float(np.median(hr)) * 1e6
                    h_spread = (max(hr) - min(hr)) * 1e6
                    out["host_us_per_call_median"] = round(h_us, 2)
                    out["host_us_per_call_min_max"] = [round(min(hr) * 1e6, 2),
                                                       round(max(hr) * 1e6, 2)]
                    out["host_spread_us"] = round(h_spread, 2)
                    out["host_over_device"] = round(h_us / d_us, 1)
                    out["host_minus_device_exceeds_spread"] = bool(
                        h_us - d_us > max(h_spread, d_spread))
                emit(out)
            # does the bucket change the device's time by more than the spread?
            base = dev_rounds[a.max_history[0]]
            for H in a.max_history[1:]:
                other = dev_rounds[H]
                diff = (float(np.median(other)) - float(np.median(base))) * 1e6
                spread = max(max(base) - min(base), max(other) - min(other)) * 1e6
                emit({"bench": "common_neighbors_bucket_delta", "label": a.label, "B": B, "K": K,
                      "max_history": H, "minus_max_history": a.max_history[0],
                      "minus_first_us": round(diff, 2), "exceeds_spread": bool(abs(diff) > spread),
                      "measured_by": a.measured_by})


if __name__ == "__main__":
    main()
