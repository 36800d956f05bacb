#!/usr/bin/env python3
"""What temporal random walks cost on the device and on the host, one GPU and one process:

  (a) device:  graph.temporal_random_walk(src, ts, L, W, recency=, max_history=)
  (b) host:    the same rule on the host: per step one graph.get_temporal_neighbors call per
               distinct visited node, the window by numpy.searchsorted, the Philox draws in
               numpy -- what a user writes today, and what (a) replaces

at B = 1 200 roots per call, (W, L) = (64, 2) and (16, 4), recency 1 and 2, max_history 0 and 64.

    python scripts/temporal_walk_bench.py [--edges 240000] [--rounds 7]

The eight device variants alternate inside every round; a round times, per variant, one pass of
--calls calls (another epoch each, so other walks) that ends in torch.cuda.synchronize(), as host
wall time per call.  (b) runs in the first --host-rounds rounds, one call per round, and its
walks are compared with (a)'s bit for bit before anything is timed.  One JSON line per variant,
appended to profiles/temporal_walk_bench.jsonl: the median round in microseconds per call, its
min and max, the edge records read per second (one per step taken; a step also reads a node
entry and usually searches timestamps) beside the 51.7 G records/s that independent random
32-byte record reads reach (profiles/r06_random_record_rate.txt), and how (b) compares.
Synthetic REDDIT-shaped graph with reverse edges, as scripts/seen_mask_bench.py builds it; the
roots are the sources of the stream's last rows at their times.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED_TAG = 0x54454D5057414C4B      # GF_WALK_SEED_TAG
RANDOM_RECORD_RATE = 51.7e9        # profiles/r06_random_record_rate.txt, 32-byte records
M32, S32 = np.uint64(0xFFFFFFFF), np.uint64(32)


def philox_first(seed, tid, call):
    """gf_philox4x32_10_first (include/gnnflow_rng.h) over a uint64 array of tids."""
    tid = np.asarray(tid, dtype=np.uint64)
    c0, c1 = tid & M32, tid >> S32
    c2 = np.full_like(tid, call & 0xFFFFFFFF)
    c3 = np.full_like(tid, (call >> 32) & 0xFFFFFFFF)
    k0, k1 = np.uint64(seed & 0xFFFFFFFF), np.uint64(seed >> 32)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> S32) ^ c1 ^ k0, p1 & M32, (p0 >> S32) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M32, (k1 + np.uint64(0xBB67AE85)) & M32
    return c0


def host_walks(graph, src, ts, L, W, recency, max_history, seed, epoch, first_row=0):
    """(b): (nodes, eids, times) as numpy arrays, by the rule of gf_graph_temporal_walks."""
    mask64 = (1 << 64) - 1
    B = len(src)
    nodes = np.full((B * W, L + 1), -1, np.int64)
    eids = np.full((B * W, L), -1, np.int64)
    times = np.zeros((B * W, L), np.float32)
    v, t = np.repeat(src, W), np.repeat(ts, W)
    nodes[:, 0] = v
    rows_ = np.arange(B, dtype=np.uint64) + np.uint64(first_row)
    with np.errstate(over="ignore"):
        tid = (rows_[:, None] * np.uint64(W) + np.arange(W, dtype=np.uint64)[None, :]).ravel()
    table_len = graph.max_vertex_id() + 1 if graph.num_vertices() else 0
    history = {}
    alive = np.ones(B * W, bool)
    for j in range(L):
        idx = np.flatnonzero(alive & (v >= 0) & (v < table_len))
        alive[:] = False
        idx = idx[np.argsort(v[idx], kind="stable")]
        if len(idx) == 0:
            break
        call = ((epoch << 8) + j) & mask64
        for rows in np.split(idx, np.flatnonzero(np.diff(v[idx])) + 1):
            node = int(v[rows[0]])
            if node not in history:
                d, h_ts, e = graph.get_temporal_neighbors(node)
                history[node] = (d[::-1], h_ts[::-1], e[::-1])      # oldest first
            h_dst, h_ts, h_eid = history[node]
            if len(h_ts) == 0:
                continue
            c = np.searchsorted(h_ts, t[rows], side="left")
            c[np.isnan(t[rows])] = 0
            n = np.minimum(c, max_history) if max_history else c
            rows, c, n = rows[n > 0], c[n > 0], n[n > 0].astype(np.uint64)
            if len(rows) == 0:
                continue
            x = np.zeros(len(rows), np.uint64)
            for a in range(recency):
                u = philox_first((seed ^ ((SEED_TAG + a) & mask64)) & mask64, tid[rows], call)
                x = np.maximum(x, (u * n) >> S32)
            k = c - n.astype(np.int64) + x.astype(np.int64)
            nodes[rows, j + 1], eids[rows, j], times[rows, j] = h_dst[k], h_eid[k], h_ts[k]
            v[rows], t[rows] = h_dst[k], h_ts[k]
            alive[rows] = True
    return nodes.reshape(B, W, L + 1), eids.reshape(B, W, L), times.reshape(B, W, L)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--edges", type=int, default=240000)
    ap.add_argument("--roots", type=int, default=1200)
    ap.add_argument("--shapes", type=int, nargs="+", default=[64, 2, 16, 4],
                    help="W L pairs")
    ap.add_argument("--recency", type=int, nargs="+", default=[1, 2])
    ap.add_argument("--max-history", type=int, nargs="+", default=[0, 64])
    ap.add_argument("--calls", type=int, default=20, help="device calls per pass")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--host-rounds", type=int, default=3,
                    help="rounds in which (b) runs too, one call each: a call takes long")
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--measured-by", default="", help="who ran this, for the record")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "temporal_walk_bench.jsonl"))
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import pandas as pd
    import torch
    if not torch.cuda.is_available():
        sys.exit("temporal_walk_bench.py needs a GPU")
    from gnnflow_amd import synthetic
    from gnnflow_amd import utils as U

    dev = torch.device("cuda", 0)
    g = synthetic.reddit_like(seed=42, num_edges=a.edges)
    df = pd.DataFrame({"src": g["src"], "dst": g["dst"], "time": g["ts"], "eid": g["eid"]})
    graph = U.build_dynamic_graph(20 << 20, 1000 << 20, "cuda", 62, 1024, "insert",
                                  undirected=True, device=0, dataset_df=df)
    B = a.roots
    src = df["src"].to_numpy()[-B:].astype(np.int64)
    ts = df["time"].to_numpy()[-B:].astype(np.float32)
    d_src, d_ts = torch.from_numpy(src).to(dev), torch.from_numpy(ts).to(dev)
    shapes = list(zip(a.shapes[0::2], a.shapes[1::2]))
    variants = [(W, L, r, m) for W, L in shapes for r in a.recency for m in a.max_history]

    def device_pass(W, L, r, m):
        for e in range(a.calls):
            graph.temporal_random_walk(d_src, d_ts, L, W, recency=r, max_history=m, seed=a.seed,
                                       epoch=e)

    def timed(fn, calls):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / calls

    steps = {}
    for W, L, r, m in variants:      # (a) and (b) agree; the steps a call takes; the warm-up
        got = graph.temporal_random_walk(d_src, d_ts, L, W, recency=r, max_history=m, seed=a.seed)
        want = host_walks(graph, src, ts, L, W, r, m, a.seed, 0)
        for x, y in zip(got, want):
            assert np.array_equal(x.cpu().numpy().view(np.int32), y.view(np.int32)), (W, L, r, m)
        taken = [int((graph.temporal_random_walk(d_src, d_ts, L, W, recency=r, max_history=m,
                                                 seed=a.seed, epoch=e).eids >= 0).sum())
                 for e in range(a.calls)]
        steps[W, L, r, m] = float(np.mean(taken))
        timed(lambda: device_pass(W, L, r, m), a.calls)
    device = {v: [] for v in variants}
    host = {v: [] for v in variants}
    for rnd in range(a.rounds):
        for v in variants:
            device[v].append(timed(lambda: device_pass(*v), a.calls))
        if rnd < a.host_rounds:
            for W, L, r, m in variants:
                host[W, L, r, m].append(timed(
                    lambda: host_walks(graph, src, ts, L, W, r, m, a.seed, rnd), 1))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    for v in variants:
        W, L, r, m = v
        d_us, h_us = np.array(device[v]) * 1e6, np.array(host[v]) * 1e6
        med = float(np.median(d_us))
        out = {"bench": "temporal_walk", "B": B, "W": W, "L": L, "recency": r, "max_history": m,
               "edges": a.edges, "calls_per_pass": a.calls, "rounds": a.rounds,
               "device_us_per_call_median": round(med, 2),
               "device_us_per_call_min_max": [round(float(d_us.min()), 2), round(float(d_us.max()), 2)],
               "steps_per_call": round(steps[v], 1),
               "steps_share_of_walk_slots": round(steps[v] / (B * W * L), 4),
               "record_reads_per_s": round(steps[v] / (med * 1e-6), 1),
               "share_of_random_record_rate": round(steps[v] / (med * 1e-6) / RANDOM_RECORD_RATE, 5),
               "note": "host wall time over one pass of all calls, ending in a device "
                       "synchronise, divided by the calls; variants alternate inside every round; "
                       "the host route is one call per round; its walks equal the device's",
               "measured_by": a.measured_by, "device": torch.cuda.get_device_name(0)}
        if len(h_us):
            out["host_rounds"] = len(h_us)
            out["host_us_per_call_median"] = round(float(np.median(h_us)), 1)
            out["host_us_per_call_min_max"] = [round(float(h_us.min()), 1), round(float(h_us.max()), 1)]
            out["host_over_device"] = round(float(np.median(h_us)) / med, 1)
        line = json.dumps(out)
        print(line, flush=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
