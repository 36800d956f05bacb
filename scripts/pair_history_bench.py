#!/usr/bin/env python3
"""What a batch of pair-history queries costs, one GPU and one process:

  (a) device:  graph.pair_history(src, dst, ts, since=, max_history=)      one kernel per call
  (b) host:    the same three arrays made on the host: per distinct source one
               graph.get_temporal_neighbors call, then numpy per row (two searchsorted for the
               window, a compare over the slice), uploaded -- what (a) replaces

for N = (1 + K) * B pairs per call, B = 600 and 4000 edges with K = 1 and 9 negatives each (an
evaluation batch: every source paired with its true destination and K random destinations),
max_history = 0 and 64, with and without `since` (ts minus a tenth of the stream's time span).

    python scripts/pair_history_bench.py [--edges 240000] [--rounds 7]

The four (max_history, since) variants of (a) alternate inside every round; a round of a variant
is one pass over --batches consecutive batches of the stream's last rows and ends in
torch.cuda.synchronize().  (b) runs in the first --host-rounds rounds over --host-batches batches
(a pass of it takes seconds), and its outputs are asserted equal to (a)'s.  One JSON line per
(B, K, max_history, since), appended to profiles/pair_history_bench.jsonl: the median round in
microseconds per call, its min and max, how (b) compares with (a), and whether the difference
exceeds the rounds' spread.  Host wall time only: the kernel alone is not traced here.  Synthetic
REDDIT-shaped graph with reverse edges, as scripts/seen_mask_bench.py builds it.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def host_pair_history(graph, src, dst, ts, since, max_history, device):
    """(b): the three outputs on `device`, from the host's view of the store."""
    import torch
    N = len(src)
    count = np.zeros(N, np.int64)
    last_ts = np.full(N, -np.inf, np.float32)
    last_eid = np.full(N, -1, np.int64)
    order = np.argsort(src, kind="stable")
    cuts = np.flatnonzero(np.diff(src[order])) + 1
    for rows in np.split(order, cuts):
        h_dst, h_ts, h_eid = graph.get_temporal_neighbors(int(src[rows[0]]))
        if len(h_dst) == 0:
            continue
        h_dst, h_ts, h_eid = h_dst[::-1], h_ts[::-1], h_eid[::-1]      # oldest first
        c = np.searchsorted(h_ts, ts[rows], side="left")
        c0 = np.minimum(c, np.searchsorted(h_ts, since[rows], side="left")) \
            if since is not None else np.zeros_like(c)
        lo = np.maximum(c0, c - max_history) if max_history else c0
        for i, a, b in zip(rows, lo, c):
            hits = np.flatnonzero(h_dst[a:b] == dst[i])
            if len(hits):
                p = a + hits[-1]
                count[i], last_ts[i], last_eid[i] = len(hits), h_ts[p], h_eid[p]
    return tuple(torch.from_numpy(x).to(device) for x in (count, last_ts, last_eid))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--edges", type=int, default=240000)
    ap.add_argument("--batch", type=int, nargs="+", default=[600, 4000])
    ap.add_argument("--neg-ratio", type=int, nargs="+", default=[1, 9])
    ap.add_argument("--batches", type=int, default=20, help="calls per round")
    ap.add_argument("--max-history", type=int, nargs="+", default=[0, 64])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--host-rounds", type=int, default=3, help="rounds in which (b) runs too")
    ap.add_argument("--host-batches", type=int, default=2,
                    help="calls per round of (b): a call of it takes up to seconds")
    ap.add_argument("--label", default="", help="a name for this run, for the record")
    ap.add_argument("--measured-by", default="", help="who ran this, for the record")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pair_history_bench.jsonl"))
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import pandas as pd
    import torch
    if not torch.cuda.is_available():
        sys.exit("pair_history_bench.py needs a GPU")
    from gnnflow_amd import synthetic
    from gnnflow_amd import utils as U

    dev = torch.device("cuda", 0)
    g = synthetic.reddit_like(seed=42, num_edges=a.edges)
    df = pd.DataFrame({"src": g["src"], "dst": g["dst"], "time": g["ts"], "eid": g["eid"]})
    graph = U.build_dynamic_graph(20 << 20, 1000 << 20, "cuda", 62, 1024, "insert",
                                  undirected=True, device=0, dataset_df=df)
    window = np.float32((df["time"].max() - df["time"].min()) / 10)
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
            # call b: [src | K more copies] against [dst | K blocks of random destinations]
            src = np.concatenate([np.tile(e_src[b * B:(b + 1) * B], 1 + K) for b in range(nb)])
            ts = np.concatenate([np.tile(e_ts[b * B:(b + 1) * B], 1 + K) for b in range(nb)])
            dst = np.concatenate([np.concatenate([e_dst[b * B:(b + 1) * B],
                                                  rng.choice(items, K * B)]) for b in range(nb)])
            lo = ts - window
            d_src, d_dst = torch.from_numpy(src).to(dev), torch.from_numpy(dst).to(dev)
            d_ts, d_lo = torch.from_numpy(ts).to(dev), torch.from_numpy(lo).to(dev)
            configs = [(mh, use) for mh in a.max_history for use in (False, True)]

            def device_pass(mh, use, calls=nb):
                out = None
                for b in range(calls):
                    s = slice(b * N, (b + 1) * N)
                    out = graph.pair_history(d_src[s], d_dst[s], d_ts[s],
                                             since=d_lo[s] if use else None, max_history=mh)
                return out

            def host_pass(mh, use):
                for b in range(a.host_batches):
                    s = slice(b * N, (b + 1) * N)
                    host_pair_history(graph, src[s], dst[s], ts[s], lo[s] if use else None, mh,
                                      dev)

            def timed(fn, calls):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                return (time.perf_counter() - t0) / calls

            seen_share = {}
            for mh, use in configs:          # (a) and (b) agree; and the warm-up of both
                s = slice(0, N)
                got = graph.pair_history(d_src[s], d_dst[s], d_ts[s],
                                         since=d_lo[s] if use else None, max_history=mh)
                want = host_pair_history(graph, src[s], dst[s], ts[s], lo[s] if use else None,
                                         mh, dev)
                assert torch.equal(got.count, want[0]) and torch.equal(got.last_eid, want[2])
                assert torch.equal(got.last_ts.view(torch.int32), want[1].view(torch.int32))
                seen_share[mh, use] = float((got.count > 0).double().mean())
                timed(lambda: device_pass(mh, use), nb)
            dev_rounds = {c: [] for c in configs}
            host_rounds = {c: [] for c in configs}
            for r in range(a.rounds):
                for mh, use in configs:
                    dev_rounds[mh, use].append(timed(lambda: device_pass(mh, use), nb))
                if r < a.host_rounds:
                    for mh, use in configs:
                        host_rounds[mh, use].append(
                            timed(lambda: host_pass(mh, use), a.host_batches))
            for mh, use in configs:
                dr, hr = dev_rounds[mh, use], host_rounds[mh, use]
                d_us = float(np.median(dr)) * 1e6
                d_spread = (max(dr) - min(dr)) * 1e6
                out = {"bench": "pair_history", "label": a.label, "B": B, "K": K, "N": N,
                       "max_history": mh, "since": bool(use), "edges": a.edges,
                       "calls_per_round": {"device": nb, "host": a.host_batches},
                       "rounds": {"device": len(dr), "host": len(hr)},
                       "device_us_per_call_median": round(d_us, 2),
                       "device_us_per_call_min_max": [round(min(dr) * 1e6, 2),
                                                      round(max(dr) * 1e6, 2)],
                       "device_spread_us": round(d_spread, 2),
                       "seen_share_first_call": round(seen_share[mh, use], 5),
                       "note": "host wall time over one pass of all calls, ending in a device "
                               "synchronise, divided by the calls; the four (max_history, "
                               "since) variants alternate inside every round; the kernel "
                               "alone was not traced",
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
                line = json.dumps(out)
                print(line, flush=True)
                os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                with open(a.out, "a") as f:
                    f.write(line + "\n")
            # does the bound or the lower end change the device's time by more than the spread?
            base = dev_rounds[a.max_history[0], False]
            for mh, use in configs[1:]:
                other = dev_rounds[mh, use]
                diff = (float(np.median(other)) - float(np.median(base))) * 1e6
                spread = max(max(base) - min(base), max(other) - min(other)) * 1e6
                line = json.dumps({"bench": "pair_history_variant_delta", "label": a.label,
                                   "B": B, "K": K, "max_history": mh, "since": bool(use),
                                   "minus_unbounded_us": round(diff, 2),
                                   "exceeds_spread": bool(abs(diff) > spread),
                                   "measured_by": a.measured_by})
                print(line, flush=True)
                with open(a.out, "a") as f:
                    f.write(line + "\n")


if __name__ == "__main__":
    main()
