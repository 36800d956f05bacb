#!/usr/bin/env python3
"""What historical negatives add to a DeviceBatchStream batch, one GPU and one process:

  (a) assemble:  DeviceBatchStream with hist_ratio = 0 (one launch per batch)
  (b) hist:      the same stream with hist_ratio = ceil(K / 2) (a second launch per batch that
                 reads the graph's edge store)
  (c) host_hist: for ONE batch size, the same draw done on the host on top of (a)'s batches:
                 per distinct source one graph.get_temporal_neighbors call, per slot a numpy
                 draw from the edges before the row's time, then the copy of the planes back to
                 the device — the loop (b) replaces

at B = 600 and 4000 with K = 1 and 9 negatives per edge.

    python scripts/hist_negatives_bench.py [--edges 240000] [--rounds 7]

The variants alternate inside every round; a round is one pass over all batches of the frame
and ends in torch.cuda.synchronize().  One JSON line per (B, K), appended to
profiles/hist_negatives_bench.jsonl: the median round of each variant in microseconds per batch,
its min and max, and whether what (b) adds exceeds the rounds' spread.  (c) takes seconds per
pass and runs in the first --host-rounds rounds only.  Synthetic REDDIT-shaped
graph with reverse edges, as scripts/batch_stream_bench.py builds it.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def host_hist_pass(stream, graph, Kh, rng):
    """(c): historical negatives for every batch of `stream` (hist_ratio = 0) on the host."""
    import torch
    for roots, ts, _ in stream:
        B = roots.shape[0] // (2 + stream.neg_ratio)
        head = roots[:2 * B].cpu().numpy()
        t = ts[:B].cpu().numpy()
        src, dst = head[:B], head[B:]
        planes = roots[2 * B:(2 + Kh) * B].cpu().numpy().reshape(Kh, B)
        order = np.argsort(src, kind="stable")
        cuts = np.flatnonzero(np.diff(src[order])) + 1
        for rows in np.split(order, cuts):
            h_dst, h_ts, _ = graph.get_temporal_neighbors(int(src[rows[0]]))
            if len(h_dst) == 0:
                continue
            h_dst, h_ts = h_dst[::-1], h_ts[::-1]      # oldest first
            c = np.searchsorted(h_ts, t[rows], side="left")
            for i, ci in zip(rows, c):
                if ci == 0:
                    continue
                cand = h_dst[rng.randint(0, ci, size=Kh)]
                keep = cand != dst[i]
                planes[keep, i] = cand[keep]
        roots[2 * B:(2 + Kh) * B] = torch.from_numpy(planes.reshape(-1)).to(roots.device)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--edges", type=int, default=240000)
    ap.add_argument("--batch", type=int, nargs="+", default=[600, 4000])
    ap.add_argument("--neg", type=int, nargs="+", default=[1, 9])
    ap.add_argument("--host-batch", type=int, default=4000,
                    help="the batch size at which the host draw (c) is timed too")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--host-rounds", type=int, default=3,
                    help="rounds in which (c) runs too: a pass of it takes seconds")
    ap.add_argument("--measured-by", default="", help="who ran this, for the record")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hist_negatives_bench.jsonl"))
    a = ap.parse_args()
    import pandas as pd
    import torch
    if not torch.cuda.is_available():
        sys.exit("hist_negatives_bench.py needs a GPU")
    import gnnflow_amd
    from gnnflow_amd import synthetic
    from gnnflow_amd import utils as U

    dev = torch.device("cuda", 0)
    g = synthetic.reddit_like(seed=42, num_edges=a.edges)
    df = pd.DataFrame({"src": g["src"], "dst": g["dst"], "time": g["ts"], "eid": g["eid"]})
    graph = U.build_dynamic_graph(20 << 20, 1000 << 20, "cuda", 62, 1024, "insert",
                                  undirected=True, device=0, dataset_df=df)
    dst_set = gnnflow_amd.DeviceDstSet(g["num_nodes"], dev, df["dst"].to_numpy())
    dst_set.check()

    for B in a.batch:
        for K in a.neg:
            Kh = (K + 1) // 2
            plain = gnnflow_amd.DeviceBatchStream.from_dataframe(df, B, dst_set, neg_ratio=K)
            hist = gnnflow_amd.DeviceBatchStream.from_dataframe(df, B, dst_set, neg_ratio=K,
                                                                graph=graph, hist_ratio=Kh)
            nb = len(plain)
            rng = np.random.RandomState(0)

            def assemble():
                for _ in plain:
                    pass

            def with_hist():
                for _ in hist:
                    pass

            variants = {"assemble": assemble, "hist": with_hist}
            if B == a.host_batch:
                variants["host_hist"] = lambda: host_hist_pass(plain, graph, Kh, rng)

            def timed(fn):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                return (time.perf_counter() - t0) / nb

            # the second launch changes the first Kh negative planes and nothing else
            p, h = plain[0][0].cpu().numpy(), hist[0][0].cpu().numpy()
            n = len(p) // (2 + K)
            assert np.array_equal(p[:2 * n], h[:2 * n]) and np.array_equal(p[(2 + Kh) * n:],
                                                                            h[(2 + Kh) * n:])
            assert not np.array_equal(p, h)
            for fn in variants.values():          # warm-up: every shape of the timed window
                timed(fn)
            hist.reset_hist_filled()
            rounds = {name: [] for name in variants}
            for r in range(a.rounds):
                for name, fn in variants.items():
                    if name != "host_hist" or r < a.host_rounds:
                        rounds[name].append(timed(fn))
            share = int(hist.hist_filled.item()) / (a.rounds * hist.rows * Kh)
            us = {n_: float(np.median(r)) * 1e6 for n_, r in rounds.items()}
            spread = {n_: (max(r) - min(r)) * 1e6 for n_, r in rounds.items()}
            added = us["hist"] - us["assemble"]
            out = {"bench": "hist_negatives", "B": B, "K": K, "Kh": Kh, "batches_per_round": nb,
                   "rounds": a.rounds, "edges": a.edges,
                   "rounds_per_variant": {n_: len(r) for n_, r in rounds.items()},
                   "us_per_batch_median": {n_: round(x, 2) for n_, x in us.items()},
                   "us_per_batch_min_max": {n_: [round(min(r) * 1e6, 2), round(max(r) * 1e6, 2)]
                                            for n_, r in rounds.items()},
                   "spread_us": {n_: round(x, 2) for n_, x in spread.items()},
                   "hist_added_us": round(added, 2),
                   "added_exceeds_spread": bool(added > max(spread["assemble"], spread["hist"])),
                   "hist_share": round(share, 4),
                   "note": "host wall time over one pass of all batches, ending in a device "
                           "synchronise, divided by the batches; variants alternate inside "
                           "every round; host_hist is assemble plus the host draw",
                   "measured_by": a.measured_by, "device": torch.cuda.get_device_name(0)}
            line = json.dumps(out)
            print(line, flush=True)
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
