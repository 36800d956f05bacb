#!/usr/bin/env python3
"""Per-batch wall time of the first stage of a training step, host against device, one GPU and
one process:

  (a) host:   utils.get_batch (numpy slices, a host RandomState, two concatenations) and
              TemporalSampler.sample on its numpy output (two pageable host-to-device copies)
  (b) device: DeviceBatchStream (one launch) and TemporalSampler.sample on its device tensors

at B = 600 and 4000 with K = 1 and 9 negatives per edge.  (a) is the code path a loop had before
DeviceBatchStream existed and uses none of the new code; utils.get_batch draws one negative per
edge, so for K > 1 the script's `host_batches` repeats its loop with K draws (the same sampler
and the same concatenations).  Also reported: the assembly alone, (a) with the two copies the
sampler would make and (b) without the sampler, each ending in one synchronise per epoch.

    python scripts/batch_stream_bench.py [--edges 240000] [--rounds 7]

The variants alternate inside every round; a round is one pass over all batches of the frame
and ends in torch.cuda.synchronize().  One JSON line per (B, K), appended to
profiles/batch_stream_bench.jsonl: the median round of each variant in microseconds per batch
and each variant's round-to-round spread (max - min).  Synthetic REDDIT-shaped graph, 2 layers
of fanout 10, most-recent sampling.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def host_batches(df, batch_size, K, neg_sampler):
    """utils.get_batch for K = 1; its loop with K draws per edge otherwise."""
    from gnnflow_amd import utils as U
    if K == 1:
        yield from U.get_batch(df, batch_size, 0, neg_sampler)
        return
    src, dst = df['src'].values, df['dst'].values
    t_all, eids = df['time'].values, df['eid'].values
    for pos in U._row_groups(df, batch_size, 0):
        neg = neg_sampler.sample(K * len(pos))
        t = t_all[pos]
        yield (np.concatenate([src[pos], dst[pos], neg]).astype(np.int64),
               np.concatenate([t] * (2 + K)).astype(np.float32), eids[pos])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--edges", type=int, default=240000)
    ap.add_argument("--batch", type=int, nargs="+", default=[600, 4000])
    ap.add_argument("--neg", type=int, nargs="+", default=[1, 9])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--measured-by", default="", help="who ran this, for the record")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_stream_bench.jsonl"))
    a = ap.parse_args()
    import pandas as pd
    import torch
    if not torch.cuda.is_available():
        sys.exit("batch_stream_bench.py needs a GPU")
    import gnnflow_amd
    from gnnflow_amd import synthetic
    from gnnflow_amd import utils as U

    dev = torch.device("cuda", 0)
    g = synthetic.reddit_like(seed=42, num_edges=a.edges)
    df = pd.DataFrame({"src": g["src"], "dst": g["dst"], "time": g["ts"], "eid": g["eid"]})
    graph = U.build_dynamic_graph(20 << 20, 1000 << 20, "cuda", 62, 1024, "insert",
                                  undirected=True, device=0, dataset_df=df)
    sampler = gnnflow_amd.TemporalSampler(graph, fanouts=[10, 10], sample_strategy="recent")
    dst_np = df["dst"].to_numpy()
    dst_set = gnnflow_amd.DeviceDstSet(g["num_nodes"], dev, dst_np)
    dst_set.check()

    for B in a.batch:
        for K in a.neg:
            host_neg = U.DstRandEdgeSampler(dst_np, seed=0)
            stream = gnnflow_amd.DeviceBatchStream.from_dataframe(df, B, dst_set, neg_ratio=K)
            nb = len(stream)

            def host_sample():
                for roots, ts, _ in host_batches(df, B, K, host_neg):
                    sampler.sample(roots, ts)

            def device_sample():
                for roots, ts, _ in stream:
                    sampler.sample(roots, ts)

            def host_assemble():
                for roots, ts, _ in host_batches(df, B, K, host_neg):
                    torch.from_numpy(roots).to(dev)
                    torch.from_numpy(ts).to(dev)

            def device_assemble():
                for _ in stream:
                    pass

            variants = {"host_get_batch_sample": host_sample, "device_stream_sample": device_sample,
                        "host_get_batch_copy": host_assemble, "device_stream": device_assemble}

            def timed(fn):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                return (time.perf_counter() - t0) / nb

            # both paths hand the sampler the same positives
            h = next(iter(host_batches(df, B, K, host_neg)))
            d = stream[0]
            assert np.array_equal(h[0][:2 * len(h[2])], d[0][:2 * len(h[2])].cpu().numpy())
            assert np.array_equal(h[1], d[1].cpu().numpy()) and h[0].shape == tuple(d[0].shape)
            for fn in variants.values():          # warm-up: every shape of the timed window
                timed(fn)
            rounds = {name: [] for name in variants}
            for _ in range(a.rounds):
                for name, fn in variants.items():
                    rounds[name].append(timed(fn))
            us = {n: float(np.median(r)) * 1e6 for n, r in rounds.items()}
            spread = {n: (max(r) - min(r)) * 1e6 for n, r in rounds.items()}
            margin = us["host_get_batch_sample"] - us["device_stream_sample"]
            out = {"bench": "batch_stream", "B": B, "K": K, "batches_per_round": nb,
                   "rounds": a.rounds, "edges": a.edges,
                   "us_per_batch_median": {n: round(x, 2) for n, x in us.items()},
                   "us_per_batch_min_max": {n: [round(min(r) * 1e6, 2), round(max(r) * 1e6, 2)]
                                            for n, r in rounds.items()},
                   "spread_us": {n: round(x, 2) for n, x in spread.items()},
                   "sample_margin_us": round(margin, 2),
                   "device_beats_host_by_more_than_spread": bool(
                       margin > max(spread["host_get_batch_sample"],
                                    spread["device_stream_sample"])),
                   "note": "host wall time over one pass of all batches, ending in a device "
                           "synchronise, divided by the batches; sampler.sample waits for its "
                           "kernels in both paths; variants alternate inside every round",
                   "measured_by": a.measured_by, "device": torch.cuda.get_device_name(0)}
            line = json.dumps(out)
            print(line, flush=True)
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
