#!/usr/bin/env python3
"""What a batch of DyGFormer pair inputs costs, one GPU and one process:

  (a) device:  graph.neighbor_cooccurrence(src, dst, ts, length=L)        one kernel per call
  (b) host:    the same five arrays made on the host: per distinct node of the call one
               graph.get_temporal_neighbors call, then numpy per row (a searchsorted per end for
               the window, one np.unique over both sequences, two bincounts), uploaded -- what
               (a) replaces

for N = (1 + K) * B pairs per call, B = 600 and 4000 edges with K = 1 and 9 negatives each (an
evaluation batch: every source paired with its true destination and K random destinations),
length L = 32, 128 and 512: the kernel's three instantiations; scripts/common_neighbors_bench.py's
graph and protocol.  The REDDIT-shaped stream is bipartite, so these pairs share no neighbour
(an element is counted on both sides only where the pair itself has met before, through the self
slots): the `previous` pairing, every source with the source of the row before, is timed as well,
where two users share communities, and every line reports its `common` share (rows in which some
history element, the self slots aside, is counted on both sides).

    python scripts/neighbor_cooccurrence_bench.py [--edges 240000] [--rounds 7]

The L variants of (a) alternate inside every round; a round of a variant is one pass over
--batches consecutive batches of the stream's last rows and ends in torch.cuda.synchronize().
(b) runs in the first --host-rounds rounds over --host-batches batches (a call of it takes up to
seconds), and its outputs are asserted equal to (a)'s.  One JSON line per (pairing, B, K, L),
appended to profiles/neighbor_cooccurrence_bench.jsonl: the median round in microseconds per call,
its min and max, how (b) compares with (a), and whether the difference exceeds the rounds' spread;
one line per (pairing, B, K, L > the first) on whether the bucket changes the device's time by more
than the spread; and one per (B, K, L) on whether the pairing does.  Host wall time only: the
kernel alone is not traced here.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def host_neighbor_cooccurrence(graph, src, dst, ts, L, device):
    """(b): the five outputs on `device`, from the host's view of the store; include_self."""
    import torch
    N, H = len(src), L - 1
    lengths = np.zeros((N, 2), np.int32)
    nodes = np.full((N, 2, L), -1, np.int64)
    eids = np.full((N, 2, L), -1, np.int64)
    times = np.zeros((N, 2, L), np.float32)
    counts = np.zeros((N, 2, L, 2), np.int32)
    hist = {}
    for v in np.unique(np.concatenate([src, dst])):
        h_dst, h_ts, h_eid = graph.get_temporal_neighbors(int(v))
        hist[int(v)] = (h_dst[::-1], h_ts[::-1], h_eid[::-1])                # oldest first
    for i in range(N):
        seqs = []
        for side, v in enumerate((src[i], dst[i])):
            h_dst, h_ts, h_eid = hist[int(v)]
            c = int(np.searchsorted(h_ts, ts[i], side="left"))
            n = min(c, H)
            lengths[i, side] = 1 + n
            nodes[i, side, 0], times[i, side, 0] = v, ts[i]
            nodes[i, side, 1:1 + n] = h_dst[c - n:c]
            eids[i, side, 1:1 + n] = h_eid[c - n:c]
            times[i, side, 1:1 + n] = h_ts[c - n:c]
            seqs.append(nodes[i, side, :1 + n])
        la = len(seqs[0])
        uniq, inv = np.unique(np.concatenate(seqs), return_inverse=True)
        a = np.bincount(inv[:la], minlength=len(uniq))
        b = np.bincount(inv[la:], minlength=len(uniq))
        known = uniq[inv] >= 0                                              # negative: not counted
        for side, part in ((0, inv[:la]), (1, inv[la:])):
            k = known[:la] if side == 0 else known[la:]
            counts[i, side, :len(part), 0] = a[part] * k
            counts[i, side, :len(part), 1] = b[part] * k
    return tuple(torch.from_numpy(x).to(device) for x in (lengths, nodes, eids, times, counts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--edges", type=int, default=240000)
    ap.add_argument("--batch", type=int, nargs="+", default=[600, 4000])
    ap.add_argument("--neg-ratio", type=int, nargs="+", default=[1, 9])
    ap.add_argument("--batches", type=int, default=20, help="calls per round")
    ap.add_argument("--length", type=int, nargs="+", default=[32, 128, 512])
    ap.add_argument("--pairing", nargs="+", default=["stream", "previous"],
                    choices=("stream", "previous"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--host-rounds", type=int, default=3, help="rounds in which (b) runs too")
    ap.add_argument("--host-batches", type=int, default=1,
                    help="calls per round of (b): a call of it takes up to seconds")
    ap.add_argument("--label", default="", help="a name for this run, for the record")
    ap.add_argument("--measured-by", default="", help="who ran this, for the record")
    ap.add_argument("--out",
                    default=os.path.join(ROOT, "profiles", "neighbor_cooccurrence_bench.jsonl"))
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import pandas as pd
    import torch
    if not torch.cuda.is_available():
        sys.exit("neighbor_cooccurrence_bench.py needs a GPU")
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

    def timed(fn, calls):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / calls

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
            ends = {"stream": np.concatenate(
                [np.concatenate([e_dst[b * B:(b + 1) * B], rng.choice(items, K * B)])
                 for b in range(nb)]),
                "previous": np.roll(src, 1)}
            d_src, d_ts = torch.from_numpy(src).to(dev), torch.from_numpy(ts).to(dev)
            medians = {}
            for pairing in a.pairing:
                dst = ends[pairing]
                d_dst = torch.from_numpy(dst).to(dev)

                def device_pass(L, calls=nb):
                    out = None
                    for b in range(calls):
                        s = slice(b * N, (b + 1) * N)
                        out = graph.neighbor_cooccurrence(d_src[s], d_dst[s], d_ts[s], length=L)
                    return out

                def host_pass(L):
                    for b in range(a.host_batches):
                        s = slice(b * N, (b + 1) * N)
                        host_neighbor_cooccurrence(graph, src[s], dst[s], ts[s], L, dev)

                share = {}
                for L in a.length:          # (a) and (b) agree; and the warm-up of both
                    s = slice(0, N)
                    got = graph.neighbor_cooccurrence(d_src[s], d_dst[s], d_ts[s], length=L)
                    want = host_neighbor_cooccurrence(graph, src[s], dst[s], ts[s], L, dev)
                    for name, x, y in zip(got._fields, got, want):
                        assert torch.equal(x, y), name
                    both = (got.eids >= 0) & (got.nodes >= 0) & (got.counts[..., 0] > 0) & \
                        (got.counts[..., 1] > 0)
                    share[L] = (float(both.reshape(N, -1).any(1).double().mean()),
                                float(got.lengths[:, 0].double().mean()),
                                float(got.lengths[:, 1].double().mean()))
                    del got, want, both
                    timed(lambda: device_pass(L), nb)
                dev_rounds = {L: [] for L in a.length}
                host_rounds = {L: [] for L in a.length}
                for r in range(a.rounds):
                    for L in a.length:
                        dev_rounds[L].append(timed(lambda: device_pass(L), nb))
                    if r < a.host_rounds:
                        for L in a.length:
                            host_rounds[L].append(timed(lambda: host_pass(L), a.host_batches))
                for L in a.length:
                    dr, hr = dev_rounds[L], host_rounds[L]
                    d_us = float(np.median(dr)) * 1e6
                    d_spread = (max(dr) - min(dr)) * 1e6
                    medians[pairing, L] = (d_us, d_spread)
                    out = {"bench": "neighbor_cooccurrence", "label": a.label, "pairing": pairing,
                           "B": B, "K": K, "N": N, "length": L, "include_self": True,
                           "edges": a.edges,
                           "calls_per_round": {"device": nb, "host": a.host_batches},
                           "rounds": {"device": len(dr), "host": len(hr)},
                           "device_us_per_call_median": round(d_us, 2),
                           "device_us_per_call_min_max": [round(min(dr) * 1e6, 2),
                                                          round(max(dr) * 1e6, 2)],
                           "device_spread_us": round(d_spread, 2),
                           "output_mb_per_call": round(N * 2 * L * 28 / 1e6, 1),
                           "common_share_first_call": round(share[L][0], 5),
                           "mean_len_src_len_dst_first_call": [round(share[L][1], 2),
                                                               round(share[L][2], 2)],
                           "note": "host wall time over one pass of all calls, ending in a device "
                                   "synchronise, divided by the calls; the length variants "
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
                base = dev_rounds[a.length[0]]
                for L in a.length[1:]:
                    other = dev_rounds[L]
                    diff = (float(np.median(other)) - float(np.median(base))) * 1e6
                    spread = max(max(base) - min(base), max(other) - min(other)) * 1e6
                    emit({"bench": "neighbor_cooccurrence_bucket_delta", "label": a.label,
                          "pairing": pairing, "B": B, "K": K, "length": L,
                          "minus_length": a.length[0], "minus_first_us": round(diff, 2),
                          "exceeds_spread": bool(abs(diff) > spread),
                          "measured_by": a.measured_by})
            # does the pairing (counts > 0 on both channels) change the device's time?
            if len(a.pairing) == 2:
                for L in a.length:
                    (x, sx), (y, sy) = medians[a.pairing[0], L], medians[a.pairing[1], L]
                    emit({"bench": "neighbor_cooccurrence_pairing_delta", "label": a.label, "B": B,
                          "K": K, "length": L, "pairing": a.pairing[1],
                          "minus_pairing": a.pairing[0], "minus_first_us": round(y - x, 2),
                          "exceeds_spread": bool(abs(y - x) > max(sx, sy)),
                          "measured_by": a.measured_by})


if __name__ == "__main__":
    main()
