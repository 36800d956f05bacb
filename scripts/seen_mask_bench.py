#!/usr/bin/env python3
"""What history filtering adds to a full ranking, one GPU and one process:

  (a) rank:       ops.edge_rank alone (k = 10, a reference score, the target skipped)
  (b) seen_rank:  graph.seen_mask(src, ts, cand, max_history) + ops.edge_rank(exclude=)
  (c) host_rank:  the mask made on the host: per distinct source one
                  graph.get_temporal_neighbors call, np.isin against the candidates per row,
                  packed into words and uploaded, then ops.edge_rank(exclude=) -- what (b) replaces

at B = 600 sources per call, C = 2 000 and 20 000 candidates and max_history = 0 and 64.

    python scripts/seen_mask_bench.py [--edges 240000] [--rounds 7]

The variants alternate inside every round; a round is one pass over --batches consecutive
batches of the stream's last rows and ends in torch.cuda.synchronize().  One JSON line per
(C, max_history), appended to profiles/seen_mask_bench.jsonl: the median round of each variant in
microseconds per call, its min and max, what (b) adds over (a), how (b) compares with (c), and
whether each difference exceeds the rounds' spread.  Synthetic REDDIT-shaped graph with reverse
edges, as scripts/hist_negatives_bench.py builds it; the embeddings are random (the ranking
kernel's time does not depend on their values).

--variants rank --package-root DIR times (a) alone with the package of another checkout (built
there), to compare the unmasked kernel across commits in one session.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def host_mask(graph, src, ts, cand, max_history, device):
    """(c)'s mask: int64 [B, W] on `device`, from the host's view of the store."""
    import torch
    B, C = len(src), len(cand)
    bits = np.zeros((B, (C + 63) // 64 * 64), bool)
    order = np.argsort(src, kind="stable")
    cuts = np.flatnonzero(np.diff(src[order])) + 1
    for rows in np.split(order, cuts):
        h_dst, h_ts, _ = graph.get_temporal_neighbors(int(src[rows[0]]))
        if len(h_dst) == 0:
            continue
        h_dst, h_ts = h_dst[::-1], h_ts[::-1]      # oldest first
        c = np.searchsorted(h_ts, ts[rows], side="left")
        for i, ci in zip(rows, c):
            lo = ci - min(ci, max_history) if max_history else 0
            bits[i, :C] = np.isin(cand, h_dst[lo:ci])
    words = np.packbits(bits.reshape(B, -1, 64), axis=-1, bitorder="little").view(np.int64)
    return torch.from_numpy(words.reshape(B, -1)).to(device)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--edges", type=int, default=240000)
    ap.add_argument("--batch", type=int, default=600)
    ap.add_argument("--batches", type=int, default=20, help="calls per round")
    ap.add_argument("--candidates", type=int, nargs="+", default=[2000, 20000])
    ap.add_argument("--max-history", type=int, nargs="+", default=[0, 64])
    ap.add_argument("--dim", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--host-rounds", type=int, default=3,
                    help="rounds in which (c) runs too: a pass of it takes seconds")
    ap.add_argument("--variants", nargs="+", default=["rank", "seen_rank", "host_rank"],
                    choices=["rank", "seen_rank", "host_rank"])
    ap.add_argument("--package-root", default=ROOT,
                    help="the checkout whose gnnflow_amd is timed (default: this one)")
    ap.add_argument("--label", default="", help="a name for this run, for the record")
    ap.add_argument("--measured-by", default="", help="who ran this, for the record")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "seen_mask_bench.jsonl"))
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.package_root))
    import pandas as pd
    import torch
    if not torch.cuda.is_available():
        sys.exit("seen_mask_bench.py needs a GPU")
    from gnnflow_amd import ops, synthetic
    from gnnflow_amd import utils as U

    dev = torch.device("cuda", 0)
    g = synthetic.reddit_like(seed=42, num_edges=a.edges)
    df = pd.DataFrame({"src": g["src"], "dst": g["dst"], "time": g["ts"], "eid": g["eid"]})
    graph = U.build_dynamic_graph(20 << 20, 1000 << 20, "cuda", 62, 1024, "insert",
                                  undirected=True, device=0, dataset_df=df)
    B, nb, D = a.batch, a.batches, a.dim
    rows = slice(len(df) - B * nb, len(df))
    src = df["src"].to_numpy()[rows].astype(np.int64)
    dst = df["dst"].to_numpy()[rows].astype(np.int64)
    ts = df["time"].to_numpy()[rows].astype(np.float32)
    d_src, d_ts = torch.from_numpy(src).to(dev), torch.from_numpy(ts).to(dev)
    gen = torch.Generator().manual_seed(0)
    h_src = torch.randn(B * nb, D, generator=gen).to(dev)
    w, bias = torch.randn(D, generator=gen).to(dev), torch.randn(1, generator=gen).to(dev)

    for C in a.candidates:
        # every destination of the stream first, then other nodes; past the number of nodes the
        # list repeats ids, which seen_mask allows
        rng = np.random.RandomState(C)
        items = np.unique(df["dst"].to_numpy())
        others = np.setdiff1d(np.arange(g["num_nodes"]), items)
        cand = np.concatenate([items, rng.permutation(others)])[:C]
        if len(cand) < C:
            cand = np.concatenate([cand, rng.choice(g["num_nodes"], C - len(cand))])
        cand = rng.permutation(cand).astype(np.int64)
        first = {int(c): i for i, c in reversed(list(enumerate(cand)))}
        target = torch.tensor([first.get(int(x), 0) for x in dst], device=dev)
        d_cand = torch.from_numpy(cand).to(dev)
        h_cand = torch.randn(C, D, generator=gen).to(dev)
        for mh in a.max_history:
            def batches():
                for b in range(nb):
                    s = slice(b * B, (b + 1) * B)
                    ref = ops.edge_score(h_src[s], h_cand[target[s]], w, bias)
                    yield s, ref

            def rank():
                for s, ref in batches():
                    ops.edge_rank(h_src[s], h_cand, w, bias, k=10, ref_score=ref, skip=target[s])

            def seen_rank():
                for s, ref in batches():
                    mask = graph.seen_mask(d_src[s], d_ts[s], d_cand, mh)
                    ops.edge_rank(h_src[s], h_cand, w, bias, k=10, ref_score=ref, skip=target[s],
                                  exclude=mask)

            def host_rank():
                for s, ref in batches():
                    mask = host_mask(graph, src[s], ts[s], cand, mh, dev)
                    ops.edge_rank(h_src[s], h_cand, w, bias, k=10, ref_score=ref, skip=target[s],
                                  exclude=mask)

            variants = {n: f for n, f in (("rank", rank), ("seen_rank", seen_rank),
                                          ("host_rank", host_rank)) if n in a.variants}

            def timed(fn):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                return (time.perf_counter() - t0) / nb

            share = None
            if "seen_rank" in variants and "host_rank" in variants:      # (b) and (c) agree
                s = slice(0, B)
                m = graph.seen_mask(d_src[s], d_ts[s], d_cand, mh)
                assert torch.equal(m, host_mask(graph, src[s], ts[s], cand, mh, dev))
                ids = torch.arange(C, device=dev)
                share = float(((m[:, ids >> 6] >> (ids & 63)) & 1).double().mean())
            for fn in variants.values():          # warm-up: every shape of the timed window
                timed(fn)
            rounds = {name: [] for name in variants}
            for r in range(a.rounds):
                for name, fn in variants.items():
                    if name != "host_rank" or r < a.host_rounds:
                        rounds[name].append(timed(fn))
            us = {n_: float(np.median(r)) * 1e6 for n_, r in rounds.items()}
            spread = {n_: (max(r) - min(r)) * 1e6 for n_, r in rounds.items()}
            out = {"bench": "seen_mask", "label": a.label, "B": B, "C": C, "D": D,
                   "max_history": mh, "calls_per_round": nb, "rounds": a.rounds, "edges": a.edges,
                   "rounds_per_variant": {n_: len(r) for n_, r in rounds.items()},
                   "us_per_call_median": {n_: round(x, 2) for n_, x in us.items()},
                   "us_per_call_min_max": {n_: [round(min(r) * 1e6, 2), round(max(r) * 1e6, 2)]
                                           for n_, r in rounds.items()},
                   "spread_us": {n_: round(x, 2) for n_, x in spread.items()},
                   "note": "host wall time over one pass of all calls, ending in a device "
                           "synchronise, divided by the calls; variants alternate inside every "
                           "round; every variant includes the edge_score call for the reference",
                   "measured_by": a.measured_by, "device": torch.cuda.get_device_name(0)}
            if share is not None:
                out["seen_share_first_batch"] = round(share, 5)
            if "rank" in us and "seen_rank" in us:
                added = us["seen_rank"] - us["rank"]
                out["seen_added_us"] = round(added, 2)
                out["added_exceeds_spread"] = bool(
                    abs(added) > max(spread["rank"], spread["seen_rank"]))
            if "host_rank" in us and "seen_rank" in us:
                out["host_over_seen"] = round(us["host_rank"] / us["seen_rank"], 2)
                out["host_minus_seen_exceeds_spread"] = bool(
                    us["host_rank"] - us["seen_rank"] > max(spread["host_rank"], spread["seen_rank"]))
            line = json.dumps(out)
            print(line, flush=True)
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(line + "\n")
            if a.variants == ["rank"]:
                break      # (a) does not depend on max_history


if __name__ == "__main__":
    main()
