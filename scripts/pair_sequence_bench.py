#!/usr/bin/env python3
"""What DyGFormer's inputs cost for a batch of pairs, one GPU and one process:

  (a) reader:  graph.pair_sequence(src, dst, ts, length=L, node_feats=, edge_feats=,
                                   time_encoder=enc)                                 one kernel
  (b) torch:   what a user writes without it, on the same build (examples/dygformer_inputs.py's
               route, finished): graph.neighbor_cooccurrence(src, dst, ts, length=L) ->
               node_table[nodes.clamp(0)] and edge_table[eids.clamp(0)] -> masked_fill of the
               slots without a row -> ts[:, None, None] - times -> FixedTimeEncode -> masked_fill
               of the padded slots

for N = (1 + K) * B pairs per call, B = 600 and 4000 edges with K = 1 and 9 (the batch's pairs and
K random destinations per source, at the edge's time), L = 32 and 128, float32 node and edge tables
of 172 columns and a time encoding of dT = 100.

    python scripts/pair_sequence_bench.py [--edges 240000] [--rounds 7]

neighbor_sequence_bench.py's protocol, unchanged: (a) and (b) alternate inside every round; a round
of a variant is one pass over --batches consecutive batches of the stream's last rows and ends in
torch.cuda.synchronize().  On the first call of every line (b)'s delta_t and three parts are
asserted equal to (a)'s bit for bit.  (b) is skipped, and the line says so, where its
intermediates (the indexed rows and the encoding, and the masked copy of each) would exceed
--max-intermediate-gb.  One JSON line per (B, K, L), appended to
profiles/pair_sequence_bench.jsonl: the median round in microseconds per call, its min and max,
how (b) compares with (a), and whether the difference exceeds the rounds' spread.  Host wall time
only: the kernel alone is not traced here.  Synthetic REDDIT-shaped graph with reverse edges, as
scripts/pair_history_bench.py builds it.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def torch_route(graph, src, dst, ts, node_table, edge_table, enc, L):
    """(b): (delta_t, node, edge, time) through neighbor_cooccurrence and torch."""
    import torch
    c = graph.neighbor_cooccurrence(src, dst, ts, length=L, include_self=True)
    padding = (torch.arange(L, device=ts.device) >= c.lengths.unsqueeze(2)).unsqueeze(3)
    node_x = node_table[c.nodes.clamp(min=0)].masked_fill((c.nodes < 0).unsqueeze(3), 0.0)
    edge_x = edge_table[c.eids.clamp(min=0)].masked_fill((c.eids < 0).unsqueeze(3), 0.0)
    delta_t = (ts[:, None, None] - c.times).masked_fill(padding.squeeze(3), 0.0)
    time_x = enc(delta_t).masked_fill(padding, 0.0)
    return delta_t, node_x, edge_x, time_x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--edges", type=int, default=240000)
    ap.add_argument("--batch", type=int, nargs="+", default=[600, 4000])
    ap.add_argument("--neg-ratio", type=int, nargs="+", default=[1, 9])
    ap.add_argument("--batches", type=int, default=20, help="calls per round")
    ap.add_argument("--length", type=int, nargs="+", default=[32, 128])
    ap.add_argument("--dim-node", type=int, default=172)
    ap.add_argument("--dim-edge", type=int, default=172)
    ap.add_argument("--dim-time", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--max-intermediate-gb", type=float, default=8.0,
                    help="(b) is skipped where its intermediates exceed this")
    ap.add_argument("--label", default="", help="a name for this run, for the record")
    ap.add_argument("--measured-by", default="", help="who ran this, for the record")
    ap.add_argument("--out",
                    default=os.path.join(ROOT, "profiles", "pair_sequence_bench.jsonl"))
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import pandas as pd
    import torch
    if not torch.cuda.is_available():
        sys.exit("pair_sequence_bench.py needs a GPU")
    from gnnflow_amd import synthetic
    from gnnflow_amd import utils as U
    from gnnflow_amd.nn import FixedTimeEncode

    dev = torch.device("cuda", 0)
    g = synthetic.reddit_like(seed=42, num_edges=a.edges)
    df = pd.DataFrame({"src": g["src"], "dst": g["dst"], "time": g["ts"], "eid": g["eid"]})
    graph = U.build_dynamic_graph(20 << 20, 1000 << 20, "cuda", 62, 1024, "insert",
                                  undirected=True, device=0, dataset_df=df)
    torch.manual_seed(0)
    dn, de, dT = a.dim_node, a.dim_edge, a.dim_time
    width = dn + de + dT
    node_table = torch.randn(g["num_nodes"], dn, device=dev)
    edge_table = torch.randn(g["num_edges"], de, device=dev)
    enc = FixedTimeEncode(dT).to(dev)
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
            # call b: the batch's sources 1 + K times against [its destinations | K blocks of
            # random destinations], at the edges' times
            src = np.concatenate([np.tile(e_src[b * B:(b + 1) * B], 1 + K) for b in range(nb)])
            dst = np.concatenate([np.concatenate([e_dst[b * B:(b + 1) * B],
                                                  rng.choice(items, K * B)]) for b in range(nb)])
            ts = np.concatenate([np.tile(e_ts[b * B:(b + 1) * B], 1 + K) for b in range(nb)])
            d_src, d_dst = torch.from_numpy(src).to(dev), torch.from_numpy(dst).to(dev)
            d_ts = torch.from_numpy(ts).to(dev)

            def reader(s, L):
                return graph.pair_sequence(d_src[s], d_dst[s], d_ts[s], length=L,
                                           node_feats=node_table, edge_feats=edge_table,
                                           time_encoder=enc)

            def reader_pass(L):
                for b in range(nb):
                    reader(slice(b * N, (b + 1) * N), L)

            def torch_pass(L):
                for b in range(nb):
                    s = slice(b * N, (b + 1) * N)
                    torch_route(graph, d_src[s], d_dst[s], d_ts[s], node_table, edge_table, enc,
                                L)

            def timed(fn):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                return (time.perf_counter() - t0) / nb

            def intermediates(L):      # indexed rows and encoding, and each one's masked copy
                return N * 2 * L * 2 * width * 4

            fits, mean_len = {}, {}
            for L in a.length:      # (a) and (b) agree; and the warm-up of both
                s = slice(0, N)
                got = reader(s, L)
                mean_len[L] = float(got.lengths.double().mean())
                fits[L] = intermediates(L) <= a.max_intermediate_gb * 2 ** 30
                if fits[L]:
                    want = torch_route(graph, d_src[s], d_dst[s], d_ts[s], node_table,
                                       edge_table, enc, L)
                    for x, y in zip((got.delta_t, got.node, got.edge, got.time), want):
                        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
                    del want
                    timed(lambda: torch_pass(L))
                del got
                timed(lambda: reader_pass(L))
            reader_rounds = {L: [] for L in a.length}
            torch_rounds = {L: [] for L in a.length}
            for r in range(a.rounds):
                for L in a.length:
                    reader_rounds[L].append(timed(lambda: reader_pass(L)))
                    if fits[L]:
                        torch_rounds[L].append(timed(lambda: torch_pass(L)))
            for L in a.length:
                rr, tr = reader_rounds[L], torch_rounds[L]
                r_us = float(np.median(rr)) * 1e6
                r_spread = (max(rr) - min(rr)) * 1e6
                out = {"bench": "pair_sequence", "label": a.label, "B": B, "K": K, "N": N,
                       "length": L, "dim_node": dn, "dim_edge": de, "dim_time": dT,
                       "edges": a.edges, "calls_per_round": nb, "rounds": len(rr),
                       "mean_length_first_call": round(mean_len[L], 2),
                       "reader_us_per_call_median": round(r_us, 2),
                       "reader_us_per_call_min_max": [round(min(rr) * 1e6, 2),
                                                      round(max(rr) * 1e6, 2)],
                       "reader_spread_us": round(r_spread, 2),
                       "parts_gb": round(N * 2 * L * width * 4 / 2 ** 30, 3),
                       "torch_intermediates_gb": round(intermediates(L) / 2 ** 30, 3),
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
                    out["torch_route"] = "skipped: its intermediates exceed {:g} GiB".format(
                        a.max_intermediate_gb)
                line = json.dumps(out)
                print(line, flush=True)
                os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                with open(a.out, "a") as f:
                    f.write(line + "\n")


if __name__ == "__main__":
    main()
