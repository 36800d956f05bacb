#!/usr/bin/env python3
"""Fused ops.time_encode_cat against the torch chain it replaces,

    torch.cat([*parts, torch.cos(F.linear(t[:, None], w, b))], 1)

forward and forward + backward, interleaved in one process and timed with device events, at the
three time encodings of one batch of the recorded TGN-shaped epoch (T = 100): the memory
updater's rows, the edges' K / V rows and the zero-time query rows.

    python scripts/time_encode_bench.py                      # -> profiles/time_encode_bench.jsonl
    python scripts/time_encode_bench.py --kernel-trace DIR   # + the chains' kernels by name

Each variant is timed in `--rounds` rounds that alternate between the variants; a round runs
enough iterations for at least `--min-seconds / --rounds` of device time.  One JSON line per
shape: the median round and the min / max rounds of both sides in microseconds per iteration
(wall time between device events, host launch overhead included), and whether the fused side
beats the torch chain by more than the torch chain's own spread (max - min round) -- the
condition for `fused_time_encode` to default to True in gnnflow_amd.nn.

--kernel-trace DIR runs this script once more as a child under `rocprofv3 --kernel-trace
--stats` (both chains, --trace-iters iterations per shape, no timing) and prints every kernel
of that run with its calls and average duration: which torch kernels the chain is made of.
"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

T = 100
SHAPES = [  # (rows, part widths, t = 0?)
    ("memory updater", 41148, (200,), False),
    ("edge K/V", 29148, (100,), False),
    ("zero-time queries", 12000, (100,), True),
]


def make_chains(n, widths, zero_t):
    import torch
    import torch.nn.functional as F
    from gnnflow_amd import ops
    dev = torch.device("cuda")
    g = torch.Generator(device="cpu").manual_seed(n)
    parts = [torch.randn(n, w, generator=g).to(dev).requires_grad_(True) for w in widths]
    t = torch.zeros(n, device=dev) if zero_t else torch.rand(n, generator=g).to(dev)
    freq = (1 / 10 ** np.linspace(0, 9, T, dtype=np.float32)).reshape(T, 1)
    w = torch.from_numpy(freq).to(dev).requires_grad_(True)
    b = torch.zeros(T, device=dev, requires_grad=True)
    gout = torch.randn(n, sum(widths) + T, generator=g).to(dev)
    leaves = parts + [w, b]

    def fused():
        return ops.time_encode_cat(parts, t, w, b)

    def chain():
        return torch.cat([*parts, torch.cos(F.linear(t[:, None], w, b))], 1)

    def fwd(fn):
        with torch.no_grad():
            fn()

    def fwd_bwd(fn):
        for x in leaves:
            x.grad = None
        fn().backward(gout)

    # same results first: the copied columns bit-equal, the rest to fp32 rounding
    a, c = fused(), chain()
    off = sum(widths)
    assert torch.equal(a[:, :off], c[:, :off]) and float((a - c).abs().max()) < 1e-5
    return {"fused_fwd": lambda: fwd(fused), "torch_fwd": lambda: fwd(chain),
            "fused_fwd_bwd": lambda: fwd_bwd(fused), "torch_fwd_bwd": lambda: fwd_bwd(chain)}


def timed(fn, iters):
    import torch
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1e-3


def bench_shape(name, n, widths, zero_t, rounds, min_seconds):
    import torch
    variants = make_chains(n, widths, zero_t)
    iters = {}
    for key, fn in variants.items():           # warm-up, then size a round
        timed(fn, 20)
        per = timed(fn, 50) / 50
        iters[key] = max(50, int(np.ceil(1.3 * min_seconds / rounds / per)))
    runs = {key: [] for key in variants}
    for _ in range(rounds):
        for key, fn in variants.items():
            runs[key].append(timed(fn, iters[key]) / iters[key] * 1e6)
    med = {k: float(np.median(r)) for k, r in runs.items()}
    spread = {k: float(max(r) - min(r)) for k, r in runs.items()}
    out = {"bench": "time_encode_cat", "shape": name, "rows": n, "parts": list(widths),
           "dim_time": T, "t": "zero" if zero_t else "uniform [0, 1)", "rounds": rounds,
           "iters_per_round": iters,
           "timed_seconds": {k: round(float(np.sum(r)) * iters[k] * 1e-6, 3)
                             for k, r in runs.items()},
           "us_per_iter_median": {k: round(v, 2) for k, v in med.items()},
           "us_per_iter_min_max": {k: [round(min(r), 2), round(max(r), 2)]
                                   for k, r in runs.items()},
           "us_per_iter_spread": {k: round(v, 2) for k, v in spread.items()},
           "speedup_fwd": round(med["torch_fwd"] / med["fused_fwd"], 3),
           "speedup_fwd_bwd": round(med["torch_fwd_bwd"] / med["fused_fwd_bwd"], 3)}
    for kind in ("fwd", "fwd_bwd"):
        gain = med["torch_" + kind] - med["fused_" + kind]
        out["fused_beats_torch_by_more_than_its_spread_" + kind] = \
            bool(gain > spread["torch_" + kind])
    out["note"] = ("us_per_iter is wall time between device events, host launch overhead of "
                   "each path included; spread = max - min round")
    out["device"] = torch.cuda.get_device_name(0)
    return out


def trace_child(iters):
    """Both chains, forward + backward, `iters` times per shape; no timing."""
    import torch
    for _name, n, widths, zero_t in SHAPES:
        variants = make_chains(n, widths, zero_t)
        for key in ("torch_fwd_bwd", "fused_fwd_bwd"):
            for _ in range(iters):
                variants[key]()
    torch.cuda.synchronize()


def kernel_trace(directory, iters):
    """Runs the child under rocprofv3 (a fresh process; this one has not touched the GPU yet)
    and returns [{name, calls, avg_us, total_us}] sorted by total time."""
    os.makedirs(directory, exist_ok=True)
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", directory, "--output-format", "csv",
           "-o", "time_encode", "--", sys.executable, os.path.abspath(__file__), "--trace-child",
           "--trace-iters", str(iters)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=540)
    if r.returncode != 0:
        raise RuntimeError("rocprofv3 failed:\n" + r.stdout[-2000:] + r.stderr[-2000:])
    files = glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True)
    if not files:
        raise RuntimeError("rocprofv3 wrote no kernel_stats.csv under " + directory)
    rows = []
    for row in csv.DictReader(open(max(files, key=os.path.getmtime))):
        calls, total = int(row["Calls"]), float(row["TotalDurationNs"]) / 1e3
        rows.append({"name": row["Name"], "calls": calls, "avg_us": round(total / max(calls, 1), 2),
                     "total_us": round(total, 1)})
    return sorted(rows, key=lambda x: -x["total_us"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--min-seconds", type=float, default=0.5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "time_encode_bench.jsonl"))
    ap.add_argument("--kernel-trace", metavar="DIR", default=None)
    ap.add_argument("--trace-iters", type=int, default=100)
    ap.add_argument("--trace-child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.trace_child:
        trace_child(a.trace_iters)
        return
    if a.kernel_trace:                         # first: before this process opens the GPU
        kernels = kernel_trace(a.kernel_trace, a.trace_iters)
        per = 3 * a.trace_iters
        print(json.dumps({"bench": "time_encode_cat kernel trace",
                          "what": "kernels of {} forward + backward passes of each chain "
                                  "({} per shape)".format(per, a.trace_iters),
                          "kernels": kernels}))
    lines = [bench_shape(name, n, widths, zero_t, a.rounds, a.min_seconds)
             for name, n, widths, zero_t in SHAPES]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for line in lines:
            text = json.dumps(line)
            print(text)
            f.write(text + "\n")


if __name__ == "__main__":
    main()
