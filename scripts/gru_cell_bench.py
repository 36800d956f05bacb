#!/usr/bin/env python3
"""nn.GRUMemoryUpdater with fused_gru on (the two GEMMs + ops.gru_cell) against off
(torch.nn.GRUCell, the cast, the clone of the memory rows and the add behind it), the whole
module forward + backward, interleaved in one process and timed with device events, at the memory
updater of the TGN-shaped epoch: N = 1 800 and 19 800 source rows, dim_memory = 100, messages of
2 * 100 + 172 columns plus 100 of time encoding; without node features (dim_node = 0) and with
them (dim_node = 100: h + updated); in float32 and under bfloat16 autocast.

    python scripts/gru_cell_bench.py          # -> profiles/gru_cell_bench.jsonl

Each variant is timed in `--rounds` rounds that alternate between the two; a round runs enough
iterations for at least `--min-seconds / --rounds` of device time.  One JSON line per shape,
dim_node and dtype: the median round and the min / max rounds of both sides in microseconds per
iteration (wall time between device events, host launch overhead included), each side's own
spread (max - min round), the number of kernels one forward + backward launches on either side
(counted by torch.profiler; null where it is not available), and whether the fused side beats the
torch side by more than the torch side's spread -- the condition, at every line, for `fused_gru`
to default to True in gnnflow_amd.nn.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROWS = (1800, 19800)
DIM_MEMORY, DIM_EDGE, DIM_TIME = 100, 172, 100
DIM_NODES = (0, 100)


class Block:
    """What GRUMemoryUpdater reads of a block."""

    def __init__(self, srcdata, num_dst):
        self.srcdata, self._num_dst = srcdata, num_dst

    def num_dst_nodes(self):
        return self._num_dst


def make_variants(N, dim_node, bf16):
    import torch
    from gnnflow_amd import nn as gnn
    dev = torch.device("cuda")
    g = torch.Generator(device="cpu").manual_seed(N + dim_node)
    torch.manual_seed(1)
    module = gnn.GRUMemoryUpdater(dim_node, DIM_EDGE, DIM_TIME, DIM_MEMORY, DIM_MEMORY).to(dev)
    R = N // 11      # the roots of a block of fanout 10
    src = {"ID": torch.arange(N, device=dev),
           "ts": (torch.rand(N, generator=g) * 100 + 100).to(dev),
           "mem_ts": (torch.rand(N, generator=g) * 100).to(dev),
           "mem_input": torch.randn(N, 2 * DIM_MEMORY + DIM_EDGE, generator=g).to(dev),
           "mem": torch.randn(N, DIM_MEMORY, generator=g).to(dev)}
    h0 = torch.randn(N, dim_node, generator=g).to(dev) if dim_node else None
    gout = torch.randn(N, DIM_MEMORY, generator=g).to(dev)

    def step(fused):
        module.fused_gru = fused
        b = Block(dict(src), R)
        if dim_node:
            b.srcdata['h'] = h0
        for p in module.parameters():
            p.grad = None
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=bf16):
            last = module(b)
        b.srcdata['h'].backward(gout)
        return b.srcdata['h'].detach(), last["last_updated_memory"]

    (h_off, m_off), (h_on, m_on) = step(False), step(True)      # the same results first
    tol = 0.1 if bf16 else 1e-4
    assert h_on.dtype == h_off.dtype == m_on.dtype == torch.float32
    assert float((h_on - h_off).abs().max()) < tol and float((m_on - m_off).abs().max()) < tol
    return {"fused": lambda: step(True), "torch": lambda: step(False)}


def timed(fn, iters):
    import torch
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1e-3


def count_kernels(fn):
    """Kernels launched by one call of fn, or None when the profiler does not work here."""
    import torch
    try:
        from torch.profiler import ProfilerActivity, profile
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        kernels = [e for e in prof.events()
                   if str(e.device_type).endswith("CUDA") and "memcpy" not in e.name.lower()
                   and "memset" not in e.name.lower()]
        return len(kernels) or None
    except Exception:      # no profiler in this build: the timing does not depend on it
        return None


def bench_shape(N, dim_node, bf16, rounds, min_seconds):
    import torch
    variants = make_variants(N, dim_node, bf16)
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
    return {"bench": "gru_memory_updater", "what": "module forward + backward, fused_gru on / off",
            "rows": N, "dim_memory": DIM_MEMORY, "dim_message": 2 * DIM_MEMORY + DIM_EDGE,
            "dim_time": DIM_TIME, "dim_node": dim_node,
            "dtype": "bfloat16 autocast" if bf16 else "float32",
            "rounds": rounds, "iters_per_round": iters,
            "us_per_iter_median": {k: round(v, 2) for k, v in med.items()},
            "us_per_iter_min_max": {k: [round(min(r), 2), round(max(r), 2)]
                                    for k, r in runs.items()},
            "us_per_iter_spread": {k: round(v, 2) for k, v in spread.items()},
            "kernels_per_step": {k: None for k in variants},
            "speedup": round(med["torch"] / med["fused"], 3),
            "fused_beats_torch_by_more_than_its_spread":
                bool(med["torch"] - med["fused"] > spread["torch"]),
            "note": "us_per_iter is wall time between device events, host launch overhead of "
                    "each path included; spread = max - min round; kernels_per_step counts the "
                    "GEMMs and the time encoding too, after the timed rounds",
            "device": torch.cuda.get_device_name(0)}, variants


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--min-seconds", type=float, default=0.5)
    ap.add_argument("--no-kernel-count", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gru_cell_bench.jsonl"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("gru_cell_bench.py needs a GPU")
    done = [bench_shape(N, dn, bf16, a.rounds, a.min_seconds)
            for N in ROWS for dn in DIM_NODES for bf16 in (False, True)]
    lines = [line for line, _ in done]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)

    def write():
        with open(a.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")
    write()      # the timings are on disk before the profiler is started
    if not a.no_kernel_count:
        for line, variants in done:
            line["kernels_per_step"] = {k: count_kernels(fn) for k, fn in variants.items()}
        write()
    for line in lines:
        print(json.dumps(line))
    print("fused ahead at every line by more than the torch side's spread: {}".format(
        all(x["fused_beats_torch_by_more_than_its_spread"] for x in lines)))


if __name__ == "__main__":
    main()
