#!/usr/bin/env python3
"""Fused ops.dropout_relu_layer_norm against the torch line it replaces in
nn.TemporalAttentionLayer.forward,

    layer_norm(F.relu(dropout(z)))            z = w_out(rst), the GEMM excluded from both sides

forward + backward, interleaved in one process and timed with device events, at the epilogues of
the recorded TGN-shaped epoch: R = 1 800 and 19 800 rows at D = 100, R = 1 800 at D = 172; each in
float32 and as it runs under bfloat16 autocast (z bfloat16: torch casts to float32 in front of
layer_norm, the op widens in the kernel), with p = 0 and p = 0.1.

    python scripts/layer_epilogue_bench.py          # -> profiles/layer_epilogue_bench.jsonl

Each variant is timed in `--rounds` rounds that alternate between the two; a round runs enough
iterations for at least `--min-seconds / --rounds` of device time.  One JSON line per shape, dtype
and p: the median round and the min / max rounds of both sides in microseconds per iteration (wall
time between device events, host launch overhead included), each side's own spread (max - min
round), and whether the fused side beats the torch chain by more than the torch chain's spread --
the condition, at every line, for `fused_epilogue` to default to True in gnnflow_amd.nn.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(1800, 100), (19800, 100), (1800, 172)]
PS = (0.0, 0.1)


def make_chains(R, D, bf16, p):
    import torch
    import torch.nn.functional as F
    from gnnflow_amd import ops
    dev = torch.device("cuda")
    g = torch.Generator(device="cpu").manual_seed(R + D)
    z = torch.randn(R, D, generator=g).to(dev)
    z = (z.bfloat16() if bf16 else z).requires_grad_(True)
    w = (1 + 0.1 * torch.randn(D, generator=g)).to(dev).requires_grad_(True)
    b = (0.1 * torch.randn(D, generator=g)).to(dev).requires_grad_(True)
    gout = torch.randn(R, D, generator=g).to(dev)
    drop = torch.nn.Dropout(p).train()
    leaves = [z, w, b]

    def fused():
        return ops.dropout_relu_layer_norm(z, w, b, 1e-5, dropout_p=p, dropout_seed=12345)

    def chain():
        if bf16:      # what autocast makes of the line: layer_norm is on its float32 list
            with torch.autocast("cuda", dtype=torch.bfloat16):
                return F.layer_norm(F.relu(drop(z)), (D,), w, b, 1e-5)
        return F.layer_norm(F.relu(drop(z)), (D,), w, b, 1e-5)

    def fwd_bwd(fn):
        for x in leaves:
            x.grad = None
        fn().backward(gout)

    if p == 0:      # same results first, to fp32 rounding (with p > 0 the masks differ)
        a, c = fused(), chain()
        assert a.dtype == c.dtype == torch.float32 and float((a - c).detach().abs().max()) < 1e-4
    return {"fused": lambda: fwd_bwd(fused), "torch": lambda: fwd_bwd(chain)}


def timed(fn, iters):
    import torch
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1e-3


def bench_shape(R, D, bf16, p, rounds, min_seconds):
    import torch
    variants = make_chains(R, D, bf16, p)
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
    return {"bench": "dropout_relu_layer_norm", "what": "forward + backward, w_out excluded",
            "rows": R, "dim": D, "dtype": "bfloat16" if bf16 else "float32", "p": p,
            "rounds": rounds, "iters_per_round": iters,
            "us_per_iter_median": {k: round(v, 2) for k, v in med.items()},
            "us_per_iter_min_max": {k: [round(min(r), 2), round(max(r), 2)]
                                    for k, r in runs.items()},
            "us_per_iter_spread": {k: round(v, 2) for k, v in spread.items()},
            "speedup": round(med["torch"] / med["fused"], 3),
            "fused_beats_torch_by_more_than_its_spread":
                bool(med["torch"] - med["fused"] > spread["torch"]),
            "note": "us_per_iter is wall time between device events, host launch overhead of "
                    "each path included; spread = max - min round",
            "device": torch.cuda.get_device_name(0)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--min-seconds", type=float, default=0.5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "layer_epilogue_bench.jsonl"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("layer_epilogue_bench.py needs a GPU")
    lines = [bench_shape(R, D, bf16, p, a.rounds, a.min_seconds)
             for R, D in SHAPES for bf16 in (False, True) for p in PS]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for line in lines:
            text = json.dumps(line)
            print(text)
            f.write(text + "\n")
    print("fused ahead at every line by more than the torch chain's spread: {}".format(
        all(x["fused_beats_torch_by_more_than_its_spread"] for x in lines)))


if __name__ == "__main__":
    main()
