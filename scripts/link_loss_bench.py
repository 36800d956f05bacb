#!/usr/bin/env python3
"""Fused ops.link_loss against the torch expression of the reference's training step
(BCEWithLogitsLoss of the positive logits against ones plus that of the negative ones against
zeros), forward + backward, interleaved in one process and timed with device events.

    python scripts/link_loss_bench.py                   # P, N = 600, 600 and 600, 5400; fp32, bf16

Per (P, N, dtype) shape, the two variants are timed in `--rounds` rounds that alternate between
them; a round runs enough iterations for at least `--min-seconds / --rounds` of device time.
The bfloat16 torch side runs under torch.autocast('cuda', dtype=torch.bfloat16), as a training
loop with --amp has it; ops.link_loss takes the bfloat16 logits as they are.  The kernel
launches of one step (forward + backward) of each variant are counted with torch's profiler in
a separate pass after the timing.  Prints one JSON line per shape and appends it to
profiles/link_loss_bench.jsonl: the median round of each variant in microseconds per step, each
variant's own round-to-round spread (max - min), the launches per step, and whether the fused
side wins by more than the torch side's spread.
"""
import argparse
import json
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", type=int, nargs="+", default=[600, 600, 600, 5400],
                    help="P N pairs")
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--min-seconds", type=float, default=0.5)
    ap.add_argument("--profile-steps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "link_loss_bench.jsonl"))
    a = ap.parse_args()
    import torch
    import torch.nn.functional as F
    from torch.profiler import ProfilerActivity, profile
    if not torch.cuda.is_available():
        sys.exit("link_loss_bench.py needs a GPU")
    from gnnflow_amd import ops

    dev = torch.device("cuda", 0)

    def timed(fn, iters):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(iters):
            fn()
        stop.record()
        stop.synchronize()
        return start.elapsed_time(stop) * 1e-3

    def launches(fn, steps):
        """Kernels per step, counted by torch's profiler (copies and memsets are not kernels)."""
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            for _ in range(steps):
                fn()
            torch.cuda.synchronize()
        names = [e.name for e in prof.events()
                 if e.device_type == torch.autograd.DeviceType.CUDA
                 and not e.name.lower().startswith(("memcpy", "memset"))]
        # a name without its template and argument lists: "at::native::reduce_kernel"
        def short(n):
            kind = "<float>" if "<float>(" in n else "<bf16>" if "<unsigned short>(" in n else ""
            n = re.sub(r"^void ", "", n).replace("(anonymous namespace)::", "")
            return n.split("<")[0].split("(")[0] + kind
        return len(names) / steps, sorted({short(n) for n in names})

    for P, N in zip(a.shapes[0::2], a.shapes[1::2]):
        for dtype in (torch.float32, torch.bfloat16):
            g = torch.Generator(device=dev).manual_seed(P + N)
            pos = (3 * torch.randn(P, 1, device=dev, generator=g)).to(dtype).requires_grad_()
            neg = (3 * torch.randn(N, 1, device=dev, generator=g)).to(dtype).requires_grad_()
            amp = torch.autocast("cuda", dtype=torch.bfloat16, enabled=dtype == torch.bfloat16)

            def fused():
                return ops.link_loss(pos, neg)

            def composed():
                with amp:
                    return F.binary_cross_entropy_with_logits(pos, torch.ones_like(pos)) + \
                        F.binary_cross_entropy_with_logits(neg, torch.zeros_like(neg))

            def fwd_bwd(fn):
                pos.grad = neg.grad = None
                fn().backward()

            variants = {"fused_fwd_bwd": lambda: fwd_bwd(fused),
                        "torch_fwd_bwd": lambda: fwd_bwd(composed)}
            # the two sides compute the same thing at the sizes timed
            lf, lt = fused().detach(), composed().detach().float()
            torch.testing.assert_close(lf, lt)
            iters = {}
            for name, fn in variants.items():          # warm-up, then size a round
                timed(fn, 20)
                per = timed(fn, 50) / 50
                iters[name] = max(50, int(np.ceil(1.3 * a.min_seconds / a.rounds / per)))
            rounds = {name: [] for name in variants}
            for _ in range(a.rounds):
                for name, fn in variants.items():
                    rounds[name].append(timed(fn, iters[name]) / iters[name])
            us = {name: float(np.median(r)) * 1e6 for name, r in rounds.items()}
            spread = {name: (max(r) - min(r)) * 1e6 for name, r in rounds.items()}
            margin = us["torch_fwd_bwd"] - us["fused_fwd_bwd"]
            counts, kernels = {}, {}
            for name, fn in variants.items():
                try:
                    counts[name], kernels[name] = launches(fn, a.profile_steps)
                except Exception as e:      # the timing above stands without the count
                    counts[name], kernels[name] = None, ["profiler failed: {!r}".format(e)]
            out = {"bench": "link_loss", "P": P, "N": N, "dtype": str(dtype).split(".")[1],
                   "rounds": a.rounds, "iters_per_round": iters,
                   "timed_seconds": {n: float(np.sum(r)) * iters[n] for n, r in rounds.items()},
                   "us_per_step_median": {n: round(x, 2) for n, x in us.items()},
                   "us_per_step_min_max": {n: [round(min(r) * 1e6, 2), round(max(r) * 1e6, 2)]
                                           for n, r in rounds.items()},
                   "spread_us": {n: round(x, 2) for n, x in spread.items()},
                   "speedup_fwd_bwd": round(us["torch_fwd_bwd"] / us["fused_fwd_bwd"], 3),
                   "fused_fwd_bwd_margin_us": round(margin, 2),
                   "fused_beats_torch_by_more_than_spread": bool(margin > spread["torch_fwd_bwd"]),
                   "kernel_launches_per_step": counts, "kernels": kernels,
                   "loss": {"fused": float(lf), "torch": float(lt)},
                   "note": "us_per_step is wall time between device events over a loop of "
                           "forward + backward steps, host launch overhead of each path "
                           "included; launches counted by torch.profiler in a pass of its own",
                   "device": torch.cuda.get_device_name(0)}
            line = json.dumps(out)
            print(line, flush=True)
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
