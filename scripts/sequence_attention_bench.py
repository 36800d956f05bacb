#!/usr/bin/env python3
"""What one of DyGFormer's encoder blocks costs, forward plus backward, on its two routes, one GPU
and one process:

  (a) torch:  models.dygformer.EncoderBlock(C, H, dropout): nn.MultiheadAttention's own attention
  (b) fused:  EncoderBlock(C, H, dropout, fused_attention=True) on the same state_dict: in_proj ->
              ops.sequence_attention -> out_proj

on x [N, S, C], C = 200 and H = 2 (head_dim 100), N in {1200, 6000, 8000, 40000}, S in {16, 64,
128}, in eval() and in training with dropout 0.1.

    python scripts/sequence_attention_bench.py [--rounds 7] [--calls 10]

scripts/patch_project_bench.py's protocol: both routes are warmed, then (b) and (a) alternate
inside every round; a round of a route is --calls calls (forward, backward to x and the
parameters) ending in torch.cuda.synchronize().  On the first call of every line the two routes'
outputs are asserted to agree in eval() to 1e-4 of the largest output.  One JSON line per (N, S,
mode), appended to profiles/sequence_attention_bench.jsonl: the median round in microseconds per
call, its min and max, each route's peak allocated memory over one call above what was held
before it, how (a) compares with (b), and whether the difference exceeds the rounds' spread.  A
line whose torch route runs out of memory says so and keeps the fused figures.  Host wall time
only: the kernels alone are not measured here.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[1200, 6000, 8000, 40000])
    ap.add_argument("--length", type=int, nargs="+", default=[16, 64, 128])
    ap.add_argument("--dim", type=int, default=200)
    ap.add_argument("--heads", type=int, default=2)
    ap.add_argument("--dropout", type=float, default=0.1)
    ap.add_argument("--calls", type=int, default=10, help="calls per round")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--label", default="", help="a name for this run, for the record")
    ap.add_argument("--measured-by", default="", help="who ran this, for the record")
    ap.add_argument("--out",
                    default=os.path.join(ROOT, "profiles", "sequence_attention_bench.jsonl"))
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    if not torch.cuda.is_available():
        sys.exit("sequence_attention_bench.py needs a GPU")
    from gnnflow_amd.models.dygformer import EncoderBlock

    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    routes = {"torch": EncoderBlock(a.dim, a.heads, a.dropout).to(dev),
              "fused": EncoderBlock(a.dim, a.heads, a.dropout, fused_attention=True).to(dev)}
    routes["fused"].load_state_dict(routes["torch"].state_dict())

    for N in a.rows:
        for S in a.length:
            x = torch.randn(N, S, a.dim, device=dev, requires_grad=True)
            dout = torch.randn(N, S, a.dim, device=dev)

            def call(block, keep=False):
                out = block(x)
                out.backward(dout)
                x.grad = None
                block.zero_grad(set_to_none=True)
                return out.detach() if keep else None

            def timed(block):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.calls):
                    call(block)
                torch.cuda.synchronize()
                return (time.perf_counter() - t0) / a.calls

            def peak(block, keep=False):      # (result, peak bytes above what is held)
                torch.cuda.synchronize()
                held = torch.cuda.memory_allocated()
                torch.cuda.reset_peak_memory_stats()
                got = call(block, keep)
                torch.cuda.synchronize()
                return got, torch.cuda.max_memory_allocated() - held

            for mode in ("eval", "train"):
                for block in routes.values():
                    block.train(mode == "train")
                out = {"bench": "sequence_attention", "label": a.label, "N": N, "S": S,
                       "dim": a.dim, "heads": a.heads, "mode": mode,
                       "dropout": a.dropout if mode == "train" else 0.0,
                       "calls_per_round": a.calls, "rounds": a.rounds,
                       "note": "host wall time over the calls of a round (one EncoderBlock "
                               "forward and backward each), ending in a device synchronise, "
                               "divided by the calls; the routes alternate inside every round; "
                               "peak memory is one call's, above what was held",
                       "measured_by": a.measured_by, "device": torch.cuda.get_device_name(0)}
                fused_out, fused_peak = peak(routes["fused"], keep=mode == "eval")
                try:
                    torch_out, torch_peak = peak(routes["torch"], keep=mode == "eval")
                    if mode == "eval":      # the two routes agree
                        assert (fused_out - torch_out).abs().max() <= 1e-4 * torch_out.abs().max()
                    del torch_out
                    timed(routes["torch"])
                    fits = True
                except torch.cuda.OutOfMemoryError:
                    fits = False
                    x.grad = None
                    torch.cuda.empty_cache()
                del fused_out
                timed(routes["fused"])
                fr, tr = [], []
                for _ in range(a.rounds):
                    fr.append(timed(routes["fused"]))
                    if fits:
                        tr.append(timed(routes["torch"]))
                f_us, f_spread = float(np.median(fr)) * 1e6, (max(fr) - min(fr)) * 1e6
                out.update({"fused_us_per_call_median": round(f_us, 1),
                            "fused_us_per_call_min_max": [round(min(fr) * 1e6, 1),
                                                          round(max(fr) * 1e6, 1)],
                            "fused_peak_gb": round(fused_peak / 2 ** 30, 3)})
                if fits:
                    t_us, t_spread = float(np.median(tr)) * 1e6, (max(tr) - min(tr)) * 1e6
                    out.update({"torch_us_per_call_median": round(t_us, 1),
                                "torch_us_per_call_min_max": [round(min(tr) * 1e6, 1),
                                                              round(max(tr) * 1e6, 1)],
                                "torch_peak_gb": round(torch_peak / 2 ** 30, 3),
                                "torch_over_fused": round(t_us / f_us, 2),
                                "difference_exceeds_spread": bool(
                                    abs(t_us - f_us) > max(t_spread, f_spread))})
                else:
                    out["torch_route"] = "skipped: out of memory"
                line = json.dumps(out)
                print(line, flush=True)
                os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                with open(a.out, "a") as f:
                    f.write(line + "\n")
            del x, dout
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
