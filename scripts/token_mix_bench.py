#!/usr/bin/env python3
"""What a GraphMixer block costs, forward plus backward, with its halves on torch or on the fused
ops, one GPU and one process: a MixerBlock(32, 100, 0.5, 4.0, dropout) on x [N, 32, 100], N in
{1200, 8000}, in eval() and in training with dropout 0.1, the plain block against

  token_mix   ..., fused_token_mix=True
  both        ..., fused_token_mix=True, fused_feed_forward=True
  ff          ..., fused_feed_forward=True          (the other half alone, from the same run)

each fused block on the plain block's state_dict.

    python scripts/token_mix_bench.py [--rounds 7] [--calls 5]

scripts/feed_forward_bench.py's protocol: both routes are warmed, then they alternate inside
every round; a round of a route is --calls calls (forward, backward to x and the parameters)
ending in torch.cuda.synchronize().  On the first call of every eval() line the two routes'
outputs are asserted to agree to 1e-4 of the largest output.  One JSON line per case, appended
to profiles/token_mix_bench.jsonl: the median round in microseconds per call, its min and max,
each route's peak allocated memory over one call above what was held before it, how torch
compares with fused, and whether the difference exceeds the rounds' spread.  Host wall time only:
the kernels alone are not measured here.
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
    ap.add_argument("--rows", type=int, nargs="+", default=[1200, 8000])
    ap.add_argument("--kinds", nargs="+", default=["token_mix", "both", "ff"])
    ap.add_argument("--dropout", type=float, default=0.1)
    ap.add_argument("--calls", type=int, default=5, help="calls per round")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--label", default="", help="a name for this run, for the record")
    ap.add_argument("--measured-by", default="", help="who ran this, for the record")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "token_mix_bench.jsonl"))
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    if not torch.cuda.is_available():
        sys.exit("token_mix_bench.py needs a GPU")
    from gnnflow_amd.models.graphmixer import MixerBlock

    dev = torch.device("cuda", 0)

    def blocks(kind):
        torch.manual_seed(0)
        pair = [MixerBlock(32, 100, 0.5, 4.0, a.dropout),
                MixerBlock(32, 100, 0.5, 4.0, a.dropout, fused_token_mix=kind != "ff",
                           fused_feed_forward=kind != "token_mix")]
        pair[1].load_state_dict(pair[0].state_dict())
        return {"torch": pair[0].to(dev), "fused": pair[1].to(dev)}

    for kind in a.kinds:
        routes = blocks(kind)
        shapes = [(N, 32, 100) for N in a.rows]
        for shape in shapes:
            x = torch.randn(shape, device=dev, requires_grad=True)
            dout = torch.randn(shape, device=dev)

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
                out = {"bench": "token_mix", "kind": kind, "label": a.label,
                       "shape": list(shape), "mode": mode,
                       "dropout": a.dropout if mode == "train" else 0.0,
                       "calls_per_round": a.calls, "rounds": a.rounds,
                       "note": "host wall time over the calls of a round (one block forward and "
                               "backward each), ending in a device synchronise, divided by the "
                               "calls; the routes alternate inside every round; peak memory is "
                               "one call's, above what was held",
                       "measured_by": a.measured_by, "device": torch.cuda.get_device_name(0)}
                fused_out, fused_peak = peak(routes["fused"], keep=mode == "eval")
                torch_out, torch_peak = peak(routes["torch"], keep=mode == "eval")
                if mode == "eval":      # the two routes agree
                    assert (fused_out - torch_out).abs().max() <= 1e-4 * torch_out.abs().max()
                del fused_out, torch_out
                timed(routes["torch"])
                timed(routes["fused"])
                fr, tr = [], []
                for _ in range(a.rounds):
                    fr.append(timed(routes["fused"]))
                    tr.append(timed(routes["torch"]))
                f_us, f_spread = float(np.median(fr)) * 1e6, (max(fr) - min(fr)) * 1e6
                t_us, t_spread = float(np.median(tr)) * 1e6, (max(tr) - min(tr)) * 1e6
                out.update({"fused_us_per_call_median": round(f_us, 1),
                            "fused_us_per_call_min_max": [round(min(fr) * 1e6, 1),
                                                          round(max(fr) * 1e6, 1)],
                            "fused_peak_gb": round(fused_peak / 2 ** 30, 3),
                            "torch_us_per_call_median": round(t_us, 1),
                            "torch_us_per_call_min_max": [round(min(tr) * 1e6, 1),
                                                          round(max(tr) * 1e6, 1)],
                            "torch_peak_gb": round(torch_peak / 2 ** 30, 3),
                            "torch_over_fused": round(t_us / f_us, 2),
                            "difference_exceeds_spread": bool(
                                abs(t_us - f_us) > max(t_spread, f_spread))})
                line = json.dumps(out)
                print(line, flush=True)
                os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                with open(a.out, "a") as f:
                    f.write(line + "\n")
            del x, dout
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
