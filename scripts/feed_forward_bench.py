#!/usr/bin/env python3
"""What a sequence model's block costs, forward plus backward, with its feed-forward on torch or
on ops.feed_forward, one GPU and one process:

  ff        EncoderBlock(C, H, dropout)                  vs  ..., fused_feed_forward=True
  ff+att    EncoderBlock(C, H, dropout)                  vs  ..., fused_attention=True,
                                                             fused_feed_forward=True
  mixer     MixerBlock(32, 100, 0.5, 4.0, dropout)       vs  ..., fused_feed_forward=True

the encoder blocks on x [N, S, C], C = 200 and H = 2, S in {16, 64}; the mixer block on x [N, 32,
100]; N in {1200, 8000}; in eval() and in training with dropout 0.1; the fused block on the torch
block's state_dict.

    python scripts/feed_forward_bench.py [--rounds 7] [--calls 10]

scripts/sequence_attention_bench.py's protocol: both routes are warmed, then they alternate inside
every round; a round of a route is --calls calls (forward, backward to x and the parameters)
ending in torch.cuda.synchronize().  On the first call of every eval() line the two routes'
outputs are asserted to agree to 1e-4 of the largest output.  One JSON line per case, appended
to profiles/feed_forward_bench.jsonl: the median round in microseconds per call, its min and max,
each route's peak allocated memory over one call above what was held before it, how torch
compares with fused, and whether the difference exceeds the rounds' spread.  Host wall time only:
the kernels alone are not measured here.

    python scripts/feed_forward_bench.py --bf16 [--kinds ff mixer]

measures fused_feed_forward="bfloat16" instead, on the ff and mixer lines and by the same protocol,
four routes alternating inside every round: `bf16` (the flag, outside autocast) against `fused`
(fused_feed_forward=True, the float32 kernels of the same build), and `bf16_autocast` (the flag
inside torch.autocast("cuda", dtype=torch.bfloat16)) against `torch_autocast` (the plain block
inside the same region).  In eval() the bf16 route's output is asserted to agree with the float32
fused route's to 2e-2 of the largest output.  One JSON line per case with "bench":
"feed_forward_bf16": every route's median, min-max and peak, and the two ratios.
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
    ap.add_argument("--length", type=int, nargs="+", default=[16, 64])
    ap.add_argument("--kinds", nargs="+", default=["ff", "ff+att", "mixer"])
    ap.add_argument("--dropout", type=float, default=0.1)
    ap.add_argument("--calls", type=int, default=10, help="calls per round")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--bf16", action="store_true",
                    help='measure fused_feed_forward="bfloat16" against its two yardsticks')
    ap.add_argument("--label", default="", help="a name for this run, for the record")
    ap.add_argument("--measured-by", default="", help="who ran this, for the record")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "feed_forward_bench.jsonl"))
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    if not torch.cuda.is_available():
        sys.exit("feed_forward_bench.py needs a GPU")
    from gnnflow_amd.models.dygformer import EncoderBlock
    from gnnflow_amd.models.graphmixer import MixerBlock

    dev = torch.device("cuda", 0)

    def make(kind, flag):
        if kind == "mixer":
            return MixerBlock(32, 100, 0.5, 4.0, a.dropout, fused_feed_forward=flag)
        return EncoderBlock(200, 2, a.dropout, fused_feed_forward=flag)

    def blocks(kind):      # route -> (block, inside bfloat16 autocast?)
        torch.manual_seed(0)
        if a.bf16:
            plain, fused, bf16 = (make(kind, flag).to(dev) for flag in (False, True, "bfloat16"))
            fused.load_state_dict(plain.state_dict())
            bf16.load_state_dict(plain.state_dict())
            return {"bf16": (bf16, False), "fused": (fused, False),
                    "bf16_autocast": (bf16, True), "torch_autocast": (plain, True)}
        if kind == "mixer":
            pair = [MixerBlock(32, 100, 0.5, 4.0, a.dropout, fused_feed_forward=f)
                    for f in (False, True)]
        else:
            pair = [EncoderBlock(200, 2, a.dropout),
                    EncoderBlock(200, 2, a.dropout, fused_attention=kind == "ff+att",
                                 fused_feed_forward=True)]
        pair[1].load_state_dict(pair[0].state_dict())
        return {"torch": (pair[0].to(dev), False), "fused": (pair[1].to(dev), False)}

    def record(out):
        line = json.dumps(out)
        print(line, flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")

    def bf16_lines(out, routes, mode, peak, timed):
        outs, peaks = {}, {}
        for name, route in routes.items():
            outs[name], peaks[name] = peak(route, keep=mode == "eval")
        if mode == "eval":      # bfloat16 operands against the float32 kernels
            assert (outs["bf16"] - outs["fused"]).abs().max() <= 2e-2 * outs["fused"].abs().max()
        outs.clear()
        for route in routes.values():
            timed(route)
        rounds = {name: [] for name in routes}
        for _ in range(a.rounds):
            for name, route in routes.items():
                rounds[name].append(timed(route))
        med = {name: float(np.median(r)) * 1e6 for name, r in rounds.items()}
        spread = {name: (max(r) - min(r)) * 1e6 for name, r in rounds.items()}
        for name, r in rounds.items():
            out[name + "_us_per_call_median"] = round(med[name], 1)
            out[name + "_us_per_call_min_max"] = [round(min(r) * 1e6, 1), round(max(r) * 1e6, 1)]
            out[name + "_peak_gb"] = round(peaks[name] / 2 ** 30, 3)
        for ours, other in (("bf16", "fused"), ("bf16_autocast", "torch_autocast")):
            out[other + "_over_" + ours] = round(med[other] / med[ours], 2)
            out[other + "_difference_exceeds_spread"] = bool(
                abs(med[other] - med[ours]) > max(spread[other], spread[ours]))
        record(out)

    for kind in a.kinds:
        if a.bf16 and kind == "ff+att":
            continue
        routes = blocks(kind)
        shapes = [(N, 32, 100) for N in a.rows] if kind == "mixer" else \
            [(N, S, 200) for N in a.rows for S in a.length]
        for shape in shapes:
            x = torch.randn(shape, device=dev, requires_grad=True)
            dout = torch.randn(shape, device=dev)

            def call(route, keep=False):
                block, cast = route
                with torch.autocast("cuda", dtype=torch.bfloat16, enabled=cast):
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
                for block, _ in routes.values():
                    block.train(mode == "train")
                out = {"bench": "feed_forward_bf16" if a.bf16 else "feed_forward", "kind": kind,
                       "label": a.label,
                       "shape": list(shape), "mode": mode,
                       "dropout": a.dropout if mode == "train" else 0.0,
                       "calls_per_round": a.calls, "rounds": a.rounds,
                       "note": "host wall time over the calls of a round (one block forward and "
                               "backward each), ending in a device synchronise, divided by the "
                               "calls; the routes alternate inside every round; peak memory is "
                               "one call's, above what was held",
                       "measured_by": a.measured_by, "device": torch.cuda.get_device_name(0)}
                if a.bf16:
                    bf16_lines(out, routes, mode, peak, timed)
                    continue
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
                record(out)
            del x, dout
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
