#!/usr/bin/env python
"""Fused ops.edge_score against the torch expression it replaces, forward + backward, timed on
the device with HIP events.

    python scripts/bench_edge_score.py [--out profiles/edge_score_microbench.txt]

Two pairs per shape (B src rows, D columns, r = 2 dst blocks):

    op      ops.edge_score(s, d, w, b)  against  out_fc(relu(s + d_pos)), out_fc(relu(s + d_neg))
            on the same leaf tensors s [B, D] and d [2B, D]
    module  nn.EdgePredictor(D) on h [3B, D] with fused_score on against off (the Linear layers
            included: one dst_fc GEMM over 2B rows against two over B rows)

Each is forward + backward with a fixed output gradient.  Method: 50 warm-up iterations of every
variant, then ROUNDS rounds in which the variants alternate; in a round a variant runs ITERS
iterations between two events on the current stream, and the round's figure is the elapsed
device time / ITERS -- the stream's time from the first launch to the last kernel's end, the gaps
in which it waits for the host to enqueue the next launch included: at these sizes that is what
a training step pays.  Reported: the median over the rounds and their min - max.  The results of
both sides of a pair are compared once before timing (not a test: tests/test_gpu_edge_score.py
is).  nn.FUSED_EDGE_SCORE_DEFAULT is True only if the fused side wins both pairs at B = 600,
D = 100."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(600, 100), (600, 172), (6000, 100), (6000, 172)]
WARMUP, ROUNDS, ITERS = 50, 30, 200


def variants(B, D):
    import torch
    import torch.nn.functional as F
    from gnnflow_amd import nn as gnn
    from gnnflow_amd import ops
    gen = torch.Generator(device="cuda").manual_seed(B + D)

    def rand(*shape):
        return torch.randn(*shape, device="cuda", generator=gen)
    s, d = rand(B, D).requires_grad_(True), rand(2 * B, D).requires_grad_(True)
    w, b = rand(1, D).requires_grad_(True), rand(1).requires_grad_(True)
    g, h = rand(2 * B, 1), rand(3 * B, D).requires_grad_(True)
    leaves = (s, d, w, b)

    def op_fused():
        out = ops.edge_score(s, d, w, b)
        return (out,) + torch.autograd.grad(out, leaves, g)

    def op_torch():
        out = torch.cat([F.linear(F.relu(s + d[:B]), w, b), F.linear(F.relu(s + d[B:]), w, b)])
        return (out,) + torch.autograd.grad(out, leaves, g)

    torch.manual_seed(B + D)
    model = gnn.EdgePredictor(D).cuda()
    params = (h,) + tuple(model.parameters())

    def module(fused):
        def run():
            model.fused_score = fused
            out = torch.cat(model(h))
            return (out,) + torch.autograd.grad(out, params, g)
        return run

    return {"op": (op_fused, op_torch), "module": (module(True), module(False))}


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "edge_score_microbench.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_edge_score.py needs a GPU")
    lines = ["edge_score microbenchmark: forward + backward, device time per iteration in "
             "microseconds (HIP events),",
             "median of {} alternating rounds of {} iterations [min - max]; {}".format(
                 ROUNDS, ITERS, torch.cuda.get_device_name(0)),
             "(time between two events around the iterations: launch gaps included, so a chain "
             "of small kernels",
             " is bound by the pace at which the host enqueues them -- B = 600 and B = 6000 "
             "cost the same)",
             "", "{:<8}{:>6}{:>5}  {:>26}  {:>26}  {:>9}".format(
                 "pair", "B", "D", "fused", "torch", "torch/fused")]
    verdict = {}
    for B, D in SHAPES:
        for name, (fused, plain) in variants(B, D).items():
            worst = max(float(((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).detach())
                        for a, b in zip(fused(), plain()))
            for _ in range(WARMUP):
                fused()
                plain()
            times = {0: [], 1: []}
            for _ in range(ROUNDS):
                for k, fn in enumerate((fused, plain)):
                    start, end = (torch.cuda.Event(enable_timing=True) for _ in range(2))
                    start.record()
                    for _ in range(ITERS):
                        fn()
                    end.record()
                    end.synchronize()
                    times[k].append(1e3 * start.elapsed_time(end) / ITERS)
            med = [statistics.median(times[k]) for k in (0, 1)]
            cell = ["{:8.2f} [{:7.2f} -{:8.2f}]".format(med[k], min(times[k]), max(times[k]))
                    for k in (0, 1)]
            lines.append("{:<8}{:>6}{:>5}  {:>26}  {:>26}  {:>9.2f}   max rel. difference {:.1e}"
                         .format(name, B, D, cell[0], cell[1], med[1] / med[0], worst))
            verdict[(name, B, D)] = med[0] < med[1]
            print(lines[-1], flush=True)
    win = verdict[("op", 600, 100)] and verdict[("module", 600, 100)]
    lines += ["", "fused ahead at B = 600, D = 100 (op and module): {} -> "
              "nn.FUSED_EDGE_SCORE_DEFAULT = {}".format("yes" if win else "no", win)]
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
