"""Times ops.edge_rank (k = 10, with a reference score) against the torch expression for the same
result: (w * relu(src[:, None] + cand[None])).sum(-1) + b over chunks of the candidates small
enough for the [B, chunk, D] intermediate to fit, two comparisons with the reference score per
chunk, torch.topk per chunk and one torch.topk over the chunks' lists.

Device events around `--iters` calls after `--warmup` calls, `--rounds` rounds alternating the
two sides; the median round and the spread of each side are printed.  The operation count of the
score is B * C * D * 4 (add, max, multiply, add; the library is built without contraction).

    python scripts/bench_edge_rank.py [--out profiles/edge_rank_microbench.txt]
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from gnnflow_amd import ops

B, D, K = 600, 100, 10
CANDIDATES = (10_000, 100_000)
TORCH_CHUNK = 2048      # [600, 2048, 100] float32 = 492 MB per intermediate


def torch_rank(src, cand, w, b, ref, k):
    vals, idx = [], []
    greater = torch.zeros(src.shape[0], dtype=torch.int64, device=src.device)
    equal = torch.zeros_like(greater)
    for a in range(0, cand.shape[0], TORCH_CHUNK):
        c = cand[a:a + TORCH_CHUNK]
        s = (torch.relu(src[:, None, :] + c[None, :, :]) * w).sum(-1) + b
        greater += (s > ref[:, None]).sum(1)
        equal += (s == ref[:, None]).sum(1)
        v, i = torch.topk(s, min(k, c.shape[0]), dim=1)
        vals.append(v)
        idx.append(i + a)
    v, pick = torch.topk(torch.cat(vals, 1), k, dim=1)
    return v, torch.cat(idx, 1).gather(1, pick), greater, equal


def time_ms(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_edge_rank needs a GPU")
    lines = ["ops.edge_rank against the chunked torch expression: B = {}, D = {}, k = {}, "
             "with ref_score; {} on {}".format(B, D, K, torch.__version__,
                                               torch.cuda.get_device_name(0)),
             "ms per call: median of {} rounds of {} calls (min .. max)".format(a.rounds, a.iters)]
    g = torch.Generator(device="cuda").manual_seed(0)
    for C in CANDIDATES:
        src = torch.randn(B, D, device="cuda", generator=g)
        cand = torch.randn(C, D, device="cuda", generator=g)
        w = torch.randn(D, device="cuda", generator=g)
        b = torch.randn(1, device="cuda", generator=g)
        ref = ops.edge_score(src, cand[:B].contiguous(), w, b).reshape(B)
        fused = lambda: ops.edge_rank(src, cand, w, b, k=K, ref_score=ref)
        plain = lambda: torch_rank(src, cand, w, b, ref, K)
        f, p = fused(), plain()
        same = bool((f.indices == p[1]).all()) and bool((f.greater == p[2]).all())
        close = float((f.values - p[0]).abs().max())
        tf, tp = [], []
        for _ in range(a.rounds):      # alternating
            tf.append(time_ms(fused, a.warmup, a.iters))
            tp.append(time_ms(plain, a.warmup, a.iters))
        mf, mp = statistics.median(tf), statistics.median(tp)
        ops_count = 4.0 * B * C * D
        lines.append("C = {:6d}  edge_rank {:8.3f} ({:.3f} .. {:.3f})   torch {:8.3f} ({:.3f} .. "
                     "{:.3f})   torch / edge_rank {:.2f}   edge_rank {:.2f} Tflop/s of score "
                     "arithmetic".format(C, mf, min(tf), max(tf), mp, min(tp), max(tp), mp / mf,
                                         ops_count / (mf * 1e-3) / 1e12))
        lines.append("            same top-{} indices and greater counts as torch: {}; largest "
                     "value difference {:.3g} (torch sums in another order)".format(K, same, close))
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
