#!/usr/bin/env python
"""A validation pass's metrics: metrics.LinkMetrics on the GPU against the reference's way,
`torch.cat([pos, neg]).sigmoid().cpu()` plus scikit-learn per batch
(scripts/offline_edge_prediction.py:141-146 of the reference).

    python scripts/bench_link_metrics.py [--out profiles/link_metrics_microbench.txt]

The pass has the reference's shape: BATCHES batches of 600 positive scores and r * 600 negative
ones (r = 1 and r = 9), already on the device as EdgePredictor leaves them ([n, 1] float32
logits, seeded), then the mean over the batches.

    device   LinkMetrics.update(pos, neg) per batch (two sigmoids and the two launches of
             ops.link_metrics, no sync), one compute() at the end
    host     per batch the concatenation, the sigmoid, the copy to the host (a sync), then
             roc_auc_score and average_precision_score; scikit-learn where it imports, otherwise
             the sort-based numpy statement of the same two functions below -- the output says
             which

Method: one warm-up pass of either side, then ROUNDS rounds in which the sides alternate; a
round's figure is the host clock around one whole pass, which ends in a synchronisation on
either side (compute() / the last .cpu()), divided by the batches.  Reported: the median over
the rounds and their min - max, and once, before timing, how far the two sides' means are apart
(not a test: tests/test_gpu_link_metrics.py is).  No default of the package depends on these
figures."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

P, RATIOS, BATCHES, ROUNDS = 600, (1, 9), 300, 10


def host_functions():
    """(name, roc_auc_score, average_precision_score) for y_true, y_score on the host."""
    try:
        import sklearn
        from sklearn.metrics import average_precision_score, roc_auc_score
        return "scikit-learn " + sklearn.__version__, roc_auc_score, average_precision_score
    except ImportError:
        pass
    import numpy as np

    def curve(y_true, y_score):
        # true and false positives at each distinct threshold, highest first
        order = np.argsort(-y_score, kind="stable")
        s, y = y_score[order], y_true[order].astype(np.float64)
        last = np.r_[np.nonzero(np.diff(s))[0], len(s) - 1]
        tp = np.cumsum(y)[last]
        return tp, 1 + last - tp

    def roc_auc_score(y_true, y_score):
        tp, fp = curve(np.asarray(y_true), np.asarray(y_score))
        tp, fp = np.r_[0, tp], np.r_[0, fp]
        return float(np.sum(np.diff(fp) * (tp[1:] + tp[:-1])) / (2 * tp[-1] * fp[-1]))

    def average_precision_score(y_true, y_score):
        tp, fp = curve(np.asarray(y_true), np.asarray(y_score))
        return float(np.sum(np.diff(np.r_[0, tp]) * tp / (tp + fp)) / tp[-1])

    return "numpy (scikit-learn does not import here)", roc_auc_score, average_precision_score


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "link_metrics_microbench.txt"))
    ap.add_argument("--batches", type=int, default=BATCHES)
    ap.add_argument("--rounds", type=int, default=ROUNDS)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_link_metrics.py needs a GPU")
    from gnnflow_amd import LinkMetrics
    host_name, roc_auc_score, average_precision_score = host_functions()
    dev = torch.device("cuda", 0)
    metrics = LinkMetrics(dev)

    def device_pass(batches):
        metrics.reset()
        for pos, neg in batches:
            metrics.update(pos, neg)
        r = metrics.compute()
        return r["ap"], r["auc"]

    def host_pass(batches):
        aps, aucs = [], []
        for pos, neg in batches:
            y_pred = torch.cat([pos, neg], dim=0).sigmoid().cpu()
            y_true = torch.cat([torch.ones(pos.size(0)), torch.zeros(neg.size(0))], dim=0)
            aucs.append(roc_auc_score(y_true, y_pred))
            aps.append(average_precision_score(y_true, y_pred))
        return float(torch.tensor(aps).mean()), float(torch.tensor(aucs).mean())

    lines = ["link-metrics microbenchmark: one validation pass of {} batches, {} positives and "
             "r * {} negatives per batch;".format(args.batches, P, P),
             "host time per batch in microseconds (wall clock around the whole pass, which ends "
             "in a synchronisation),",
             "median of {} alternating rounds [min - max]; {}; host side: {}".format(
                 args.rounds, torch.cuda.get_device_name(0), host_name),
             "", "{:>3}  {:>30}  {:>30}  {:>11}  {}".format(
                 "r", "device (LinkMetrics)", "host (.sigmoid().cpu() + host)", "host/device",
                 "|mean ap| and |mean auc| apart")]
    for r in RATIOS:
        gen = torch.Generator(device=dev).manual_seed(100 + r)
        batches = [(torch.randn(P, 1, device=dev, generator=gen) + 0.5,
                    torch.randn(r * P, 1, device=dev, generator=gen))
                   for _ in range(args.batches)]
        (d_ap, d_auc), (h_ap, h_auc) = device_pass(batches), host_pass(batches)      # warm-up
        times = {0: [], 1: []}
        for _ in range(args.rounds):
            for k, fn in enumerate((device_pass, host_pass)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn(batches)
                times[k].append(1e6 * (time.perf_counter() - t0) / args.batches)
        med = [statistics.median(times[k]) for k in (0, 1)]
        cell = ["{:9.1f} [{:8.1f} -{:9.1f}]".format(med[k], min(times[k]), max(times[k]))
                for k in (0, 1)]
        lines.append("{:>3}  {:>30}  {:>30}  {:>11.1f}  {:.1e} {:.1e}".format(
            r, cell[0], cell[1], med[1] / med[0], abs(d_ap - h_ap), abs(d_auc - h_auc)))
        print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
