"""evaluation.precision_recall_curve on one MI355X at the reference's size, on synthetic input: one process, one shape.

    python tools/pr_curve_probe.py --out profiles/pr_curve_probe.json

The reference's results script sweeps smoothness + 1 = 301 thresholds over 200 000 queries x 300 hits
(pfam/proteins.py:626-648).  Here: uniform random float32 scores, a fifth of the cells correct, totals = correct cells per
row (1 at least), 301 given thresholds (evenly spaced quantile levels, computed once outside the timing: the quantiles
are host work and not what is probed).  One warm call, then the wall clock around --reps calls of
evaluation.precision_recall_curve with pageable host arrays in and out: the uploads, the kernels, the downloads.
Prints one JSON line (and writes it to --out).  Nothing is gated on it."""
import argparse
import json
import os
import socket
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from knn_for_homology_amd import _lib, evaluation  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nq", type=int, default=200000)
    ap.add_argument("--k", type=int, default=300)
    ap.add_argument("--nthr", type=int, default=301)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    rng = np.random.default_rng(0)
    scores = rng.random((args.nq, args.k), dtype=np.float32)
    correct = rng.random((args.nq, args.k), dtype=np.float32) < 0.2
    totals = np.maximum(correct.sum(axis=1), 1).astype(np.int64)
    thresholds = np.quantile(scores[:2000], np.linspace(0, 1, args.nthr))
    evaluation.precision_recall_curve(correct, scores, totals, args.k, thresholds=thresholds)
    ts = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        recall, precision, _, counts = evaluation.precision_recall_curve(correct, scores, totals, args.k, thresholds=thresholds,
                                                                        want_counts=True)
        ts.append(time.perf_counter() - t0)
    # a direct count of the first and the middle threshold: the probe measures a call that computes the right thing
    same = all(int(counts[0][j]) == int((scores > thresholds[j]).sum()) for j in (0, args.nthr // 2))
    rec = {"box": socket.gethostname(), "library": _lib.lib().knn_version().decode(), "nq": args.nq, "k": args.k, "limit": args.k,
           "nthr": args.nthr, "input_bytes": int(scores.nbytes + correct.nbytes + totals.nbytes), "reps": args.reps,
           "median_ms": 1e3 * float(np.median(ts)), "min_ms": 1e3 * min(ts), "max_ms": 1e3 * max(ts),
           "counts_equal_a_direct_count": bool(same), "recall_first": float(recall[0]), "precision_first": float(precision[0])}
    line = json.dumps(rec)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
