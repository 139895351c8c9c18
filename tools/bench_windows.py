"""rolling_means and even_bins on one MI355X at the size the rest of the evaluation suite is timed at, beside the
reference's statement in numpy, timed in the same run on the same machine.

    python tools/bench_windows.py --out profiles/windows_probe.json

seqvec_search/utils.py:103 takes numpy.convolve(data[order], ones(W) / W, "valid") of the key and of every correctness
column; hist_evenly takes mean and std over slices of the same order.  Here: 200 000 x 300 float32 keys flattened, five
boolean columns, W = 1000, then even_bins with 10 bins.  One warm call on a small array, then --reps timed calls of each;
of every call the wall clock and what knn_last_windows_info reports: the device allocations (host clock), then by HIP
events the uploads, the sort, the gather with the scans, the chains, the columns' means, the bins, the downloads.
The reference's statement (argsort, six convolutions) is timed on the first rows of the same arrays, doubling the row
count until a run takes about --numpy-seconds; the row count is reported, nothing is extrapolated.  On those rows the
columns' means are compared exactly with count / W and the key's means within the contract's bound.  Nothing is gated
on a speed.  Prints one JSON line (and writes it to --out)."""
import argparse
import json
import os
import socket
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from knn_for_homology_amd import _lib, evaluation  # noqa: E402


def reference_statement(keys, columns, window):
    """what the reference's scripts do, written for this tool: one argsort, rolling_mean of the key and of every column"""
    weights = np.ones(window) / window
    order = np.argsort(keys)
    return np.convolve(keys[order], weights, mode="valid"), [np.convolve(c[order], weights, mode="valid") for c in columns]


def spread(values):
    return {"min": min(values), "median": float(np.median(values)), "max": max(values)}


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return out, time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=200000)
    ap.add_argument("--k", type=int, default=300)
    ap.add_argument("--columns", type=int, default=5)
    ap.add_argument("--window", type=int, default=1000)
    ap.add_argument("--bins", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--numpy-seconds", type=float, default=10.0)
    ap.add_argument("--skip-numpy", action="store_true", help="the device side only")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    rng = np.random.default_rng(103)
    n = args.rows * args.k
    # n consecutive float32 bit patterns from 0x30000000 (positive, finite, no two equal) in random order
    keys = (np.uint32(0x30000000) + rng.permutation(n).astype(np.uint32)).view(np.float32).reshape(args.rows, args.k)
    columns = rng.random((args.columns, args.rows, args.k)) < 0.25
    evaluation.rolling_means(keys[:64], columns[:, :64], window=args.window)
    evaluation.even_bins(keys[:64], columns[:, :64], args.bins)
    rolling_calls, bin_calls = [], []
    for _ in range(args.reps):
        rolling, seconds = timed(lambda: evaluation.rolling_means(keys, columns, window=args.window))
        rolling_calls.append({"wall_ms": 1e3 * seconds, **evaluation.last_windows_info()})
        bins, seconds = timed(lambda: evaluation.even_bins(keys, columns, args.bins))
        bin_calls.append({"wall_ms": 1e3 * seconds, **evaluation.last_windows_info()})
    rec = {"box": socket.gethostname(), "library": _lib.lib().knn_version().decode(), "numpy": np.__version__, "rows": args.rows, "k": args.k,
           "columns": args.columns, "window": args.window, "bins": args.bins, "reps": args.reps,
           "rolling_means_wall_ms": spread([c["wall_ms"] for c in rolling_calls]), "even_bins_wall_ms": spread([c["wall_ms"] for c in bin_calls]),
           "rolling_means_calls": rolling_calls, "even_bins_calls": bin_calls}
    if not args.skip_numpy:
        rows, seconds = max(args.window // args.k + 1, 64), 0.0
        while True:
            flat, cols = keys[:rows].reshape(-1), [c[:rows].reshape(-1) for c in columns]
            (np_keys, np_cols), seconds = timed(lambda: reference_statement(flat, cols, args.window))
            if seconds >= args.numpy_seconds / 2 or rows >= args.rows:
                break
            rows = min(2 * rows, args.rows)
        ours = evaluation.rolling_means(flat, cols, window=args.window)
        bound = (2 * args.window + 4) * 2.0 ** -53 * np.convolve(np.abs(flat[np.argsort(flat)]).astype(np.float64), np.ones(args.window), mode="valid") / args.window
        rec.update({"numpy_rows": rows, "numpy_s": seconds, "numpy_columns_max_abs_diff": float(max(np.abs(a - b).max() for a, b in zip(ours.values, np_cols))),
                    "numpy_keys_within_bound": bool((np.abs(ours.keys - np_keys) <= bound * (1 + 1e-9)).all())})
    line = json.dumps(rec)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
