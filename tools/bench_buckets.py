"""bucketed_accuracy and accuracy_over_hits on one MI355X at the reference's size, beside the numpy statements they
replace, timed in the same run on the same machine.

    python tools/bench_buckets.py --out profiles/buckets_probe.json

pfam/proteins.py:689-729 bins a [200 000, 300] float32 score array into 300 buckets in a Python loop, every iteration a
few passes over the whole array; proteins.py:502-507 takes cumsum / tile / mean over the correctness matrix of the same
shape.  One warm call of each function on a small array, then --reps timed calls at the full size, for three score
distributions -- uniform over (0, 1), clustered (normal, about twenty of the 300 buckets hold nearly every cell) and
single (every cell in one bucket, the worst case for an LDS histogram) -- and for bucketed_accuracy with and without the
merging of equal bins inside a wave (KNN355_BUCKET_AGG=1).  Of every timed call the wall clock and what last_buckets_ms reports by HIP events: uploads, kernels, downloads.
The numpy side (`numpy_buckets` and `numpy_accuracy_over_hits`, the reference's statements written out for this tool) runs
once on the first --reference-rows rows of the same arrays (the loop takes minutes at the full size); the row count it ran
on is printed, and its results are compared with the device's on those rows.  Nothing is gated on a speed.  Prints one JSON
line (and writes it to --out)."""
import argparse
import json
import os
import socket
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from knn_for_homology_amd import _lib, evaluation  # noqa: E402


def numpy_sem(a):
    """scipy.stats.sem's formula (its default ddof of 1) in numpy, for a box without scipy"""
    return np.std(a, ddof=1) / np.sqrt(len(a))


def numpy_buckets(correct, scores, smoothness, sem):
    """the host computation that bucketed_accuracy replaces: one mask per bucket over the whole array"""
    precision, errors = [], []
    for low in np.linspace(0, 1 - (1 / smoothness), smoothness):
        mask = (low < scores) & (scores <= low + (1 / smoothness))
        if mask.sum() == 0:
            continue
        inside = correct[mask]
        precision.append(inside.mean())
        errors.append(sem(inside))
    return np.asarray(precision), np.asarray(errors)


def numpy_accuracy_over_hits(correct, totals):
    """the host computation that accuracy_over_hits replaces"""
    return (correct.cumsum(axis=1) / np.tile(totals, (correct.shape[1], 1)).T).mean(axis=0)


def spread(values):
    return {"min": min(values), "median": float(np.median(values)), "max": max(values)}


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return out, time.perf_counter() - t0


def summary(calls):
    return {"wall_ms": spread([c["wall_ms"] for c in calls]), "upload_ms": spread([c["upload_ms"] for c in calls]),
            "kernel_ms": spread([c["kernel_ms"] for c in calls]), "download_ms": spread([c["download_ms"] for c in calls])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=200000)
    ap.add_argument("--k", type=int, default=300)
    ap.add_argument("--smoothness", type=int, default=300)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--reference-rows", type=int, default=20000, help="rows the numpy statements run on (0: skip them)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    try:
        from scipy.stats import sem
        sem_name = "scipy.stats.sem"
    except ImportError:
        sem, sem_name = numpy_sem, "numpy std / sqrt(n)"
    rng = np.random.default_rng(689)
    shape = (args.rows, args.k)
    correct = rng.random(shape) < 0.25
    totals = np.maximum(correct.sum(axis=1) + rng.integers(0, 100, args.rows), 1)
    inputs = {"uniform": rng.random(shape, dtype=np.float32),
              "clustered": np.clip(rng.normal(0.6, 0.011, shape), 0, 1).astype(np.float32),
              "single": np.full(shape, np.float32(0.6012))}
    evaluation.bucketed_accuracy(correct[:64], inputs["uniform"][:64], limit=args.k, smoothness=args.smoothness)
    evaluation.accuracy_over_hits(correct[:64], totals[:64], limit=args.k)
    rec = {"box": socket.gethostname(), "library": _lib.lib().knn_version().decode(), "numpy": np.__version__, "rows": args.rows, "k": args.k,
           "smoothness": args.smoothness, "reps": args.reps, "sem": sem_name}
    part = min(args.reference_rows, args.rows)
    for name, scores in inputs.items():
        for mode in ("merged", "plain"):
            os.environ["KNN355_BUCKET_AGG"] = "0" if mode == "plain" else "1"
            calls = []
            for _ in range(args.reps):
                got, seconds = timed(lambda: evaluation.bucketed_accuracy(correct, scores, limit=args.k, smoothness=args.smoothness))
                calls.append({"wall_ms": 1e3 * seconds, **evaluation.last_buckets_ms()["bucket_counts"]})
            rec[f"bucketed_accuracy_{name}_{mode}"] = summary(calls)
        os.environ.pop("KNN355_BUCKET_AGG")
        rec[f"buckets_filled_{name}"] = int(np.count_nonzero(got.count))
        rec[f"buckets_holding_99_percent_{name}"] = int(np.searchsorted(np.cumsum(np.sort(got.count)[::-1]), 0.99 * got.count.sum()) + 1)
        if part:
            (np_precision, np_sem), seconds = timed(lambda: numpy_buckets(correct[:part], scores[:part], args.smoothness, sem))
            dev = evaluation.bucketed_accuracy(correct[:part], scores[:part], limit=args.k, smoothness=args.smoothness)
            precision, errors = dev.reference_arrays()
            rec[f"numpy_buckets_{name}_s"] = seconds
            rec[f"precision_equal_bits_{name}"] = bool(np.array_equal(precision.view(np.uint64), np_precision.view(np.uint64)))
            ok = np_sem > 0
            rec[f"sem_max_relative_{name}"] = float(np.max(np.abs(errors[ok] - np_sem[ok]) / np_sem[ok])) if ok.any() else 0.0
    calls = []
    for _ in range(args.reps):
        curve, seconds = timed(lambda: evaluation.accuracy_over_hits(correct, totals, limit=args.k))
        calls.append({"wall_ms": 1e3 * seconds, **evaluation.last_buckets_ms()["hit_curve"]})
    rec["accuracy_over_hits"] = summary(calls)
    if part:
        np_curve, seconds = timed(lambda: numpy_accuracy_over_hits(correct[:part], totals[:part]))
        dev = evaluation.accuracy_over_hits(correct[:part], totals[:part], limit=args.k)
        rec["numpy_accuracy_over_hits_s"] = seconds
        rec["curve_equal_bits"] = bool(np.array_equal(dev.view(np.uint64), np_curve.view(np.uint64)))
    rec["reference_rows"] = part
    line = json.dumps(rec)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
