"""One density.density_curves call on one MI355X at the reference's size, and the same curves through scipy on the same
box's CPU, on synthetic input.

    python tools/bench_kde.py --out profiles/kde_probe.json

pfam/reverse_evaluate.py:65-70 draws DataFrame({"original": ..., "reversed": ...}).plot.density() over the first
principal component of the forward and the scrambled proteins: two columns, scipy.stats.gaussian_kde(column).evaluate on
pandas' 1000-point grid for each.  Here: [200 000, 2] float32, m = 1000.  One warm call, then --reps timed ones (wall
clock around the call, which ends with the results on the host); of the last call the split into the uploads, the
statistics kernels and the evaluation (HIP events inside knn_kde_stats / knn_kde_eval).  Then scipy's
gaussian_kde(column).evaluate(grid) over the same columns and grids, once, timed the same way, and the largest relative
difference between the two sets of curves.  Prints one JSON line (and writes it to --out).  Nothing is gated on it."""
import argparse
import json
import os
import socket
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from knn_for_homology_amd import _lib, density  # noqa: E402


def synthetic(n, c, seed):
    """bimodal float32 columns: the shape of a principal component over forward and scrambled proteins"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, c)) * np.where(rng.random((n, c)) < 0.5, 1.0, 0.6) + np.where(rng.random((n, c)) < 0.5, -2.5, 3.5)
    return np.ascontiguousarray(x.astype(np.float32))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=200000)
    ap.add_argument("--columns", type=int, default=2)
    ap.add_argument("--m", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-scipy", action="store_true", help="skip the CPU side")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    x = synthetic(args.n, args.columns, args.n)
    density.density_curves(x, args.m)
    ts = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        grids, dens = density.density_curves(x, args.m)
        ts.append(time.perf_counter() - t0)
    ms = density.last_ms()
    terms = float(args.n) * args.m * args.columns
    rec = {"box": socket.gethostname(), "library": _lib.lib().knn_version().decode(), "n": args.n, "columns": args.columns, "m": args.m,
           "dtype": "float32", "reps": args.reps, "density_curves_median_ms": 1e3 * float(np.median(ts)), "density_curves_min_ms": 1e3 * min(ts),
           "upload_ms": ms["upload"], "stats_kernels_ms": ms["stats"], "eval_kernels_ms": ms["eval"],
           "eval_gterms_per_s": terms / (ms["eval"] * 1e-3) / 1e9 if ms["eval"] > 0 else None, "finite": bool(np.isfinite(dens).all())}
    if not args.no_scipy:
        import scipy
        from scipy.stats import gaussian_kde
        t0 = time.perf_counter()
        theirs = np.stack([gaussian_kde(x[:, j]).evaluate(grids[j]) for j in range(args.columns)])
        rec["scipy_seconds_cpu"] = time.perf_counter() - t0
        rec["scipy"] = scipy.__version__
        rec["cpus"] = os.cpu_count()
        rec["ratio_scipy_over_median"] = rec["scipy_seconds_cpu"] / float(np.median(ts))
        rec["max_relative_difference"] = float(np.max(np.abs(dens - theirs) / theirs))
    line = json.dumps(rec)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
