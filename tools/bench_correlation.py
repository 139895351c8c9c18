"""correlations (Pearson's r and Spearman's rho from one call) on one MI355X at the size the rest of the evaluation suite
is timed at, beside the reference's two statements in scipy, timed once in the same run on the same machine and arrays.

    python tools/bench_correlation.py --out profiles/correlation_probe.json

cath/cath.py:949-952 prints scipy.stats.pearsonr(scores_best, logged) and scipy.stats.spearmanr(scores_best,
e_values_cath).  Here: 200 000 x 300 float32 cosine-like scores against as many float64 E-values with the ties such data
has (scores repeat at float32 resolution, E-values repeat and underflow to exact zeros), flattened.  One warm call on a
small array, then --reps timed calls of evaluation.correlations(scores, logged); of every call the wall clock and what
knn_last_correlate_info reports: the device allocations (host clock), then by HIP events the uploads, the two sorts, the
ranks (tie runs and scatter), the moments and the downloads.  The two scipy statements run once each.  The statistics of
both sides are reported with their differences.  Nothing is gated on a speed.  Prints one JSON line (and writes it to
--out)."""
import argparse
import json
import os
import socket
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from knn_for_homology_amd import _lib, evaluation  # noqa: E402


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
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--skip-scipy", action="store_true", help="the device side only")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    rng = np.random.default_rng(949)
    n = args.rows * args.k
    e_values = np.exp(np.minimum(rng.normal(-300, 200, n), 700))  # about one in seventy underflows to an exact zero
    repeat = rng.random(n) < 0.1
    e_values[repeat] = e_values[rng.integers(0, n, int(repeat.sum()))]
    scores = np.clip(0.5 - 0.002 * np.log10(e_values + 1e-300) + rng.normal(0, 0.1, n), -1, 1).astype(np.float32)
    with np.errstate(divide="ignore"):
        logged = np.log(e_values)
    logged[np.isinf(logged)] = -(10 ** 9)
    evaluation.correlations(scores[:4096], logged[:4096])
    calls, results = [], None
    for _ in range(args.reps):
        results, seconds = timed(lambda: evaluation.correlations(scores, logged))
        calls.append({"wall_ms": 1e3 * seconds, **evaluation.last_correlate_ms()})
    rec = {"box": socket.gethostname(), "library": _lib.lib().knn_version().decode(), "numpy": np.__version__, "rows": args.rows, "k": args.k, "reps": args.reps,
           "zeros": int((e_values == 0).sum()), "distinct_scores": int(np.unique(scores).size), "distinct_e_values": int(np.unique(e_values).size),
           "pearson": results[0].statistic, "spearman": results[1].statistic, "wall_ms": spread([c["wall_ms"] for c in calls]), "calls": calls}
    if not args.skip_scipy:
        import scipy
        from scipy.stats import pearsonr, spearmanr
        theirs_r, r_seconds = timed(lambda: pearsonr(scores, logged))
        theirs_rho, rho_seconds = timed(lambda: spearmanr(scores, e_values))
        rec.update({"scipy": scipy.__version__, "scipy_pearsonr_s": r_seconds, "scipy_spearmanr_s": rho_seconds, "scipy_pearson": float(theirs_r.statistic),
                    "scipy_spearman": float(theirs_rho.statistic), "pearson_abs_diff": abs(float(theirs_r.statistic) - results[0].statistic),
                    "spearman_abs_diff": abs(float(theirs_rho.statistic) - results[1].statistic)})
    line = json.dumps(rec)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
