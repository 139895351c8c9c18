"""ranked_precision_recall and score_quantiles on one MI355X at the reference's size, beside the host computation they
replace, timed in the same run on the same machine.

    python tools/bench_rank.py --out profiles/rank_probe.json

pfam/pfam.py:570-583 ranks every hit of a [200 000, 300] score array at once and reads precision and recall at 10 000
recall levels; pfam/proteins.py:626-648 takes numpy.quantile of the same array at 301 points.  Per key type (float32,
float64): one warm call of each function on a small array, then --reps timed calls at the full size; of every timed call
the wall clock and what knn_last_rank_info reports -- on the host's clock the device allocations and the packing of the
columns, by HIP events the upload of the two arrays, the sort, the scan of the flags, the look-ups with their downloads
-- and the passes the sort ran and skipped.  What the wall clock holds beyond those six is the host side of the
function (levels and targets, the divisions, the interpolation) and the freeing of the device buffers as the call
returns.  --limit ranks the first columns only (the reference's `first_10` curve is --limit 10).
The host side (`host_curve`, written for this tool, and numpy.quantile) runs once on the same arrays.  The results are
compared (the curve exactly when no two scores are equal, the quantiles exactly) and the outcome is recorded; nothing is
gated on a speed.  Prints one JSON line per key type (and writes them to --out)."""
import argparse
import json
import os
import socket
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from knn_for_homology_amd import _lib, evaluation  # noqa: E402


def host_curve(scores, correct, total, levels):
    """The host computation that ranked_precision_recall replaces, written for this tool: rank every score with numpy's
    default sort, count the correct hits along the ranking, and read recall and precision at the first rank whose recall
    reaches each level (the last rank when none does).  All levels are looked up in one vectorised searchsorted; the
    reference looks them up one at a time in a Python loop, which this figure therefore does not hold."""
    ranking = np.argsort(scores, axis=None)
    found = np.cumsum(np.take(correct, ranking))
    reached = found / total
    at = np.minimum(np.searchsorted(reached, levels), found.size - 1)
    return reached[at], found[at] / (at + 1)


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
    ap.add_argument("--points", type=int, default=10000)
    ap.add_argument("--smoothness", type=int, default=300)
    ap.add_argument("--limit", type=int, default=None, help="rank the first LIMIT columns only (default: all k)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip-numpy", action="store_true", help="the device side only")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    rng = np.random.default_rng(561)
    n = args.rows * args.k
    correct = rng.random((args.rows, args.k)) < 0.25
    total = int(correct.sum()) + 1000  # (the curve stops short of recall 1: the clip is taken)
    q = np.linspace(0, 1, args.smoothness + 1)
    lines = []
    for dtype in (np.float32, np.float64):
        # float32: n consecutive bit patterns from 0x30000000 (positive, finite, no two equal) in random order;
        # float64: e-value-like
        scores = (np.uint32(0x30000000) + rng.permutation(n).astype(np.uint32)).view(np.float32).reshape(args.rows, args.k) if dtype == np.float32 else \
            np.exp(rng.normal(-20, 15, (args.rows, args.k)))
        tie_free = len(np.unique(scores)) == n
        small = scores[:64]
        evaluation.ranked_precision_recall(correct[:64], small, 100, points=10)
        evaluation.score_quantiles(small, q)
        curve_calls, quantile_calls = [], []
        for _ in range(args.reps):
            (recall, precision), seconds = timed(lambda: evaluation.ranked_precision_recall(correct, scores, total, limit=args.limit, points=args.points))
            curve_calls.append({"wall_ms": 1e3 * seconds, **evaluation.last_rank_info()})
            quantiles, seconds = timed(lambda: evaluation.score_quantiles(scores, q, limit=args.limit))
            quantile_calls.append({"wall_ms": 1e3 * seconds, **evaluation.last_rank_info()})
        rec = {"box": socket.gethostname(), "library": _lib.lib().knn_version().decode(), "numpy": np.__version__, "rows": args.rows, "k": args.k,
               "limit": args.limit or args.k, "dtype": np.dtype(dtype).name, "points": args.points, "quantile_points": len(q), "tie_free": bool(tie_free),
               "reps": args.reps, "ranked_precision_recall_wall_ms": spread([c["wall_ms"] for c in curve_calls]),
               "score_quantiles_wall_ms": spread([c["wall_ms"] for c in quantile_calls]),
               "ranked_precision_recall_calls": curve_calls, "score_quantiles_calls": quantile_calls}
        if not args.skip_numpy:
            part, part_correct = scores[:, :args.limit], correct[:, :args.limit]
            (np_recall, np_precision), np_curve_s = timed(lambda: host_curve(part, part_correct, total, np.linspace(0, 1, args.points)))
            np_quantiles, np_quantile_s = timed(lambda: np.quantile(part, q))
            rec.update({"host_curve_s": np_curve_s, "numpy_quantile_s": np_quantile_s,
                        "curve_equal_bits": bool(np.array_equal(recall.view(np.uint64), np_recall.view(np.uint64))
                                                 and np.array_equal(precision.view(np.uint64), np_precision.view(np.uint64))),
                        "quantiles_equal_bits": bool(np.array_equal(quantiles.view(np.uint64), np.asarray(np_quantiles, np.float64).view(np.uint64)))})
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
