"""One evaluate_slices call on one MI355X: 20 000 annotated rows x 100 hits over 200 000 slices, synthetic input.

    python tools/bench_slices_eval.py

The shape is that of tests/golden/make_slices_eval_golden.py --time, which runs the reference's own statements
(pfam/slices/slices.py:49-80 and evaluate) where the reference is at hand: proteins of 1 .. 8 overlapping windows of 128
residues, 0 .. 4 domains each out of 3000 families, every fifth protein with one family twice.  Each row starts with a
run of 0 .. 30 hits of the query's family and goes on with random slices.  Prints one JSON line: the median seconds of
--reps calls after --warmup calls (wall clock around evaluate_slices with ignore_unannotated and the column counts:
host buffers in and out, uploads, the kernel, downloads), and the seconds of the one slice_tables call in front of them.
Nothing is gated on the numbers."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from knn_for_homology_amd import _lib  # noqa: E402
from knn_for_homology_amd.evaluation import evaluate_slices, slice_tables  # noqa: E402

SLICE_LEN, STEP = 128, 64


def synthetic(rng, n_slices, n_families):
    slices, protein_to_domain = [], {}
    p = 0
    while len(slices) < n_slices:
        name = f"P{p:06d}"
        n = int(rng.integers(1, 9))
        slices.extend((name, (i * STEP, i * STEP + SLICE_LEN)) for i in range(n))
        span = (n - 1) * STEP + SLICE_LEN
        domains = []
        for _ in range(int(rng.integers(0, 5))):
            start = 32 * int(rng.integers(0, span // 32)) if rng.random() < 0.6 else int(rng.integers(0, span))
            domains.append((f"PF{int(rng.integers(n_families)):05d}", (start, start + int(rng.integers(10, 150)))))
        if p % 5 == 0:
            family = f"PF{int(rng.integers(n_families)):05d}"
            domains += [(family, (16, 80)), (family, (SLICE_LEN - 24, SLICE_LEN + 40))]
        protein_to_domain[name] = domains
        p += 1
    return slices[:n_slices], protein_to_domain


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slices", type=int, default=200000)
    ap.add_argument("--rows", type=int, default=20000)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--families", type=int, default=3000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    args = ap.parse_args()
    L = _lib.lib()
    rng = np.random.default_rng(1)
    slices, protein_to_domain = synthetic(rng, args.slices, args.families)
    t0 = time.perf_counter()
    tables = slice_tables(slices, protein_to_domain)
    tables_s = time.perf_counter() - t0
    rows = np.flatnonzero(tables.has_annotation)[:args.rows]
    if len(rows) < args.rows:
        raise SystemExit(f"only {len(rows)} annotated slices")
    order = np.argsort(tables.annotation[tables.has_annotation], kind="stable")
    annotated = np.flatnonzero(tables.has_annotation)[order]  # the annotated slices, by family: each family's pool of hits
    first = np.searchsorted(tables.annotation[annotated], np.arange(len(tables.families) + 1))
    hits = rng.integers(0, args.slices, (args.rows, args.k)).astype(np.int64)
    for r, a in enumerate(tables.annotation[rows]):
        run = int(rng.integers(0, min(31, args.k + 1)))
        hits[r, :run] = annotated[rng.integers(first[a], first[a + 1], run)]
    for _ in range(args.warmup):
        evaluate_slices(hits, tables, query_rows=rows, ignore_unannotated=True, want_column_counts=True)
    ts = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        is_correct, is_ignore, auc1s, columns = evaluate_slices(hits, tables, query_rows=rows, ignore_unannotated=True, want_column_counts=True)
        ts.append(time.perf_counter() - t0)
    print(json.dumps({"evaluate_slices_median_seconds": float(np.median(ts)), "min_seconds": min(ts), "max_seconds": max(ts), "reps": args.reps,
                      "warmup": args.warmup, "slice_tables_seconds": tables_s, "slices": args.slices, "rows": args.rows, "k": args.k,
                      "domains": int(tables.domain_family.size), "families": len(tables.families), "correct_hits": int(is_correct.sum()),
                      "ignored_hits": int(is_ignore.sum()), "mean_auc1": float(auc1s.mean()), "library": L.knn_version().decode()}))


if __name__ == "__main__":
    main()
