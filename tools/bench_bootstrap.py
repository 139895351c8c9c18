"""One evaluation.class_accuracies(bootstrap=True) call on one MI355X at CATH20's size, on synthetic input.

    python tools/bench_bootstrap.py --out profiles/bootstrap_probe.json

The reference's accuracy table bootstraps every method on its own: 500 resamples of the 10 874 evaluable domains, a
Counter and a Python list per resample (cath/cath.py:404-438), for more than 20 methods.  Here: 25 synthetic methods over
10 874 rows in about 2 500 superfamilies of two members at least, the 500 resamples drawn once on the host
(evaluation.bootstrap_samples, numpy's stream: host work, timed separately) and one batched GPU pass for all methods.  One
warm call, then the wall clock around --reps calls of class_accuracies with the resamples handed in: the point
estimates, the uploads, the kernel, the downloads, the sorts.  --reference-seconds takes the figure that
tests/golden/make_bootstrap_golden.py --time printed (the reference's function, one method, on a CPU) and records it and
the ratio beside the measurement.  Prints one JSON line (and writes it to --out).  Nothing is gated on it."""
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
    ap.add_argument("--n", type=int, default=10874)
    ap.add_argument("--families", type=int, default=2500)
    ap.add_argument("--methods", type=int, default=25)
    ap.add_argument("--replicates", type=int, default=500)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--reference-seconds", type=float, default=None, help="make_bootstrap_golden.py --time: one method on a CPU")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    rng = np.random.default_rng(0)
    level0 = np.concatenate([np.arange(args.families).repeat(2), rng.integers(0, args.families, args.n - 2 * args.families)])
    mapping_array = np.stack([rng.permutation(level0), rng.integers(0, 40, args.n)], axis=1)
    methods = {f"method {m}": rng.random(args.n) < p for m, p in enumerate(np.linspace(0.3, 0.9, args.methods))}
    t0 = time.perf_counter()
    sample_ids = evaluation.bootstrap_samples(args.n, args.replicates)
    samples_ms = 1e3 * (time.perf_counter() - t0)
    evaluation.class_accuracies(methods, mapping_array, bootstrap=True, sample_ids=sample_ids)
    ts = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        table = evaluation.class_accuracies(methods, mapping_array, bootstrap=True, sample_ids=sample_ids)
        ts.append(time.perf_counter() - t0)
    # one method's raw replicates against numpy: the probe measures a call that computes the right thing
    name = next(iter(methods))
    boot_raw = np.sort(methods[name][sample_ids].mean(axis=1))
    mean = methods[name].mean()
    same = table[name][3] == max(mean - boot_raw[int(args.replicates * 0.025)], boot_raw[int(args.replicates * 0.975)] - mean)
    rec = {"box": socket.gethostname(), "library": _lib.lib().knn_version().decode(), "n": args.n, "families": args.families,
           "methods": args.methods, "replicates": args.replicates, "reps": args.reps, "median_ms": 1e3 * float(np.median(ts)),
           "min_ms": 1e3 * min(ts), "max_ms": 1e3 * max(ts), "bootstrap_samples_ms": samples_ms,
           "raw_stderr_equals_numpy": bool(same), "best": list(table)[0], "best_row": [float(v) for v in table[list(table)[0]]]}
    if args.reference_seconds is not None:
        rec["reference_seconds_one_method_cpu"] = args.reference_seconds
        rec["reference_seconds_all_methods_cpu_scaled"] = args.reference_seconds * args.methods
        rec["ratio_scaled_reference_over_median"] = args.reference_seconds * args.methods / float(np.median(ts))
    line = json.dumps(rec)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
