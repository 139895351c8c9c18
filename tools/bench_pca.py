"""One decomposition.PCA(2).fit_transform on one MI355X at the reference's sizes, on synthetic input.

    python tools/bench_pca.py --out profiles/pca_probe.json

pfam/reverse_evaluate.py:34-44 runs sklearn's PCA(n_components=2).fit_transform over the forward and the scrambled
embeddings together: [28 866, 1024] for the CATH file doubled, and [200 000, 1024] as the larger size.  Per size: one warm
call, then --reps timed ones; of the last call the split into the upload of the rows, the column sums and the mean, the
covariance kernel, the reduce over the row groups (HIP events inside knn_pca_moments), the host eigh (wall clock around
the same call decomposition.PCA.fit makes), and the projection kernel (HIP events inside knn_pca_project; its slab copies
are in the wall clock only).  --reference-seconds takes the figure tests/golden/make_pca_golden.py --time printed (the
reference's statement at [200 000, 1024] on a CPU) and records it beside the measurement.  Prints one JSON line per size
(and writes them to --out).  Nothing is gated on it."""
import argparse
import json
import os
import socket
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from knn_for_homology_amd import _lib, decomposition  # noqa: E402


def synthetic(n, d, seed):
    """two strong directions over unit noise and a column mean, float32"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, d), dtype=np.float32)
    u = rng.standard_normal((2, d), dtype=np.float32) / np.float32(np.sqrt(d))
    x += rng.standard_normal((n, 1), dtype=np.float32) * (np.float32(20) * u[0]) + rng.standard_normal((n, 1), dtype=np.float32) * (np.float32(10) * u[1])
    x += rng.standard_normal(d, dtype=np.float32)
    return x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="28866,200000", help="row counts, comma separated")
    ap.add_argument("--d", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--reference-seconds", type=float, default=None, help="make_pca_golden.py --time: the statement at [200 000, 1024] on a CPU")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []
    for n in (int(v) for v in args.sizes.split(",")):
        x = synthetic(n, args.d, n)
        decomposition.PCA(2).fit_transform(x)
        ts = []
        for _ in range(args.reps):
            pca = decomposition.PCA(2)
            t0 = time.perf_counter()
            y = pca.fit_transform(x)
            ts.append(time.perf_counter() - t0)
        moments_ms, project_ms = decomposition.last_ms()
        t0 = time.perf_counter()
        decomposition.components_from_covariance(pca.covariance_, n, 2)
        eigh_ms = 1e3 * (time.perf_counter() - t0)
        rec = {"box": socket.gethostname(), "library": _lib.lib().knn_version().decode(), "n": n, "d": args.d, "n_components": 2,
               "reps": args.reps, "fit_transform_median_ms": 1e3 * float(np.median(ts)), "fit_transform_min_ms": 1e3 * min(ts),
               "upload_ms": moments_ms["upload"], "column_sums_ms": moments_ms["colsum"], "covariance_kernel_ms": moments_ms["cov"],
               "reduce_ms": moments_ms["reduce"], "host_eigh_ms": eigh_ms, "projection_kernel_ms": project_ms,
               "covariance_kernel_tflops": 2.0 * n * args.d * (args.d + 128) / 2 / (moments_ms["cov"] * 1e-3) / 1e12 if moments_ms["cov"] > 0 else None,
               "explained_variance": [float(v) for v in pca.explained_variance_], "finite": bool(np.isfinite(y).all())}
        if args.reference_seconds is not None and n == 200000 and args.d == 1024:
            rec["reference_seconds_cpu"] = args.reference_seconds
            rec["ratio_reference_over_median"] = args.reference_seconds / float(np.median(ts))
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
