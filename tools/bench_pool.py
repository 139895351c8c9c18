"""pooling.pool_ranges on one MI355X at the reference's sizes, on synthetic input.

    python tools/bench_pool.py --out profiles/pool_probe.json

Per-protein case: --proteins proteins (20 000), lengths drawn uniformly from [mean / 2, 3 mean / 2] around --mean-length
(350), d = 1024, float32 and float16 residues, plain and normalizing: the device entry on a matrix made on the device
(kernel time from knn_pool_last_ms, --reps calls after a warm one: median, min, max), and its achieved bytes per second
-- every residue byte counted ONCE, plus the output -- as a fraction of what this box's HBM gives a plain read kernel
(knn_flat_read_rate, same process).  The normalizing build reads the rows twice: its fraction shows what the second
read and the one-lane-per-row norms cost.
Pfam-domain case: --domain-sequences sequences at d = 3072, float32, three overlapping ranges per sequence.
Host entry: --host-proteins proteins (a subset: the host matrix is made by numpy) through knn_pool_ranges, wall clock
and the upload / kernel / download split, next to the reference's loop on the same rows (numpy's mean(axis=0) per
protein, on this machine's CPU) -- both on the subset, neither scaled.  Prints one JSON line per measurement (and writes
them to --out).  Nothing is gated on it."""
import argparse
import ctypes
import json
import os
import socket
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from knn_for_homology_amd import _lib, faiss, pooling  # noqa: E402


def lengths_of(n, mean, seed):
    return np.random.default_rng(seed).integers(mean // 2, mean + mean // 2 + 1, n).astype(np.int64)


def read_rate_gbs(d):
    """this box's plain read rate over 4 GiB of index rows"""
    n = (4 << 30) // (d * 4)
    x = torch.randn((n, d), device="cuda", dtype=torch.float32)
    index = faiss.IndexFlat(d, faiss.METRIC_INNER_PRODUCT)
    _lib.check(_lib.lib().knn_flat_add_dev(index._h, x.data_ptr(), n, None))
    del x
    ms, nbytes = ctypes.c_float(), ctypes.c_int64()
    _lib.check(_lib.lib().knn_flat_read_rate(index._h, 5, ctypes.byref(ms), ctypes.byref(nbytes)))
    return nbytes.value / (ms.value * 1e-3) / 1e9


def device_case(name, x, starts, stops, normalize, reps, stream_gbs):
    pooling.pool_ranges(x, starts, stops, normalize=normalize)
    ms = []
    for _ in range(reps):
        pooling.pool_ranges(x, starts, stops, normalize=normalize)
        ms.append(pooling.last_ms()["kernel"])
    d = x.shape[1]
    nbytes = int((stops - starts).sum().item()) * d * x.element_size() + len(starts) * d * 4
    gbs = nbytes / (float(np.median(ms)) * 1e-3) / 1e9
    return {"case": name, "entry": "device", "dtype": str(x.dtype).split(".")[-1], "normalize": bool(normalize), "ranges": len(starts), "rows": x.shape[0], "d": d,
            "reps": reps, "kernel_median_ms": float(np.median(ms)), "kernel_min_ms": min(ms), "kernel_max_ms": max(ms), "bytes_counted_once": nbytes,
            "achieved_gbs": gbs, "read_rate_gbs": stream_gbs, "fraction_of_read_rate": gbs / stream_gbs}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--proteins", type=int, default=20000)
    ap.add_argument("--host-proteins", type=int, default=2000)
    ap.add_argument("--domain-sequences", type=int, default=3000)
    ap.add_argument("--mean-length", type=int, default=350)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    box = {"box": socket.gethostname(), "library": _lib.lib().knn_version().decode()}
    lines = []

    def emit(rec):
        lines.append(json.dumps({**box, **rec}))
        print(lines[-1], flush=True)

    stream_gbs = read_rate_gbs(1024)
    lengths = lengths_of(args.proteins, args.mean_length, 1)
    stops = torch.from_numpy(np.cumsum(lengths)).cuda()
    starts = stops - torch.from_numpy(lengths).cuda()
    for dtype in (torch.float32, torch.float16):
        x = torch.randn((int(lengths.sum()), 1024), device="cuda", dtype=dtype)
        for normalize in (False, True):
            emit(device_case("per-protein", x, starts, stops, normalize, args.reps, stream_gbs))
        del x
    # Pfam domains: three ranges per sequence, each a random stretch of it, so they overlap
    lengths = lengths_of(args.domain_sequences, args.mean_length, 2)
    first = np.cumsum(lengths) - lengths
    rng = np.random.default_rng(3)
    a = rng.integers(0, lengths[:, None], (len(lengths), 3))
    b = rng.integers(a + 1, lengths[:, None] + 1)
    dom_starts, dom_stops = (first[:, None] + a).ravel(), (first[:, None] + b).ravel()
    x = torch.randn((int(lengths.sum()), 3072), device="cuda", dtype=torch.float32)
    emit(device_case("pfam-domains", x, torch.from_numpy(dom_starts).cuda(), torch.from_numpy(dom_stops).cuda(), False, args.reps, stream_gbs))
    del x
    torch.cuda.empty_cache()
    # the host entry and the reference's loop, on the same subset
    lengths = lengths_of(args.host_proteins, args.mean_length, 4)
    stops_h = np.cumsum(lengths)
    starts_h = stops_h - lengths
    xh = np.random.default_rng(5).standard_normal((int(lengths.sum()), 1024), dtype=np.float32)
    for dtype in (np.float32, np.float16):
        xd = xh.astype(dtype)
        for normalize in (False, True):
            pooling.pool_ranges(xd, starts_h, stops_h, normalize=normalize)
            ts, split = [], None
            for _ in range(args.reps):
                t0 = time.perf_counter()
                out = pooling.pool_ranges(xd, starts_h, stops_h, normalize=normalize)
                ts.append(time.perf_counter() - t0)
                split = pooling.last_ms()
            emit({"case": "per-protein", "entry": "host", "dtype": np.dtype(dtype).name, "normalize": normalize, "ranges": len(lengths), "rows": xd.shape[0],
                  "d": 1024, "reps": args.reps, "wall_median_s": float(np.median(ts)), "wall_min_s": min(ts), "wall_max_s": max(ts),
                  "upload_ms": split["upload"], "kernel_ms": split["kernel"], "download_ms": split["download"], "finite": bool(np.isfinite(out).all())})
    ts = []
    for _ in range(3):
        t0 = time.perf_counter()
        loop = np.stack([xh[a:b].mean(axis=0) for a, b in zip(starts_h, stops_h)])
        ts.append(time.perf_counter() - t0)
    same = bool(np.array_equal(loop.view(np.uint32), pooling.pool_ranges(xh, starts_h, stops_h).view(np.uint32)))
    emit({"case": "per-protein", "entry": "numpy loop (the reference's reduce_per_protein, this machine's CPU)", "dtype": "float32", "ranges": len(lengths),
          "rows": xh.shape[0], "d": 1024, "reps": 3, "wall_median_s": float(np.median(ts)), "wall_min_s": min(ts), "wall_max_s": max(ts), "same_bits_as_the_gpu": same})
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
