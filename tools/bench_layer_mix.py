"""LayerMix.sweep on one MI355X at CATH size: 14 433 rows, d = 1024, three layers, the simplex grids of granularity 5 and 11
(15 and 66 mixes).

    python tools/bench_layer_mix.py --out profiles/layer_mix_probe.json

Beside it, on the same machine and in the same process, the way without LayerMix: per ratio the numpy mix on the host,
cath.search.search of it (upload, normalise, self-search, download) and compute_is_correct of the hits.  Per configuration
--reps calls of each (three by default); of a sweep the wall clock and what knn_mix_last_ms gives by HIP events, summed over
the mixes and divided by their number; the one-off upload of the layers (the LayerMix constructor) is timed on its own.
The counts of both ways are compared.  One process, which opens the device once; no time limit of its own: the caller sets
it.  Nothing is gated on a speed.  Prints one JSON line (and writes it to --out)."""
import argparse
import ctypes
import json
import os
import socket
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def inputs(rng, rows, d, classes):
    """three layers around class centres and four label levels: accuracy differs from mix to mix"""
    fine = rng.integers(0, classes, rows)
    mapping = np.stack([fine, fine // 3, fine // 12, fine // 60], axis=1).astype(np.int32)
    layers = []
    for noise in (2.0, 3.0, 5.0):
        centres = rng.standard_normal((classes, d)).astype(np.float32)
        layers.append(centres[fine] + np.float32(noise) * rng.standard_normal((rows, d), dtype=np.float32))
    return layers, mapping


def host_way(layers, ratios, mapping, level):
    """the reference's statements, once per ratio: (counts [G], seconds spent mixing, searching, scoring)"""
    from knn_for_homology_amd.cath.search import search
    from knn_for_homology_amd.evaluation import compute_is_correct
    counts, t_mix, t_search, t_score = [], 0.0, 0.0, 0.0
    for ratio in ratios:
        w = [np.float32(v) for v in ratio]
        t0 = time.perf_counter()
        mixed = w[0] * layers[0] + w[1] * layers[1] + w[2] * layers[2]
        t1 = time.perf_counter()
        hits, _ = search(mixed, hits=1)
        t2 = time.perf_counter()
        counts.append(int(compute_is_correct(hits, mapping)[:, level, 0].sum()))
        t3 = time.perf_counter()
        t_mix, t_search, t_score = t_mix + t1 - t0, t_search + t2 - t1, t_score + t3 - t2
    return np.asarray(counts, np.int64), t_mix, t_search, t_score


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=14433)
    ap.add_argument("--d", type=int, default=1024)
    ap.add_argument("--classes", type=int, default=1500)
    ap.add_argument("--granularities", type=int, nargs="+", default=[5, 11])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from knn_for_homology_amd import _lib
    from knn_for_homology_amd.layers import LayerMix, simplex_ratios
    layers, mapping = inputs(np.random.default_rng(56), args.rows, args.d, args.classes)
    level = 0
    # the first calls of a process load the code objects: a small sweep and a small search, not timed
    small = [x[:512] for x in layers]
    LayerMix(small).sweep(simplex_ratios(3), mapping[:512])
    host_way(small, simplex_ratios(3), mapping[:512], level)
    uploads = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        lm = LayerMix(layers)
        uploads.append(1e3 * (time.perf_counter() - t0))
    # what a plain read of the mixed rows costs on this box, for the mix kernel's three reads and one write
    best_ms, nbytes = ctypes.c_float(), ctypes.c_int64()
    _lib.check(_lib.lib().knn_flat_read_rate(lm.index((1.0, 0.0, 0.0))._h, 5, ctypes.byref(best_ms), ctypes.byref(nbytes)))
    rec = {"box": socket.gethostname(), "library": _lib.lib().knn_version().decode(), "numpy": np.__version__, "rows": args.rows, "d": args.d,
           "reps": args.reps, "layer_upload_ms": uploads, "read_rate": {"ms": best_ms.value, "bytes": nbytes.value}, "configs": []}
    for g in args.granularities:
        ratios = simplex_ratios(g)
        sweeps, hosts, equal = [], [], True
        for _ in range(args.reps):
            t0 = time.perf_counter()
            got = lm.sweep(ratios, mapping, level=level)
            wall = 1e3 * (time.perf_counter() - t0)
            ms = lm.last_ms()
            sweeps.append({"wall_ms": wall, "per_mix_ms": {k: v / len(ratios) for k, v in ms.items()}})
        for _ in range(args.reps):
            t0 = time.perf_counter()
            counts, t_mix, t_search, t_score = host_way(layers, ratios, mapping, level)
            hosts.append({"wall_ms": 1e3 * (time.perf_counter() - t0),
                          "per_mix_ms": {"mix": 1e3 * t_mix / len(ratios), "search": 1e3 * t_search / len(ratios), "score": 1e3 * t_score / len(ratios)}})
            equal = equal and bool(np.array_equal(counts, got.counts))
        rec["configs"].append({"granularity": g, "mixes": len(ratios), "sweep": sweeps, "host_way": hosts, "counts_equal": equal,
                               "count_min": int(got.counts.min()), "count_max": int(got.counts.max()),
                               "best_ratio": min(h["wall_ms"] for h in hosts) / min(s["wall_ms"] for s in sweeps)})
    line = json.dumps(rec)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0 if all(c["counts_equal"] for c in rec["configs"]) else 1


if __name__ == "__main__":
    sys.exit(main())
