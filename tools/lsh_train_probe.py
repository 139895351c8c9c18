#!/usr/bin/env python3
"""IndexLSH train_thresholds timing: train(x) against add(x) of the same rows (same upload, same projection work), with
the training's upload / projection / selection split (HIP events, knn_lsh_last_train_ms), and one pfam/search.py-shaped
search (k = 1000 over every row) with and without thresholds.
usage: lsh_train_probe.py [out.json] [--search]   (default: profiles/lsh_thresholds.json)
       lsh_train_probe.py out.json --encode     (add(x) alone, repeated: the encoder's time, for comparing two builds)"""
import ctypes
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from knn_for_homology_amd import _lib, faiss  # noqa: E402


def rows(n, seed=21):
    rng = np.random.default_rng(seed)
    cent = rng.standard_normal((2000, 1024), dtype=np.float32)
    x = cent[rng.integers(0, 2000, n)] + 0.35 * rng.standard_normal((n, 1024), dtype=np.float32)
    faiss.normalize_L2(x)
    return x


def train_ms(idx):
    v = [ctypes.c_float() for _ in range(3)]
    _lib.check(_lib.lib().knn_lsh_last_train_ms(idx._h, *[ctypes.byref(c) for c in v]))
    return [round(c.value, 3) for c in v]


def leg(x, nbits, runs=3):
    out = {"rows": int(x.shape[0]), "d": int(x.shape[1]), "nbits": nbits, "train_wall_ms": [], "train_upload_ms": [],
           "train_project_ms": [], "train_select_ms": [], "add_wall_ms": []}
    for _ in range(runs + 1):  # (the first round warms the workspaces up and is dropped)
        idx = faiss.IndexLSH(x.shape[1], nbits, True, True)
        t0 = time.perf_counter(); idx.train(x); tw = (time.perf_counter() - t0) * 1e3
        up, pr, se = train_ms(idx)
        t0 = time.perf_counter(); idx.add(x); ta = (time.perf_counter() - t0) * 1e3
        for key, v in (("train_wall_ms", tw), ("train_upload_ms", up), ("train_project_ms", pr), ("train_select_ms", se), ("add_wall_ms", ta)):
            out[key].append(round(v, 3))
        ones = np.unpackbits(idx.codes(), axis=1, bitorder="little")[:, :nbits].mean(0)
        out["mean_abs_ones_minus_half"] = round(float(np.abs(ones - 0.5).mean()), 6)
        del idx
    for key in ("train_wall_ms", "train_upload_ms", "train_project_ms", "train_select_ms", "add_wall_ms"):
        out[key] = out[key][1:]
    print(json.dumps(out), flush=True)
    return out


def search_leg(x, nbits, thresholds, runs=5, k=1000):
    idx = faiss.IndexLSH(x.shape[1], nbits, True, thresholds)
    idx.train(x)
    idx.add(x)
    idx.search(x[:4096], k)
    times = []
    for _ in range(runs + 1):
        t0 = time.perf_counter(); idx.search(x, k); times.append(round(time.perf_counter() - t0, 4))
    out = {"rows": int(x.shape[0]), "nbits": nbits, "k": k, "train_thresholds": thresholds, "search_all_rows_s": times[1:]}
    print(json.dumps(out), flush=True)
    return out


def encode_leg(x, nbits, thresholds, runs=12):
    """add(x) of the same rows over and over on one handle (reset() keeps the allocation): upload + lsh_encode_kernel, host
    wall clock; the first round warms the workspaces up and is dropped"""
    idx = faiss.IndexLSH(x.shape[1], nbits, True, thresholds)
    idx.train(x)
    times = []
    for _ in range(runs + 1):
        idx.reset()
        t0 = time.perf_counter(); idx.add(x); times.append(round((time.perf_counter() - t0) * 1e3, 3))
    out = {"rows": int(x.shape[0]), "d": int(x.shape[1]), "nbits": nbits, "train_thresholds": thresholds, "library": Path(_lib.LIB_PATH).name,
           "add_wall_ms": times[1:]}
    print(json.dumps(out), flush=True)
    return out


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    dest = Path(args[0]) if args else ROOT / "profiles" / "lsh_thresholds.json"
    if "--encode" in sys.argv:  # the encoder alone: one series per (thresholds, code width), for comparing two builds (KNN355_LIB)
        x = rows(200_000)
        res = {"what": "IndexLSH add(x) of 200 000 x 1024 rows: upload + lsh_encode_kernel, host wall clock in ms",
               "legs": [encode_leg(x, nbits, thr) for nbits in (1024, 2048) for thr in (False, True)]}
        dest.parent.mkdir(parents=True, exist_ok=True)
        dest.write_text(json.dumps(res, indent=1) + "\n")
        return
    res = {"what": "IndexLSH train_thresholds: train(x) vs add(x) of the same rows; times in ms (HIP events for the split, host wall clock otherwise)",
           "legs": [], "search": []}
    x = rows(200_000)
    res["legs"].append(leg(x, 1024))
    res["legs"].append(leg(x, 2048))
    res["legs"].append(leg(np.ascontiguousarray(x[:14_433]), 1024))
    if "--search" in sys.argv:
        for thresholds in (False, True, False, True):
            res["search"].append(search_leg(x, 1024, thresholds, runs=3))
    dest.parent.mkdir(parents=True, exist_ok=True)
    dest.write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
