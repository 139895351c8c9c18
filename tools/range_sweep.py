#!/usr/bin/env python3
"""One-GPU measurement of IndexFlat.range_search against search(k) on the same resident index and the same host queries:
a 10 M x 1024 fp32 normalised index (built as bench.py builds it: torch.randn on the device, normalised there), IP with
nq in {1, 32, 128, 1024} and squared L2 with nq = 19 (the difference build).  The radius of a cell is the median over
its queries of the k-th score `search` returns (k = 10, 1000): about k hits per query.  Every time is the best of three
repetitions of wall-clock calls (results downloaded), with the floor max(HBM time, MFMA time) of one pass over the rows
in the style of tools/nq_sweep.py.  Prints JSON.
usage: range_sweep.py [rows=N]"""
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from knn_for_homology_amd import faiss, _lib  # noqa: E402

L = _lib.lib()
dev = torch.device("cuda:0")
torch.cuda.set_device(0)
opts = dict(a.split("=") for a in sys.argv[1:] if "=" in a)
nb = int(opts.get("rows", 10_000_000))
d = 1024
HBM, MFMA = 8e12, 157.3e12
CELLS = [(faiss.METRIC_INNER_PRODUCT, nq, k) for nq in (1, 32, 128, 1024) for k in (10, 1000)] + \
        [(faiss.METRIC_L2, 19, k) for k in (10, 1000)]


def build(metric):
    g = torch.Generator(device=dev)
    g.manual_seed(23)
    index = faiss.IndexFlat(d, metric)
    _lib.check(L.knn_flat_reserve(index._h, nb))
    for i0 in range(0, nb, 500_000):
        m = min(500_000, nb - i0)
        x = torch.randn((m, d), generator=g, device=dev)
        _lib.check(L.knn_normalize_l2_dev(x.data_ptr(), m, d, None))
        torch.cuda.synchronize()
        _lib.check(L.knn_flat_add_dev(index._h, x.data_ptr(), m, None))
        del x
    torch.cuda.synchronize()
    return index


def best_of(fn, reps=3):
    fn()
    best = None
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        t = time.perf_counter() - t0
        best = t if best is None else min(best, t)
    return best, out


out = {"workload": f"{nb}x{d} normalised rows, host queries, wall clock per call (results on the host)", "cells": []}
rng = np.random.default_rng(7)
for metric in (faiss.METRIC_INNER_PRODUCT, faiss.METRIC_L2):
    cells = [c for c in CELLS if c[0] == metric]
    index = build(metric)
    for _, nq, k in cells:
        xq = rng.standard_normal((nq, d)).astype(np.float32)
        faiss.normalize_L2(xq)
        t_search, (D, _) = best_of(lambda: index.search(xq, k))
        search_info = index.last_scan()
        r = np.float32(np.median(D[:, k - 1]))
        t_range, (lims, _, _) = best_of(lambda: index.range_search(xq, r))
        info = index.last_scan()
        t_hbm = nb * d * 4 / HBM
        t_mfma = 2.0 * nq * nb * d / MFMA
        floor = max(t_hbm, t_mfma)
        rec = {"metric": "ip" if metric == faiss.METRIC_INNER_PRODUCT else "l2", "nq": nq, "k": k, "radius": float(r),
               "hits_per_query": float(lims[-1]) / nq, "range_ms": 1e3 * t_range, "search_ms": 1e3 * t_search,
               "range_over_search": t_range / t_search, "range_kernel": info["kernel"], "range_grid": info["grid"],
               "range_scan_ms": info["ms"], "range": index.last_range(), "search_kernel": search_info["kernel"],
               "floor_ms": 1e3 * floor, "bound": "hbm" if t_hbm >= t_mfma else "mfma",
               "range_frac_of_floor": floor / t_range, "search_frac_of_floor": floor / t_search}
        out["cells"].append(rec)
        print(json.dumps(rec), file=sys.stderr, flush=True)
    del index
print(json.dumps(out))
