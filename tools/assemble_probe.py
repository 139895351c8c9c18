"""knn_eval_assemble on one MI355X against a straightforward host loop of the same contract, on synthetic input.

    python tools/assemble_probe.py --groups 4000 --out profiles/assemble_probe.json

No slice dataset ships with the project: --groups query proteins of 1..40 slices each (uniform), k = 100 hits per slice,
the database is the same slices (a self-search), hits are uniform over the database slices and scores are Gaussian, in
no order.  Per (depth, k_out), after one warm-up call:
  device    wall clock around the C call, host buffers in and out (median, min, max of --reps calls): uploads, the
            kernel, downloads
  host      the per-protein loop the call replaces, with numpy doing the sort: concatenate the protein's rows, stable
            argsort of the negated scores, cut at depth, walk with a set of picked proteins (--host-reps calls)
and whether the two agree in every output.  Nothing is gated on the ratio."""
import argparse
import json
import os
import socket
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from knn_for_homology_amd import _lib  # noqa: E402

FMAX = np.finfo(np.float32).max


def stats(ts):
    ts = sorted(ts)
    return {"median_ms": 1e3 * float(np.median(ts)), "min_ms": 1e3 * ts[0], "max_ms": 1e3 * ts[-1], "reps": len(ts)}


def host_loop(hits, scores, offsets, row_group, depth, k_out):
    k = hits.shape[1]
    ng = len(offsets) - 1
    nb = len(row_group)
    groups = np.full((ng, k_out), -1, np.int64)
    out_scores = np.full((ng, k_out), -FMAX, np.float32)
    qrow = np.full((ng, k_out), -1, np.int64)
    hit_out = np.full((ng, k_out), -1, np.int64)
    for g in range(ng):
        lo, hi = offsets[g], offsets[g + 1]
        h = hits[lo:hi].reshape(-1)
        s = scores[lo:hi].reshape(-1)
        picked = set()
        for p in np.argsort(-s, kind="stable")[:depth].tolist():
            hit = h[p]
            if hit < 0 or hit >= nb:
                continue
            grp = row_group[hit]
            if grp in picked:
                continue
            at = len(picked)
            if at == k_out:
                break
            picked.add(grp)
            groups[g, at], out_scores[g, at], qrow[g, at], hit_out[g, at] = grp, s[p], lo + p // k, hit
    return groups, out_scores, qrow, hit_out


def device_call(L, hits, scores, offsets, row_group, depth, k_out):
    ng = len(offsets) - 1
    out = (np.empty((ng, k_out), np.int64), np.empty((ng, k_out), np.float32), np.empty((ng, k_out), np.int64),
           np.empty((ng, k_out), np.int64))
    _lib.check(L.knn_eval_assemble(hits.ctypes.data, scores.ctypes.data, hits.shape[0], hits.shape[1], offsets.ctypes.data, ng,
                                   row_group.ctypes.data, len(row_group), None, depth, k_out, 0, out[0].ctypes.data, out[1].ctypes.data,
                                   out[2].ctypes.data, out[3].ctypes.data))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", type=int, default=4000)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--max-slices", type=int, default=40)
    ap.add_argument("--shapes", type=int, nargs="+", default=[100, 100, 1000, 1000, 2048, 100],
                    help="pairs of depth and k_out")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--host-reps", type=int, default=2)
    ap.add_argument("--out", default="profiles/assemble_probe.json")
    args = ap.parse_args()
    L = _lib.lib()
    rng = np.random.default_rng(0)
    sizes = rng.integers(1, args.max_slices + 1, args.groups)
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    ns = int(offsets[-1])
    row_group = np.repeat(np.arange(args.groups, dtype=np.int32), sizes)
    hits = rng.integers(0, ns, (ns, args.k)).astype(np.int64)
    scores = rng.standard_normal((ns, args.k)).astype(np.float32)
    doc = {"box": socket.gethostname(), "library": L.knn_version().decode(), "groups": args.groups, "slices": ns, "k": args.k,
           "input_bytes": int(hits.nbytes + scores.nbytes), "results": []}
    for depth, k_out in zip(args.shapes[0::2], args.shapes[1::2]):
        device_call(L, hits, scores, offsets, row_group, depth, k_out)
        ts = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            got = device_call(L, hits, scores, offsets, row_group, depth, k_out)
            ts.append(time.perf_counter() - t0)
        hs = []
        for _ in range(args.host_reps):
            t0 = time.perf_counter()
            want = host_loop(hits, scores, offsets, row_group, depth, k_out)
            hs.append(time.perf_counter() - t0)
        same = all(np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a, b.view(np.uint32) if b.dtype == np.float32 else b)
                   for a, b in zip(got, want))
        rec = {"depth": depth, "k_out": k_out, "device": stats(ts), "host": stats(hs), "same_outputs": bool(same)}
        rec["host_over_device"] = rec["host"]["median_ms"] / rec["device"]["median_ms"]
        doc["results"].append(rec)
        print(json.dumps(rec), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
