"""knn_eval_fuse on one MI355X against a straightforward host loop of the same contract, on synthetic input.

    python tools/fuse_probe.py --rows 200000 --out profiles/fuse_probe.json

No Pfam result arrays ship with the project: --rows queries, two lists of --ka and --kb hits each, ids uniform over
200 000 database rows (so the lists share few ids), e-values 10^u with u uniform in [-300, 3], ascending within a list as
a search returns them.  Per mode, after one warm-up call:
  device     wall clock around the C call, host buffers in and out (median, min, max of --reps calls): uploads, the
             kernel, downloads, slab by slab
  host       the per-row loop the call replaces with numpy doing the sort (stable argsort of the concatenated scores, a
             walk with a set of seen ids; or the kept prefix, a set, and a walk over B), on the first --host-rows rows,
             scaled up to --rows
  reference  the reference's own loop nodes as tests/golden/make_fuse_golden.py --time ran them (seconds for 2000 rows of
             300 + 300, given with --reference-combined / --reference-both where that script was run; scaled up to --rows)
and whether device and host agree in every output on those rows.  Nothing is gated on the ratios."""
import argparse
import json
import os
import socket
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from knn_for_homology_amd import _lib  # noqa: E402

DBL_MAX = np.finfo(np.float64).max
PREFIX_FILL, SORTED_UNION = 0, 1


def stats(ts):
    ts = sorted(ts)
    return {"median_ms": 1e3 * float(np.median(ts)), "min_ms": 1e3 * ts[0], "max_ms": 1e3 * ts[-1], "reps": len(ts)}


def host_union(hits_a, scores_a, hits_b, scores_b, k_out):
    nq = hits_a.shape[0]
    hits = np.full((nq, k_out), -1, np.int64)
    scores = np.full((nq, k_out), DBL_MAX, np.float64)
    source = np.full((nq, k_out), -1, np.int32)
    filled = np.zeros(nq, np.int32)
    for q in range(nq):
        h = np.concatenate([hits_a[q], hits_b[q]])
        s = np.concatenate([scores_a[q], scores_b[q]])
        seen = set()
        at = 0
        for p in np.argsort(s, kind="stable").tolist():  # (no NaN and no negative id in the probe's input)
            hit = h[p]
            if hit in seen:
                continue
            if at == k_out:
                break
            seen.add(hit)
            hits[q, at], scores[q, at], source[q, at] = hit, s[p], p
            at += 1
        filled[q] = at
    return hits, scores, source, filled


def host_prefix(hits_a, scores_a, keep_a, hits_b, scores_b, k_out):
    nq, ka = hits_a.shape
    hits = np.full((nq, k_out), -1, np.int64)
    scores = np.full((nq, k_out), -DBL_MAX, np.float64)
    source = np.full((nq, k_out), -1, np.int32)
    filled = np.zeros(nq, np.int32)
    for q in range(nq):
        cols = np.nonzero(keep_a[q])[0][:k_out]
        at = len(cols)
        hits[q, :at], scores[q, :at], source[q, :at] = hits_a[q, cols], scores_a[q, cols], cols
        members = set(hits_a[q][keep_a[q] != 0].tolist())
        for j, hit in enumerate(hits_b[q].tolist()):
            if at == k_out:
                break
            if hit not in members:
                hits[q, at], scores[q, at], source[q, at] = hit, scores_b[q, j], ka + j
                at += 1
        filled[q] = at
    return hits, scores, source, filled


def device_call(L, hits_a, scores_a, keep_a, hits_b, scores_b, mode, ascending, k_out):
    nq = hits_a.shape[0]
    out = (np.empty((nq, k_out), np.int64), np.empty((nq, k_out), np.float64), np.empty((nq, k_out), np.int32), np.empty(nq, np.int32))
    _lib.check(L.knn_eval_fuse(hits_a.ctypes.data, scores_a.ctypes.data, None if keep_a is None else keep_a.ctypes.data, hits_a.shape[1],
                               hits_b.ctypes.data, scores_b.ctypes.data, hits_b.shape[1], nq, mode, ascending, k_out,
                               out[0].ctypes.data, out[1].ctypes.data, out[2].ctypes.data, out[3].ctypes.data))
    return out


def e_value_lists(rng, nq, k, nb):
    hits = rng.integers(0, nb, (nq, k)).astype(np.int64)
    e_values = np.sort(10.0 ** rng.uniform(-300.0, 3.0, (nq, k)), axis=1)
    return hits, e_values


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=200000)
    ap.add_argument("--ka", type=int, default=300)
    ap.add_argument("--kb", type=int, default=300)
    ap.add_argument("--nb", type=int, default=200000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--host-rows", type=int, default=2000)
    ap.add_argument("--reference-combined", type=float, default=None, help="make_fuse_golden.py --time: reference_combined_seconds")
    ap.add_argument("--reference-both", type=float, default=None, help="make_fuse_golden.py --time: reference_both_aligned_seconds")
    ap.add_argument("--out", default="profiles/fuse_probe.json")
    args = ap.parse_args()
    L = _lib.lib()
    rng = np.random.default_rng(0)
    nq, ka, kb, sub = args.rows, args.ka, args.kb, min(args.host_rows, args.rows)
    hits_a, e_a = e_value_lists(rng, nq, ka, args.nb)
    hits_b, e_b = e_value_lists(rng, nq, kb, args.nb)
    keep_a = (e_a < 0.1).astype(np.uint8)
    with np.errstate(divide="ignore"):
        log_a = -np.log(e_a + 10**-200)
    knn_scores = -np.sort(-rng.random((nq, kb)), axis=1)
    doc = {"box": socket.gethostname(), "library": L.knn_version().decode(), "rows": nq, "ka": ka, "kb": kb, "k_out": ka,
           "input_bytes": int(hits_a.nbytes + e_a.nbytes + hits_b.nbytes + e_b.nbytes), "host_rows": sub, "results": []}
    cases = (("sorted_union", SORTED_UNION, 1, (hits_a, e_a, None, hits_b, e_b), args.reference_both),
             ("prefix_fill", PREFIX_FILL, 0, (hits_a, log_a, keep_a, hits_b, knn_scores), args.reference_combined))
    for name, mode, ascending, arrays, ref_seconds in cases:
        device_call(L, *arrays, mode, ascending, ka)
        ts = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            got = device_call(L, *arrays, mode, ascending, ka)
            ts.append(time.perf_counter() - t0)
        head = [None if a is None else a[:sub] for a in arrays]
        t0 = time.perf_counter()
        want = host_union(head[0], head[1], head[3], head[4], ka) if mode == SORTED_UNION else host_prefix(*head, ka)
        host_s = time.perf_counter() - t0
        same = all(np.array_equal(a[:sub].view(np.uint64) if a.dtype == np.float64 else a[:sub], b.view(np.uint64) if b.dtype == np.float64 else b)
                   for a, b in zip(got, want))
        rec = {"mode": name, "device": stats(ts), "host_loop_ms_measured": 1e3 * host_s, "host_loop_ms_scaled": 1e3 * host_s * nq / sub,
               "same_outputs": bool(same), "filled_mean": float(got[3].mean())}
        rec["host_over_device"] = rec["host_loop_ms_scaled"] / rec["device"]["median_ms"]
        if ref_seconds is not None:
            rec["reference_loop_ms_scaled"] = 1e3 * ref_seconds * nq / 2000
            rec["reference_over_device"] = rec["reference_loop_ms_scaled"] / rec["device"]["median_ms"]
        doc["results"].append(rec)
        print(json.dumps(rec), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
