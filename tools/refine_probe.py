"""IndexRefineFlat(IndexLSH) on one MI355X: what the re-scoring gather reaches, and the whole search against the way the
same result was obtained before the fused path existed.

    python tools/refine_probe.py --nb 200000 2000000 --baseline --out profiles/refine_probe.json

d = 1024, normalised Gaussian rows, inner product.  Per (nb, nbits, nq, (k, kb)), after two warm-up calls:
  refined   wall clock around IndexRefineFlat.search (median, min, max of --reps calls) and the HIP-event times of its
            rescore and final-selection launches (knn_last_refine_ms); gather rate = nq * kb * dp * 4 bytes / rescore time,
            next to the streaming read rate of the same rows on the same box (knn_flat_read_rate)
  baseline  (--baseline) IndexLSH.search(x, kb), knn_gather_distances on the returned ids, numpy sort per row: the public
            interface without IndexRefineFlat.  Calls slower than a second are repeated --slow-reps times only.
  flat      IndexFlat.search at the same (nb, nq, k), three calls, and recall@k of the refined result against it
Results are appended to the output file shape by shape, so a run that is cut short keeps what it measured."""
import argparse
import json
import os
import socket
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ctypes  # noqa: E402

from knn_for_homology_amd import _lib, faiss  # noqa: E402

D = 1024


def stats(ts):
    ts = sorted(ts)
    return {"median_ms": 1e3 * float(np.median(ts)), "min_ms": 1e3 * ts[0], "max_ms": 1e3 * ts[-1], "reps": len(ts)}


def timed(fn, reps, slow_reps):
    out = None
    ts = []
    while len(ts) < reps:
        t0 = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - t0)
        if ts[-1] > 1.0 and len(ts) >= slow_reps:
            break
    return stats(ts), out


def baseline_search(lsh, flat, xq, k, kb):
    """the same result through the public interface without IndexRefineFlat (inner product)"""
    nq = xq.shape[0]
    _, I = lsh.search(xq, kb)
    off = np.arange(nq + 1, dtype=np.int64) * kb
    scores = np.empty(nq * kb, np.float32)
    _lib.check(_lib.lib().knn_gather_distances(flat._h, xq.ctypes.data, nq, I.ctypes.data, off.ctypes.data, scores.ctypes.data))
    scores = scores.reshape(nq, kb)
    order = np.argsort(-scores, axis=1, kind="stable")[:, :k]
    return np.take_along_axis(scores, order, 1), np.take_along_axis(I, order, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nb", type=int, nargs="+", default=[200_000, 2_000_000])
    ap.add_argument("--nbits", type=int, nargs="+", default=[1024, 2048])
    ap.add_argument("--nq", type=int, nargs="+", default=[32, 1024, 16384])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--slow-reps", type=int, default=5)
    ap.add_argument("--baseline", action="store_true")
    ap.add_argument("--out", default="profiles/refine_probe.json")
    args = ap.parse_args()
    shapes = [(100, 2048), (1000, 2000)]
    L = _lib.lib()
    doc = {"box": socket.gethostname(), "library": L.knn_version().decode(), "d": D, "metric": "inner product",
           "rows": "normalised Gaussian", "reps": args.reps, "results": []}

    def flush():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)

    rng = np.random.default_rng(0)
    xq_all = rng.standard_normal((max(args.nq), D)).astype(np.float32)
    xq_all /= np.linalg.norm(xq_all, axis=1, keepdims=True)
    for nb in args.nb:
        flat = faiss.IndexFlat(D, faiss.METRIC_INNER_PRODUCT)
        refined = {}
        for nbits in args.nbits:
            r = faiss.IndexRefineFlat(faiss.IndexLSH(D, nbits), metric=faiss.METRIC_INNER_PRODUCT)
            r.refine_index = flat  # one copy of the rows for every code width
            refined[nbits] = r
        for i0 in range(0, nb, 200_000):
            x = rng.standard_normal((min(200_000, nb - i0), D)).astype(np.float32)
            x /= np.linalg.norm(x, axis=1, keepdims=True)
            flat.add(x)
            for r in refined.values():
                r.base_index.add(x)
        ms, nbytes = ctypes.c_float(), ctypes.c_int64()
        _lib.check(L.knn_flat_read_rate(flat._h, 3, ctypes.byref(ms), ctypes.byref(nbytes)))
        stream_gbs = nbytes.value / (ms.value * 1e-3) / 1e9
        flat_ref = {}
        for nq in args.nq:
            xq = np.ascontiguousarray(xq_all[:nq])
            for k, kb in shapes:
                st, (_, If) = timed(lambda: flat.search(xq, k), 3, 2)
                flat_ref[(nq, k)] = (st, If)
        for nbits in args.nbits:
            r = refined[nbits]
            for nq in args.nq:
                xq = np.ascontiguousarray(xq_all[:nq])
                for k, kb in shapes:
                    r.k_factor = kb / k
                    assert int(np.float32(k) * np.float32(r.k_factor)) == kb
                    for _ in range(2):
                        r.search(xq, k)
                    resc, sel, ts = [], [], []
                    I = None
                    for _ in range(args.reps):
                        t0 = time.perf_counter()
                        _, I = r.search(xq, k)
                        ts.append(time.perf_counter() - t0)
                        t = r.last_refine()
                        resc.append(t["rescore_ms"])
                        sel.append(t["select_ms"])
                    gathered = nq * kb * D * 4
                    rec = {"nb": nb, "nbits": nbits, "nq": nq, "k": k, "kb": kb, "refined": stats(ts),
                           "rescore_ms": {"median": float(np.median(resc)), "min": min(resc), "max": max(resc)},
                           "select_ms": {"median": float(np.median(sel)), "min": min(sel), "max": max(sel)},
                           "gather_bytes": gathered, "gather_GBps": gathered / (float(np.median(resc)) * 1e-3) / 1e9,
                           "stream_read_GBps": stream_gbs}
                    fst, If = flat_ref[(nq, k)]
                    rec["flat_search"] = fst
                    rec["recall_at_k"] = float(np.mean([len(np.intersect1d(I[i], If[i])) / k for i in range(nq)]))
                    if args.baseline:
                        for _ in range(2 if nq * kb < 1 << 22 else 1):
                            baseline_search(r.base_index, flat, xq, k, kb)
                        bst, (_, Ib) = timed(lambda: baseline_search(r.base_index, flat, xq, k, kb), args.reps, args.slow_reps)
                        rec["baseline"] = bst
                        rec["refined_over_baseline"] = rec["refined"]["median_ms"] / bst["median_ms"]
                        rec["baseline_same_id_sets"] = bool(all(set(I[i]) == set(Ib[i]) for i in range(0, nq, max(1, nq // 64))))
                    doc["results"].append(rec)
                    flush()
                    print(json.dumps(rec), flush=True)
        del refined, flat, flat_ref
        L.knn_trim()


if __name__ == "__main__":
    main()
