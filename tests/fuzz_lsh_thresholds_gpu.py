#!/usr/bin/env python3
"""Developer fuzz: IndexLSH with trained thresholds on random d / nbits / training rows / database / k against the exact
host restatement (tests/lsh_thresholds_reference.py -- not FAISS: no FAISS binary exists here): thresholds, codes and
search results bit for bit.  Exact inputs only (a +-1 rotation, small-integer rows); value sets of both parities, a few
distinct rows, constant rows, rotate_data=False.
usage: fuzz_lsh_thresholds_gpu.py [ncases] [seed] [budget seconds]"""
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(Path(__file__).resolve().parent))
from knn_for_homology_amd import faiss  # noqa: E402
from lsh_reference import codes_diff, int_rows, pm1_rotation, ref_search, search_diff  # noqa: E402
from lsh_thresholds_reference import ref_codes_thr, ref_thresholds  # noqa: E402

VALUES = [(-3, -1, 1, 3), (-2, 0, 2), (-2, -1, 0, 1, 2), (0, 1), (-5, 0, 0, 0, 7)]


def run(ncases=200, seed=1, budget_s=None):
    """-> (failures, cases run); budget_s: stop starting new cases after that many seconds"""
    rng = np.random.default_rng(seed)
    fails = 0
    t0 = time.time()
    ran = 0
    for case in range(ncases):
        if budget_s is not None and time.time() - t0 > budget_s:
            break
        ran = case + 1
        nbits = int(rng.choice([1, 7, 8, 63, 64, 65, 127, 128, 129, 200, 256, 257, 513, 777, 1024, 1025, 2047, 2048]))
        d = int(rng.choice([1, 2, 7, 31, 32, 33, 64, 100, 257]))
        nt = int(rng.choice([1, 2, 3, 4, 5, 63, 127, 128, 129, 255, 256, 1000, 1001, 4097, 20000]))
        nb = int(rng.choice([1, 7, 255, 257, 1000, 4097, 20000]))
        nq = int(rng.choice([1, 2, 31, 33, 100, 600]))
        k = int(rng.choice([1, 10, 100, 1000, 1401, 2048]))
        if nt * d * nbits > 1e9:
            nt = max(1, int(1e9 / (d * nbits)))
        if nb * d * nbits > 1e9:
            nb = max(1, int(1e9 / (d * nbits)))
        W = 2
        while W * 64 < nbits:
            W *= 2
        if nq * nb * W > 2e7:  # (the host restatement's cost)
            nq = max(1, int(2e7 / (nb * W)))
        kind = int(rng.integers(0, 4))
        identity = kind == 3 and nbits <= d
        R = np.eye(d, dtype=np.float32)[:nbits] if identity else pm1_rotation(rng, nbits, d)
        values = VALUES[int(rng.integers(0, len(VALUES)))]
        if kind == 1:  # a few distinct rows: every column is a handful of tie groups
            base = int_rows(rng, 3, d, values=values)
            xt = np.ascontiguousarray(base[rng.integers(0, 3, nt)])
        elif kind == 2 and rng.integers(0, 2):  # constant rows
            xt = np.full((nt, d), float(rng.choice([-1.0, 0.0, 2.0])), np.float32)
        else:  # two value sets mixed: both parities, half-integer medians for even nt
            xt = int_rows(rng, nt, d, values=values)
            other = int_rows(rng, nt, d, values=VALUES[int(rng.integers(0, len(VALUES)))])
            pick = rng.integers(0, 2, nt).astype(bool)
            xt[pick] = other[pick]
        xb = int_rows(rng, nb, d, values=values)
        xb[: min(nb, nt)] = xt[: min(nb, nt)]  # rows on the thresholds
        xq = int_rows(rng, nq, d, values=values)
        idx = faiss.IndexLSH(d, nbits, not identity, True, _rotation=None if identity else R)
        idx.train(xt)
        t = ref_thresholds(xt, R)
        got = idx.thresholds
        msg = None
        if got.shape != t.shape or (got.view(np.uint32) != t.view(np.uint32)).any():
            j = int(np.flatnonzero(got.view(np.uint32) != t.view(np.uint32))[0]) if got.shape == t.shape else -1
            msg = f"thresholds differ; first: bit {j}: got {got[j]!r}, expected {t[j]!r}"
        if msg is None:
            idx.add(xb)
            cb = ref_codes_thr(xb, R, t)
            msg = codes_diff(idx.codes(), cb)
        if msg is None:
            D, I = idx.search(xq, k)
            De, Ie = ref_search(cb, ref_codes_thr(xq, R, t), k)
            msg = search_diff(D, I, De, Ie)
        what = f"nbits={nbits} d={d} nt={nt} nb={nb} nq={nq} k={k} kind={kind} values={values}"
        if msg is not None:
            fails += 1
            print(f"FAIL case {case}: {what}: {msg}", flush=True)
        elif case % 20 == 0:
            print(f"case {case} ok ({time.time()-t0:.0f}s): {what}", flush=True)
    print(f"FUZZ FAILS: {fails} of {ran}")
    return fails, ran


if __name__ == "__main__":
    _n = int(sys.argv[1]) if len(sys.argv) > 1 else 200
    _s = int(sys.argv[2]) if len(sys.argv) > 2 else 1
    _b = float(sys.argv[3]) if len(sys.argv) > 3 else None
    sys.exit(1 if run(_n, _s, _b)[0] else 0)
