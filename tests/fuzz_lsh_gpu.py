#!/usr/bin/env python3
"""Developer fuzz: random nbits / d / nb / nq / k of IndexLSH against the exact host restatement (tests/lsh_reference.py),
codes and results bit for bit.  Data mixes: gaussian integers (zero projections), a few distinct rows (tie groups across
every chunk), duplicated rows, constant rows, database codes loaded through add_codes (read_index's path).
usage: fuzz_lsh_gpu.py [ncases] [seed] [budget seconds]"""
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(Path(__file__).resolve().parent))
from knn_for_homology_amd import _lib, faiss  # noqa: E402
from lsh_reference import codes_diff, int_rows, pm1_rotation, rand_codes, ref_codes, ref_search, search_diff  # noqa: E402


def run(ncases=200, seed=1, budget_s=None):
    """-> (failures, cases run); budget_s: stop starting new cases after that many seconds (the -m gpu tests run a bounded batch)"""
    rng = np.random.default_rng(seed)
    fails = 0
    t0 = time.time()
    ran = 0
    for case in range(ncases):
        if budget_s is not None and time.time() - t0 > budget_s:
            break
        ran = case + 1
        nbits = int(rng.choice([1, 7, 8, 63, 64, 65, 127, 128, 129, 200, 255, 256, 257, 511, 512, 513, 777, 1000, 1024, 1025,
                                1500, 2047, 2048]))
        d = int(rng.choice([1, 2, 7, 31, 32, 33, 64, 100, 128, 257]))
        nb = int(rng.choice([1, 2, 7, 63, 255, 256, 257, 1000, 4097, 8193, 20000, 70001, 150000]))
        nq = int(rng.choice([1, 2, 31, 32, 33, 64, 65, 100, 300, 600]))
        k = int(rng.choice([1, 2, 10, 31, 100, 101, 256, 512, 1000, 1400, 1401, 1536, 1537, 2048]))
        W = 2
        while W * 64 < nbits:
            W *= 2
        if nq * nb * W > 2e7:  # (the host restatement's cost)
            nq = max(1, int(2e7 / (nb * W)))
        kind = int(rng.integers(0, 5))
        if kind == 0 and nb * d * nbits > 2e9:
            kind = 1
        R = pm1_rotation(rng, nbits, d)
        xb = cb = None
        if kind == 0:  # gaussian integers: zeros in the rows, zero projections
            xb = np.rint(3 * rng.standard_normal((nb, d))).astype(np.float32)
        elif kind in (1, 2):  # a few distinct rows (ties everywhere) / duplicated rows
            base = int_rows(rng, 3 if kind == 1 else max(1, nb // 7), d, values=(-2, -1, 0, 1, 2))
            assign = rng.integers(0, base.shape[0], nb)
            xb = np.ascontiguousarray(base[assign])
            cb = ref_codes(base, R)[assign]
        elif kind == 3:  # constant rows (0: every projection zero)
            xb = np.full((nb, d), float(rng.choice([-1.0, 0.0, 2.0])), np.float32)
            cb = np.repeat(ref_codes(xb[:1], R), nb, axis=0)
        else:  # codes through add_codes
            cb = rand_codes(rng, nb, nbits)
        if cb is None:
            cb = ref_codes(xb, R)
        xq = np.rint(3 * rng.standard_normal((nq, d))).astype(np.float32)
        if xb is not None and rng.integers(0, 3) == 0:
            xq[: min(nq, nb)] = xb[: min(nq, nb)]
        idx = faiss.IndexLSH(d, nbits, _rotation=R)
        if xb is not None:
            idx.add(xb)
        else:
            _lib.check(_lib.lib().knn_lsh_add_codes(idx._h, cb.ctypes.data, nb, cb.shape[1]))
        D, I = idx.search(xq, k)
        De, Ie = ref_search(cb, ref_codes(xq, R), k)
        msg = search_diff(D, I, De, Ie)
        if msg is None and xb is not None and rng.integers(0, 4) == 0:
            msg = codes_diff(idx.codes(), cb)
        if msg is not None:
            fails += 1
            print(f"FAIL case {case}: nbits={nbits} d={d} nb={nb} nq={nq} k={k} kind={kind}: {msg}", flush=True)
        elif case % 20 == 0:
            print(f"case {case} ok ({time.time()-t0:.0f}s): nbits={nbits} d={d} nb={nb} nq={nq} k={k} kind={kind}", flush=True)
    print(f"FUZZ FAILS: {fails} of {ran}")
    return fails, ran


if __name__ == "__main__":
    _n = int(sys.argv[1]) if len(sys.argv) > 1 else 200
    _s = int(sys.argv[2]) if len(sys.argv) > 2 else 1
    _b = float(sys.argv[3]) if len(sys.argv) > 3 else None  # stop starting new cases after that many seconds
    sys.exit(1 if run(_n, _s, _b)[0] else 0)
