#!/usr/bin/env python3
"""Developer fuzz of the prefilter on 12-bit row copies (knn_flat_set_scan16 mode 2), on the model of
tests/fuzz_scan16_gpu.py, with the tuning flags and the chunk count varied as well (a seed the fp32 search would take from a
strided sample, no pairs, no pool, an explicit reset): every case searches one index with
the prefilter forced on (KNN_TUNE_SCAN16_ANY_NB) and with it off (KNN_TUNE_NO_SCAN16) and compares D / I bit for bit, and
against the CPU oracle.  Random shapes, k, batch sizes and data kinds: gaussian, L2-normalised, rows scaled by powers
of two up to 2^+-40, magnitudes mixed inside rows, duplicated and zero rows, near-duplicates of a query that fp16 cannot
tell apart (the device fallback), constant rows, and the adversarial generators of tests/scan16_reference.py (copy errors
aligned with the query, flushed entries, rows at the exponent clamp and subnormals, the exponent gate) at the case's d;
those bring their own rows, queries and k; the clamped-maximum and rounds-to-zero cases of tests/scan12_reference.py.
usage: fuzz_scan12_gpu.py [ncases] [seed]"""
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from knn_for_homology_amd import faiss  # noqa: E402
from knn_for_homology_amd import _lib  # noqa: E402
from knn_for_homology_amd._lib import KNN_TUNE_NO_SCAN16, KNN_TUNE_SCAN16_ANY_NB  # noqa: E402
from oracle import knn_oracle as ko  # noqa: E402
sys.path.insert(0, str(ROOT / "tests"))
import scan12_reference as s12  # noqa: E402
import scan16_reference as sr  # noqa: E402

FLAGS = (0, 0, 0, _lib.KNN_TUNE_EXACT_SEED, _lib.KNN_TUNE_NO_TILE_MIN_SEED, _lib.KNN_TUNE_NO_PAIRS, _lib.KNN_TUNE_NO_POOL, _lib.KNN_TUNE_NO_SEED,
         _lib.KNN_TUNE_ALWAYS_RESET, _lib.KNN_TUNE_NO_TILE_MIN_SEED | _lib.KNN_TUNE_NO_PAIRS, 1 << _lib.KNN_TUNE_PUB_ROUNDS_SHIFT)

KINDS = ("gauss", "normed", "scaled", "mixed", "dups", "near", "const", "aligned", "flushed", "tiny", "gate", "clamped", "planted")


def adversarial(rng, kind, d):
    """(xb, xq, k) of one of the reference's generators at d (even: the aligned rows come in pairs of entries) and a random
    seed / background size / k.  Of the tiny kind only the subnormal query and the p = -130 scores always fall back."""
    seed, k = int(rng.integers(1, 1 << 30)), int(rng.choice([1, 2, 10, 50]))
    if kind == "clamped":
        c = s12.clamped_max(d, seed, k=k, nbg=int(rng.integers(300, 3000)))
    elif kind == "flushed" and rng.random() < 0.5:
        c = s12.rounds_to_zero(bool(rng.random() < 0.5), d, seed, k=k, nbg=int(rng.integers(300, 3000)))
    elif kind == "aligned":
        c = sr.aligned_rows(d, seed, nbg=int(rng.integers(300, 3000)), k=max(2, k)) if rng.random() < 0.5 else sr.aligned_query(d, seed, nbg=int(rng.integers(300, 3000)), k=max(2, k))
    elif kind == "flushed":
        c = sr.flushed(bool(rng.random() < 0.5), d, seed, k=k, nbg=int(rng.integers(300, 3000)))
    elif kind == "tiny":
        which = int(rng.integers(0, 4))
        if which == 0:
            c = sr.tiny(d, seed, k=k, subq=bool(rng.random() < 0.25))
        elif which == 1:
            c = sr.subnormal_query_case(d, seed, k=k, nb=int(rng.integers(300, 3000)))
        else:
            c = sr.subnormal_scores(d, seed, k=k, nb=int(rng.integers(300, 3000)), p=int(rng.choice([-130, -125, -122, -118])))
    else:
        c = sr.gate(bool(rng.random() < 0.5), d, seed, k=k, nbg=int(rng.integers(300, 3000)))
    return c.xb, c.xq, c.k


def data(rng, kind, nb, d, nq):
    xb = rng.standard_normal((nb, d), dtype=np.float32)
    xq = rng.standard_normal((nq, d), dtype=np.float32)
    if kind == "normed":
        xb /= np.linalg.norm(xb, axis=1, keepdims=True)
        xq /= np.linalg.norm(xq, axis=1, keepdims=True)
    elif kind == "scaled":
        xb *= np.exp2(rng.integers(-40, 41, size=(nb, 1))).astype(np.float32)
        xq *= np.float32(2.0 ** int(rng.integers(-20, 21)))
    elif kind == "mixed":
        xb[:, : max(1, d // 3)] *= np.float32(2.0 ** 18)
    elif kind == "dups":
        src = rng.integers(0, nb, size=nb // 4)
        xb[rng.integers(0, nb, size=nb // 4)] = xb[src]
        xb[rng.integers(0, nb, size=max(1, nb // 50))] = 0.0
    elif kind == "near":
        m = int(min(nb // 2, rng.integers(50, 3000)))
        j = int(rng.integers(0, nq))
        xb[:m] = xq[j] + rng.standard_normal((m, d), dtype=np.float32) * np.float32(1e-6)
    elif kind == "const":
        xb[:] = np.float32(rng.standard_normal())
    elif kind == "planted":  # every query's best rows at the starts of the 8-row blocks a seed sample would take
        xb[::8] += xq[np.arange(len(xb[::8])) % nq] * np.float32(0.5)
    return xb, xq


def run(ncases=1000, seed=1):
    rng = np.random.default_rng(seed)
    orc = ko.oracle()
    fails = used = fallbacks = 0
    t0 = time.time()
    for case in range(ncases):
        d = int(rng.choice([8, 16, 32, 40, 64, 100, 128, 256, 300]))
        nb = int(rng.integers(300, 40000))
        nq = int(rng.integers(1, 33))
        k = int(min(nb, rng.choice([1, 2, 10, 50, 100, 256, 500, 1000, 1500])))
        kind = KINDS[case % len(KINDS)]
        if kind in ("aligned", "flushed", "tiny", "gate", "clamped"):
            xb, xq, k = adversarial(rng, kind, d)
            nb, nq = len(xb), len(xq)
        else:
            xb, xq = data(rng, kind, nb, d, nq)
        idx = faiss.IndexFlat(d, faiss.METRIC_INNER_PRODUCT)
        flags = int(FLAGS[int(rng.integers(0, len(FLAGS)))])
        nchunks = int(rng.choice([0, 0, 0, 1, 3, 7, 64]))
        idx.set_scan16(2)
        idx.add(xb)
        fb0 = idx.last_scan16()["fallbacks"]
        idx.set_tuning(0, nchunks, KNN_TUNE_SCAN16_ANY_NB | flags)
        D, I = idx.search(xq, k)
        info = idx.last_scan16()
        info["flags"], info["nchunks"] = flags, nchunks
        idx.set_tuning(0, nchunks, KNN_TUNE_NO_SCAN16 | flags)
        D0, I0 = idx.search(xq, k)
        Do, Io = orc.flat_search(xb, xq, k, faiss.METRIC_INNER_PRODUCT)
        ok = (np.array_equal(I, I0) and np.array_equal(D.view(np.uint32), D0.view(np.uint32))
              and np.array_equal(I, Io) and np.array_equal(D.view(np.uint32), Do.view(np.uint32)))
        ok = ok and (not info["used"] or info["format"] == 12)
        used += info["used"]
        fallbacks += info["fallbacks"] - fb0
        if not ok:
            fails += 1
            print(f"FAIL case {case}: d={d} nb={nb} nq={nq} k={k} kind={kind} {info}", flush=True)
        elif case % 50 == 0:
            print(f"case {case} ok ({time.time() - t0:.0f}s): d={d} nb={nb} nq={nq} k={k} kind={kind} {info}", flush=True)
    print(f"SCAN12 FUZZ: {fails} failures of {ncases} cases; {used} took the prefilter, {fallbacks} fell back on the device "
          f"({time.time() - t0:.0f}s)")
    return fails


if __name__ == "__main__":
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 1000
    s = int(sys.argv[2]) if len(sys.argv) > 2 else 1
    sys.exit(1 if run(n, s) else 0)
