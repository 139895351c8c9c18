#!/usr/bin/env python3
"""Regenerates tests/golden/reference_fuse.npz -- run ONLY in the build container (needs /root/reference).

The reference's results script pfam/proteins.py is a notebook-style file that loads the whole Pfam dataset at import, so it
cannot be imported.  This script parses it with `ast` and picks out two `for` nodes: the "combined" loop, whose target
unpacks `t5_hits_row, t5_row_scores, mmseqs_hits_row, mmseqs_row_e_values` (lines 216-238), and the "both aligned" loop
over `zip(tqdm(both_aligned_hits_base), both_aligned_e_values_base)` (lines 342-370).  It compiles those nodes as they are
and runs them in a namespace that holds synthetic arrays, the few assignments in front of the loops restated (`threshold`,
the empty lists, `mmseqs_hits`, the two concatenations), `numpy` and an identity `tqdm`; the `numpy.asarray` calls behind
the loops are restated too.  No reference source is copied: the fixture holds the inputs and the arrays the reference's
code produced from them, under this container's numpy (version stored in the file).

The inputs are chosen so that the reference alone is deterministic and does not raise: scores are distinct within a row
(numpy.argsort's default sort is not stable) except for the MMseqs2-style padding (id 0, e-value 100000), whose tied
entries all carry the same id, so that any order among them gives the same row; every combined row fills before B's last
entry (the reference's `for ... else` raises otherwise).

    python tests/golden/make_fuse_golden.py            # writes the fixture
    python tests/golden/make_fuse_golden.py --time     # the two loop nodes on 2000 x 300 (+ 300): prints seconds
"""
import argparse
import ast
import json
import time
from pathlib import Path

import numpy

REFERENCE = Path("/root/reference/pfam/proteins.py")
OUT = Path(__file__).resolve().parent / "reference_fuse.npz"
COMBINED_NAMES = ["t5_hits_row", "t5_row_scores", "mmseqs_hits_row", "mmseqs_row_e_values"]
PAD_ID, PAD_E_VALUE = 0, 100000.0


def reference_nodes():
    tree = ast.parse(REFERENCE.read_text())
    combined = both = None
    for node in ast.walk(tree):
        if not isinstance(node, ast.For):
            continue
        for t in ast.walk(node.target):
            if isinstance(t, ast.Tuple) and [getattr(e, "id", None) for e in t.elts] == COMBINED_NAMES:
                combined = node
        it = node.iter
        if (isinstance(it, ast.Call) and getattr(it.func, "id", None) == "zip" and len(it.args) == 2
                and isinstance(it.args[0], ast.Call) and getattr(it.args[0].func, "id", None) == "tqdm"
                and getattr(it.args[0].args[0], "id", None) == "both_aligned_hits_base"
                and getattr(it.args[1], "id", None) == "both_aligned_e_values_base"):
            both = node
    assert combined is not None and both is not None, "the reference's nodes were not found"
    return combined, both


def run_node(node, namespace):
    module = ast.Module(body=[node], type_ignores=[])
    exec(compile(module, str(REFERENCE), "exec"), namespace)


def run_combined(node, mmseqs_hits, mmseqs_e_values, t5_hits, t5_scores):
    """-> (combined_hits, combined_scores) as the reference's own loop builds them"""
    ns = {"numpy": numpy, "tqdm": lambda x, *a, **k: x, "threshold": 0.1, "combined_hits": [], "combined_scores": [],
          "t5_hits": t5_hits, "t5_scores": t5_scores, "mmseqs_hits": mmseqs_hits, "mmseqs_e_values": mmseqs_e_values}
    run_node(node, ns)
    return numpy.asarray(ns["combined_hits"]), numpy.asarray(ns["combined_scores"])  # (proteins.py:239-240)


def run_both(node, mmseqs_hits, mmseqs_e_values, t5_aligned_hits, t5_aligned_e_values):
    """-> (both_aligned_hits, both_aligned_e_values)"""
    ns = {"numpy": numpy, "tqdm": lambda x, *a, **k: x, "mmseqs_hits": mmseqs_hits, "both_aligned_hits": [], "both_aligned_e_values": [],
          # proteins.py:335-338
          "both_aligned_hits_base": numpy.concatenate([mmseqs_hits, t5_aligned_hits], axis=1),
          "both_aligned_e_values_base": numpy.concatenate([mmseqs_e_values, t5_aligned_e_values], axis=1)}
    run_node(node, ns)
    return numpy.asarray(ns["both_aligned_hits"]), numpy.asarray(ns["both_aligned_e_values"])  # (proteins.py:371-372)


def e_value_list(rng, nq, width, nb, real_counts, exponents=(-300.0, 3.0)):
    """MMseqs2-style rows: n real hits (distinct ids from 1 .. nb - 1, e-values 10^u ascending, most of them far below
    float32's range), then the padding"""
    hits = numpy.full((nq, width), PAD_ID, numpy.int64)
    e_values = numpy.full((nq, width), PAD_E_VALUE, numpy.float64)
    for q in range(nq):
        n = int(real_counts[q])
        hits[q, :n] = rng.choice(numpy.arange(1, nb), n, replace=False)
        e_values[q, :n] = numpy.sort(10.0 ** rng.uniform(exponents[0], exponents[1], n))
    return hits, e_values


def share_ids(rng, hits, other, other_real, count):
    """puts up to `count` of the other list's real ids of each row into the row, at random columns, keeping the row's ids distinct"""
    for q in range(len(hits)):
        pool = [h for h in other[q, :other_real[q]] if h not in set(hits[q])]
        take = min(count, len(pool))
        real = int((hits[q] != PAD_ID).sum())
        if take and real:
            cols = rng.choice(real, min(take, real), replace=False)
            hits[q, cols] = rng.choice(pool, len(cols), replace=False)


def combined_case(rng, nq=36, width=30, kb=40, nb=600):
    real = rng.integers(0, width + 1, nq)
    real[1::6] = width                      # no padding: with small e-values the kept prefix is the whole of A
    mm_hits, mm_e = e_value_list(rng, nq, width, nb, real)
    for q in range(0, nq, 6):               # nothing under the threshold: the kept prefix is empty
        mm_e[q, :real[q]] = numpy.sort(10.0 ** rng.uniform(-0.9, 3.0, real[q]))
    for q in range(1, nq, 6):
        mm_e[q] = numpy.sort(10.0 ** rng.uniform(-300.0, -1.5, width))
    mm_e[2, 0] = 0.0                        # log(0 + 10**-200)
    perm = rng.permutation(width)           # one row out of order: the kept entries are not a prefix
    mm_hits[3], mm_e[3] = mm_hits[3, perm], mm_e[3, perm]
    t5_hits = numpy.stack([rng.choice(numpy.arange(1, nb), kb, replace=False) for _ in range(nq)]).astype(numpy.int64)
    share_ids(rng, t5_hits, mm_hits, real, 8)
    t5_scores = -numpy.sort(-rng.random((nq, kb)).astype(numpy.float32), axis=1)
    for q in range(nq):
        assert len(set(t5_hits[q])) == kb and len(set(t5_scores[q])) == kb
        kept = set(mm_hits[q][mm_e[q] < 0.1])
        assert int((mm_e[q] < 0.1).sum()) + sum(h not in kept for h in t5_hits[q, :-1]) >= width, "a row would not fill"
    assert any(len(set(mm_hits[q][mm_e[q] < 0.1]) & set(t5_hits[q])) for q in range(nq))
    return mm_hits, mm_e, t5_hits, t5_scores


def both_case(rng, nq, width_a, width_b, nb=400):
    real_a = rng.integers(0, width_a + 1, nq)
    real_b = rng.integers(0, width_b + 1, nq)
    real_a[0], real_b[0] = width_a, width_b  # no padding at all
    real_a[1], real_b[1] = 2, 3              # nearly all padding: the row stays short
    a_hits, a_e = e_value_list(rng, nq, width_a, nb, real_a)
    b_hits, b_e = e_value_list(rng, nq, width_b, nb, real_b)
    share_ids(rng, b_hits, a_hits, real_a, 10)
    shared = tiny = 0
    for q in range(nq):
        row = numpy.concatenate([a_e[q, :real_a[q]], b_e[q, :real_b[q]]])
        assert len(set(row)) == len(row) and PAD_E_VALUE not in row, "scores must be distinct within a row"
        shared += len(set(a_hits[q, :real_a[q]]) & set(b_hits[q, :real_b[q]]))
        tiny += int(((a_e[q] > 1e-300) & (a_e[q] < 1e-46)).any() and ((b_e[q] > 1e-300) & (b_e[q] < 1e-46)).any())
    assert shared > nq and tiny > nq // 2
    return a_hits, a_e, b_hits, b_e


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--time", action="store_true", help="time the reference's two loops on 2000 rows of 300 (+ 300) entries")
    args = ap.parse_args()
    combined, both = reference_nodes()
    if args.time:
        rng = numpy.random.default_rng(1)
        nq, w = 2000, 300
        mm_hits, mm_e = e_value_list(rng, nq, w, 200000, numpy.full(nq, w), exponents=(-300.0, -2.0))
        mm_e[:, w // 2:] = PAD_E_VALUE  # half of every row is kept, the other half is filled from the k-NN hits
        t5_hits = rng.integers(1, 200000, (nq, w)).astype(numpy.int64)
        t5_scores = rng.random((nq, w)).astype(numpy.float32)
        t0 = time.perf_counter()
        run_combined(combined, mm_hits, mm_e, t5_hits, t5_scores)
        t1 = time.perf_counter()
        al_hits, al_e = e_value_list(rng, nq, w, 200000, rng.integers(0, w + 1, nq))
        t2 = time.perf_counter()
        run_both(both, mm_hits, mm_e, al_hits, al_e)
        t3 = time.perf_counter()
        print(json.dumps({"reference_combined_seconds": t1 - t0, "reference_both_aligned_seconds": t3 - t2, "nq": nq, "ka": w, "kb": w,
                          "numpy": numpy.__version__}))
        return
    rng = numpy.random.default_rng(20250)
    arrays = {"numpy_version": numpy.asarray(numpy.__version__)}
    a_hits, a_e, b_hits, b_scores = combined_case(rng)
    hits, scores = run_combined(combined, a_hits, a_e, b_hits, b_scores)
    assert hits.shape == a_hits.shape and hits.dtype == numpy.int64 and scores.dtype == numpy.float64
    arrays.update(combined_hits_a=a_hits, combined_e_values_a=a_e, combined_hits_b=b_hits, combined_scores_b=b_scores,
                  combined_hits=hits, combined_scores=scores)
    for name, nq, wa, wb in (("both", 36, 30, 30), ("both_uneven", 12, 40, 17)):
        a_hits, a_e, b_hits, b_e = both_case(rng, nq, wa, wb)
        hits, scores = run_both(both, a_hits, a_e, b_hits, b_e)
        assert hits.shape == a_hits.shape and hits.dtype == numpy.int64 and scores.dtype == numpy.float64
        arrays.update({f"{name}_hits_a": a_hits, f"{name}_e_values_a": a_e, f"{name}_hits_b": b_hits, f"{name}_e_values_b": b_e,
                       f"{name}_hits": hits, f"{name}_e_values": scores})
    numpy.savez_compressed(OUT, **arrays)
    print(f"wrote {OUT} ({OUT.stat().st_size} bytes)")


if __name__ == "__main__":
    main()
