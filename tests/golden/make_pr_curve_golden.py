#!/usr/bin/env python3
"""Regenerates tests/golden/reference_pr_curve.npz -- run ONLY in the build container (needs /root/reference).

The reference's results script pfam/proteins.py is a notebook-style file that loads the whole Pfam dataset at import, so it
cannot be imported.  This script parses it with `ast`, picks out two nodes -- the function `compute_correctness_array`
(lines 201-207) and the loop `for correct, scores, label in prec_recall_data:` (lines 626-648) -- compiles those nodes as
they are and runs them in a namespace that holds synthetic `homologous_proteins_int`, `correct_totals`,
`prec_recall_data`, `limit`, `smoothness`, `numpy` and an identity `tqdm`.  No reference source is copied: the fixture
holds the inputs and the arrays the reference's code produced from them (the correctness matrices and plot_data's recall /
precision / thresholds), under this container's numpy (version stored in the file).

    python tests/golden/make_pr_curve_golden.py            # writes the fixture
    python tests/golden/make_pr_curve_golden.py --time     # the same loop node on 2000 x 300, smoothness 300: prints seconds
"""
import argparse
import ast
import json
import time
from pathlib import Path

import numpy

REFERENCE = Path("/root/reference/pfam/proteins.py")
OUT = Path(__file__).resolve().parent / "reference_pr_curve.npz"


def reference_nodes():
    tree = ast.parse(REFERENCE.read_text())
    func = loop = None
    for node in ast.walk(tree):
        if isinstance(node, ast.FunctionDef) and node.name == "compute_correctness_array":
            func = node
        if (isinstance(node, ast.For) and isinstance(node.iter, ast.Name) and node.iter.id == "prec_recall_data"
                and isinstance(node.target, ast.Tuple) and [e.id for e in node.target.elts] == ["correct", "scores", "label"]):
            loop = node
    assert func is not None and loop is not None, "the reference's nodes were not found"
    return func, loop


def run_node(node, namespace):
    module = ast.Module(body=[node], type_ignores=[])
    exec(compile(module, str(REFERENCE), "exec"), namespace)


def namespace(homologous, totals, limit, smoothness):
    return {"numpy": numpy, "ndarray": numpy.ndarray, "tqdm": lambda x, *a, **k: x, "homologous_proteins_int": homologous,
            "correct_totals": totals, "limit": limit, "smoothness": smoothness, "plot_data": dict()}


def reference_run(func, loop, hits, homologous, scores, limit, smoothness):
    """-> (correct, recall, precision, thresholds, totals) as the reference's own code computes them"""
    # pfam/proteins.py:194-198, the totals (three lines of plain Python around a set; restated, not compiled)
    totals = numpy.asarray([len(set(homologous[i])) for i in range(len(hits))])
    ns = namespace(homologous, totals, limit, smoothness)
    run_node(func, ns)
    correct = ns["compute_correctness_array"](hits)
    ns["prec_recall_data"] = [(correct, scores, "case")]
    run_node(loop, ns)
    recall, precision, thresholds = ns["plot_data"]["case"]
    return correct, numpy.asarray(recall, numpy.float64), numpy.asarray(precision, numpy.float64), numpy.asarray(thresholds), totals


def make_sets(rng, nq, nb, sizes):
    return [rng.integers(0, nb, int(rng.choice(sizes))).tolist() for _ in range(nq)]  # (repeats happen: the set drops them)


def make_hits(rng, homologous, k, nb):
    """half of each row from the query's set, the rest from the whole database, -1 here and there"""
    nq = len(homologous)
    hits = rng.integers(-1, nb, (nq, k)).astype(numpy.int64)
    for q in range(nq):
        pick = rng.random(k) < 0.5
        hits[q, pick] = rng.choice(homologous[q], int(pick.sum()))
    return hits


def cases():
    rng = numpy.random.default_rng(20240)
    out = {}
    # descending cosine-like scores
    for name, nq, k, limit, smoothness in (("small", 37, 12, 7, 10), ("wide", 300, 20, 20, 16)):
        homologous = make_sets(rng, nq, 500, [1, 2, 5, 30])
        hits = make_hits(rng, homologous, k, 500)
        scores = -numpy.sort(-rng.random((nq, k)).astype(numpy.float32), axis=1)
        out[name] = (hits, homologous, scores, limit, smoothness)
    # five score values only: tied quantiles, equal thresholds; some rows hold the lowest value everywhere, which no
    # threshold selects
    nq, k = 600, 9
    homologous = make_sets(rng, nq, 200, [1, 3, 8])
    hits = make_hits(rng, homologous, k, 200)
    scores = rng.choice(numpy.array([0.125, 0.25, 0.5, 0.75, 1.0], numpy.float32), (nq, k))
    scores[::7] = 0.125
    out["tied"] = (hits, homologous, scores.astype(numpy.float32), 6, 12)
    # negated e-values; the last column is a -1e6 sentinel (an e-value of 1e6 pads rows with too few hits)
    nq, k = 50, 10
    homologous = make_sets(rng, nq, 300, [1, 4, 20])
    hits = make_hits(rng, homologous, k, 300)
    e_values = numpy.sort(numpy.exp(rng.normal(-20, 15, (nq, k))).astype(numpy.float32), axis=1)
    e_values[:, -1] = 1e6
    e_values[::5, 6:] = 1e6
    out["evalues"] = (hits, homologous, -e_values, 10, 20)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--time", action="store_true", help="time the reference's loop on 2000 x 300 rows, smoothness 300")
    args = ap.parse_args()
    func, loop = reference_nodes()
    if args.time:
        rng = numpy.random.default_rng(1)
        nq, k = 2000, 300
        correct = rng.random((nq, k)) < 0.2
        scores = rng.random((nq, k)).astype(numpy.float32)
        totals = numpy.maximum(correct.sum(axis=1), 1)
        ns = namespace(None, totals, 300, 300)
        ns["prec_recall_data"] = [(correct, scores, "timed")]
        t0 = time.perf_counter()
        run_node(loop, ns)
        seconds = time.perf_counter() - t0
        print(json.dumps({"reference_loop_seconds": seconds, "nq": nq, "k": k, "limit": 300, "smoothness": 300,
                          "numpy": numpy.__version__}))
        return
    arrays = {"numpy_version": numpy.asarray(numpy.__version__), "cases": numpy.asarray(sorted(cases()))}
    for name, (hits, homologous, scores, limit, smoothness) in cases().items():
        correct, recall, precision, thresholds, totals = reference_run(func, loop, hits, homologous, scores, limit, smoothness)
        assert correct.shape == hits.shape and correct.dtype == bool and len(recall) == smoothness + 1
        members = [sorted(set(h)) for h in homologous]
        arrays.update({
            f"{name}_hits": hits.astype(numpy.int32), f"{name}_scores": scores,
            f"{name}_set_offsets": numpy.concatenate([[0], numpy.cumsum([len(m) for m in members])]).astype(numpy.int64),
            f"{name}_set_members": numpy.concatenate([numpy.asarray(m, numpy.int32) for m in members]),
            f"{name}_totals": totals.astype(numpy.int64), f"{name}_limit": numpy.asarray(limit), f"{name}_smoothness": numpy.asarray(smoothness),
            f"{name}_correct": correct, f"{name}_recall": recall, f"{name}_precision": precision, f"{name}_thresholds": thresholds,
        })
    numpy.savez_compressed(OUT, **arrays)
    print(f"wrote {OUT} ({OUT.stat().st_size} bytes)")


if __name__ == "__main__":
    main()
