#!/usr/bin/env python3
"""Regenerates tests/golden/reference_buckets.npz -- run ONLY in the build container (needs /root/reference and scipy).

Built as make_pr_curve_golden.py is: the reference's results script pfam/proteins.py cannot be imported (it loads the whole
Pfam dataset at import), so this script parses it with `ast` and picks out four nodes -- the assignment
`score_buckets = numpy.linspace(...)` (line 692), the loop `for i in tqdm(score_buckets):` (lines 696-705), the function
`make_accuracy_over_hit` (lines 502-507) and the assignment `recall_per_query = ...` (line 478) -- compiles those nodes as
they are and runs them in a namespace that holds synthetic `plot_subset_scores`, `plot_subset_correct`, `correct`,
`correct_totals`, `smoothness`, `numpy`, an identity `tqdm` and scipy's `sem`.  The `sem` handed in also notes the length
and the sum of every array the loop passes to it: the counts of the non-empty buckets, from the reference's own masks.
No reference source is copied: the fixture holds the inputs and the arrays the reference's code produced from them, under
this container's numpy and scipy (versions stored in the file).

    python tests/golden/make_buckets_golden.py
"""
import ast
from pathlib import Path

import numpy
import scipy
from scipy.stats import sem

REFERENCE = Path("/root/reference/pfam/proteins.py")
OUT = Path(__file__).resolve().parent / "reference_buckets.npz"


def _assigns(node, name):
    return isinstance(node, ast.Assign) and len(node.targets) == 1 and isinstance(node.targets[0], ast.Name) and node.targets[0].id == name


def reference_nodes():
    tree = ast.parse(REFERENCE.read_text())
    edges = loop = func = recall = None
    for node in ast.walk(tree):
        if _assigns(node, "score_buckets"):
            edges = node
        if (isinstance(node, ast.For) and isinstance(node.iter, ast.Call) and getattr(node.iter.func, "id", None) == "tqdm"
                and len(node.iter.args) == 1 and getattr(node.iter.args[0], "id", None) == "score_buckets"):
            loop = node
        if isinstance(node, ast.FunctionDef) and node.name == "make_accuracy_over_hit":
            func = node
        if _assigns(node, "recall_per_query"):
            recall = node
    assert None not in (edges, loop, func, recall), "the reference's nodes were not found"
    return edges, loop, func, recall


def run_node(node, namespace):
    module = ast.Module(body=[node], type_ignores=[])
    exec(compile(module, str(REFERENCE), "exec"), namespace)


def reference_run(nodes, correct, scores, totals, limit, smoothness):
    edges, loop, func, recall = nodes
    seen = []

    def noting_sem(a):
        seen.append((len(a), int(a.sum())))
        return sem(a)

    ns = {"numpy": numpy, "ndarray": numpy.ndarray, "tqdm": lambda x, *a, **k: x, "sem": noting_sem, "smoothness": smoothness,
          "correct_totals": totals, "plot_subset_scores": scores[:, :limit], "plot_subset_correct": correct[:, :limit],
          "t5_quantized_precision": [], "t5_quantized_precision_sem": [], "correct": correct}
    run_node(edges, ns)
    run_node(loop, ns)
    run_node(func, ns)
    run_node(recall, ns)  # (correct[:, :300]: every case here has k <= 300, so this is limit = k)
    assert correct.shape[1] <= 300
    return {
        "score_buckets": numpy.asarray(ns["score_buckets"], numpy.float64),
        "precision": numpy.asarray(ns["t5_quantized_precision"], numpy.float64),
        "sem": numpy.asarray(ns["t5_quantized_precision_sem"], numpy.float64),
        "nonempty_count": numpy.asarray([n for n, _ in seen], numpy.int64),
        "nonempty_correct": numpy.asarray([c for _, c in seen], numpy.int64),
        "accuracy_over_hit": numpy.asarray(ns["make_accuracy_over_hit"](correct[:, :limit]), numpy.float64),
        "recall_per_query": numpy.asarray(ns["recall_per_query"], numpy.float64),
    }


def make_totals(rng, correct):
    """at least the row's count; totals of 1 (those rows keep their first correct hit only), large ones here and there"""
    for q in range(0, len(correct), 9):
        first = numpy.flatnonzero(correct[q])[:1]
        correct[q] = False
        correct[q, first] = True
    found = correct.sum(axis=1)
    totals = numpy.maximum(found + rng.integers(0, 40, len(found)), 1).astype(numpy.int64)
    totals[::9] = numpy.maximum(found[::9], 1)
    totals[4::11] = 10 ** 6 + 3
    return totals


def cases():
    rng = numpy.random.default_rng(20241)
    out = {}
    # descending cosine-like float32 scores, the default 300 buckets
    nq, k, limit = 80, 24, 20
    scores = -numpy.sort(-(0.25 + 0.75 * rng.random((nq, k)) ** 2).astype(numpy.float32), axis=1)
    scores[::10, 0] = 1.0  # exact self-hit cosines: the last upper edge may lie below them
    correct = rng.random((nq, k)) < scores
    correct[3] = False
    correct[5] = True
    out["cosine"] = (correct, scores, limit, 300)
    # five tied dyadic values, twelve buckets: 0.25, 0.5 and 0.75 are edges
    nq, k = 200, 9
    scores = rng.choice(numpy.array([0.125, 0.25, 0.5, 0.75, 1.0], numpy.float32), (nq, k))
    out["tied"] = (rng.random((nq, k)) < 0.4, scores.astype(numpy.float32), 6, 12)
    # two clusters with empty buckets in the middle, below and above: the reference `continue`s over them
    nq, k = 60, 10
    scores = numpy.where(rng.random((nq, k)) < 0.5, 0.1 + 0.2 * rng.random((nq, k)), 0.7 + 0.2 * rng.random((nq, k))).astype(numpy.float32)
    out["gaps"] = (rng.random((nq, k)) < 0.3, scores, 10, 50)
    # float64 scores that sit on the 300 default edges and their neighbours: cells in two buckets and in none
    nq, k = 40, 30
    lo = numpy.linspace(0, 1 - (1 / 300), 300)
    pool = numpy.concatenate([lo, lo + (1 / 300), numpy.nextafter(lo, 2), numpy.nextafter(lo + (1 / 300), -1), [1.0]])
    out["edges64"] = (rng.random((nq, k)) < 0.5, rng.choice(pool, (nq, k)), 30, 300)
    # limit = 1: numpy sums the one column pairwise
    nq, k = 1000, 3
    out["one"] = (rng.random((nq, k)) < 0.6, rng.random((nq, k)).astype(numpy.float32), 1, 7)
    return out


def sem_grid():
    """scipy.stats.sem of boolean arrays of n cells, c of them True (shuffled), n from 2 to 3 000 000 and the rate c / n
    from 0 to 1 -> (n, c, sem): what the closed form of evaluation.bucketed_accuracy is measured against"""
    rng = numpy.random.default_rng(7)
    ns, cs, sems = [], [], []
    for n in (2, 3, 4, 5, 7, 10, 33, 100, 1000, 12345, 100000, 1000000, 3000000):
        for c in sorted({0, 1, n // 1000, n // 100, n // 10, n // 3, n // 2, n - n // 3, n - n // 10, n - n // 1000, n - 1, n}):
            a = numpy.zeros(n, bool)
            a[:c] = True
            rng.shuffle(a)
            ns.append(n)
            cs.append(c)
            sems.append(sem(a))
    return numpy.asarray(ns, numpy.int64), numpy.asarray(cs, numpy.int64), numpy.asarray(sems, numpy.float64)


def main():
    nodes = reference_nodes()
    arrays = {"numpy_version": numpy.asarray(numpy.__version__), "scipy_version": numpy.asarray(scipy.__version__),
              "cases": numpy.asarray(sorted(cases()))}
    arrays["sem_grid_n"], arrays["sem_grid_c"], arrays["sem_grid_sem"] = sem_grid()
    for name, (correct, scores, limit, smoothness) in cases().items():
        totals = make_totals(numpy.random.default_rng(len(name)), correct)
        got = reference_run(nodes, correct, scores, totals, limit, smoothness)
        assert len(got["score_buckets"]) == smoothness and len(got["accuracy_over_hit"]) == limit
        arrays.update({f"{name}_correct": correct, f"{name}_scores": scores, f"{name}_totals": totals, f"{name}_limit": numpy.asarray(limit),
                       f"{name}_smoothness": numpy.asarray(smoothness)})
        arrays.update({f"{name}_{key}": value for key, value in got.items()})
    numpy.savez_compressed(OUT, **arrays)
    print(f"wrote {OUT} ({OUT.stat().st_size} bytes)")


if __name__ == "__main__":
    main()
