#!/usr/bin/env python3
"""Regenerates tests/golden/reference_bootstrap.npz -- run ONLY in the build container (needs /root/reference).

The reference's results script cath/cath.py is a notebook-style file that loads the CATH20 search results at import, so
it cannot be imported.  This script parses it with `ast` and picks out two nodes: the function `bootstrap_scores` (lines
404-438) and the `for _ in tqdm(range(500)):` loop inside it (lines 408-419).  The function node, compiled as it is and
run in a namespace that holds synthetic `mapping_array` and `is_possible`, `Counter`, `Tuple`, `ndarray`, `numpy` and an
identity `tqdm`, gives the final tuple.  The loop node, run in the same namespace with the two lists and a generator that
records what `choice` returns, gives the 500 resamples and the two 500-entry lists.  No reference source is copied: the
fixture holds the inputs and what the reference's code produced from them, under this container's numpy (version stored
in the file).  Every method of a case draws the same resamples (default_rng(42), the same row count), so they are stored
once per row count, as uint16.

    python tests/golden/make_bootstrap_golden.py            # writes the fixture
    python tests/golden/make_bootstrap_golden.py --time     # the function on 10 874 rows, about 2 500 families: seconds
"""
import argparse
import ast
import json
import time
from collections import Counter
from pathlib import Path
from typing import Tuple

import numpy

REFERENCE = Path("/root/reference/cath/cath.py")
OUT = Path(__file__).resolve().parent / "reference_bootstrap.npz"


def reference_nodes():
    tree = ast.parse(REFERENCE.read_text())
    func = loop = None
    for node in ast.walk(tree):
        if isinstance(node, ast.FunctionDef) and node.name == "bootstrap_scores":
            func = node
    assert func is not None, "the reference's bootstrap_scores was not found"
    for node in func.body:
        if isinstance(node, ast.For):
            assert loop is None
            loop = node
    assert loop is not None, "the loop inside bootstrap_scores was not found"
    return func, loop


def run_node(node, namespace):
    module = ast.Module(body=[node], type_ignores=[])
    exec(compile(module, str(REFERENCE), "exec"), namespace)


class RecordingGenerator:
    """numpy's generator, keeping what choice() returned"""

    def __init__(self, seed):
        self.rng = numpy.random.default_rng(seed)
        self.drawn = []

    def choice(self, *args, **kwargs):
        out = self.rng.choice(*args, **kwargs)
        self.drawn.append(out)
        return out


def namespace(mapping_array, is_possible):
    return {"numpy": numpy, "ndarray": numpy.ndarray, "Tuple": Tuple, "Counter": Counter, "tqdm": lambda x, *a, **k: x,
            "mapping_array": mapping_array, "is_possible": is_possible}


def reference_run(func, loop, mapping_array, is_possible, is_correct, normalized):
    """-> (the final tuple, the resamples [500, n], bootstrapped_normalized [500], bootstrapped_raw [500])"""
    ns = namespace(mapping_array, is_possible)
    run_node(func, ns)
    plus_minus = ns["bootstrap_scores"](is_correct, normalized)
    ns = namespace(mapping_array, is_possible)
    rng = RecordingGenerator(42)  # cath.py:405, restated: the loop node starts one line below it
    ns.update({"rng": rng, "is_correct": is_correct, "bootstrapped_normalized": [], "bootstrapped_raw": []})
    run_node(loop, ns)
    boot_normalized = numpy.asarray(ns["bootstrapped_normalized"], numpy.float64)
    boot_raw = numpy.asarray(ns["bootstrapped_raw"], numpy.float64)
    return (numpy.asarray(plus_minus, numpy.float64), numpy.asarray(rng.drawn), boot_normalized, boot_raw)


def normalized_of(mapping_array, column):
    """cath.py:94-109 and :446 for one method (restated: a few lines of numpy around a Counter)"""
    sizes = Counter(mapping_array[:, 0].tolist())
    member = numpy.asarray([sizes[f] for f in mapping_array[:, 0].tolist()])
    normalization = numpy.asarray([1 / s for s in member.tolist()])
    normalization[member <= 1] = 0
    return (column * normalization).sum() / sum(size > 1 for size in sizes.values()), member > 1


def cases():
    """name -> (mapping_array [n_all, levels], is_possible bool [n_all], is_correct bool [nm, n_all])"""
    rng = numpy.random.default_rng(20241)
    out = {}
    for n, nfam in ((37, 5), (150, 40), (400, 300), (400, 1)):
        labels = rng.integers(0, nfam, n) * 7 + 1000  # (labels are not dense codes)
        labels[:nfam] = rng.permutation(nfam) * 7 + 1000  # every family occurs
        mapping_array = numpy.stack([labels, rng.integers(0, 3, n)], axis=1)
        is_correct = rng.random((1, n)) < 0.6
        out[f"n{n}_f{nfam}"] = (mapping_array, numpy.ones(n, bool), is_correct)
    # a larger table of which is_possible keeps the rows of the families with two members at least; three methods
    n_all = 130
    labels = numpy.concatenate([rng.integers(0, 25, 100), numpy.arange(100, 130)])  # 30 singletons
    order = rng.permutation(n_all)
    mapping_array = numpy.stack([labels[order], rng.integers(0, 4, n_all), rng.integers(0, 9, n_all)], axis=1)
    sizes = Counter(mapping_array[:, 0].tolist())
    is_possible = numpy.asarray([sizes[f] > 1 for f in mapping_array[:, 0].tolist()])
    is_correct = numpy.stack([rng.random(n_all) < p for p in (0.3, 0.6, 0.9)])
    out["possible"] = (mapping_array, is_possible, is_correct)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--time", action="store_true", help="time the reference's function on 10 874 rows, about 2 500 families")
    args = ap.parse_args()
    func, loop = reference_nodes()
    if args.time:
        rng = numpy.random.default_rng(1)
        n, nfam = 10874, 2500
        mapping_array = rng.integers(0, nfam, (n, 1))
        ns = namespace(mapping_array, numpy.ones(n, bool))
        run_node(func, ns)
        is_correct = rng.random(n) < 0.7
        t0 = time.perf_counter()
        ns["bootstrap_scores"](is_correct, 0.7)
        seconds = time.perf_counter() - t0
        print(json.dumps({"reference_bootstrap_scores_seconds": seconds, "n": n, "families": int(len(numpy.unique(mapping_array))),
                          "replicates": 500, "numpy": numpy.__version__}))
        return
    arrays = {"numpy_version": numpy.asarray(numpy.__version__), "cases": numpy.asarray(sorted(cases()))}
    for name, (mapping_array, is_possible, is_correct) in cases().items():
        n = int(is_possible.sum())
        tuples, boot_normalized, boot_raw, normalized = [], [], [], []
        for column in is_correct:
            x, possible = normalized_of(mapping_array, column)
            assert numpy.array_equal(possible, is_possible) or is_possible.all()
            plus_minus, samples, bn, br = reference_run(func, loop, mapping_array, is_possible, column[is_possible], x)
            assert samples.shape == (500, n) and bn.shape == br.shape == (500,) and samples.max() < 65536
            key = f"samples_{n}"
            assert key not in arrays or numpy.array_equal(arrays[key], samples), "the resamples depend on the row count only"
            arrays[key] = samples.astype(numpy.uint16)
            # the function and the loop node are the same statements: the tuple follows from the lists
            bn_sorted, br_sorted, mean = numpy.sort(bn), numpy.sort(br), column[is_possible].mean()
            assert plus_minus[0] == max(x - bn_sorted[12], bn_sorted[487] - x) and plus_minus[1] == max(mean - br_sorted[12], br_sorted[487] - mean)
            tuples.append(plus_minus)
            boot_normalized.append(bn)
            boot_raw.append(br)
            normalized.append(x)
        arrays.update({
            f"{name}_mapping_array": mapping_array.astype(numpy.int32), f"{name}_is_possible": is_possible, f"{name}_is_correct": is_correct,
            f"{name}_normalized": numpy.asarray(normalized, numpy.float64), f"{name}_plus_minus": numpy.asarray(tuples),
            f"{name}_boot_normalized": numpy.asarray(boot_normalized), f"{name}_boot_raw": numpy.asarray(boot_raw),
        })
    numpy.savez_compressed(OUT, **arrays)
    print(f"wrote {OUT} ({OUT.stat().st_size} bytes)")
    assert OUT.stat().st_size < 1000000


if __name__ == "__main__":
    main()
