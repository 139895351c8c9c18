#!/usr/bin/env python3
"""Regenerates tests/golden/reference_slices_eval.npz -- run ONLY in the build container (needs /root/reference).

The reference's results script pfam/slices/slices.py is a notebook-style file that loads the whole Pfam dataset at import,
so it cannot be imported.  This script parses it with `ast` and picks out, among the module's top-level statements: the
set-building loop over `slices` with the two list assignments in front of it (lines 49-68), the `family_sizes`
statements (70-74), the `has_annotation` statements (76-80) and the definition of `evaluate` (101-142).  It compiles
those nodes as they are and runs them, in source order, in a namespace that holds synthetic `slices` and
`protein_to_domain`, `numpy`, `defaultdict`, the two names of the function's annotations and an identity `tqdm`.  No
reference source is copied: the fixture holds the inputs and what the reference's code produced from them, under this
container's numpy (version stored in the file).

The inputs are chosen so that the reference alone is well-defined: no hit is below 0 (a negative hit indexes the
reference's lists from their end) and every protein has an entry in protein_to_domain (a missing one raises KeyError).

    python tests/golden/make_slices_eval_golden.py            # writes the fixture
    python tests/golden/make_slices_eval_golden.py --time     # the nodes on 200 000 slices, 20 000 rows x 100 hits: seconds
"""
import argparse
import ast
import json
import time
from collections import defaultdict
from pathlib import Path
from typing import Tuple

import numpy
from numpy import ndarray

REFERENCE = Path("/root/reference/pfam/slices/slices.py")
OUT = Path(__file__).resolve().parent / "reference_slices_eval.npz"
ASSIGNED = {"slices_pfams_matching", "slices_pfams_intersecting", "family_sizes", "has_annotation", "slices_pfams_matching_annotated"}
SLICE_LEN, STEP = 128, 64


def reference_nodes():
    """-> (the statements of lines 49-80 in source order, the definition of evaluate)"""
    tree = ast.parse(REFERENCE.read_text())
    tables, evaluate = [], None
    for node in tree.body:
        if isinstance(node, ast.Assign) and len(node.targets) == 1 and getattr(node.targets[0], "id", None) in ASSIGNED:
            tables.append(node)
        elif isinstance(node, ast.For) and getattr(node.iter, "id", None) in ("slices", "slices_pfams_matching"):
            tables.append(node)
        elif isinstance(node, ast.FunctionDef) and node.name == "evaluate":
            evaluate = node
    kinds = [type(n).__name__ for n in tables]
    assert kinds == ["Assign", "Assign", "For", "Assign", "For", "Assign", "Assign", "Assign", "For"], kinds
    assert evaluate is not None, "the reference's evaluate was not found"
    return tables, evaluate


def run_tables(tables, slices, protein_to_domain):
    """the reference's lines 49-80 over the inputs -> the namespace they leave behind"""
    ns = {"numpy": numpy, "defaultdict": defaultdict, "tqdm": lambda x, *a, **k: x, "Tuple": Tuple, "ndarray": ndarray,
          "slices": slices, "protein_to_domain": protein_to_domain}
    exec(compile(ast.Module(body=tables, type_ignores=[]), str(REFERENCE), "exec"), ns)
    return ns


def define_evaluate(evaluate, ns):
    exec(compile(ast.Module(body=[evaluate], type_ignores=[]), str(REFERENCE), "exec"), ns)
    return ns["evaluate"]


def synthetic(rng, n_proteins, n_families):
    """proteins of 1 .. 8 overlapping windows, 0 .. 4 domains each, most of them on a grid of 32 so that domain and slice
    boundaries coincide often; every fifth protein carries a family twice, once inside a window and once across its edge"""
    families = [f"PF{f:05d}" for f in range(n_families)]
    slices, protein_to_domain = [], {}
    for p in range(n_proteins):
        name = f"P{p:06d}"
        n_slices = int(rng.integers(1, 9))
        for i in range(n_slices):
            slices.append((name, (i * STEP, i * STEP + SLICE_LEN)))
        span = (n_slices - 1) * STEP + SLICE_LEN
        domains = []
        for _ in range(int(rng.integers(0, 5))):
            family = families[int(rng.integers(n_families))]
            if rng.random() < 0.6:
                start, length = 32 * int(rng.integers(0, span // 32)), 32 * int(rng.integers(1, 5))
            else:
                start, length = int(rng.integers(0, span)), int(rng.integers(10, 150))
            domains.append((family, (start, start + length)))
        if p % 5 == 0:
            family = families[int(rng.integers(n_families))]
            domains.append((family, (16, 80)))                       # inside the first window
            domains.append((family, (SLICE_LEN - 24, SLICE_LEN + 40)))  # across its right edge
        protein_to_domain[name] = domains
    return slices, protein_to_domain


def pools(ns):
    """per family: the slices it matches in, the slices it only intersects; and the slices without any matching family"""
    correct, ignored = defaultdict(list), defaultdict(list)
    for s, (m, i) in enumerate(zip(ns["slices_pfams_matching"], ns["slices_pfams_intersecting"])):
        for f in m:
            correct[f].append(s)
        for f in i - m:
            ignored[f].append(s)
    empty = [s for s, m in enumerate(ns["slices_pfams_matching"]) if not m]
    return correct, ignored, empty


def crafted_hits(rng, ns, k):
    """one row per annotated slice, in six patterns: a foreign hit first; a run that ends in the middle; a run that never
    ends; a run that only unannotated hits interrupt; random hits; correct, intersecting and unannotated hits only"""
    n = len(ns["slices_pfams_matching"])
    correct, ignored, empty = pools(ns)
    hits = rng.integers(0, n, (len(ns["slices_pfams_matching_annotated"]), k)).astype(numpy.int64)
    for r, family in enumerate(ns["slices_pfams_matching_annotated"]):
        good = correct[family] + ignored[family]
        foreign = [s for s in rng.integers(0, n, 8) if family not in ns["slices_pfams_matching"][s]
                   and family not in ns["slices_pfams_intersecting"][s] and ns["slices_pfams_matching"][s]]
        pattern = r % 6
        if pattern == 0 and foreign:
            hits[r, 0] = foreign[0]
        elif pattern == 1 and foreign:
            cut = int(rng.integers(1, k - 1))
            hits[r, :cut] = rng.choice(good, cut)
            hits[r, cut] = foreign[0]
        elif pattern == 2:
            hits[r] = rng.choice(good, k)
        elif pattern == 3 and foreign:
            cut = int(rng.integers(4, k - 1))
            hits[r, :cut] = rng.choice(correct[family], cut)
            hits[r, 1:cut:3] = rng.choice(empty, len(range(1, cut, 3)))
            hits[r, cut] = foreign[0]
        elif pattern == 5:
            hits[r] = rng.choice(good + empty, k)
    return hits


def run_end(correct, ignore):
    for j, (c, i) in enumerate(zip(correct, ignore)):
        if not c and not i:
            return j
    return len(correct)


def check_coverage(slices, protein_to_domain, ns, k, plain, flagged):
    counts = {len(m) for m in ns["slices_pfams_matching"]}
    assert {0, 1, 2} <= counts, counts
    assert any(m & i for m, i in zip(ns["slices_pfams_matching"], ns["slices_pfams_intersecting"])), "no family both matching and intersecting"
    equal = set()
    for protein, (s0, s1) in slices:
        for _, (d0, d1) in protein_to_domain[protein]:
            equal |= {name for name, hit in (("s0==d0", s0 == d0), ("d1==s1", d1 == s1), ("s0==d1", s0 == d1), ("d0==s1", d0 == s1)) if hit}
    assert len(equal) == 4, equal
    ends = {min(run_end(c, i), 1) if run_end(c, i) < k else 2 for c, i in zip(plain[0], plain[1])}
    assert ends == {0, 1, 2}, "runs must end at hit 0, in the middle and nowhere"
    assert any(run_end(c, i) == k for c, i in zip(flagged[0], flagged[1]))
    assert (flagged[2] > plain[2]).sum() >= 5, "rows where only ignore_unannotated lengthens the run"
    assert (flagged[2] >= plain[2]).all() and numpy.array_equal(plain[0], flagged[0])


def pairs(sets):
    out = sorted((s, f) for s, members in enumerate(sets) for f in members)
    return numpy.asarray([s for s, _ in out], numpy.int64), numpy.asarray([f for _, f in out], dtype=str)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--time", action="store_true", help="time the reference's nodes on 200 000 slices and 20 000 rows of 100 hits")
    args = ap.parse_args()
    tables, evaluate_node = reference_nodes()
    if args.time:
        rng = numpy.random.default_rng(1)
        slices, protein_to_domain = synthetic(rng, 48000, 3000)
        slices = slices[:200000]
        assert len(slices) == 200000
        t0 = time.perf_counter()
        ns = run_tables(tables, slices, protein_to_domain)
        t1 = time.perf_counter()
        rows, k = 20000, 100
        assert int(ns["has_annotation"].sum()) >= rows
        ns["slices_pfams_matching_annotated"] = ns["slices_pfams_matching_annotated"][:rows]  # (its zip stops at the shortest)
        hits = crafted_hits(rng, ns, k)
        evaluate = define_evaluate(evaluate_node, ns)
        t2 = time.perf_counter()
        evaluate(hits, False)
        t3 = time.perf_counter()
        print(json.dumps({"reference_tables_seconds": t1 - t0, "reference_evaluate_seconds": t3 - t2, "slices": len(slices),
                          "rows": rows, "k": k, "numpy": numpy.__version__}))
        return
    rng = numpy.random.default_rng(20251)
    k = 40
    slices, protein_to_domain = synthetic(rng, 60, 9)
    ns = run_tables(tables, slices, protein_to_domain)
    hits = crafted_hits(rng, ns, k)
    assert hits.min() >= 0 and hits.max() < len(slices)
    evaluate = define_evaluate(evaluate_node, ns)
    plain = evaluate(hits, False)
    flagged = evaluate(hits, True)
    check_coverage(slices, protein_to_domain, ns, k, plain, flagged)
    domain_rows = [(p, f, d0, d1) for p, domains in protein_to_domain.items() for f, (d0, d1) in domains]
    matching_slice, matching_family = pairs(ns["slices_pfams_matching"])
    intersecting_slice, intersecting_family = pairs(ns["slices_pfams_intersecting"])
    sizes = sorted(ns["family_sizes"].items())
    arrays = {
        "numpy_version": numpy.asarray(numpy.__version__),
        "protein_names": numpy.asarray(list(protein_to_domain), dtype=str),
        "slice_protein": numpy.asarray([p for p, _ in slices], dtype=str),
        "slice_start": numpy.asarray([s for _, (s, _) in slices], numpy.int64),
        "slice_stop": numpy.asarray([s for _, (_, s) in slices], numpy.int64),
        "domain_protein": numpy.asarray([r[0] for r in domain_rows], dtype=str),
        "domain_pfam": numpy.asarray([r[1] for r in domain_rows], dtype=str),
        "domain_start": numpy.asarray([r[2] for r in domain_rows], numpy.int64),
        "domain_stop": numpy.asarray([r[3] for r in domain_rows], numpy.int64),
        "hits": hits,
        "matching_slice": matching_slice, "matching_family": matching_family,
        "intersecting_slice": intersecting_slice, "intersecting_family": intersecting_family,
        "family_size_names": numpy.asarray([f for f, _ in sizes], dtype=str),
        "family_size_counts": numpy.asarray([c for _, c in sizes], numpy.int64),
        "has_annotation": ns["has_annotation"],
        "annotated": numpy.asarray(ns["slices_pfams_matching_annotated"], dtype=str),
    }
    for tag, (is_correct, is_ignore, auc1s) in (("plain", plain), ("ignore_unannotated", flagged)):
        assert is_correct.dtype == numpy.bool_ and is_ignore.dtype == numpy.bool_ and auc1s.dtype == numpy.float64
        arrays.update({f"is_correct_{tag}": is_correct, f"is_ignore_{tag}": is_ignore, f"auc1s_{tag}": auc1s})
    numpy.savez_compressed(OUT, **arrays)
    print(f"wrote {OUT} ({OUT.stat().st_size} bytes); {len(slices)} slices, {int(ns['has_annotation'].sum())} annotated rows")


if __name__ == "__main__":
    main()
