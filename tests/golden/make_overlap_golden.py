#!/usr/bin/env python3
"""Regenerates tests/golden/reference_overlap.npz -- run ONLY in the build container (needs /root/reference).

The reference's results script pfam/pfam.py is a notebook-style file that loads the whole Pfam dataset at import, so it
cannot be imported.  This script parses it with `ast` and picks out three `for` nodes: the loop that appends to `knn_tp`
and `mmseqs_tp` (lines 352-355), the loop over `zip(mmseqs_tp, knn_tp)` that adds up the three counts (lines 360-363), and
the `tqdm(range(len(knn_hits)))` loop whose body starts by assigning `knn_hits_set` (auc1s_optimal, lines 605-622).  It
compiles those nodes as they are and runs them in a namespace that holds synthetic arrays, the few assignments in front of
the loops restated (the empty lists, the three zero counts, `family_sizes = dict(Counter(train_to_family))`), and an
identity `tqdm`.  No reference source is copied: the fixture holds the inputs and what the reference's code produced from
them.  The reference works on sets, so it is deterministic on any input.

The reference's lists are ragged (one array per query); the library's are rectangular, an id of -1 standing for "no entry".
The rectangular arrays are the fixture's inputs, and the reference is given each row's entries with id >= 0, in column
order.  List A is MMseqs2's (`mmseqs_hits` with its own flags `mmseqs_correct`), list B the k-NN search's (`knn_hits` in
the first node, `knn_aligned_hits` in the third; flags from `train_to_family`).  The third node takes both lists' flags
from `train_to_family`, so the first and second node run twice: with `mmseqs_correct` equal to those flags (tp), and with
flags of its own that disagree with them (tp_alt).  The second node runs once over all rows for the totals and once per
row for the per-query triples; the third once over all rows for auc1s_optimal and once per row, to read the two sets it
leaves behind.

    python tests/golden/make_overlap_golden.py            # writes the fixture
    python tests/golden/make_overlap_golden.py --time     # the three loop nodes on 2000 x 300 against 300: prints seconds
"""
import argparse
import ast
import json
import time
from collections import Counter
from pathlib import Path

import numpy

REFERENCE = Path("/root/reference/pfam/pfam.py")
OUT = Path(__file__).resolve().parent / "reference_overlap.npz"


def _calls_append_on(node, name):
    return any(isinstance(c, ast.Call) and isinstance(c.func, ast.Attribute) and c.func.attr == "append"
               and getattr(c.func.value, "id", None) == name for c in ast.walk(node))


def _is_call(node, name, nargs):
    return isinstance(node, ast.Call) and getattr(node.func, "id", None) == name and len(node.args) == nargs


def reference_nodes():
    tree = ast.parse(REFERENCE.read_text())
    fill = count = optimal = None
    for node in ast.walk(tree):
        if not isinstance(node, ast.For):
            continue
        if _calls_append_on(node, "knn_tp") and _calls_append_on(node, "mmseqs_tp"):
            fill = node
        it = node.iter
        if _is_call(it, "zip", 2) and [getattr(a, "id", None) for a in it.args] == ["mmseqs_tp", "knn_tp"]:
            count = node
        if (_is_call(it, "tqdm", 1) and _is_call(it.args[0], "range", 1) and _is_call(it.args[0].args[0], "len", 1)
                and getattr(it.args[0].args[0].args[0], "id", None) == "knn_hits"
                and isinstance(node.body[0], ast.Assign) and getattr(node.body[0].targets[0], "id", None) == "knn_hits_set"):
            optimal = node
    assert fill is not None and count is not None and optimal is not None, "the reference's nodes were not found"
    return fill, count, optimal


def run_node(node, namespace):
    module = ast.Module(body=[node], type_ignores=[])
    exec(compile(module, str(REFERENCE), "exec"), namespace)


def ragged(hits, flags=None):
    """the existing entries of every row, in column order: what the reference's lists hold"""
    keep = hits >= 0
    return [(hits if flags is None else flags)[q][keep[q]] for q in range(len(hits))]


def run_fill(node, mmseqs_hits, mmseqs_correct, knn_hits, train_to_family, test_to_family):
    """-> (mmseqs_tp, knn_tp), the reference's two lists of sets (pfam.py:349-355)"""
    ns = {"mmseqs_tp": [], "knn_tp": [], "knn_hits": knn_hits, "mmseqs_hits": mmseqs_hits, "mmseqs_correct": mmseqs_correct,
          "train_to_family": train_to_family, "test_to_family": test_to_family}
    run_node(node, ns)
    return ns["mmseqs_tp"], ns["knn_tp"]


def run_count(node, mmseqs_tp, knn_tp):
    """-> (only MMseqs2, both, only knn) as the reference adds them up (pfam.py:357-363)"""
    ns = {"tp_count_mmseqs": 0, "tp_count_both": 0, "tp_count_knn": 0, "mmseqs_tp": mmseqs_tp, "knn_tp": knn_tp}
    run_node(node, ns)
    return [ns["tp_count_mmseqs"], ns["tp_count_both"], ns["tp_count_knn"]]


def run_optimal(node, mmseqs_hits, knn_aligned_hits, train_to_family, test_to_family):
    """-> (auc1s_optimal as a list, the namespace): pfam.py:602-622"""
    ns = {"tqdm": lambda x, *a, **k: x, "auc1s_optimal": [], "knn_hits": knn_aligned_hits, "knn_aligned_hits": knn_aligned_hits,
          "mmseqs_hits": mmseqs_hits, "train_to_family": train_to_family, "test_to_family": test_to_family,
          "family_sizes": dict(Counter(train_to_family))}  # (pfam.py:604)
    run_node(node, ns)
    return ns["auc1s_optimal"], ns


def tp_outputs(fill, count, hits_a, correct_a, hits_b, train_to_family, test_to_family):
    """-> (per-query triples [nq, 3], totals [3]) from the first two nodes"""
    mmseqs_tp, knn_tp = run_fill(fill, ragged(hits_a), ragged(hits_a, correct_a != 0), ragged(hits_b), train_to_family, test_to_family)
    totals = run_count(count, mmseqs_tp, knn_tp)
    rows = [run_count(count, [m], [k]) for m, k in zip(mmseqs_tp, knn_tp)]
    return numpy.asarray(rows, numpy.int32), numpy.asarray(totals, numpy.int64)


def lead_outputs(optimal, hits_a, hits_b, train_to_family, test_to_family):
    """-> (per-query triples [nq, 3] from the two sets the node leaves behind, auc1s_optimal float64 [nq])"""
    a, b = ragged(hits_a), ragged(hits_b)
    auc1s, _ = run_optimal(optimal, a, b, train_to_family, test_to_family)
    rows = []
    for q in range(len(a)):
        _, ns = run_optimal(optimal, a[q:q + 1], b[q:q + 1], train_to_family, test_to_family[q:q + 1])
        mm, knn = ns["mmseqs_hits_set"], ns["knn_hits_set"]
        rows.append([len(mm - knn), len(mm & knn), len(knn - mm)])
        assert len(mm | knn) / ns["family_sizes"][test_to_family[q]] == auc1s[q]
    return numpy.asarray(rows, numpy.int32), numpy.asarray(auc1s)  # (pfam.py:624)


def family_flags(hits, train_to_family, test_to_family, rng):
    """train_to_family[hit] == the query's family; under an id of -1 any byte (it is never looked at)"""
    flags = (train_to_family[numpy.maximum(hits, 0)] == test_to_family[:, None]).astype(numpy.uint8)
    none = hits < 0
    flags[none] = rng.integers(0, 2, int(none.sum()))
    return flags


def case(rng, nq=40, ka=30, kb=40, nb=600, nfam=12):
    train_to_family = rng.permutation(numpy.arange(nb) % nfam).astype(numpy.int64)  # nb / nfam = 50 members each
    test_to_family = rng.integers(0, nfam, nq).astype(numpy.int64)
    hits_a = numpy.full((nq, ka), -1, numpy.int64)
    hits_b = numpy.full((nq, kb), -1, numpy.int64)
    for q in range(nq):
        own = numpy.flatnonzero(train_to_family == test_to_family[q])
        other = numpy.flatnonzero(train_to_family != test_to_family[q])
        pool_own, pool_other = rng.choice(own, 45, replace=False), rng.choice(other, 45, replace=False)  # both lists draw from these: shared ids
        kind = q % 8
        for hits, width, which in ((hits_a, ka, 0), (hits_b, kb, 1)):
            real = width if kind in (2, 5) or q < 2 else int(rng.integers(1, width + 1))
            if kind == 1:    # no true positive
                row = rng.choice(pool_other, real, replace=False)
            elif kind == 2:  # the leading run is the whole list
                row = rng.choice(pool_own, real, replace=False)
            elif kind == 3:  # the leading run is empty
                row = numpy.concatenate([rng.choice(pool_other, 1), rng.choice(numpy.concatenate([pool_own, pool_other]), real - 1, replace=False)])
            elif kind == 4:  # A whole, B empty
                row = rng.choice(pool_own, real, replace=False) if which == 0 else numpy.concatenate(
                    [rng.choice(pool_other, 1), rng.choice(pool_own, real - 1, replace=False)])
            elif kind == 5:  # repeats inside the list, in the run and behind it
                row = numpy.concatenate([rng.choice(pool_own[:6], real // 3), rng.choice(numpy.concatenate([pool_own[:10], pool_other[:10]]), real - real // 3)])
            else:            # a run of random length, then a mix
                run = int(rng.integers(0, real + 1))
                row = numpy.concatenate([rng.choice(pool_own, run, replace=False),
                                         rng.choice(numpy.concatenate([pool_own, pool_other]), real - run, replace=False)])
            hits[q, :real] = row
        if kind == 6:  # entries that do not exist inside the run and in front of it
            hits_a[q, 0] = -1
            hits_b[q, [1, 3]] = -1
    hits_a[7] = -1  # no entry at all in A, in B
    hits_b[15] = -1
    correct_a = family_flags(hits_a, train_to_family, test_to_family, rng)
    correct_b = family_flags(hits_b, train_to_family, test_to_family, rng)
    correct_a_alt = numpy.where(rng.random(correct_a.shape) < 0.3, 1 - correct_a, correct_a).astype(numpy.uint8)
    return hits_a, correct_a, correct_a_alt, hits_b, correct_b, train_to_family, test_to_family


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--time", action="store_true", help="time the reference's three loops on 2000 rows of 300 against 300 entries")
    args = ap.parse_args()
    fill, count, optimal = reference_nodes()
    if args.time:
        rng = numpy.random.default_rng(1)
        nq, w, nb = 2000, 300, 200000
        train_to_family = rng.integers(0, 2, nb).astype(numpy.int64)
        test_to_family = rng.integers(0, 2, nq).astype(numpy.int64)
        hits_a = rng.integers(0, nb, (nq, w)).astype(numpy.int64)
        hits_b = rng.integers(0, nb, (nq, w)).astype(numpy.int64)
        hits_b[:, ::3] = hits_a[:, ::3]  # a third of the ids are shared
        correct_a = train_to_family[hits_a] == test_to_family[:, None]
        a, ca, b = ragged(hits_a), ragged(hits_a, correct_a), ragged(hits_b)
        t0 = time.perf_counter()
        mmseqs_tp, knn_tp = run_fill(fill, a, ca, b, train_to_family, test_to_family)
        run_count(count, mmseqs_tp, knn_tp)
        t1 = time.perf_counter()
        run_optimal(optimal, a, b, train_to_family, test_to_family)  # (with the Counter of pfam.py:604)
        t2 = time.perf_counter()
        print(json.dumps({"reference_tp_overlap_seconds": t1 - t0, "reference_auc1s_optimal_seconds": t2 - t1, "nq": nq, "ka": w, "kb": w,
                          "numpy": numpy.__version__}))
        return
    rng = numpy.random.default_rng(20251)
    hits_a, correct_a, correct_a_alt, hits_b, correct_b, train_to_family, test_to_family = case(rng)
    tp, tp_totals = tp_outputs(fill, count, hits_a, correct_a, hits_b, train_to_family, test_to_family)
    tp_alt, tp_alt_totals = tp_outputs(fill, count, hits_a, correct_a_alt, hits_b, train_to_family, test_to_family)
    lead, auc1s_optimal = lead_outputs(optimal, hits_a, hits_b, train_to_family, test_to_family)
    assert auc1s_optimal.dtype == numpy.float64 and tp.shape == lead.shape == (len(hits_a), 3)
    assert (tp.sum(axis=1) == 0).any() and (lead.sum(axis=1) == 0).any() and (tp[:, 1] > 0).any() and (lead[:, 1] > 0).any()
    assert not numpy.array_equal(tp, tp_alt)
    family_sizes = numpy.asarray([Counter(train_to_family.tolist())[f] for f in test_to_family.tolist()], numpy.int64)
    numpy.savez_compressed(OUT, numpy_version=numpy.asarray(numpy.__version__), hits_a=hits_a, correct_a=correct_a, correct_a_alt=correct_a_alt,
                           hits_b=hits_b, correct_b=correct_b, train_to_family=train_to_family, test_to_family=test_to_family,
                           family_sizes=family_sizes, tp=tp, tp_totals=tp_totals, tp_alt=tp_alt, tp_alt_totals=tp_alt_totals, lead=lead,
                           auc1s_optimal=auc1s_optimal)
    print(f"wrote {OUT} ({OUT.stat().st_size} bytes)")


if __name__ == "__main__":
    main()
