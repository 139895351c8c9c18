#!/usr/bin/env python3
"""Regenerates tests/golden/reference_rank.npz -- run ONLY in the build container (needs /root/reference).

The reference's results script pfam/pfam.py is a notebook-style file that loads the whole Pfam dataset at import, so it
cannot be imported.  This script parses it with `ast`, picks out one node -- the loop `for name, limit in [("first_10",
slice(10)), ("300", slice(max_hits))]:` of lines 561-598, the dataset-wide precision-recall curves -- compiles that node
as it is and runs it in a namespace that holds synthetic score and correctness arrays under the reference's names, a
`train_to_family` of the wanted size, `max_hits`, `numpy`, `Counter`, a `plt` whose every call does nothing, a no-op
`endfig`, and `figures` pointing to a temporary directory.  No reference source is copied: the fixture holds the inputs
and the `recall` / `precision` arrays the reference's code saved (precision_recall_<name>.npz), under this container's
numpy (version stored in the file).

The reference sorts with numpy's default, unstable, sort: what it computes among equal scores is not defined.  So every
case here meets one of two conditions, which the maker asserts and the fixture records per case (`<case>_ties`):
  "none"       the case has no two equal scores
  "one_value"  every group of equal scores has one `correct` value -- the e-value padding 100000, always False, included
Under either the sequence of `correct` in sorted order, and with it the curve, is the same for every order inside the
groups.  The maker also computes each curve from a stable sort (tests/rank_reference.py) and refuses a case where the
two differ.

    python tests/golden/make_rank_golden.py
"""
import ast
import tempfile
from collections import Counter
from pathlib import Path

import numpy

REFERENCE = Path("/root/reference/pfam/pfam.py")
OUT = Path(__file__).resolve().parent / "reference_rank.npz"
SETS = (("mmseqs", "mmseqs_e_value_array", "mmseqs_correct_array"), ("k-nn", "knn_scores", "knn_correct"),
        ("k-nn + alignment", "knn_aligned_e_value_array", "knn_aligned_correct_array"))
NAMES = (("first_10", 10), ("300", None))  # the loop's own list; None: max_hits


def reference_node():
    tree = ast.parse(REFERENCE.read_text())
    found = [node for node in ast.walk(tree)
             if isinstance(node, ast.For) and isinstance(node.target, ast.Tuple)
             and [getattr(e, "id", None) for e in node.target.elts] == ["name", "limit"] and isinstance(node.iter, ast.List)]
    assert len(found) == 1 and (found[0].lineno, found[0].end_lineno) == (561, 598), "the reference's loop was not found"
    return found[0]


class Nothing:
    """plt: every attribute is a function that does nothing"""

    def __getattr__(self, name):
        return lambda *args, **kwargs: None


def reference_run(node, arrays, n_train, max_hits):
    """-> {(label, name): (recall, precision)} as the reference's own code saved them"""
    with tempfile.TemporaryDirectory() as tmp:
        ns = {"numpy": numpy, "Counter": Counter, "plt": Nothing(), "endfig": lambda *args, **kwargs: None, "figures": Path(tmp),
              "max_hits": max_hits, "train_to_family": [f"f{i % 7}" for i in range(n_train)], **arrays}
        exec(compile(ast.Module(body=[node], type_ignores=[]), str(REFERENCE), "exec"), ns)
        out = {}
        for name, _ in NAMES:
            saved = numpy.load(Path(tmp) / f"precision_recall_{name}.npz")
            for i, label in enumerate(saved["label"]):
                out[(str(label), name)] = (numpy.asarray(saved["recall"][i], numpy.float64), numpy.asarray(saved["precision"][i], numpy.float64))
        return out


def tie_condition(scores, correct, limit):
    """"none" / "one_value" as the docstring defines them; anything else is refused"""
    s, c = scores[:, :limit].flatten(), correct[:, :limit].flatten()
    values, inverse, counts = numpy.unique(s, return_inverse=True, return_counts=True)
    if (counts == 1).all():
        return "none"
    trues = numpy.bincount(inverse, weights=c)
    assert ((trues == 0) | (trues == counts)).all(), "a group of equal scores holds both values of `correct`"
    return "one_value"


def e_values(rng, rows, k, pad_from):
    """sorted float64 e-values per row, distinct over the whole array; row r is padded with 100000 from column pad_from[r]"""
    e = numpy.sort(numpy.exp(rng.normal(-20, 15, (rows, k))), axis=1)
    assert len(numpy.unique(e)) == e.size
    for r in range(rows):
        e[r, pad_from[r]:] = 100000
    return e


def make_run(rng, rows, k, p_correct):
    pad = rng.integers(3, k + 1, rows)
    pad[::3] = k  # a third of the rows are full
    arrays = {}
    for label, s_name, c_name in SETS:
        correct = rng.random((rows, k)) < p_correct
        if label == "k-nn":  # float32 similarities, no two equal
            scores = ((rng.permutation(rows * k) + 0.25) / (rows * k)).astype(numpy.float32).reshape(rows, k)
            assert len(numpy.unique(scores)) == scores.size
        else:
            scores = e_values(rng, rows, k, pad if label == "mmseqs" else numpy.minimum(pad + 2, k))
            correct &= scores != 100000
        arrays[s_name], arrays[c_name] = scores, correct
    return arrays


def main():
    node = reference_node()
    rng = numpy.random.default_rng(561598)
    out = {"numpy_version": numpy.asarray(numpy.__version__), "runs": numpy.asarray(["never", "reached"]),
           "sets": numpy.asarray([s[0] for s in SETS]), "names": numpy.asarray([n[0] for n in NAMES])}
    import sys
    sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
    import rank_reference as rr
    for run, rows, k, p_correct in (("never", 240, 24, 0.3), ("reached", 300, 16, 0.6)):
        arrays = make_run(rng, rows, k, p_correct)
        if run == "never":  # ten times the rows of the training set: far more than there are correct hits, the clip is taken
            n_train = rows
        else:  # the k-NN set reaches recall 1 exactly at its last correct hit; the total is a multiple of 10
            found = int(arrays["knn_correct"].sum())
            drop = found % 10
            flat = arrays["knn_correct"].reshape(-1)
            flat[numpy.flatnonzero(flat)[:drop]] = False
            n_train = int(arrays["knn_correct"].sum()) // 10
        curves = reference_run(node, {n: a.copy() for n, a in arrays.items()}, n_train, k)
        out[f"{run}_total"] = numpy.asarray(n_train * 10)
        out[f"{run}_max_hits"] = numpy.asarray(k)
        for label, s_name, c_name in SETS:
            out[f"{run}_{label}_scores"], out[f"{run}_{label}_correct"] = arrays[s_name], arrays[c_name]
            for name, limit in NAMES:
                limit = k if limit is None else limit
                recall, precision = curves[(label, name)]
                assert recall.shape == precision.shape == (10000,)
                out[f"{run}_{label}_{name}_ties"] = numpy.asarray(tie_condition(arrays[s_name], arrays[c_name], limit))
                stable = rr.precision_recall_direct(arrays[c_name], arrays[s_name], n_train * 10, limit)
                assert numpy.array_equal(stable[0], recall) and numpy.array_equal(stable[1], precision), "the curve depends on the tie order"
                out[f"{run}_{label}_{name}_limit"] = numpy.asarray(limit)
                out[f"{run}_{label}_{name}_recall"], out[f"{run}_{label}_{name}_precision"] = recall, precision
        reached = [bool((curves[(label, name)][0] >= 1).any()) for label, _, _ in SETS for name, _ in NAMES]
        assert any(reached) == (run == "reached"), reached
    numpy.savez_compressed(OUT, **out)
    print(f"wrote {OUT} ({OUT.stat().st_size} bytes)")


if __name__ == "__main__":
    main()
