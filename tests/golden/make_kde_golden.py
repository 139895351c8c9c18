#!/usr/bin/env python3
"""Regenerates tests/golden/reference_density.npz -- run ONLY in the build container (needs /root/reference, pandas,
scipy and matplotlib).

The reference's pfam/reverse_evaluate.py is a notebook-style file that loads its embedding files at import, so it cannot
be imported.  This script parses it with `ast` and picks out every `DataFrame({...}).plot.density(...)` statement: the
two over the first principal component (lines 65-70), the one over the raw embedding dimension with the largest loading
(113-118) and the one inside the loop over the three largest (140-142).  The nodes, compiled as they are, run under
matplotlib's Agg backend in a namespace that holds `DataFrame`, the synthetic matrices they index (the column pairs of
tests/kde_reference.bimodal_columns) and the axes they draw on; the plotted lines are read back from the axes.  Case k
runs statement k, so every statement runs once.  No reference source is copied: the fixture holds the seeds of the
inputs, a digest of them, the line data (x and y per column) that the reference's statements produced under this
container's pandas, scipy and numpy (versions stored in the file), and the recorded curve's largest relative deviation
from the long-double truth of tests/kde_reference.py.

    python tests/golden/make_kde_golden.py
"""
import ast
import json
import sys
from pathlib import Path

import matplotlib

matplotlib.use("Agg")
import matplotlib.pyplot as plt  # noqa: E402
import numpy  # noqa: E402
import pandas  # noqa: E402
import scipy  # noqa: E402

HERE = Path(__file__).resolve().parent
sys.path[:0] = [str(HERE.parent), str(HERE.parent.parent)]
import kde_reference as ref  # noqa: E402

REFERENCE = Path("/root/reference/pfam/reverse_evaluate.py")
OUT = HERE / "reference_density.npz"


def is_density_statement(node):
    """Expr: DataFrame(...).plot.density(...)"""
    if not (isinstance(node, ast.Expr) and isinstance(node.value, ast.Call)):
        return False
    f = node.value.func
    return (isinstance(f, ast.Attribute) and f.attr == "density" and isinstance(f.value, ast.Attribute) and f.value.attr == "plot"
            and isinstance(f.value.value, ast.Call) and getattr(f.value.value.func, "id", None) == "DataFrame")


def reference_nodes():
    nodes = [node for node in ast.walk(ast.parse(REFERENCE.read_text())) if is_density_statement(node)]
    nodes.sort(key=lambda node: node.lineno)
    assert len(nodes) == 4, f"expected the reference's four plot.density statements, found {len(nodes)}"
    return nodes


def run_statement(node, X):
    """-> [(label, x, y)] of the lines the statement drew over the columns ref.COLUMNS of X"""
    original, scrambled = X[:, 0:2], X[:, 2:4]
    fig, (ax1, ax2) = plt.subplots(1, 2)
    ns = {"DataFrame": pandas.DataFrame, "ax1": ax1, "ax2": ax2, "scrambled_name": "reversed", "best_dimension": 0, "dim": 0,
          "original_pca_reverse": original, "scrambled_pca_reverse": scrambled, "original_pca_shuffle": original,
          "scrambled_pca_shuffle": scrambled, "forward_data": original, "reverse_data": scrambled}
    before = set(plt.get_fignums())
    exec(compile(ast.Module(body=[node], type_ignores=[]), str(REFERENCE), "exec"), ns)
    axes = [ax for ax in (ax1, ax2) if ax.get_lines()]
    for num in set(plt.get_fignums()) - before:  # a statement without ax= opens a figure of its own
        axes += [ax for ax in plt.figure(num).axes if ax.get_lines()]
    assert len(axes) == 1, "the statement drew on one axes"
    lines = [(line.get_label(), numpy.asarray(line.get_xdata()), numpy.asarray(line.get_ydata())) for line in axes[0].get_lines()]
    plt.close("all")
    assert len(lines) == 2 and lines[0][0] == "original"
    return lines


def main():
    assert ref.has_long_double()
    nodes = reference_nodes()
    arrays = {"numpy_version": numpy.asarray(numpy.__version__), "scipy_version": numpy.asarray(scipy.__version__),
              "pandas_version": numpy.asarray(pandas.__version__), "columns": numpy.asarray(ref.COLUMNS, numpy.int64),
              "statement_lines": numpy.asarray([node.lineno for node in nodes], numpy.int64)}
    report = {}
    for i, (n, dtype) in enumerate(ref.CASES):
        name, seed = ref.case_name(n, dtype), ref.SEED0 + i
        X = ref.bimodal_columns(n, seed, dtype)
        lines = run_statement(nodes[i], X)
        arrays.update({f"{name}_seed": numpy.asarray(seed), f"{name}_digest": ref.input_digest(X)})
        mn, mx, _, var = ref.stats_reference(X[:, list(ref.COLUMNS)])
        worst = 0.0
        for j, (label, x, y) in enumerate(lines):
            assert x.dtype == numpy.dtype(dtype) and y.dtype == numpy.float64 and len(x) == 1000
            arrays[f"{name}_x{j}"] = x
            arrays[f"{name}_y{j}"] = y
            truth = ref.truth_density(X[:, ref.COLUMNS[j]], x, *ref.scales_reference(var[j], n, ref.factor_reference(n)))
            worst = max(worst, float(numpy.max(numpy.abs(y.astype(numpy.longdouble) - truth) / truth)))
        arrays[f"{name}_scipy_deviation"] = numpy.asarray(worst)
        report[name] = {"statement_line": nodes[i].lineno, "scipy_relative_deviation": worst}
    numpy.savez_compressed(OUT, **arrays)
    print(json.dumps(report, indent=1))
    print(f"wrote {OUT} ({OUT.stat().st_size} bytes)")
    assert OUT.stat().st_size < 1000000


if __name__ == "__main__":
    main()
