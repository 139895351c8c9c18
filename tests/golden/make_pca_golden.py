#!/usr/bin/env python3
"""Regenerates tests/golden/reference_pca.npz -- run ONLY in the build container (needs /root/reference and sklearn).

The reference's pfam/reverse_evaluate.py is a notebook-style file that loads its embedding files at import, so it cannot
be imported.  This script parses it with `ast` and picks out three statements: the first
`... = PCA(n_components=2).fit_transform(numpy.concatenate((forward_data, reverse_data), axis=0))` (lines 34-36) and the
pair `pca = PCA(n_components=2)`, `pca.fit(numpy.concatenate((forward_data, (reverse_data)), axis=0))` (lines 100-101).
The nodes, compiled as they are, run in a namespace that holds `numpy`, synthetic `forward_data` / `reverse_data` (the
two halves of tests/pca_reference.planted_input) and a `PCA` that is sklearn's class, keeping every instance it makes.
That gives two separate fits per case: for more than 1000 columns sklearn's `auto` solver is the randomized one, and two
fits differ.  No reference source is copied: the fixture holds the seeds of the inputs, a digest of them, and what the
reference's statements produced under this container's sklearn and numpy (versions stored in the file).

Beside sklearn's outputs the fixture holds the float64 truth (float64 centring, eigh, the same sign rule:
pca_reference.truth_pca), the solver sklearn picked, the truth of the one case that is also run with 1000 added to every
entry, and the measured deviations from the truth of sklearn's two fits and of the restatement tests/pca_reference.py.

    python tests/golden/make_pca_golden.py            # writes the fixture
    python tests/golden/make_pca_golden.py --time     # the fit_transform statement at [200 000, 1024]: seconds
"""
import argparse
import ast
import json
import sys
import time
from pathlib import Path

import numpy
import sklearn
import sklearn.decomposition

HERE = Path(__file__).resolve().parent
sys.path[:0] = [str(HERE.parent), str(HERE.parent.parent)]
import pca_reference as ref  # noqa: E402

REFERENCE = Path("/root/reference/pfam/reverse_evaluate.py")
OUT = HERE / "reference_pca.npz"
SEED0 = 7100


def is_pca_call(node):
    return isinstance(node, ast.Call) and isinstance(node.func, ast.Name) and node.func.id == "PCA"


def reference_nodes():
    """-> (the first fit_transform assignment, the `pca = PCA(...)` assignment, the `pca.fit(...)` statement)"""
    tree = ast.parse(REFERENCE.read_text())
    fit_transform = make = fit = None
    for node in tree.body:
        if isinstance(node, ast.Assign) and isinstance(node.value, ast.Call) and isinstance(node.value.func, ast.Attribute):
            f = node.value.func
            if f.attr == "fit_transform" and is_pca_call(f.value) and fit_transform is None:
                fit_transform = node
        if isinstance(node, ast.Assign) and is_pca_call(node.value) and len(node.targets) == 1 and getattr(node.targets[0], "id", None) == "pca":
            assert make is None
            make = node
        if isinstance(node, ast.Expr) and isinstance(node.value, ast.Call) and isinstance(node.value.func, ast.Attribute):
            f = node.value.func
            if f.attr == "fit" and getattr(f.value, "id", None) == "pca":
                assert fit is None
                fit = node
    assert fit_transform is not None and make is not None and fit is not None, "the reference's PCA statements were not found"
    assert ast.unparse(fit_transform.value.func.value) == ast.unparse(make.value) == "PCA(n_components=2)"
    return fit_transform, make, fit


def run_nodes(nodes, namespace):
    exec(compile(ast.Module(body=list(nodes), type_ignores=[]), str(REFERENCE), "exec"), namespace)


def reference_fits(nodes, X):
    """-> two dicts (the fit_transform statement's fit, the pca.fit statement's fit) of pca_reference.QUANTITIES, and the
    solver sklearn picked"""
    made = []

    def PCA(*args, **kwargs):
        made.append(sklearn.decomposition.PCA(*args, **kwargs))
        return made[-1]

    half = X.shape[0] // 2
    ns = {"numpy": numpy, "PCA": PCA, "forward_data": X[:half], "reverse_data": X[half:]}
    run_nodes(nodes, ns)
    assert len(made) == 2 and made[1] is ns["pca"]
    target = nodes[0].targets[0].id
    outs = []
    for pca, y in ((made[0], ns[target]), (made[1], made[1].transform(X))):
        assert y.dtype == numpy.float32
        outs.append({"transform": y, "components_": pca.components_, "explained_variance_": pca.explained_variance_,
                     "explained_variance_ratio_": pca.explained_variance_ratio_, "singular_values_": pca.singular_values_})
    assert made[0]._fit_svd_solver == made[1]._fit_svd_solver
    return outs[0], outs[1], made[0]._fit_svd_solver


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--time", action="store_true", help="time the reference's fit_transform statement at [200 000, 1024]")
    args = ap.parse_args()
    nodes = reference_nodes()
    if args.time:
        X = ref.planted_input(200000, 1024, SEED0)
        ns = {"numpy": numpy, "PCA": sklearn.decomposition.PCA, "forward_data": X[:100000], "reverse_data": X[100000:]}
        t0 = time.perf_counter()
        run_nodes(nodes[:1], ns)
        print(json.dumps({"reference_pca_fit_transform_seconds": time.perf_counter() - t0, "shape": [200000, 1024],
                          "sklearn": sklearn.__version__, "numpy": numpy.__version__}))
        return
    arrays = {"numpy_version": numpy.asarray(numpy.__version__), "sklearn_version": numpy.asarray(sklearn.__version__),
              "cases": numpy.asarray(ref.CASES, numpy.int64), "offset_case": numpy.asarray(ref.OFFSET_CASE, numpy.int64)}
    report = {}
    for i, (n, d) in enumerate(ref.CASES):
        name, seed = ref.case_name(n, d), SEED0 + i
        X = ref.planted_input(n, d, seed)
        truth = ref.truth_pca(X, 2)
        w = numpy.linalg.eigvalsh(numpy.cov(X.astype(numpy.float64), rowvar=False))[::-1]
        assert w[1] / w[2] >= 4, (name, w[:3])
        fit1, fit2, solver = reference_fits(nodes, X)
        restated = ref.fit_reference(X, 2)
        arrays.update({f"{name}_seed": numpy.asarray(seed), f"{name}_digest": ref.input_digest(X), f"{name}_solver": numpy.asarray(solver),
                       f"{name}_gap": numpy.asarray(w[1] / w[2])})
        for q in ref.QUANTITIES:
            arrays[f"{name}_truth_{q}"] = truth[q]
            arrays[f"{name}_fit1_{q}"] = fit1[q]
            arrays[f"{name}_fit2_{q}"] = fit2[q]
        devs = {"fit1": ref.deviations(fit1, truth), "fit2": ref.deviations(fit2, truth), "restated": ref.deviations(restated, truth)}
        if (n, d) == ref.OFFSET_CASE:
            Xo = X + numpy.float32(1000.0)
            assert Xo.dtype == numpy.float32
            truth_o = ref.truth_pca(Xo, 2)
            arrays[f"{name}_offset_digest"] = ref.input_digest(Xo)
            for q in ref.QUANTITIES:
                arrays[f"{name}_offset_truth_{q}"] = truth_o[q]
            devs["restated_offset"] = ref.deviations(ref.fit_reference(Xo, 2), truth_o)
        for who, dev in devs.items():
            arrays[f"{name}_dev_{who}"] = numpy.asarray([dev[q] for q in ref.QUANTITIES])
        report[name] = {"solver": solver, "gap": float(w[1] / w[2]), **{who: ref.pooled(dev) for who, dev in devs.items()}}
    numpy.savez_compressed(OUT, **arrays)
    print(json.dumps(report, indent=1))
    print(f"wrote {OUT} ({OUT.stat().st_size} bytes)")
    assert OUT.stat().st_size < 1000000


if __name__ == "__main__":
    main()
