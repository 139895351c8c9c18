#!/usr/bin/env python3
"""Regenerates tests/golden/reference_correlation.npz -- run ONLY in the build container (needs /root/reference and scipy).

The reference's correlations are the last statements of a notebook-style file that loads whole datasets at import, so
nothing of it can be imported.  This script parses cath/cath.py with `ast`, picks out the top-level statements of lines
949-952 (logged = numpy.log(e_values_cath); the -inf of exact zeros moved to -1e9; print(pearsonr(scores_best, logged));
print(spearmanr(scores_best, e_values_cath))), compiles them as they are and runs them on synthetic arrays under the
reference's names, with scipy.stats' pearsonr and spearmanr and a `print` that records its argument.  scipy.stats.rankdata
runs on the same inputs.  No reference source is copied: the fixture holds the inputs, `logged`, the ranks, both statistics
and both p-values, under this container's numpy and scipy (versions stored in the file).

    python tests/golden/make_correlation_golden.py
"""
import ast
import warnings
from pathlib import Path

import numpy
import scipy
from scipy.stats import pearsonr, rankdata, spearmanr

REFERENCE = Path("/root/reference")
OUT = Path(__file__).resolve().parent / "reference_correlation.npz"


def statements(path, first, last):
    tree = ast.parse((REFERENCE / path).read_text())
    found = [n for n in tree.body if first <= n.lineno and n.end_lineno <= last]
    assert [type(n) for n in found] == [ast.Assign, ast.Assign, ast.Expr, ast.Expr], f"{path}:{first}-{last} is not the four statements"
    return compile(ast.Module(body=found, type_ignores=[]), str(REFERENCE / path), "exec")


def evalues(rng, n, zeros):
    e = numpy.exp(rng.normal(-12, 10, n))
    e[rng.choice(n, n // 5, replace=False)] = rng.choice(e, n // 5)  # repeats of values that are there
    e[rng.choice(n, zeros, replace=False)] = 0.0                      # exact zeros: log gives -inf
    return e


def inputs(rng):
    cases = {}
    # float32 cosine-like scores with repeated values against float64 E-values with exact zeros
    e = evalues(rng, 2000, 9)
    cos = numpy.round(numpy.clip(0.55 - 0.02 * numpy.log10(e + 1e-300) / 3 + rng.normal(0, 0.08, 2000), -1, 1), 3).astype(numpy.float32)
    assert len(numpy.unique(cos)) < 1500 and (e == 0).sum() == 9
    cases["cath"] = (cos, e)
    # [rows, k] arrays with whole rows copied (ties between rows) and -0.0 beside +0.0
    x = numpy.round(rng.normal(0, 0.3, (60, 20)), 2).astype(numpy.float32)
    y = evalues(rng, 1200, 5).reshape(60, 20)
    for dst, src in ((7, 3), (8, 3), (41, 40), (59, 0)):
        x[dst], y[dst] = x[src], y[src]
    x[x == 0] = 0.0
    x[5, :6] = [0.0, -0.0, 0.0, -0.0, -0.0, 0.0]
    assert numpy.signbit(x[5, 1]) and not numpy.signbit(x[5, 0])
    cases["ties"] = (x, y)
    # a +inf among the E-values: the reference moves every infinite logarithm to -1e9, this one too; the ranks keep it on top
    e = evalues(rng, 500, 2)
    e[123] = numpy.inf
    cases["inf"] = (rng.normal(0.4, 0.2, 500).astype(numpy.float32), e)
    # no two equal, one more than a wave
    cases["distinct"] = ((rng.permutation(65) / 65 - 0.3).astype(numpy.float32), numpy.exp(rng.permutation(65) - 40.0))
    # the types the other way round: float64 scores, float32 E-values
    e = evalues(rng, 1500, 4).astype(numpy.float32)
    cases["f64_f32"] = (numpy.round(rng.normal(0.5, 0.15, 1500), 4), e)
    return cases


def main():
    rng = numpy.random.default_rng(949952)
    code = statements("cath/cath.py", 949, 952)
    out = {"numpy_version": numpy.asarray(numpy.__version__), "scipy_version": numpy.asarray(scipy.__version__)}
    cases = inputs(rng)
    out["cases"] = numpy.asarray(list(cases))
    total = 0
    for name, (scores, e) in cases.items():
        printed = []
        ns = {"numpy": numpy, "pearsonr": pearsonr, "spearmanr": spearmanr, "print": printed.append, "scores_best": scores.reshape(-1),
              "e_values_cath": e.reshape(-1)}
        with numpy.errstate(divide="ignore", invalid="ignore"), warnings.catch_warnings():
            warnings.simplefilter("ignore")
            exec(code, ns)
        assert len(printed) == 2
        out[f"{name}_x"], out[f"{name}_y"], out[f"{name}_logged"] = scores, e, ns["logged"].reshape(e.shape)
        out[f"{name}_rank_x"], out[f"{name}_rank_y"] = rankdata(scores.reshape(-1), "average"), rankdata(e.reshape(-1), "average")
        out[f"{name}_pearson"] = numpy.asarray([printed[0].statistic, printed[0].pvalue], numpy.float64)
        out[f"{name}_spearman"] = numpy.asarray([printed[1].statistic, printed[1].pvalue], numpy.float64)
        total += scores.size
        print(name, scores.shape, scores.dtype, e.dtype, out[f"{name}_pearson"], out[f"{name}_spearman"])
    numpy.savez_compressed(OUT, **out)
    print(f"wrote {OUT} ({OUT.stat().st_size} bytes, {total} pairs)")


if __name__ == "__main__":
    main()
