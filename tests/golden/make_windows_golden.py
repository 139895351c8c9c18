#!/usr/bin/env python3
"""Regenerates tests/golden/reference_windows.npz -- run ONLY in the build container (needs /root/reference).

The reference's windowed curves are statements of notebook-style files that load whole datasets at import, so nothing of
them can be imported.  This script parses the files with `ast`, picks out four nodes, compiles each as it is and runs it
on synthetic arrays under the reference's names:
  seqvec_search/utils.py:103-113  def rolling_mean (numpy.convolve(data, ones(W) / W, "valid")), called here the way
                                  pfam/pfam.py:247-253 and cath/cath.py:799-813, 913-919 call it: on arrays indexed by
                                  numpy.argsort(key) or numpy.argsort(-key)
  cath/cath.py:863-875            def hist_evenly (ticks print the keys themselves)
  pfam/pfam.py:282-297            def hist_evenly (the same arithmetic; ticks in 0.0E format)
  cath/cath.py:834-850            the loop over length_plot_data with the fixed length bins
with a `plt` that records every errorbar call (x ticks, y, yerr, label) and does nothing else.  No reference source is
copied: the fixture holds the inputs and the arrays the reference's code handed to errorbar or returned, under this
container's numpy (version stored in the file).

The reference sorts with numpy's default, unstable, sort.  What it computes from an order among equal keys is not
defined, so the fixture says per input whether it is tie-free (`<input>_tie_free`), and for inputs with ties only
quantities that no permutation inside a group of equal keys can change are recorded: the rolling mean of the keys
themselves and the fixed-edge bins (which are masks, not orders).

    python tests/golden/make_windows_golden.py
"""
import ast
from pathlib import Path

import numpy

REFERENCE = Path("/root/reference")
OUT = Path(__file__).resolve().parent / "reference_windows.npz"
WINDOWS = (1000, 37)
BINS = (7, 10)


def node(path, kind, first, last, name=None):
    tree = ast.parse((REFERENCE / path).read_text())
    found = [n for n in ast.walk(tree) if isinstance(n, kind) and (n.lineno, n.end_lineno) == (first, last) and (name is None or n.name == name)]
    assert len(found) == 1, f"{path}:{first}-{last} was not found"
    return compile(ast.Module(body=found, type_ignores=[]), str(REFERENCE / path), "exec")


class Recorder:
    """plt: errorbar calls are recorded, every other attribute is a function that does nothing"""

    def __init__(self):
        self.calls = []

    def errorbar(self, **kwargs):
        self.calls.append(kwargs)

    def __getattr__(self, name):
        return lambda *args, **kwargs: None


def inputs(rng):
    n = 3000
    e = numpy.exp(rng.normal(-20, 15, n))                      # E-value-like, no two equal
    assert len(numpy.unique(e)) == n
    e_ties = e.copy()
    e_ties[rng.choice(n, 600, replace=False)] = rng.choice(e, 600)  # repeats of values that are there
    e_ties[rng.choice(n, 6, replace=False)] = 0.0               # a handful of exact zeros
    assert len(numpy.unique(e_ties)) < n - 100
    cos = ((rng.permutation(2500) - 700 + 0.25) / 2500).astype(numpy.float32)  # float32 cosine scores, negatives included, no two equal
    assert len(numpy.unique(cos)) == cos.size and (cos < 0).any()
    lengths = numpy.minimum(rng.gamma(2.2, 70, n).astype(numpy.int64) + 11, 1500)  # protein lengths: heavy ties
    assert len(numpy.unique(lengths)) < n // 2
    lengths_distinct = rng.choice(numpy.arange(20, 9000), n, replace=False).astype(numpy.int64)
    return {"evalue": e, "evalue_ties": e_ties, "cosine": cos, "lengths": lengths, "lengths_distinct": lengths_distinct}


def main():
    rng = numpy.random.default_rng(103863)
    ns = {"numpy": numpy, "ndarray": numpy.ndarray}
    exec(node("seqvec_search/utils.py", ast.FunctionDef, 103, 113, "rolling_mean"), ns)
    rolling_mean = ns["rolling_mean"]
    hist = {}
    for which, path, first, last in (("cath", "cath/cath.py", 863, 875), ("pfam", "pfam/pfam.py", 282, 297)):
        plt = Recorder()
        hns = {"numpy": numpy, "ndarray": numpy.ndarray, "plt": plt}
        exec(node(path, ast.FunctionDef, first, last, "hist_evenly"), hns)
        hist[which] = (hns["hist_evenly"], plt)
    length_bins = node("cath/cath.py", ast.For, 834, 850)

    keys = inputs(rng)
    out = {"numpy_version": numpy.asarray(numpy.__version__), "inputs": numpy.asarray(list(keys)), "windows": numpy.asarray(WINDOWS),
           "bins": numpy.asarray(BINS)}
    for name, k in keys.items():
        n = k.size
        cols = numpy.stack([rng.random(n) < p for p in (0.8, 0.5, 0.07)])  # three correctness columns
        tie_free = len(numpy.unique(k)) == n
        out[f"{name}_keys"], out[f"{name}_columns"], out[f"{name}_tie_free"] = k, cols, numpy.asarray(tie_free)
        for descending in (False, True):
            # the reference's own two spellings: numpy.argsort(key) (cath/cath.py:794, 911) and numpy.argsort(-key) (pfam/pfam.py:245)
            sorting = numpy.argsort(-k) if descending else numpy.argsort(k)
            tag = f"{name}_{'desc' if descending else 'asc'}"
            for w in WINDOWS:
                out[f"{tag}_w{w}_keys"] = rolling_mean(k[sorting], w)
                if tie_free:
                    out[f"{tag}_w{w}_columns"] = numpy.stack([rolling_mean(c[sorting], w) for c in cols])
            if tie_free:
                for bins in BINS:
                    for which, (fn, plt) in hist.items():
                        plt.calls.clear()
                        for c in cols:
                            fn(k[sorting], c[sorting], bins, "x")
                        out[f"{tag}_b{bins}_{which}_y"] = numpy.asarray([c["y"] for c in plt.calls], numpy.float64)
                        out[f"{tag}_b{bins}_{which}_yerr"] = numpy.asarray([c["yerr"] for c in plt.calls], numpy.float64)
                        out[f"{tag}_b{bins}_{which}_ticks"] = numpy.asarray(plt.calls[0]["x"])
        if k.dtype.kind == "i":  # the fixed length bins: masks over the lengths, whatever the order
            plt = Recorder()
            lns = {"numpy": numpy, "plt": plt, "lengths": k, "bin_size": 50, "buckets": 6, "length_plot_data": {f"c{i}": c for i, c in enumerate(cols)}}
            with numpy.errstate(all="ignore"):
                exec(length_bins, lns)
            assert len(plt.calls) == 3
            out[f"{name}_edges"] = numpy.arange(0, 50 * 6, 50)
            out[f"{name}_edge_y"] = numpy.asarray([c["y"] for c in plt.calls], numpy.float64)
            out[f"{name}_edge_yerr"] = numpy.asarray([c["yerr"] for c in plt.calls], numpy.float64)
    numpy.savez_compressed(OUT, **out)
    print(f"wrote {OUT} ({OUT.stat().st_size} bytes)")


if __name__ == "__main__":
    main()
