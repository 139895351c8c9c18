"""The kernel-density arithmetic contract of include/knn355.h (above knn_kde_stats) restated on the CPU -- test
infrastructure.  Vectorised numpy only; nothing of the library under test is touched.

numpy's elementwise ``*``, ``+`` and ``-`` on float64 arrays are single IEEE operations (no fused multiply-add), sums
that must run first to last are ``add.accumulate`` or explicit loops over a leading axis, ``numpy.rint`` rounds ties to
even and ``numpy.ldexp`` rounds once into the subnormal range (tests/test_kde_reference.py checks that claim).

Also here, because the fixture script and the tests must agree on them: the host half of the estimate (factor,
bandwidth, grid), the synthetic columns (``bimodal_columns``), the long-double truth (``truth_density``) and the bound.
"""
import math
from pathlib import Path

import numpy as np

CHUNK, LANES, TILE = 16384, 256, 16
LOG2E = float.fromhex("0x1.71547652b82fep+0")
LN2_HI = float.fromhex("0x1.62e42fee00000p-1")
LN2_LO = float.fromhex("0x1.a39ef35793c76p-33")
CUT = -745.0
COEF = [1.0 / float(math.factorial(i)) for i in range(14)]  # i! is exact in float64 up to 13!, the division rounds once


def group_rows(n):
    """rows per group of the statistics: L = 4096 * ceil(n / (4096 * 256)), a function of n alone"""
    return 4096 * -(-n // (4096 * 256))


def _seq_sum64(a):
    """sum over axis 0 in float64, strictly first to last, starting from the first entry"""
    return np.add.accumulate(np.asarray(a, np.float64), axis=0)[-1]


def _grouped_sum(a):
    n = a.shape[0]
    L = group_rows(n)
    return _seq_sum64(np.stack([_seq_sum64(a[r0:min(n, r0 + L)]) for r0 in range(0, n, L)]))


def stats_reference(X):
    """(min, max, mean, var) float64 [c] of the columns of X [n, c] (or [n]: c = 1), as knn_kde_stats defines them"""
    X = np.asarray(X)
    X = (X.reshape(len(X), -1)).astype(np.float64)  # widening is exact
    n = X.shape[0]
    mean = _grouped_sum(X) / np.float64(n)
    d = X - mean
    var = _grouped_sum(d * d) / np.float64(n - 1)
    return X.min(axis=0), X.max(axis=0), mean, var


def kexp(t):
    """exp(t) for t <= 0 as the contract spells it"""
    t = np.asarray(t, np.float64)
    tc = np.maximum(t, CUT - 1.0)  # (keeps k small whatever t is; such a t takes the cut below)
    k = np.rint(tc * LOG2E)
    r = (tc - k * LN2_HI) - k * LN2_LO
    p = np.full_like(r, COEF[13])
    for i in range(12, -1, -1):
        p = p * r + COEF[i]
    return np.where(t < CUT, 0.0, np.ldexp(p, k.astype(np.int32)))


def _tree(acc):
    """[256, .] -> [.]: adjacent pairs, strides 1, 2, 4, ..., 128"""
    while acc.shape[0] > 1:
        acc = acc[0::2] + acc[1::2]
    return acc[0]


def evaluate_reference(x, grid, inv_h, norm, block=64):
    """float64 [m]: the density of the sample x [n] (float32 or float64) at grid [m], as knn_kde_eval defines it"""
    x = np.asarray(x).astype(np.float64)
    grid = np.asarray(grid, np.float64)
    inv_h, norm = np.float64(inv_h), np.float64(norm)
    n, m = len(x), len(grid)
    out = np.empty(m, np.float64)
    with np.errstate(over="ignore"):
        for p0 in range(0, m, block):
            g = grid[p0:p0 + block]
            total = None
            for r0 in range(0, n, CHUNK):
                xs = x[r0:r0 + CHUNK]
                z = (g[None, :] - xs[:, None]) * inv_h
                terms = kexp((z * z) * -0.5)
                steps = -(-len(xs) // LANES)
                padded = np.zeros((steps * LANES, len(g)), np.float64)  # +0.0 changes no sum of non-negative terms
                padded[:len(xs)] = terms
                padded = padded.reshape(steps, LANES, len(g))
                acc = np.zeros((LANES, len(g)), np.float64)
                for s in range(steps):
                    acc = acc + padded[s]
                chunk_sum = _tree(acc)
                total = chunk_sum if total is None else total + chunk_sum
            out[p0:p0 + block] = total * norm
    return out


# ---- the host half: factor, bandwidth, grid (density.py spells the same expressions) --------------------------------
def factor_reference(n, bw_method=None):
    if bw_method is None or bw_method == "scott":
        return float(n) ** (-1.0 / 5.0)
    if bw_method == "silverman":
        return (float(n) * 3.0 / 4.0) ** (-1.0 / 5.0)
    return float(bw_method)


def scales_reference(var, n, factor):
    """(inv_h, norm) float64 from the ddof=1 variance"""
    h = math.sqrt(float(var)) * float(factor)
    return 1.0 / h, 1.0 / (float(n) * h * math.sqrt(2.0 * math.pi))


def grid_reference(mn, mx, m, dtype):
    """pandas 2.3.3 KdePlot._get_ind on a column of `dtype` whose extremes are mn, mx: the same expression on numpy
    scalars of that dtype (for float32 columns numpy >= 2 keeps it, linspace included, in float32), widened to float64"""
    lo, hi = np.dtype(dtype).type(mn), np.dtype(dtype).type(mx)
    sample_range = hi - lo
    return np.linspace(lo - 0.5 * sample_range, hi + 0.5 * sample_range, m).astype(np.float64)


def curves_reference(X, m=1000, bw_method=None):
    """(grids [c, m], densities [c, m]) float64: what density_curves(X, m, bw_method) must return bit for bit"""
    X = np.asarray(X)
    n, c = X.shape
    mn, mx, _, var = stats_reference(X)
    factor = factor_reference(n, bw_method)
    grids = np.stack([grid_reference(mn[j], mx[j], m, X.dtype) for j in range(c)])
    dens = np.stack([evaluate_reference(X[:, j], grids[j], *scales_reference(var[j], n, factor)) for j in range(c)])
    return grids, dens


# ---- the truth and the bound ----------------------------------------------------------------------------------------
def has_long_double():
    return np.finfo(np.longdouble).nmant >= 63


def truth_density(x, grid, inv_h, norm, block=64):
    """long double [m]: sum_i exp(-0.5 ((g - x_i) inv_h)^2) * norm with the float64 inv_h and norm"""
    ld = np.longdouble
    x = np.asarray(x).astype(ld)
    grid = np.asarray(grid, np.float64).astype(ld)
    out = np.empty(len(grid), ld)
    for p0 in range(0, len(grid), block):
        z = (grid[None, p0:p0 + block] - x[:, None]) * ld(inv_h)
        out[p0:p0 + block] = np.exp(z * z * ld(-0.5)).sum(axis=0) * ld(norm)
    return out


SWEEP_SEED, SWEEP_COUNT = 20240, 2_000_000


def kexp_ulp_error():
    """E: kexp's largest error in ulps of the true value against long-double exp, over a fixed seeded sweep of
    t in (-700, 0] (results are normal numbers there)"""
    t = -np.random.default_rng(SWEEP_SEED).uniform(0.0, 700.0, SWEEP_COUNT)
    t[:4] = (0.0, -0.0, -700.0, -1e-300)
    want = np.exp(t.astype(np.longdouble))
    ulp = np.spacing(want.astype(np.float64)).astype(np.longdouble)
    return float(np.max(np.abs(kexp(t).astype(np.longdouble) - want) / ulp))


def relative_bound(E, n):
    """|ours - truth| <= this * truth (plus one smallest subnormal): E ulps of kexp, three roundings of t each amplified
    by |t| <= 745, 72 adds deep inside a chunk (64 per lane and 8 tree levels; all terms are positive, so the bound on
    the sum is relative), the adds over the chunks and the final product"""
    nchunks = -(-n // CHUNK)
    return (E + 3 * 745 + 72 + nchunks) * 2.0 ** -53


TINY = 5e-324  # the smallest subnormal


# ---- the fixture tests/golden/reference_density.npz (tests/golden/make_kde_golden.py) -------------------------------
CASES = ((300, "float32"), (5000, "float32"), (300, "float64"), (5000, "float64"))
COLUMNS = (0, 2)  # the columns of bimodal_columns' matrix that the reference's statements plot
SEED0 = 8100


def case_name(n, dtype):
    return f"n{n}_{dtype}"


def bimodal_columns(n, seed, dtype):
    """[n, 4] of `dtype`, every column a mixture of two normal modes (weights 0.6 / 0.4, about six standard deviations
    apart, a different place and scale per column): the shape of a principal component over forward and scrambled
    proteins.  Columns 0:2 play the part of the original matrix, 2:4 of the scrambled one."""
    rng = np.random.default_rng(seed)
    centre = rng.uniform(-3.0, 3.0, 4)
    scale = rng.uniform(0.5, 2.0, 4)
    mode = rng.random((n, 4)) < 0.6
    x = rng.standard_normal((n, 4)) * np.where(mode, 1.0, 0.6) + np.where(mode, -2.5, 3.5)
    return np.ascontiguousarray((x * scale + centre).astype(dtype))


def input_digest(X):
    """a few float64 numbers that pin a regenerated input to the one the fixture was made from"""
    X = np.asarray(X, np.float64)
    return np.array([X.sum(), np.abs(X).sum(), X[::7, ::3].sum(), X[-1, -1]])


def load_golden():
    with np.load(Path(__file__).resolve().parent / "golden" / "reference_density.npz") as f:
        return {name: f[name] for name in f.files}


def case_input(golden, n, dtype):
    name = case_name(n, dtype)
    X = bimodal_columns(n, int(golden[f"{name}_seed"]), dtype)
    assert np.array_equal(input_digest(X), golden[f"{name}_digest"]), "the regenerated input is not the fixture's"
    return X
