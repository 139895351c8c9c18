"""No GPU: tests/kde_reference.py (the restatement of the kernel-density contract above knn_kde_stats in
include/knn355.h) against the fixture tests/golden/reference_density.npz, which holds what the reference's
plot.density statements drew under pandas and scipy, and against a long-double evaluation of the same formula.

The bound on the density, relative to the truth: (E + 3 * 745 + 72 + nchunks) * 2**-53, plus one smallest subnormal.
E is kexp's largest ulp error against long-double exp over a fixed seeded sweep, measured here (1.14 on the build
machine); 3 * 745 covers the three roundings of t (the subtraction, the scaling and the square; the halving is exact),
each amplified by |t| <= 745; 72 is the depth of the sum inside a chunk (64 adds per lane, 8 tree levels), relative
because every term is positive; nchunks covers the adds over the chunks and the final product.  The recorded scipy curve
is compared with the same truth and its deviation printed, not gated: scipy whitens with a Cholesky factor of a
covariance from numpy.cov and differs from the formula by up to 1.5e-13 of the density in the tails."""
import ctypes
import math

import numpy as np
import pytest

import kde_reference as ref


@pytest.fixture(scope="module")
def golden():
    return ref.load_golden()


@pytest.fixture(scope="module")
def E():
    if not ref.has_long_double():
        pytest.skip("numpy.longdouble is no wider than float64 here")
    e = ref.kexp_ulp_error()
    print(f"kexp: at most {e:.3f} ulp from long-double exp over {ref.SWEEP_COUNT} values of t in (-700, 0]")
    return e


def test_kexp_is_within_two_ulps(E):
    assert E < 2.0


def test_kexp_edges():
    assert ref.kexp(np.array([0.0, -0.0])).tolist() == [1.0, 1.0]
    just_below = np.nextafter(ref.CUT, -np.inf)
    got = ref.kexp(np.array([just_below, ref.CUT, -1e300, -np.inf]))
    assert got[0] == 0.0 and got[2] == 0.0 and got[3] == 0.0 and not np.signbit(got).any()
    assert got[1] == ref.TINY, "exp(-745) is 0.57 of the smallest subnormal and rounds to it"
    # the exactness of k * LN2_HI: 32 significant bits times 11
    assert int(np.float64(ref.LN2_HI).view(np.uint64)) & ((1 << 21) - 1) == 0
    assert ref.COEF[13] == 1.0 / 6227020800.0 and ref.LOG2E == 1.4426950408889634


def test_numpy_ldexp_rounds_once_into_the_subnormal_range():
    """kexp's last step through numpy.ldexp gives the bits of Python's math.ldexp (C ldexp, correctly rounded) for
    every result that is subnormal or next to it, and of the exact 2**k product where the result is normal"""
    t = -np.random.default_rng(3).uniform(700.0, 746.0, 20000)
    t[:3] = (ref.CUT, -708.3964185322641, -709.0)
    tc = np.maximum(t, ref.CUT - 1.0)
    k = np.rint(tc * ref.LOG2E)
    r = (tc - k * ref.LN2_HI) - k * ref.LN2_LO
    p = np.full_like(r, ref.COEF[13])
    for i in range(12, -1, -1):
        p = p * r + ref.COEF[i]
    assert k.min() >= -1076 and k.max() <= -1009 and p.min() > 0.70 and p.max() < 1.42
    want = np.array([math.ldexp(float(pi), int(ki)) for pi, ki in zip(p, k)])
    want[t < ref.CUT] = 0.0
    got = ref.kexp(t)
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
    sub = (got > 0) & (got < 2.2250738585072014e-308)
    assert sub.sum() > 5000 and (~sub).sum() > 1000
    # one rounding, not two: the exact value p * 2**k against the two neighbouring subnormals
    from fractions import Fraction
    tiny = Fraction(ref.TINY)
    for ti, pi, ki, gi in zip(t[:3000], p[:3000], k[:3000], got[:3000]):
        if ti >= ref.CUT and ki < -1022:
            exact = Fraction(float(pi)) * Fraction(2) ** int(ki)
            assert abs(Fraction(float(gi)) - exact) <= tiny / 2


@pytest.mark.parametrize("n,dtype", ref.CASES)
def test_grid_is_the_recorded_one(golden, n, dtype):
    X = ref.case_input(golden, n, dtype)
    mn, mx, _, _ = ref.stats_reference(X[:, list(ref.COLUMNS)])
    for j in range(2):
        x = golden[f"{ref.case_name(n, dtype)}_x{j}"]
        assert x.dtype == np.dtype(dtype) and len(x) == 1000
        grid = ref.grid_reference(mn[j], mx[j], 1000, dtype)
        assert grid.dtype == np.float64
        assert np.array_equal(grid.view(np.uint64), x.astype(np.float64).view(np.uint64)), "the grid differs from pandas' in some bit"


@pytest.mark.parametrize("n,dtype", ref.CASES)
def test_density_is_within_the_bound_of_the_truth(golden, E, n, dtype):
    name = ref.case_name(n, dtype)
    X = ref.case_input(golden, n, dtype)[:, list(ref.COLUMNS)]
    grids, dens = ref.curves_reference(X)
    _, _, _, var = ref.stats_reference(X)
    bound = ref.relative_bound(E, n)
    for j in range(2):
        truth = ref.truth_density(X[:, j], grids[j], *ref.scales_reference(var[j], n, ref.factor_reference(n)))
        err = np.abs(dens[j].astype(np.longdouble) - truth)
        scipy_dev = float(np.max(np.abs(golden[f"{name}_y{j}"].astype(np.longdouble) - truth) / truth))
        print(f"{name} column {j}: restatement {float(np.max(err / truth)):.3e} of the truth (bound {bound:.3e}), "
              f"scipy {scipy_dev:.3e} (recorded {float(golden[f'{name}_scipy_deviation']):.3e})")
        assert (err <= bound * truth + ref.TINY).all()


def test_statistics_restatement_against_numpy():
    X = ref.bimodal_columns(9000, 5, "float32")
    mn, mx, mean, var = ref.stats_reference(X)
    X64 = X.astype(np.float64)
    assert np.array_equal(mn, X64.min(axis=0)) and np.array_equal(mx, X64.max(axis=0))
    assert np.allclose(mean, X64.mean(axis=0), rtol=1e-13, atol=0) and np.allclose(var, X64.var(axis=0, ddof=1), rtol=1e-13, atol=0)
    one = ref.stats_reference(X[:, 1])
    assert all(np.array_equal(a, b[1:2]) for a, b in zip(one, (mn, mx, mean, var)))
    assert ref.group_rows(2) == 4096 and ref.group_rows(4096 * 256) == 4096 and ref.group_rows(4096 * 256 + 1) == 8192


def test_evaluation_restatement_order():
    """the chunk sum of the restatement is the contract's: 256 strided partials, then the tree of adjacent pairs"""
    rng = np.random.default_rng(11)
    x = rng.standard_normal(ref.CHUNK + 700)
    g = np.array([0.25, 40.0])
    inv_h, norm = 2.0, 0.125
    z = (g[None, :] - x[:, None]) * inv_h
    terms = ref.kexp((z * z) * -0.5)
    total = None
    for r0 in range(0, len(x), ref.CHUNK):
        part = [np.zeros(2) for _ in range(256)]
        for i in range(r0, min(len(x), r0 + ref.CHUNK)):
            part[(i - r0) % 256] = part[(i - r0) % 256] + terms[i]
        stride = 1
        while stride < 256:
            for j in range(0, 256, 2 * stride):
                part[j] = part[j] + part[j + stride]
            stride *= 2
        total = part[0] if total is None else total + part[0]
    want = total * norm
    got = ref.evaluate_reference(x, g, inv_h, norm)
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
    assert got[1] == 0.0, "40 bandwidths... every term is past the cut"
    assert np.array_equal(ref.evaluate_reference(x, g, inv_h, norm, block=1).view(np.uint64), got.view(np.uint64))


# ---- refusals: ValueError in Python before the library is asked; the invalid-argument code from C -----------------
def test_refusals_python():
    from knn_for_homology_amd import density
    good = np.linspace(0.0, 1.0, 50)
    with pytest.raises(ValueError, match="2 values"):
        density.gaussian_kde(np.array([1.0]))
    with pytest.raises(ValueError, match="1-D"):
        density.gaussian_kde(np.zeros((2, 50)))
    for bad in (np.nan, np.inf, -np.inf):
        x = good.copy()
        x[7] = bad
        with pytest.raises(ValueError, match="NaN or an infinity"):
            density.gaussian_kde(x)
        with pytest.raises(ValueError, match="NaN or an infinity"):
            density.density_curves(np.stack([good, x], axis=1))
    for factor in (0.0, -1.0, np.nan, np.inf, "nonsense", True):
        with pytest.raises(ValueError, match="bw_method|factor"):
            density.gaussian_kde(good, bw_method=factor)
    with pytest.raises(ValueError, match="grid point"):
        density.density_curves(np.stack([good, good], axis=1), ind=0)
    with pytest.raises(ValueError, match="2-D"):
        density.density_curves(good)
    with pytest.raises(ValueError, match="one length"):
        density.density_curves({"a": good, "b": good[:-1]})
    with pytest.raises(ValueError, match="NaN or an infinity"):
        density.density_curves(np.stack([good, good], axis=1), ind=np.array([0.0, np.nan]))


def test_refusals_c():
    """every refusal comes before the device is looked for, so it is the same answer with and without a GPU"""
    from knn_for_homology_amd import _lib
    L = _lib.lib()
    INVALID = -1
    x = np.linspace(0.0, 1.0, 60).reshape(20, 3)
    st = np.full((4, 3), 7.0)
    grid = np.tile(np.linspace(-1.0, 2.0, 5), (3, 1))
    ih, nm, out = np.full(3, 2.0), np.full(3, 0.1), np.full((3, 5), 7.0)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    stats = lambda xx, dtype, n, c, stride: L.knn_kde_stats(p(xx), dtype, n, c, stride, p(st[0]), p(st[1]), p(st[2]), p(st[3]))  # noqa: E731
    ev = lambda xx, n, c, stride, g, m, a, b: L.knn_kde_eval(p(xx), 1, n, c, stride, p(g), m, p(a), p(b), p(out))  # noqa: E731
    assert stats(x, 2, 20, 3, 3) == INVALID and b"dtype" in L.knn_last_error()
    assert stats(x, 1, 1, 3, 3) == INVALID and b"n >= 2" in L.knn_last_error()
    assert stats(x, 1, 20, 0, 3) == INVALID
    assert stats(x, 1, 20, 4097, 4097) == INVALID
    assert stats(x, 1, 20, 3, 2) == INVALID and b"row_stride" in L.knn_last_error()
    assert stats(x, 1, 65535 * 16384 + 1, 3, 3) == INVALID
    assert L.knn_kde_stats(None, 1, 20, 3, 3, p(st[0]), p(st[1]), p(st[2]), p(st[3])) == INVALID
    assert L.knn_kde_stats(p(x), 1, 20, 3, 3, p(st[0]), None, p(st[2]), p(st[3])) == INVALID
    for bad in (np.nan, np.inf):
        xb = x.copy()
        xb[19, 2] = bad
        assert stats(xb, 1, 20, 3, 3) == INVALID and b"NaN" in L.knn_last_error()
        assert ev(xb, 20, 3, 3, grid, 5, ih, nm) == INVALID
        gb = grid.copy()
        gb[2, 4] = bad
        assert ev(x, 20, 3, 3, gb, 5, ih, nm) == INVALID and b"grid" in L.knn_last_error()
        for which in (0, 1):
            scale = [ih.copy(), nm.copy()]
            scale[which][1] = bad
            assert ev(x, 20, 3, 3, grid, 5, *scale) == INVALID
    xf = x.astype(np.float32)
    xf[3, 1] = np.nan
    assert stats(xf, 0, 20, 3, 3) == INVALID and b"NaN" in L.knn_last_error()
    for value in (0.0, -2.0):
        assert ev(x, 20, 3, 3, grid, 5, np.array([2.0, value, 2.0]), nm) == INVALID and b"positive" in L.knn_last_error()
        assert ev(x, 20, 3, 3, grid, 5, ih, np.array([0.1, 0.1, value])) == INVALID
    assert ev(x, 20, 3, 3, grid, 0, ih, nm) == INVALID and b"m >= 1" in L.knn_last_error()
    assert ev(x, 20, 3, 3, grid, (1 << 24) + 1, ih, nm) == INVALID
    assert ev(x, 1, 3, 3, grid, 5, ih, nm) == INVALID
    assert L.knn_kde_eval(p(x), 1, 20, 3, 3, None, 5, p(ih), p(nm), p(out)) == INVALID
    assert L.knn_kde_eval(p(x), 1, 20, 3, 3, p(grid), 5, p(ih), p(nm), None) == INVALID
    assert L.knn_kde_last_ms(None, None) == INVALID
    assert (st == 7).all() and (out == 7).all(), "a refused call wrote to its outputs"
