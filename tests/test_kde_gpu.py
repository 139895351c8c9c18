"""GPU: knn_kde_stats, knn_kde_eval, density.gaussian_kde and density.density_curves, bit for bit against
tests/kde_reference.py (the CPU restatement of the contract above knn_kde_stats in include/knn355.h).

Shapes are the smallest that reach each way the kernels can go wrong.  Rows: two (one lane with a row), a lane tail on
either side of 256, a chunk hit exactly and passed by one row, three chunks with a tail.  Grid points: one, a tile less
one, a tile, a tile and one, and the reference's 1000.  Both input types; one column and the three columns of a C-order
[n, 3] matrix read where they lie.  A grid 40 bandwidths outside the data (exactly 0.0), a grid across the -745 cut
(subnormal terms and sums).  Statistics at less than eight rows, two groups, and the first n at which a group is 8192
rows.  End to end: the fixture's n = 5000 case against the restatement bit for bit and against the curve the
reference's statement drew under scipy."""
import ctypes

import numpy as np
import pytest

import kde_reference as ref

pytestmark = pytest.mark.gpu

EVAL_SHAPES = [(2, 1), (2, 17), (255, 16), (256, 15), (256, 1000), (257, 1), (257, 17), (16384, 16), (16384, 1), (16385, 15), (16385, 17),
               (40000, 1), (40000, 16), (40000, 17), (16385, 1000)]


@pytest.fixture(scope="module")
def den(gpu_faiss):
    from knn_for_homology_amd import density
    return density


def sample(n, c, seed, dtype):
    """bimodal columns with different places and scales"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, c)) * rng.uniform(0.5, 2.0, c) + np.where(rng.random((n, c)) < 0.6, -2.5, 3.5) + rng.uniform(-3.0, 3.0, c)
    return np.ascontiguousarray(x.astype(dtype))


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype == np.float64 and a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def check_curves(got, X, m):
    grids, dens = got
    rgrids, rdens = ref.curves_reference(X, m)
    assert same_bits(grids, rgrids), "the grids differ"
    bad = np.argwhere(dens.view(np.uint64) != rdens.view(np.uint64))
    assert dens.shape == rdens.shape and len(bad) == 0, f"the density differs at {len(bad)} of {dens.size} points, first {bad[:4].tolist()}"
    assert (dens >= 0).all() and dens.max() > 0


@pytest.mark.parametrize("n,m", EVAL_SHAPES)
def test_curves_bit_for_bit(den, n, m):
    dtype = np.float32 if (n + m) % 2 else np.float64
    X = sample(n, 1, 1000 + n + m, dtype)
    keep = X.copy()
    check_curves(den.density_curves(X, m), X, m)
    assert np.array_equal(X, keep), "the input was modified"


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("n,m", [(257, 17), (16385, 33)])
def test_three_columns_and_strided_views(den, dtype, n, m):
    X = sample(n, 3, 77 + n, dtype)
    got = den.density_curves(X, m)
    check_curves(got, X, m)
    # two neighbouring columns of the matrix, read where they lie (row stride 3)
    check_curves(den.density_curves(X[:, 1:], m), X[:, 1:], m)
    # a dict of the columns gives the same curves
    again = den.density_curves({"a": X[:, 0], "b": X[:, 1], "c": X[:, 2]}, m)
    assert same_bits(again[0], got[0]) and same_bits(again[1], got[1])
    # gaussian_kde on a strided column view: no host copy, the same bits
    for j in range(3):
        col = X[:, j]
        kde = den.gaussian_kde(col)
        assert np.shares_memory(kde.dataset, X) and kde.dataset.shape == (1, n)
        assert kde.n == n and kde.d == 1 and kde.factor == ref.factor_reference(n)
        _, _, _, var = ref.stats_reference(col)
        assert same_bits(kde.covariance, np.array([[var[0] * kde.factor ** 2]]))
        assert same_bits(kde.evaluate(got[0][j]), got[1][j])
        assert same_bits(kde(got[0][j][None, :]), got[1][j])


@pytest.mark.parametrize("bw", ["scott", "silverman", 0.3])
def test_bandwidth_methods_and_explicit_grid(den, bw):
    X = sample(700, 2, 5, np.float32)
    ind = np.linspace(-9.0, 11.0, 37)
    grids, dens = den.density_curves(X, ind, bw)
    factor = ref.factor_reference(700, bw)
    _, _, _, var = ref.stats_reference(X)
    for j in range(2):
        assert same_bits(grids[j], ind)
        want = ref.evaluate_reference(X[:, j], ind, *ref.scales_reference(var[j], 700, factor))
        assert same_bits(dens[j], want)
        assert same_bits(den.gaussian_kde(X[:, j], bw_method=bw)(ind), want)
    ms = den.last_ms()
    assert set(ms) == {"upload", "stats", "eval"} and all(v >= 0 for v in ms.values()) and ms["eval"] > 0


def test_grid_far_outside_is_exactly_zero(den):
    x = sample(16385, 1, 9, np.float64)[:, 0]
    kde = den.gaussian_kde(x)
    h = 1.0 / ref.scales_reference(ref.stats_reference(x)[3][0], len(x), kde.factor)[0]
    points = np.array([x.max() + 40.0 * h, x.min() - 40.0 * h, x.max() + 1e6 * h, 1e300, -1e300] + [x.max() + 41.0 * h] * 13)
    out = kde(points)
    assert out.shape == (18,) and not out.any() and not np.signbit(out).any(), "every term is past the -745 cut: exactly +0.0"


def test_grid_across_the_cut_sums_subnormal_terms(den):
    """points 37.0 to 38.8 bandwidths beyond the largest value: t of the nearest sample runs from -684 to -753, so the
    sums pass through the subnormal range down to the smallest subnormal and to zero"""
    x = sample(600, 1, 21, np.float64)[:, 0]
    kde = den.gaussian_kde(x)
    inv_h, norm = ref.scales_reference(ref.stats_reference(x)[3][0], len(x), kde.factor)
    points = x.max() + np.linspace(37.0, 38.8, 181) / inv_h
    want = ref.evaluate_reference(x, points, inv_h, norm)
    tiny_normal = 2.2250738585072014e-308
    assert ((want > 0) & (want < tiny_normal)).sum() >= 20 and (want == 0).sum() >= 5 and (want >= tiny_normal).sum() >= 5, "the case is what it claims"
    got = kde(points)
    bad = np.flatnonzero(got.view(np.uint64) != want.view(np.uint64))
    assert len(bad) == 0, f"{len(bad)} points differ, first {bad[:4].tolist()}: {got[bad[:4]]} against {want[bad[:4]]}"


@pytest.mark.parametrize("c", [1, 3])
@pytest.mark.parametrize("n", [5, 4097, 1048581])
def test_statistics_bit_for_bit(den, n, c):
    X = sample(n, 3, 300 + n, np.float32 if c == 3 else np.float64)
    V = X if c == 3 else X[:, 1:2]  # one column: a strided view
    got = den._stats(den._rows(V))
    want = ref.stats_reference(V)
    for name, g, w in zip(("min", "max", "mean", "var"), got, want):
        assert same_bits(g, w), f"{name}: {g} against {w}"


@pytest.fixture(scope="module")
def fixture_case(den):
    golden = ref.load_golden()
    X = ref.case_input(golden, 5000, "float32")
    cols = {"original": X[:, 0:2][:, 0], "reversed": X[:, 2:4][:, 0]}  # the reference's statement, columns as it picks them
    return golden, X, den.density_curves(cols)


def test_fixture_case_bit_for_bit(fixture_case):
    _, X, got = fixture_case
    check_curves(got, X[:, list(ref.COLUMNS)], 1000)


def test_fixture_case_against_the_recorded_scipy_curve(fixture_case):
    """the curves the reference's plot.density statement drew: the same x bit for bit; y within the bound of
    tests/test_kde_reference.py of the truth, plus scipy's own recorded deviation from it"""
    golden, X, (grids, dens) = fixture_case
    name = ref.case_name(5000, "float32")
    E = ref.kexp_ulp_error()
    slack = ref.relative_bound(E, 5000) + float(golden[f"{name}_scipy_deviation"])
    _, _, _, var = ref.stats_reference(X[:, list(ref.COLUMNS)])
    for j in range(2):
        x, y = golden[f"{name}_x{j}"], golden[f"{name}_y{j}"]
        assert same_bits(grids[j], x.astype(np.float64))
        truth = ref.truth_density(X[:, ref.COLUMNS[j]], grids[j], *ref.scales_reference(var[j], 5000, ref.factor_reference(5000)))
        dev = np.abs(dens[j].astype(np.longdouble) - y.astype(np.longdouble))
        print(f"column {j}: at most {float(np.max(dev / truth)):.3e} of the density from scipy's curve, allowed {slack:.3e}")
        assert (dev <= slack * truth + ref.TINY).all()


# ---- refusals ---------------------------------------------------------------------------------------------------------
def test_zero_variance_is_refused(den):
    with pytest.raises(ValueError, match="zero variance"):
        den.gaussian_kde(np.full(300, 2.5, np.float32))
    with pytest.raises(ValueError, match="zero variance"):
        den.density_curves(np.stack([np.linspace(0, 1, 300), np.full(300, -1.0)], axis=1))


def test_refusals_leave_the_outputs_untouched(den):
    from knn_for_homology_amd import _lib
    L = _lib.lib()
    INVALID = -1
    x = sample(40, 3, 1, np.float64)
    grid = np.tile(np.linspace(-8.0, 8.0, 5), (3, 1))
    st, out = np.full((4, 3), 7.0), np.full((3, 5), 7.0)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    ev = lambda xx, g, a, b: L.knn_kde_eval(p(xx), 1, 40, 3, 3, p(g), 5, p(a), p(b), p(out))  # noqa: E731
    ih, nm = np.full(3, 2.0), np.full(3, 0.1)
    xb = x.copy()
    xb[39, 2] = np.nan
    assert L.knn_kde_stats(p(xb), 1, 40, 3, 3, p(st[0]), p(st[1]), p(st[2]), p(st[3])) == INVALID
    assert L.knn_kde_stats(p(x), 1, 1, 3, 3, p(st[0]), p(st[1]), p(st[2]), p(st[3])) == INVALID
    assert ev(xb, grid, ih, nm) == INVALID
    gb = grid.copy()
    gb[1, 1] = np.inf
    assert ev(x, gb, ih, nm) == INVALID
    assert ev(x, grid, np.array([2.0, np.inf, 2.0]), nm) == INVALID, "what a zero variance gives"
    assert ev(x, grid, ih, np.array([0.1, 0.0, 0.1])) == INVALID
    assert L.knn_kde_eval(p(x), 1, 40, 3, 3, p(grid), 0, p(ih), p(nm), p(out)) == INVALID
    assert (st == 7).all() and (out == 7).all(), "a refused call wrote to its outputs"
    # the element next to the used columns is not looked at, and the same arrays then hold the answer
    assert L.knn_kde_stats(p(xb), 1, 40, 2, 3, p(st[0]), p(st[1]), p(st[2]), p(st[3])) == 0
    want = ref.stats_reference(x[:, :2])
    assert all(same_bits(st[i, :2], want[i]) for i in range(4)) and (st[:, 2] == 7).all()
    assert ev(x, grid, ih, nm) == 0
    assert same_bits(out[1], ref.evaluate_reference(x[:, 1], grid[1], 2.0, 0.1))
