"""GPU: knn_pca_moments, knn_pca_project and decomposition.PCA, bit for bit against tests/pca_reference.py (the CPU
restatement of the contract above knn_pca_moments in include/knn355.h).

Shapes are the smallest that reach each way the kernels can go wrong: less than one block of 8 rows; off-diagonal
128-column tiles and an odd row tail; two row groups with a 3-row tail and a partial-width edge tile; a group boundary
hit exactly with d no multiple of 32; the reference's widths with fewer rows than columns; 129 groups of 8192 rows.
The projection: one row, d no multiple of 8; 2 and 32 components at d = 1024; three slabs of the walker.  End to end:
the fixture's (700, 1024) case, bit for bit against the restatement and within the bound of test_pca_reference.py of
the float64 truth."""
import ctypes

import numpy as np
import pytest

import pca_reference as ref

pytestmark = pytest.mark.gpu

KNOB = "KNN355_EVAL_SLAB_ROWS"
MOMENT_SHAPES = [(5, 32), (37, 96), (4099, 160), (8192, 36), (300, 1024), (64, 1280), (1048581, 8)]


@pytest.fixture(scope="module")
def dec(gpu_faiss):
    from knn_for_homology_amd import decomposition
    return decomposition


def rows_of(n, d, seed):
    """correlated columns around a non-zero mean: every covariance entry is far from zero"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, d), dtype=np.float32)
    x += rng.standard_normal((n, 1), dtype=np.float32) * rng.uniform(0.5, 1.5, d).astype(np.float32)
    x += rng.uniform(-2.0, 2.0, d).astype(np.float32)
    return x


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


@pytest.mark.parametrize("n,d", MOMENT_SHAPES)
def test_moments_bit_for_bit(dec, n, d):
    x = rows_of(n, d, 100 + d)
    keep = x.copy()
    mean, cov = dec.moments(x)
    assert np.array_equal(x, keep), "the input was modified"
    rmean, rcov = ref.moments_reference(x)
    assert same_bits(mean, rmean), f"mean differs in {(mean != rmean).sum()} of {d} columns"
    bad = np.argwhere(cov.view(np.uint64) != rcov.view(np.uint64))
    assert len(bad) == 0, f"cov differs at {len(bad)} entries, first {bad[:4].tolist()}"


@pytest.fixture(scope="module")
def with_constant_column(dec):
    x = rows_of(37, 96, 7)
    x[:, 40] = np.float32(1.75)
    return x, dec.moments(x)


def test_covariance_is_its_transpose(with_constant_column):
    _, (_, cov) = with_constant_column
    assert same_bits(cov, cov.T)


def test_constant_column_gives_zero_row_and_column(with_constant_column):
    x, (mean, cov) = with_constant_column
    assert mean[40] == np.float32(1.75)
    assert not cov[40].any() and not cov[:, 40].any()
    assert np.count_nonzero(cov) == 95 * 95
    assert same_bits(cov, ref.moments_reference(x)[1])


def projection_inputs(n, d, nc, seed):
    rng = np.random.default_rng(seed)
    x = rows_of(n, d, seed)
    mean = rng.uniform(-2.0, 2.0, d).astype(np.float32)
    comp = rng.standard_normal((nc, d), dtype=np.float32)
    return x, mean, comp


@pytest.mark.parametrize("n,d,nc", [(1, 36, 1), (70, 1024, 2), (70, 1024, 32)])
def test_projection_bit_for_bit(dec, monkeypatch, n, d, nc):
    monkeypatch.delenv(KNOB, raising=False)
    x, mean, comp = projection_inputs(n, d, nc, 300 + nc)
    keep = x.copy()
    out = dec.project(x, mean, comp)
    assert np.array_equal(x, keep), "the input was modified"
    assert same_bits(out, ref.project_reference(x, mean, comp))


@pytest.mark.parametrize("slab", [50, 65])
def test_projection_across_slabs(dec, monkeypatch, slab):
    """130 rows in slabs of 50 (three slabs, none a multiple of the kernel's 64 rows) and of 65 (two)"""
    x, mean, comp = projection_inputs(130, 64, 2, 11)
    monkeypatch.delenv(KNOB, raising=False)
    whole = dec.project(x, mean, comp)
    monkeypatch.setenv(KNOB, str(slab))
    out = dec.project(x, mean, comp)
    assert same_bits(out, whole)
    assert same_bits(out, ref.project_reference(x, mean, comp))


def test_fit_transform_end_to_end(dec):
    golden = ref.load_golden()
    n, d = 700, 1024
    x = ref.case_input(golden, n, d)
    pca = dec.PCA(2)
    y = pca.fit_transform(x)
    want = ref.fit_reference(x, 2)
    assert pca.n_samples_ == n and y.shape == (n, 2) and y.dtype == np.float32
    for name in ("mean_", "covariance_", "components_", "explained_variance_", "explained_variance_ratio_", "singular_values_"):
        assert same_bits(getattr(pca, name), want[name]), name
    assert same_bits(y, want["transform"])
    assert same_bits(pca.transform(x), y)
    assert same_bits(dec.PCA(2).fit(x).components_, pca.components_)
    got = {q: (y if q == "transform" else getattr(pca, q)) for q in ref.QUANTITIES}
    dev = ref.pooled(ref.deviations(got, ref.case_arrays(golden, n, d, "truth")))
    bound = ref.sklearn_bound(golden)
    print("end to end:", dev, "bound:", bound)
    for kind, v in dev.items():
        assert v <= bound[kind], (kind, v, bound[kind])


# ---- refusals: ValueError in Python, the invalid-argument code from C, nothing launched ----------------------------
def test_refused_shapes_python(dec):
    rng = np.random.default_rng(0)
    with pytest.raises(ValueError, match="multiple of 4"):
        dec.PCA(2).fit(rng.standard_normal((50, 30), dtype=np.float32))
    with pytest.raises(ValueError, match="multiple of 4"):
        dec.PCA(2).fit(np.zeros((8, 2052), np.float32))
    with pytest.raises(ValueError, match="row"):
        dec.PCA(1).fit(rng.standard_normal((1, 8), dtype=np.float32))
    with pytest.raises(ValueError, match="n_components"):
        dec.PCA(33)
    with pytest.raises(ValueError, match="n_components"):
        dec.PCA(0)
    with pytest.raises(ValueError, match="at most min"):
        dec.PCA(4).fit(rng.standard_normal((3, 8), dtype=np.float32))
    with pytest.raises(ValueError, match="at most min"):
        dec.PCA(5).fit(rng.standard_normal((30, 4), dtype=np.float32))
    with pytest.raises(TypeError):
        dec.PCA(2, whiten=True)
    with pytest.raises(ValueError, match="not fitted"):
        dec.PCA(2).transform(np.zeros((4, 8), np.float32))


def test_refused_shapes_c(dec):
    from knn_for_homology_amd import _lib
    L = _lib.lib()
    x = np.ones((8, 2052), np.float32)
    mean = np.full(2052, np.float32(7.0))
    cov = np.full((8, 8), 7.0)
    out = np.full((8, 40), np.float32(7.0))
    comp = np.ones((40, 2052), np.float32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    INVALID = -1
    assert L.knn_pca_moments(p(x), 8, 30, p(mean), p(cov)) == INVALID
    assert b"multiple of 4" in L.knn_last_error()
    assert L.knn_pca_moments(p(x), 8, 2052, p(mean), p(cov)) == INVALID
    assert L.knn_pca_moments(p(x), 8, 0, p(mean), p(cov)) == INVALID
    assert L.knn_pca_moments(p(x), 1, 8, p(mean), p(cov)) == INVALID
    assert L.knn_pca_moments(None, 8, 8, p(mean), p(cov)) == INVALID
    assert L.knn_pca_project(p(x), 8, 30, p(mean), p(comp), 2, p(out)) == INVALID
    assert L.knn_pca_project(p(x), 8, 64, p(mean), p(comp), 33, p(out)) == INVALID
    assert L.knn_pca_project(p(x), 8, 64, p(mean), p(comp), 0, p(out)) == INVALID
    assert L.knn_pca_project(p(x), 8, 8, p(mean), p(comp), 9, p(out)) == INVALID
    assert L.knn_pca_project(p(x), -1, 8, p(mean), p(comp), 2, p(out)) == INVALID
    assert L.knn_pca_project(p(x), 8, 8, p(mean), None, 2, p(out)) == INVALID
    assert L.knn_pca_project(None, 0, 8, None, None, 2, None) == 0
    assert (mean == 7).all() and (cov == 7).all() and (out == 7).all(), "a refused call wrote to its outputs"


@pytest.mark.parametrize("bad", [np.nan, np.inf])
def test_non_finite_input_raises(dec, bad):
    x = rows_of(40, 16, 5)
    x[17, 3] = bad
    with pytest.raises(ValueError, match="not finite"):
        dec.PCA(2).fit(x)
    with pytest.raises(ValueError, match="not finite"):
        dec.PCA(2).fit_transform(x)
