"""The PCA arithmetic contract of include/knn355.h (above knn_pca_moments) restated on the CPU -- test infrastructure.

Nothing of the library under test is touched: float64 sums are numpy's sequential ``add.accumulate``, every fp32 chain
is the CPU oracle's ``orc_dot`` (oracle/knn_oracle.c: one fmaf per step, blocks of 8 visited 0,4,1,5,2,6,3,7, the last
block zero padded), and the host half of ``fit`` (eigh, order, sign, the derived vectors) is written out again here.

Also here, because the fixture script and the tests must agree on them: the synthetic inputs (``planted_input``), the
float64 truth (``truth_pca``) and the deviation measure (``deviations``).
"""
import numpy as np

from oracle import knn_oracle as ko

P8 = np.array([0, 4, 1, 5, 2, 6, 3, 7])


def group_rows(n):
    """rows per group: L = 4096 * ceil(n / (4096 * 256)), a function of n alone"""
    return 4096 * -(-n // (4096 * 256))


def _groups(n):
    L = group_rows(n)
    return [(r0, min(n, r0 + L)) for r0 in range(0, n, L)]


def _seq_sum64(a):
    """sum over axis 0 in float64, strictly first to last (numpy's sum is pairwise; accumulate is not)"""
    return np.add.accumulate(np.asarray(a, np.float64), axis=0)[-1]


def mean_reference(X):
    X = np.ascontiguousarray(X, np.float32)
    n = X.shape[0]
    sums = np.stack([_seq_sum64(X[r0:r1]) for r0, r1 in _groups(n)])
    return (_seq_sum64(sums) / np.float64(n)).astype(np.float32)


def _ascending_chain_layout(cols):
    """cols float32 [d, rows] -> [d, rows padded to 8] with every block of 8 permuted so that orc_dot's visit order
    0,4,1,5,2,6,3,7 walks the original entries first to last"""
    d, rows = cols.shape
    rp = -(-rows // 8) * 8
    out = np.zeros((d, rp), np.float32)
    src = np.zeros((d, rp), np.float32)
    src[:, :rows] = cols
    out.reshape(d, rp // 8, 8)[:, :, P8] = src.reshape(d, rp // 8, 8)
    return out


def moments_reference(X):
    """(mean float32 [d], cov float64 [d, d]) as knn_pca_moments defines them"""
    X = np.ascontiguousarray(X, np.float32)
    n, d = X.shape
    mean = mean_reference(X)
    iu, ju = np.triu_indices(d)
    iu, ju = iu.astype(np.int64), ju.astype(np.int64)
    orc = ko.oracle()
    partial = []
    for r0, r1 in _groups(n):
        xc = X[r0:r1] - mean  # one fp32 subtraction per entry
        assert xc.dtype == np.float32
        cols = _ascending_chain_layout(np.ascontiguousarray(xc.T))
        partial.append(orc.pair_distances(cols, cols, iu, ju, ko.METRIC_INNER_PRODUCT))
    upper = _seq_sum64(np.stack(partial)) / np.float64(n - 1)
    cov = np.empty((d, d), np.float64)
    cov[iu, ju] = upper
    cov[ju, iu] = upper
    return mean, cov


def project_reference(X, mean, components):
    """float32 [n, nc] as knn_pca_project defines it"""
    X = np.ascontiguousarray(X, np.float32)
    mean = np.ascontiguousarray(mean, np.float32)
    components = np.ascontiguousarray(components, np.float32)
    n, nc = X.shape[0], components.shape[0]
    xc = X - mean
    assert xc.dtype == np.float32
    rows = np.repeat(np.arange(n, dtype=np.int64), nc)
    comps = np.tile(np.arange(nc, dtype=np.int64), n)
    return ko.oracle().pair_distances(components, xc, rows, comps, ko.METRIC_INNER_PRODUCT).reshape(n, nc)


def top_components(cov, n, nc):
    """the host half of fit in float64: (components [nc, d], explained_variance, explained_variance_ratio,
    singular_values [nc]); eigh, descending, the largest-magnitude entry of every eigenvector (the first on ties)
    made positive"""
    w, v = np.linalg.eigh(cov)
    order = np.argsort(w, kind="stable")[::-1][:nc]
    w_top = w[order]
    comp = np.ascontiguousarray(v[:, order].T)
    for c in comp:
        if c[np.argmax(np.abs(c))] < 0:
            c *= -1.0
    return comp, w_top, w_top / np.trace(cov), np.sqrt(w_top * (n - 1))


def fit_reference(X, nc):
    """the attributes PCA(nc).fit(X) must hold, bit for bit, and its fit_transform output"""
    X = np.ascontiguousarray(X, np.float32)
    mean, cov = moments_reference(X)
    comp, ev, evr, sv = top_components(cov, X.shape[0], nc)
    out = {"mean_": mean, "covariance_": cov, "components_": comp.astype(np.float32), "explained_variance_": ev.astype(np.float32),
           "explained_variance_ratio_": evr.astype(np.float32), "singular_values_": sv.astype(np.float32)}
    out["transform"] = project_reference(X, mean, out["components_"])
    return out


# ---- what the fixture script and the tests share ------------------------------------------------------------------
CASES = ((300, 64), (3000, 128), (700, 1024), (3000, 1024))
OFFSET_CASE = (3000, 128)  # the case that is also run with 1000 added to every entry
QUANTITIES = ("transform", "components_", "explained_variance_", "explained_variance_ratio_", "singular_values_")


def case_name(n, d):
    return f"n{n}_d{d}"


def planted_input(n, d, seed):
    """float32 [n, d] with a planted spectrum: two orthonormal directions with variances 400 and 100 over independent
    columns with variances in [0.5, 2], plus a column mean of order 1.  Population ratio of the second to the third
    eigenvalue: 50 at least; the sample ratio at n < d (bulk edge about 2 (1 + sqrt(d / n))^2) stays above 4, which the
    fixture script asserts.  Entries are of order 1, as embeddings' are."""
    rng = np.random.default_rng(seed)
    u = np.linalg.qr(rng.standard_normal((d, 2)))[0].T  # [2, d] orthonormal rows
    x = rng.standard_normal((n, d)) * np.sqrt(rng.uniform(0.5, 2.0, d))
    x += np.outer(rng.standard_normal(n) * 20.0, u[0]) + np.outer(rng.standard_normal(n) * 10.0, u[1])
    x += rng.standard_normal(d)
    return x.astype(np.float32)


def input_digest(X):
    """a few float64 numbers that pin a regenerated input to the one the fixture was made from"""
    X = np.asarray(X, np.float64)
    return np.array([X.sum(), np.abs(X).sum(), X[::7, ::5].sum(), X[-1, -1]])


def truth_pca(X, nc):
    """float64 throughout: centring, covariance, eigh, the same order and sign rule, the projection"""
    X = np.asarray(X, np.float64)
    n = X.shape[0]
    xc = X - X.mean(axis=0)
    cov = xc.T @ xc / (n - 1)
    comp, ev, evr, sv = top_components(cov, n, nc)
    return {"transform": xc @ comp.T, "components_": comp, "explained_variance_": ev, "explained_variance_ratio_": evr,
            "singular_values_": sv}


def deviations(got, truth):
    """quantity -> max |got - truth| relative to the truth's largest magnitude (transform: max |Y_truth|; components_ and
    the three variance vectors: their own maximum)"""
    out = {}
    for q in QUANTITIES:
        t = np.asarray(truth[q], np.float64)
        out[q] = float(np.abs(np.asarray(got[q], np.float64) - t).max() / np.abs(t).max())
    return out


def pooled(dev):
    """the three kinds a bound is kept for: the transform, the components, the three variance vectors together"""
    return {"transform": dev["transform"], "components_": dev["components_"],
            "variances": max(dev["explained_variance_"], dev["explained_variance_ratio_"], dev["singular_values_"])}


# ---- the fixture tests/golden/reference_pca.npz (tests/golden/make_pca_golden.py) -------------------------------
FACTOR = 8.0  # a deviation may be this many times the reference's own


def load_golden():
    from pathlib import Path
    with np.load(Path(__file__).resolve().parent / "golden" / "reference_pca.npz") as f:
        return {name: f[name] for name in f.files}


def case_arrays(golden, n, d, who):
    """who: truth, fit1, fit2 (sklearn's two fits), offset_truth"""
    return {q: golden[f"{case_name(n, d)}_{who}_{q}"] for q in QUANTITIES}


def case_input(golden, n, d):
    X = planted_input(n, d, int(golden[f"{case_name(n, d)}_seed"]))
    assert np.array_equal(input_digest(X), golden[f"{case_name(n, d)}_digest"]), "the regenerated input is not the fixture's"
    return X


def sklearn_bound(golden):
    """kind -> FACTOR x the largest deviation from the truth of sklearn's two fits over all cases"""
    worst = {}
    for n, d in CASES:
        truth = case_arrays(golden, n, d, "truth")
        for fit in ("fit1", "fit2"):
            for kind, v in pooled(deviations(case_arrays(golden, n, d, fit), truth)).items():
                worst[kind] = max(worst.get(kind, 0.0), v)
    return {kind: FACTOR * v for kind, v in worst.items()}
