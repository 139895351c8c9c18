"""The slice of ``sklearn.decomposition`` the reference uses, on the GPU.

pfam/reverse_evaluate.py:34-44, 100-108 runs ``PCA(n_components=2)`` over the concatenated forward and scrambled
embeddings and reads ``fit_transform``'s output, ``components_``, ``explained_variance_``, ``explained_variance_ratio_``
and ``singular_values_``.  Swap the import::

    from knn_for_homology_amd.decomposition import PCA     # was: from sklearn.decomposition import PCA

The mean, the d x d covariance (fp32 MFMA, float64 across row groups) and the projection are GPU passes
(``knn_pca_moments`` / ``knn_pca_project``; their arithmetic contract is in include/knn355.h); the eigen-solve of the
covariance is ``numpy.linalg.eigh`` in float64 on the host.  Rows are centred before any product is formed, so a large
common offset of the embeddings costs no accuracy.

Not here: a device eigen-solver, reuse of the uploaded rows between ``fit`` and ``transform`` (``fit_transform``
uploads twice), ``whiten``, ``inverse_transform``, other solvers and keywords, several GPUs.
"""
import numpy as np

from . import _lib

MAX_COMPONENTS = 32  # KNN_PCA_MAX_COMPONENTS
MAX_D = 2048         # KNN_PCA_MAX_D


def _rows(X, n_min):
    X = np.ascontiguousarray(X, np.float32)
    if X.ndim != 2:
        raise ValueError("X must be 2-D, [rows, d]")
    n, d = X.shape
    if n < n_min:
        raise ValueError(f"X needs {n_min} row(s) at least, not {n}")
    if d < 4 or d > MAX_D or d % 4:
        raise ValueError(f"d must be a multiple of 4 in [4, {MAX_D}], not {d}")
    return X


def moments(X):
    """(mean float32 [d], covariance float64 [d, d]) of the rows of X, as knn_pca_moments defines them"""
    X = _rows(X, 2)
    n, d = X.shape
    mean = np.empty(d, np.float32)
    cov = np.empty((d, d), np.float64)
    _lib.check(_lib.lib().knn_pca_moments(X.ctypes.data, n, d, mean.ctypes.data, cov.ctypes.data))
    return mean, cov


def project(X, mean, components):
    """float32 [n, nc]: the centred rows of X against the rows of components, as knn_pca_project defines it"""
    X = _rows(X, 1)
    n, d = X.shape
    mean = np.ascontiguousarray(mean, np.float32)
    components = np.ascontiguousarray(components, np.float32)
    if mean.shape != (d,):
        raise ValueError(f"mean must have shape ({d},), not {mean.shape}")
    if components.ndim != 2 or components.shape[1] != d:
        raise ValueError(f"components must be [nc, {d}], not {components.shape}")
    nc = components.shape[0]
    if nc < 1 or nc > min(MAX_COMPONENTS, d):
        raise ValueError(f"need 1 <= nc <= min(d, {MAX_COMPONENTS}), not {nc}")
    out = np.empty((n, nc), np.float32)
    _lib.check(_lib.lib().knn_pca_project(X.ctypes.data, n, d, mean.ctypes.data, components.ctypes.data, nc, out.ctypes.data))
    return out


def last_ms():
    """({upload, colsum, cov, reduce} of this thread's last moments(), the projection kernel of its last project()),
    HIP-event milliseconds (tools/bench_pca.py)"""
    m = (_lib.c_float * 4)()
    p = _lib.c_float()
    _lib.check(_lib.lib().knn_pca_last_ms(m, p))
    return dict(zip(("upload", "colsum", "cov", "reduce"), (float(v) for v in m))), float(p.value)


def components_from_covariance(cov, n_samples, n_components):
    """The host half of fit: (components float64 [nc, d], explained_variance, explained_variance_ratio,
    singular_values, all float64 [nc]) from the float64 covariance.  eigh, the top nc eigenpairs in descending order,
    every eigenvector flipped so that its largest-magnitude entry (the first one on ties) is positive: sklearn's
    svd_flip convention."""
    cov = np.asarray(cov, np.float64)
    w, v = np.linalg.eigh(cov)
    order = np.argsort(w, kind="stable")[::-1][:n_components]
    w_top = w[order]
    comp = v[:, order].T.copy()
    big = np.argmax(np.abs(comp), axis=1)
    comp *= np.where(comp[np.arange(comp.shape[0]), big] < 0, -1.0, 1.0)[:, None]
    ratio = w_top / np.trace(cov)
    singular = np.sqrt(w_top * (n_samples - 1))
    return comp, w_top, ratio, singular


class PCA:
    """``sklearn.decomposition.PCA(n_components)`` with 1 <= n_components <= 32; no other keyword is accepted.

    X is a host array [N, d], converted with ``np.ascontiguousarray(X, float32)`` and never modified: N >= 2, d a
    multiple of 4 with 4 <= d <= 2048, n_components <= min(N, d).  Anything else is a ValueError, raised before any
    GPU work; so is a non-finite covariance (a NaN or an infinity in X), raised before the eigen-solve.
    ``covariance_`` (float64 [d, d]) is kept beside sklearn's attributes."""

    def __init__(self, n_components):
        if isinstance(n_components, bool) or not isinstance(n_components, (int, np.integer)):
            raise ValueError("n_components must be an integer")
        if n_components < 1 or n_components > MAX_COMPONENTS:
            raise ValueError(f"n_components must be in [1, {MAX_COMPONENTS}], not {n_components}")
        self.n_components = int(n_components)

    def fit(self, X):
        X = _rows(X, 2)
        n, d = X.shape
        if self.n_components > min(n, d):
            raise ValueError(f"n_components={self.n_components} must be at most min(n_samples, d) = {min(n, d)}")
        mean, cov = moments(X)
        if not np.isfinite(cov).all():
            raise ValueError("the covariance is not finite: X holds a NaN or an infinity, or its values overflow float32")
        comp, var, ratio, singular = components_from_covariance(cov, n, self.n_components)
        self.mean_ = mean
        self.covariance_ = cov
        self.components_ = comp.astype(np.float32)
        self.explained_variance_ = var.astype(np.float32)
        self.explained_variance_ratio_ = ratio.astype(np.float32)
        self.singular_values_ = singular.astype(np.float32)
        self.n_samples_ = n
        self.n_components_ = self.n_components
        self.n_features_in_ = d
        return self

    def transform(self, X):
        if not hasattr(self, "components_"):
            raise ValueError("this PCA is not fitted yet: call fit first")
        return project(X, self.mean_, self.components_)

    def fit_transform(self, X):
        X = _rows(X, 2)
        return self.fit(X).transform(X)
