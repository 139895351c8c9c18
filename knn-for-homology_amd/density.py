"""The slice of ``scipy.stats`` and of pandas' ``plot.density`` the reference uses, on the GPU.

pfam/reverse_evaluate.py:63-70, 113-118, 139-142 draws ``DataFrame({...}).plot.density()`` over the first principal
component and over the raw embedding dimensions with the largest loadings; pandas turns every column into
``scipy.stats.gaussian_kde(column).evaluate(grid)`` on a 1000-point grid.  Swap the import, or ask for the curves of all
columns in one call::

    from knn_for_homology_amd.density import gaussian_kde       # was: from scipy.stats import gaussian_kde
    grids, densities = density_curves({"original": a[:, 0], "reversed": b[:, 0]})   # what plot.density draws

The statistics (minimum, maximum, mean, ddof=1 variance) and the n x m exponentials are GPU passes (``knn_kde_stats`` /
``knn_kde_eval``; their arithmetic contract is in include/knn355.h); the factor, the bandwidth h = sqrt(var) * factor,
the normalisation and the grid are a few float64 numpy statements on the host between the two.

One-dimensional data only.  Not here: multivariate estimates, weights, the dropping of NaNs that pandas does in front
of scipy (a NaN is refused), a callable ``bw_method``, ``set_bandwidth``, ``integrate_*``, ``resample``, a
device-resident hand-off from ``PCA.transform``, several GPUs.
"""
import math

import numpy as np

from . import _lib

MAX_COLS = 4096           # KNN_KDE_MAX_COLS
MAX_ROWS = 65535 * 16384  # KNN_KDE_MAX_ROWS
MAX_POINTS = 1 << 24      # KNN_KDE_MAX_POINTS


def _factor(n, bw_method):
    if bw_method is None or (isinstance(bw_method, str) and bw_method == "scott"):
        return float(n) ** (-1.0 / 5.0)
    if isinstance(bw_method, str) and bw_method == "silverman":
        return (float(n) * 3.0 / 4.0) ** (-1.0 / 5.0)
    if isinstance(bw_method, str) or callable(bw_method) or isinstance(bw_method, bool) or not np.isscalar(bw_method):
        raise ValueError("bw_method must be None, 'scott', 'silverman' or a positive scalar")
    factor = float(bw_method)
    if not (math.isfinite(factor) and factor > 0.0):
        raise ValueError(f"the bandwidth factor must be positive and finite, not {bw_method}")
    return factor


def _rows(X):
    """X [n, c] as the C entries read it: float32 or float64, columns adjacent, rows a whole number of elements apart;
    a view that already is (a column block of a C-order matrix) is passed as it lies, anything else is converted"""
    X = np.asarray(X)
    if X.dtype not in (np.float32, np.float64):
        X = X.astype(np.float64)
    item = X.dtype.itemsize
    n, c = X.shape
    if n > 1 and not ((c == 1 or X.strides[1] == item) and X.strides[0] >= c * item and X.strides[0] % item == 0 and X.dtype.isnative
                      and X.ctypes.data % item == 0):
        X = np.ascontiguousarray(X)
    if n < 2:
        raise ValueError(f"the dataset needs 2 values at least, not {n}")
    if n > MAX_ROWS:
        raise ValueError(f"the dataset has more than {MAX_ROWS} values")
    if c < 1 or c > MAX_COLS:
        raise ValueError(f"need 1 to {MAX_COLS} columns, not {c}")
    if not np.isfinite(X).all():
        raise ValueError("the dataset holds a NaN or an infinity (NaNs are not dropped the way pandas drops them)")
    return X


def _call_args(X):
    return X.ctypes.data, int(X.dtype == np.float64), X.shape[0], X.shape[1], X.strides[0] // X.dtype.itemsize


def _stats(X):
    """(min, max, mean, var ddof=1) float64 [c] of the columns of X, as knn_kde_stats defines them"""
    out = np.empty((4, X.shape[1]), np.float64)
    _lib.check(_lib.lib().knn_kde_stats(*_call_args(X), *(row.ctypes.data for row in out)))
    return out


def _scales(var, n, factor):
    """(1 / h, 1 / (n h sqrt(2 pi))) of one column"""
    if not var > 0.0:
        raise ValueError("the dataset has zero variance: every value is the same")
    h = math.sqrt(float(var)) * factor
    inv_h, norm = 1.0 / h, 1.0 / (float(n) * h * math.sqrt(2.0 * math.pi))
    if not (math.isfinite(inv_h) and inv_h > 0.0 and math.isfinite(norm) and norm > 0.0):
        raise ValueError("the bandwidth is not a positive finite number")
    return inv_h, norm


def _evaluate(X, grids, inv_h, norm):
    """float64 [c, m]: column j of X at grids[j], as knn_kde_eval defines it"""
    grids = np.ascontiguousarray(grids, np.float64)
    c, m = grids.shape
    if m < 1:
        raise ValueError("need one grid point at least")
    if m > MAX_POINTS:
        raise ValueError(f"more than {MAX_POINTS} grid points")
    if not np.isfinite(grids).all():
        raise ValueError("the grid holds a NaN or an infinity")
    inv_h = np.ascontiguousarray(inv_h, np.float64)
    norm = np.ascontiguousarray(norm, np.float64)
    out = np.empty((c, m), np.float64)
    _lib.check(_lib.lib().knn_kde_eval(*_call_args(X), grids.ctypes.data, m, inv_h.ctypes.data, norm.ctypes.data, out.ctypes.data))
    return out


def last_ms():
    """{upload, stats, eval} of this thread's last statistics and evaluation calls, HIP-event milliseconds
    (tools/bench_kde.py); upload is the sum of the two calls' uploads, eval the evaluation kernel plus its reduce"""
    s = (_lib.c_float * 2)()
    e = (_lib.c_float * 3)()
    _lib.check(_lib.lib().knn_kde_last_ms(s, e))
    return {"upload": float(s[0]) + float(e[0]), "stats": float(s[1]), "eval": float(e[1]) + float(e[2])}


class gaussian_kde:
    """``scipy.stats.gaussian_kde(dataset, bw_method)`` for one-dimensional data.

    dataset is a 1-D float32 or float64 array (anything else is converted to float64); a strided column view such as
    ``Y[:, 0]`` of a C-order matrix is read where it lies and not copied on the host (the call uploads the rows it
    spans).  bw_method is None or "scott" (factor n**(-1/5)), "silverman" ((n*3/4)**(-1/5)) or a positive scalar factor.
    Attributes: ``n``, ``d`` (1), ``factor``, ``covariance`` ([[var(ddof=1) * factor**2]], float64), ``dataset``
    ([1, n], a view of the input).  ValueError, before any GPU work: fewer than 2 values, more than 1-D data, a NaN or an
    infinity, a factor that is not positive and finite, and zero variance (where scipy raises numpy.linalg.LinAlgError
    from its Cholesky factorisation)."""

    def __init__(self, dataset, bw_method=None):
        x = np.asarray(dataset)
        if x.ndim != 1:
            raise ValueError(f"the dataset must be 1-D, not {x.ndim}-D (multivariate estimates are not supported)")
        self._rows = _rows(x.reshape(len(x), 1))  # (a view of a view: no copy)
        self.n, self.d = len(x), 1
        self.factor = _factor(self.n, bw_method)
        self._min, self._max, self._mean, self._var = (float(v[0]) for v in _stats(self._rows))
        self._inv_h, self._norm = _scales(self._var, self.n, self.factor)
        self.covariance = np.array([[self._var * self.factor ** 2]], np.float64)
        self.dataset = self._rows.T

    def evaluate(self, points):
        """float64 [m]: the estimated density at points (1-D, or scipy's [1, m])"""
        points = np.asarray(points, np.float64)
        if points.ndim == 2 and points.shape[0] == 1:
            points = points[0]
        if points.ndim != 1:
            raise ValueError("points must be 1-D")
        return _evaluate(self._rows, points[None, :], [self._inv_h], [self._norm])[0]

    __call__ = evaluate


def _grid(lo, hi, m, dtype):
    # pandas 2.3.3, KdePlot._get_ind, on scalars of the column's dtype as numpy.nanmin / nanmax return them there (for a
    # float32 column numpy >= 2 keeps the expression and linspace in float32; the widening afterwards is exact)
    lo, hi = dtype.type(lo), dtype.type(hi)
    sample_range = hi - lo
    return np.linspace(lo - 0.5 * sample_range, hi + 0.5 * sample_range, m).astype(np.float64)


def density_curves(columns, ind=None, bw_method=None):
    """What ``DataFrame(columns).plot.density(ind=ind, bw_method=bw_method)`` draws: (grids [c, m], densities [c, m]),
    float64, for a 2-D [n, c] array or a dict of equal-length 1-D columns (in the dict's order), all columns in one
    library call.

    ind None or an integer m (default 1000): per column the grid
    ``numpy.linspace(min - 0.5 * (max - min), max + 0.5 * (max - min), m)``, evaluated in the column's dtype as pandas
    does.  An array ind is the grid of every column.  ValueError as for gaussian_kde, and for m < 1."""
    if isinstance(columns, dict):
        cols = [np.asarray(v) for v in columns.values()]
        if not cols or any(v.ndim != 1 or len(v) != len(cols[0]) for v in cols):
            raise ValueError("columns must be a non-empty dict of 1-D arrays of one length")
        dtype = np.float32 if all(v.dtype == np.float32 for v in cols) else np.float64
        X = np.stack(cols, axis=1).astype(dtype, copy=False)
    else:
        X = np.asarray(columns)
        if X.ndim != 2:
            raise ValueError("columns must be a 2-D [n, c] array or a dict of 1-D columns")
    X = _rows(X)
    n, c = X.shape
    factor = _factor(n, bw_method)
    if ind is None or (isinstance(ind, (int, np.integer)) and not isinstance(ind, bool)):
        m = 1000 if ind is None else int(ind)
        if m < 1:
            raise ValueError(f"need one grid point at least, not {m}")
        if m > MAX_POINTS:
            raise ValueError(f"more than {MAX_POINTS} grid points")
        explicit = None
    else:
        explicit = np.asarray(ind, np.float64)
        if explicit.ndim != 1 or len(explicit) < 1:
            raise ValueError("ind must be None, an integer or a 1-D array with one point at least")
        if not np.isfinite(explicit).all():
            raise ValueError("the grid holds a NaN or an infinity")
    mn, mx, _, var = _stats(X)
    scales = [_scales(v, n, factor) for v in var]
    if explicit is None:
        grids = np.stack([_grid(mn[j], mx[j], m, X.dtype) for j in range(c)])
    else:
        grids = np.broadcast_to(explicit, (c, len(explicit)))
    grids = np.ascontiguousarray(grids, np.float64)
    return grids, _evaluate(X, grids, [s[0] for s in scales], [s[1] for s in scales])
