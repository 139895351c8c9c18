"""Host restatement of the windowed statistics (knn_eval_windows in include/knn355.h; evaluation.rolling_means,
even_bins, edge_bins): numpy only, on the stable order of tests/rank_reference.py.  test_windows_reference.py checks
this file against what the reference's own statements produced (tests/golden/reference_windows.npz);
test_windows_gpu.py checks the device against this file, bit for bit."""
import numpy as np

import rank_reference as rr


def as_keys(keys):
    """the keys as the product takes them: flattened row by row; integers become float64"""
    keys = np.asarray(keys)
    if keys.dtype.kind in "iu":
        keys = keys.astype(np.float64)
    return keys.reshape(-1)


def columns(values, n):
    """bool [M, N]"""
    if values is None or len(values) == 0:
        return np.zeros((0, n), bool)
    return np.stack([np.asarray(v).reshape(-1) != 0 for v in values])


def running_counts(keys, values, descending=False):
    """-> (C int64 [M, N], order int64 [N]): C[c, r] = set cells of column c among the ranks 0 .. r"""
    keys = as_keys(keys)
    o = rr.order(keys, None, descending)
    return np.cumsum(columns(values, keys.size)[:, o], axis=1, dtype=np.int64), o


def value_means(C, window):
    """(C_c(i + W - 1) - C_c(i - 1)) / W: one float64 division of two exact integers"""
    before = np.concatenate([np.zeros((C.shape[0], 1), np.int64), C[:, :C.shape[1] - window]], axis=1)
    return (C[:, window - 1:] - before) / np.float64(window)


def chains(x, window):
    """-> (P, S) float64 [N]: per block of `window` ranks the forward and the backward chain of sequential additions.
    numpy.cumsum adds sequentially along the axis of the [blocks, W] reshape and starts with the first element itself."""
    x = np.asarray(x, np.float64)
    n = x.size
    full = n // window * window
    P, S = np.empty(n), np.empty(n)
    with np.errstate(invalid="ignore", over="ignore"):
        body = x[:full].reshape(-1, window)
        P[:full] = np.cumsum(body, axis=1).reshape(-1)
        S[:full] = np.cumsum(body[:, ::-1], axis=1)[:, ::-1].reshape(-1)
        P[full:] = np.cumsum(x[full:])
        S[full:] = np.cumsum(x[full:][::-1])[::-1]
    return P, S


def key_means(keys, window, descending=False):
    keys = as_keys(keys)
    x = keys[rr.order(keys, None, descending)].astype(np.float64)
    P, S = chains(x, window)
    i = np.arange(x.size - window + 1)
    with np.errstate(invalid="ignore", over="ignore"):
        return np.where(i % window == 0, P[i + window - 1], S[i] + P[i + window - 1]) / np.float64(window)


def rolling_means(keys, values, window, descending=False):
    """-> (key means float64 [N - W + 1], column means float64 [M, N - W + 1], order)"""
    C, o = running_counts(keys, values, descending)
    return key_means(keys, window, descending), value_means(C, window), o


def finish(start, stop, counts):
    """mean and standard error of every bin from its exact counts, in float64; nan, silently, for an empty bin"""
    n = (stop - start).astype(np.float64)
    c = counts.astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = c / n
        stderr = np.sqrt((c * (1 - mean) * (1 - mean) + (n - c) * mean * mean) / n) / np.sqrt(n)
    return mean, stderr


def counts_in(C, start, stop):
    at = lambda r: np.where(r > 0, C[:, np.maximum(r - 1, 0)], 0)
    return at(stop) - at(start)


def even_bins(keys, values, bins, descending=False):
    """-> dict(start, stop, counts, mean, stderr, key_lo, key_hi): hist_evenly's slices of the ranked order"""
    k = as_keys(keys)
    C, o = running_counts(keys, values, descending)
    cuts = k.size * np.arange(bins + 1, dtype=np.int64) // (bins + 1)
    start, stop = cuts[:-1], cuts[1:]
    counts = counts_in(C, start, stop)
    mean, stderr = finish(start, stop, counts)
    return dict(start=start, stop=stop, counts=counts, mean=mean, stderr=stderr, key_lo=k[o[start]], key_hi=k[o[np.minimum(stop, k.size - 1)]])


def edge_bins(keys, values, edges):
    """-> the same dict for edges[i] <= key < edges[i + 1], the last bin open above; NaN keys in no bin"""
    k = as_keys(keys)
    C, o = running_counts(keys, values, False)
    e = np.asarray(edges, np.float64).astype(k.dtype)
    s = k[o]
    finite = int(np.count_nonzero(~np.isnan(s)))  # NaN ranks last
    start = np.searchsorted(s[:finite], e, side="left").astype(np.int64)
    stop = np.append(start[1:], finite).astype(np.int64)
    counts = counts_in(C, start, stop)
    mean, stderr = finish(start, stop, counts)
    return dict(start=start, stop=stop, counts=counts, mean=mean, stderr=stderr, key_lo=e, key_hi=np.append(e[1:], np.asarray(np.inf, k.dtype)))
