"""Weighted mixes of embedding layers, made, searched and scored on the device.

Reference call sites (konstin/knn-for-homology):
  cath/compare_seqvec_layer.py:44-56   ratio[0] * cnn + ratio[1] * lstm1 + ratio[2] * lstm2 per point of a simplex grid
  cath/compare_seqvec_layer.py:58-91   each mix through cath.search.search, of which is_correct[:, 3, 0].mean() is kept
  seqvec_search/figures/layers.py:37-47, lstm1_vs_sum.py   sums, differences and column blocks of one [N, 3072] matrix

The layers go up once (``LayerMix``); a mix is written straight into the rows of a flat index (mix_rows_kernel), searched
where it lies and scored there, and a sweep brings back ``[G, levels]`` integers.  A mix has the bits of numpy's statement
on float32 arrays with float32 weights -- which is what the reference computes under numpy 1.x, whose value-based casting
turns the float64 scalars of its grid into float32 before they meet a float32 array.  The weights are cast to float32 here
by hand, so the numpy in use does not matter.
"""
import ctypes
from typing import NamedTuple, Optional

import numpy as np
from numpy import ndarray

from . import _lib
from .faiss import METRIC_INNER_PRODUCT, IndexFlat

MAX_LAYERS = 4  # KNN_MIX_MAX_LAYERS
MAX_LEVELS = 8  # KNN_MIX_MAX_LEVELS


def simplex_ratios(granularity: int, layers: int = 3) -> ndarray:
    """float64 [G, layers]: the points of the grid linspace(0, 1, granularity) ** layers whose coordinates sum to 1 under
    numpy.isclose, the first coordinate varying slowest -- the grid, the order and the filter of
    cath/compare_seqvec_layer.py:44-47 (15 / 66 / 231 rows for granularity 5 / 11 / 21 and three layers)."""
    axis = np.linspace(0, 1, int(granularity))
    grid = np.stack(np.meshgrid(*([axis] * int(layers)), indexing="ij"), axis=-1).reshape(-1, int(layers))
    return grid[np.isclose(grid.sum(axis=1), 1)]


class LayerSweep(NamedTuple):
    counts: ndarray            # int64 [G, levels] ([G] for one level): rows whose scored hit shares their label
    means: ndarray             # float64, counts / N: numpy's .mean() of the bool column, exactly
    hits: Optional[ndarray]    # int64 [G, N, hits] with the self column dropped (want_hits), else None
    scores: Optional[ndarray]  # float32 [G, N, hits]


def _is_device(x):
    return hasattr(x, "data_ptr") and getattr(x, "is_cuda", False)


class LayerMix:
    """``layers``: a sequence of L <= 4 float32 ``[N, d]`` arrays, or one ``[N, L * d]`` array with ``d`` given (its column
    blocks are the layers, as in figures/layers.py).  numpy arrays are uploaded once; torch tensors on the GPU are used
    where they lie, whatever their row stride, and are kept alive by this object."""

    def __init__(self, layers, metric=METRIC_INNER_PRODUCT, d=None):
        self._h = ctypes.c_void_p()
        if isinstance(layers, np.ndarray) or _is_device(layers):
            if layers.ndim != 2 or d is None or layers.shape[1] % int(d):
                raise ValueError("one array of layers must be [N, L * d], with d given")
            views = [layers[:, i * int(d):(i + 1) * int(d)] for i in range(layers.shape[1] // int(d))]
        else:
            views = list(layers)
        if not 1 <= len(views) <= MAX_LAYERS:
            raise ValueError(f"1 .. {MAX_LAYERS} layers, not {len(views)}")
        shape = tuple(views[0].shape)
        if len(shape) != 2 or any(tuple(v.shape) != shape for v in views):
            raise ValueError("every layer must be [N, d], all of one shape")
        self._n, self._d, self._metric = int(shape[0]), int(shape[1]), int(metric)
        self._keep = views  # (device layers are borrowed, not copied)
        L = _lib.lib()
        _lib.check(L.knn_mix_create(self._d, len(views), ctypes.byref(self._h)))
        for i, v in enumerate(views):
            if _is_device(v):
                import torch
                if v.dtype != torch.float32 or v.stride(1) != 1:
                    raise TypeError("a device layer must be float32 with unit column stride")
                torch.cuda.synchronize(v.device)  # (the rows are complete before the first mix reads them)
                _lib.check(L.knn_mix_set_layer_dev(self._h, i, v.data_ptr(), self._n, v.stride(0), None))
            else:
                if not isinstance(v, np.ndarray) or v.dtype != np.float32:
                    raise TypeError("a layer must be a float32 numpy.ndarray (or a torch tensor on the GPU)")
                if v.strides[1] != 4 or v.strides[0] % 4 or v.strides[0] < 4 * self._d:
                    v = np.ascontiguousarray(v)
                _lib.check(L.knn_mix_set_layer(self._h, i, v.ctypes.data, self._n, v.strides[0] // 4))
        self._nlayers = len(views)
        self._flat = IndexFlat(self._d, self._metric)

    @property
    def d(self):
        return self._d

    @property
    def ntotal(self):
        return self._n

    @property
    def nlayers(self):
        return self._nlayers

    def _weights(self, weights, rows=None):
        w = np.ascontiguousarray(np.asarray(weights, dtype=np.float64).astype(np.float32))  # the cast numpy 1.x makes by value
        want = (self._nlayers,) if rows is None else (w.shape[0] if w.ndim == 2 else -1, self._nlayers)
        if w.shape != want:
            raise ValueError(f"weights must have {self._nlayers} entries per mix, got shape {w.shape}")
        return w

    def index(self, weights) -> IndexFlat:
        """The IndexFlat that holds the mix (normalised rows for the inner product, as cath.search.search stores them).  It
        is this object's one index: the next mix replaces its rows."""
        w = self._weights(weights)
        _lib.check(_lib.lib().knn_mix_into(self._h, w.ctypes.data, self._flat._h, 1 if self._metric == METRIC_INNER_PRODUCT else 0))
        return self._flat

    def search(self, weights, hits: int = 10):
        """``cath.search.search(mix, hits)``: ``(hits int64 [N, hits], scores float32 [N, hits])``, the self column dropped."""
        scores, neighbours = self.index(weights).search_self(int(hits) + 1)
        return neighbours[:, 1:], scores[:, 1:]

    def sweep(self, ratios, mapping_array, hits: int = 1, level: Optional[int] = None, want_hits: bool = False) -> LayerSweep:
        """Every row of ``ratios`` ([G, L]) mixed, searched for ``hits`` neighbours and scored: counts[g][l] = rows whose first
        hit behind the self column shares their label at level l of ``mapping_array`` ([N, levels], any dtype), which is
        ``compute_is_correct(search(mix))[:, l, 0].sum()``.  ``level``: score that level alone (counts and means are [G])."""
        w = self._weights(ratios, rows=True)
        G, k = w.shape[0], int(hits) + 1
        mapping = np.asarray(mapping_array)
        if mapping.ndim != 2 or mapping.shape[0] != self._n:
            raise ValueError(f"mapping_array must be [{self._n}, levels]")
        if level is not None:
            mapping = mapping[:, [int(level)]]
        # arbitrary label values -> dense int32 codes per level (equality is all that matters)
        codes = np.empty(mapping.shape, np.int32)
        for l in range(mapping.shape[1]):
            _, codes[:, l] = np.unique(mapping[:, l], return_inverse=True)
        counts = np.zeros((G, mapping.shape[1]), np.int64)
        D = _lib.result_array((G, self._n, k), np.float32) if want_hits else None
        I = _lib.result_array((G, self._n, k), np.int64) if want_hits else None
        _lib.check(_lib.lib().knn_mix_sweep(self._h, w.ctypes.data, G, self._flat._h, k, codes.ctypes.data, codes.shape[1], 1, counts.ctypes.data,
                                            D.ctypes.data if want_hits else None, I.ctypes.data if want_hits else None))
        if level is not None:
            counts = counts[:, 0]
        means = counts.astype(np.float64) / np.float64(self._n)
        return LayerSweep(counts, means, I[:, :, 1:] if want_hits else None, D[:, :, 1:] if want_hits else None)

    def last_ms(self):
        """HIP-event milliseconds of this thread's last sweep, summed over its mixes: {"mix", "search", "score"}"""
        a, b, c = ctypes.c_float(), ctypes.c_float(), ctypes.c_float()
        _lib.check(_lib.lib().knn_mix_last_ms(ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)))
        return {"mix": a.value, "search": b.value, "score": c.value}

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            try:
                _lib.lib().knn_mix_free(h)
            except Exception:
                pass
            self._h = None
