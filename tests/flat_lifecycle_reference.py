"""Host model of one flat index handle and its views, for tests/test_flat_lifecycle_gpu.py and
tests/test_flat_lifecycle_reference.py: plain numpy plus the CPU oracle, nothing of the library under test.

The model's state is the parent's rows (float32 [n][d]) and row capacity, and per view the row count at its creation and
whether it is alive or stale.  Its rules restate the storage rules of csrc/flat_index.inc
(knn_flat_reserve: flat_info.inc, knn_flat_normalize_rows: flat_search.inc):

  add(x)            grow_index -> move_storage: the first add (capacity 0) fits exactly; a later add beyond the
                    capacity grows to max(need, cap + cap // 2); storage that moves (there was some: capacity > 0) makes
                    every view stale (move_storage bumps storage_gen); an add that fits leaves the views alive with their old row count.
  reserve(n)        knn_flat_reserve -> move_storage: beyond the capacity the capacity becomes exactly n and the views go
                    stale (again only if there was storage to move); otherwise nothing happens.
  reset()           knn_reset -> free_index_buffers: no rows, capacity 0, every view stale.
  free()            knn_free -> free_index_buffers: the same, and the parent is gone.
  normalize_rows()  knn_flat_normalize_rows: the rows become oracle.normalize_l2 of themselves, in place: live
                    views see the new values of their first n rows (storage is shared and does not move).
  view(of)          knn_flat_view: of the parent, or of a live view (the same rows, stale together with it,
                    which here is: with every other view); of a stale view it is refused (Refused).

Expected answers are the oracle's on the model's rows: flat_search with FAISS's batch rule for `search` and for a window
of own rows, the range expectation read off the oracle's full ranking (expected_range; test_range_search_gpu.py imports
it from here), refine_reference.ref_refine for given labels, pair_distances for knn_gather_distances."""
import numpy as np

from refine_reference import ref_refine

IP, L2 = 0, 1
FLT_MAX = np.float32(np.finfo(np.float32).max)


class Refused(Exception):
    """the library is expected to refuse this call (KNN_ERR_INVALID)"""


def better(D, r, metric):
    return D > np.float32(r) if metric == IP else D < np.float32(r)


def expected_range(oracle, xb, xq, r, metric, l2_mode=0):
    """(lims, D, I) from the oracle's full ranking"""
    D, I = oracle.flat_search(xb, xq, xb.shape[0], metric, l2_mode=l2_mode)
    lims, Ds, Is = [0], [], []
    for q in range(xq.shape[0]):
        keep = (I[q] >= 0) & better(D[q], r, metric)
        ids, d = I[q][keep], D[q][keep]
        o = np.argsort(ids, kind="stable")
        Is.append(ids[o])
        Ds.append(d[o])
        lims.append(lims[-1] + int(keep.sum()))
    cat = lambda parts, dt: np.concatenate(parts).astype(dt) if parts else np.zeros(0, dt)
    return np.array(lims, np.uint64), cat(Ds, np.float32), cat(Is, np.int64)


def radius_for(oracle, xb, xq, metric, frac):
    """a radius that about `frac` (0 < frac < 1) of the (query, row) pairs beat"""
    D, I = oracle.flat_search(xb, xq, xb.shape[0], metric)
    v = np.sort(D[I >= 0].ravel())
    return np.float32(v[int((1 - frac) * (len(v) - 1))] if metric == IP else v[int(frac * (len(v) - 1))])


class ViewModel:
    def __init__(self, n):
        self.n = n          # rows at creation
        self.alive = True


class FlatModel:
    def __init__(self, oracle, d, metric):
        self.oracle, self.d, self.metric = oracle, d, metric
        self.rows = np.zeros((0, d), np.float32)
        self.cap = 0
        self.freed = False
        self.views = []

    # ---- state -------------------------------------------------------------------------------------------------------
    @property
    def n(self):
        return self.rows.shape[0]

    def _moved(self):
        for v in self.views:
            v.alive = False

    def add(self, x):
        assert not self.freed and x.dtype == np.float32 and x.ndim == 2 and x.shape[1] == self.d
        if x.shape[0] == 0:
            return
        need = self.n + x.shape[0]
        if need > self.cap:
            if self.cap > 0:
                self._moved()
                self.cap = max(need, self.cap + self.cap // 2)
            else:
                self.cap = need
        self.rows = np.concatenate([self.rows, x], 0)

    def reserve(self, n):
        assert not self.freed
        if n <= self.cap:
            return
        if self.cap > 0:
            self._moved()
        self.cap = n

    def reset(self):
        assert not self.freed
        self._moved()
        self.rows = np.zeros((0, self.d), np.float32)
        self.cap = 0

    def free(self):
        self.reset()
        self.freed = True

    def normalize_rows(self):
        assert not self.freed
        rows = np.ascontiguousarray(self.rows.copy())
        if rows.shape[0]:
            self.oracle.normalize_l2(rows)
        self.rows = rows

    def view(self, of=None):
        """of: None = the parent, or a ViewModel"""
        assert not self.freed or of is not None
        if of is not None and not of.alive:
            raise Refused("view of a stale view")
        v = ViewModel(self.n if of is None else of.n)
        self.views.append(v)
        return v

    def drop(self, v):
        self.views.remove(v)

    def rows_of(self, v=None):
        """the rows a handle serves: the parent's (v None) or a live view's"""
        if v is None:
            assert not self.freed
            return self.rows
        if not v.alive:
            raise Refused("stale view")
        return self.rows[:v.n]

    # ---- expected answers on given rows ----------------------------------------------------------------------------
    def _pads(self, nq, k):
        return (np.full((nq, k), -FLT_MAX if self.metric == IP else FLT_MAX, np.float32), np.full((nq, k), -1, np.int64))

    def search(self, rows, xq, k):
        if rows.shape[0] == 0:
            return self._pads(xq.shape[0], k)
        return self.oracle.flat_search(rows, xq, k, self.metric)

    def search_self(self, rows, row0, nrows, k):
        return self.search(rows, np.ascontiguousarray(rows[row0:row0 + nrows]), k)

    def range_search(self, rows, xq, r):
        if rows.shape[0] == 0:
            return np.zeros(xq.shape[0] + 1, np.uint64), np.zeros(0, np.float32), np.zeros(0, np.int64)
        return expected_range(self.oracle, rows, xq, r, self.metric)

    def range_search_self(self, rows, row0, nrows, r):
        return self.range_search(rows, np.ascontiguousarray(rows[row0:row0 + nrows]), r)

    def refine(self, rows, xq, labels, k):
        return ref_refine(self.oracle, rows, xq, labels, k, self.metric)

    def gather(self, rows, xq, cand, offs):
        counts = np.diff(offs)
        qidx = np.repeat(np.arange(xq.shape[0]), counts).astype(np.int64)
        if qidx.size == 0:
            return np.zeros(0, np.float32)
        return self.oracle.pair_distances(rows, xq, qidx, cand, self.metric)
