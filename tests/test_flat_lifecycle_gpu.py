"""GPU: the state a flat index handle carries between calls, against the host model of tests/flat_lifecycle_reference.py.
Every comparison is exact: ids, lims and the score bits.

check_all runs every query path of a handle (search in both squared-L2 forms and at k in {1, 10, ntotal + 3}, search_self
and range_search_self on a window that ends at the last row, range_search, knn_flat_refine, knn_gather_distances,
reconstruct, ntotal) against the model's rows; on a stale view every one of them must raise, with the output arrays of
reconstruct_into and knn_gather_distances left as they were (ntotal is a plain getter: it keeps the view's row count).

  (a) a scripted lifecycle whose row counts cross the 256-row tile ends, check_all after every step on the parent and on
      every view, alive or stale
  (b) seeded random sequences of add / reserve / reset / normalize_rows / view / view-of-view / drop
  (c) an index built in pool memory that a freed index filled with NaNs: padding columns, tail rows, the norms' tail and
      the scratch buffers (knn_trim's return value proves the victim really took pooled memory)
  (d) two streaming searches of one shape with something in between: the second must not inherit state it should not
      (LevelBufs::clean_sig), with and without KNN_TUNE_ALWAYS_RESET"""
import ctypes

import numpy as np
import pytest

from flat_lifecycle_reference import IP, L2, FlatModel, Refused, better, radius_for
from knn_for_homology_amd import _lib
from knn_for_homology_amd._lib import KNN_TUNE_ALWAYS_RESET, KNN_TUNE_NO_PAIRS, Knn355Error

pytestmark = pytest.mark.gpu

SENTINEL = np.float32(7.25)
_QUERIES = {}


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _queries(d):
    """the 5 (squared L2: difference form) and 33 (norm formula; leaves the 32-query tile) queries of dimension d"""
    if d not in _QUERIES:
        rng = np.random.default_rng(9000 + d)
        _QUERIES[d] = (rng.standard_normal((5, d)).astype(np.float32), rng.standard_normal((33, d)).astype(np.float32))
    return _QUERIES[d]


def _same_knn(got, want, what):
    (D, I), (wD, wI) = got, want
    assert D.dtype == np.float32 and I.dtype == np.int64 and D.shape == wD.shape and I.shape == wI.shape, what
    assert np.array_equal(I, wI), f"{what}: {int((I != wI).sum())} ids differ, first at {np.argwhere(I != wI)[:3].tolist()}"
    assert np.array_equal(_bits(D), _bits(wD)), f"{what}: {int((_bits(D) != _bits(wD)).sum())} scores differ"


def _same_range(got, want, what):
    (lims, D, I), (wl, wD, wI) = got, want
    assert lims.dtype == np.uint64 and D.dtype == np.float32 and I.dtype == np.int64, what
    assert np.array_equal(lims, wl), f"{what}: lims differ at {np.flatnonzero(lims != wl)[:5]}"
    assert np.array_equal(I, wI), f"{what}: {int((I != wI).sum())} ids differ"
    assert np.array_equal(_bits(D), _bits(wD)), f"{what}: {int((_bits(D) != _bits(wD)).sum())} scores differ"


def _refine(h, xq, labels, k):
    labels = np.ascontiguousarray(labels, np.int64)
    D = np.full((xq.shape[0], k), SENTINEL, np.float32)
    I = np.full((xq.shape[0], k), -7, np.int64)
    _lib.check(_lib.lib().knn_flat_refine(h._h, xq.ctypes.data, xq.shape[0], labels.ctypes.data, labels.shape[1], k, D.ctypes.data, I.ctypes.data))
    return D, I


def _gather(h, xq, cand, offs, out):
    cand = np.ascontiguousarray(cand, np.int64)
    offs = np.ascontiguousarray(offs, np.int64)
    _lib.check(_lib.lib().knn_gather_distances(h._h, xq.ctypes.data, xq.shape[0], cand.ctypes.data, offs.ctypes.data, out.ctypes.data))


def _labels(n, seed):
    """[5][6] labels with a -1, a repeat and the last row in every query, and a query without any candidate"""
    lab = np.random.default_rng(seed).integers(0, n, (5, 6)).astype(np.int64)
    lab[:, 0] = -1
    lab[:, 1] = lab[:, 2]
    lab[:, 3] = n - 1
    lab[4] = -1
    return lab


def _cands(n, seed):
    """candidate lists of 0, 1 and 70 rows for three queries; the last row is among them"""
    cand = np.random.default_rng(seed).integers(0, n, 71).astype(np.int64)
    cand[0] = n - 1
    cand[70] = n - 1
    return cand, np.array([0, 0, 1, 71], np.int64)


def check_all(h, model, rows, what):
    """every query path of a live handle against the model's `rows`"""
    n, d = rows.shape
    xq5, xq33 = _queries(d)
    assert h.ntotal == n, what
    assert np.array_equal(_bits(h.reconstruct_n(0, n)), _bits(rows)), f"{what}: reconstruct_n"
    for xq in (xq5, xq33):
        for k in (1, 10, n + 3):
            if k <= 2048:
                _same_knn(h.search(xq, k), model.search(rows, xq, k), f"{what}: search nq {xq.shape[0]} k {k}")
    if n == 0:
        _same_range(h.range_search(xq33, 0.0), model.range_search(rows, xq33, 0.0), f"{what}: range_search")
        _same_knn(_refine(h, xq5, np.full((5, 6), -1), 4), model.refine(rows, xq5, np.full((5, 6), -1), 4), f"{what}: refine")
        return
    row0 = max(0, n - 37)  # a window that ends at the last row
    _same_knn(h.search_self(10, row0, n - row0), model.search_self(rows, row0, n - row0, 10), f"{what}: search_self [{row0}, {n})")
    for xq in (xq5, xq33):  # a radius that about 5 % of the pairs beat
        r = radius_for(model.oracle, rows, xq, model.metric, 0.05)
        _same_range(h.range_search(xq, r), model.range_search(rows, xq, r), f"{what}: range_search nq {xq.shape[0]} r {r}")
    _same_range(h.range_search_self(r, row0, n - row0), model.range_search_self(rows, row0, n - row0, r), f"{what}: range_search_self [{row0}, {n}) r {r}")
    lab = _labels(n, n)
    _same_knn(_refine(h, xq5, lab, 4), model.refine(rows, xq5, lab, 4), f"{what}: refine")
    cand, offs = _cands(n, n + 1)
    out = np.full(71, SENTINEL, np.float32)
    _gather(h, xq5[:3], cand, offs, out)
    assert np.array_equal(_bits(out), _bits(model.gather(rows, xq5[:3], cand, offs))), f"{what}: gather_distances"
    out1 = np.full(1, SENTINEL, np.float32)
    _gather(h, xq5[1:2], cand[:1], np.array([0, 1], np.int64), out1)  # a one-element list: the pair of query 1 above
    assert _bits(out1)[0] == _bits(out)[0], f"{what}: gather_distances of one pair"
    _gather(h, xq5[:1], cand[:0], np.zeros(2, np.int64), out1)        # an empty list
    assert _bits(out1)[0] == _bits(out)[0], f"{what}: gather_distances of nothing wrote something"


def check_stale(h, d, what):
    """every query path of a stale view raises before anything is copied or launched"""
    xq5, xq33 = _queries(d)
    n = h.ntotal  # (a plain getter: the row count the view was made with)
    lab = np.zeros((5, 6), np.int64)
    out = np.full(71, SENTINEL, np.float32)
    rec = np.full((1, d), SENTINEL, np.float32)
    ms, nbytes = ctypes.c_float(-3.0), ctypes.c_int64(-3)
    cand, offs = np.zeros(71, np.int64), np.array([0, 0, 1, 71], np.int64)
    calls = {
        "search nq 5": lambda: h.search(xq5, 1),
        "search nq 33": lambda: h.search(xq33, 10),
        "search k ntotal + 3": lambda: h.search(xq5, min(n + 3, 2048)),
        "search_self": lambda: h.search_self(10, 0, 1),
        "range_search": lambda: h.range_search(xq33, 0.0),
        "range_search_self": lambda: h.range_search_self(0.0, 0, 1),
        "refine": lambda: _refine(h, xq5, lab, 4),
        "gather_distances of nothing": lambda: _gather(h, xq5[:1], cand[:0], np.zeros(2, np.int64), out),
        "gather_distances of one pair": lambda: _gather(h, xq5[:1], cand[:1], np.array([0, 1], np.int64), out),
        "gather_distances": lambda: _gather(h, xq5[:3], cand, offs, out),
        "reconstruct_n": lambda: h.reconstruct_n(0, n),
        "reconstruct_into": lambda: h.reconstruct_into(rec, 0),
        "read_rate": lambda: _lib.check(_lib.lib().knn_flat_read_rate(h._h, 1, ctypes.byref(ms), ctypes.byref(nbytes))),
        "view": lambda: h.view(),
    }
    for name, call in calls.items():
        try:
            call()
        except Knn355Error as e:
            assert "stale" in str(e), f"{what}: {name} on a stale view: {e}"
        else:
            raise AssertionError(f"{what}: {name} on a stale view did not raise")
    assert (out == SENTINEL).all() and (rec == SENTINEL).all(), f"{what}: a refused call wrote to its output"
    assert ms.value == -3.0 and nbytes.value == -3, f"{what}: a refused read_rate wrote to its output"


def check_handle(h, model, v, what):
    """v: the model's view behind h (None: h is the parent)"""
    if v is not None and not v.alive:
        check_stale(h, model.d, what)
    else:
        check_all(h, model, model.rows_of(v), what)


def _free_now(idx):
    """knn_free through the C ABI, now (the Python object must not free it again)"""
    _lib.lib().knn_free(idx._h)
    idx._h = None


# ---- (a) the scripted lifecycle ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [24, 40, 64, 100])  # dp 32, 64, 64 (no padding), 128
@pytest.mark.parametrize("metric", [IP, L2], ids=["ip", "l2"])
def test_scripted_lifecycle(gpu_faiss, oracle, metric, d):
    rng = np.random.default_rng(100 * d + metric)
    rows = lambda n: rng.standard_normal((n, d)).astype(np.float32) * np.float32(1.5)
    model = FlatModel(oracle, d, metric)
    idx = gpu_faiss.IndexFlat(d, metric)
    handles = {}  # name -> (handle, model view)
    state = {"step": "empty"}

    def check():
        if not model.freed:
            check_all(idx, model, model.rows, f"after '{state['step']}': parent")
        for name, (h, v) in handles.items():
            check_handle(h, model, v, f"after '{state['step']}': view {name}")

    def step(name, fn):
        state["step"] = name
        fn()
        check()

    def add(n):
        x = rows(n)
        idx.add(x)
        model.add(x)

    def view(name, of=None):
        handles[name] = (idx.view(), model.view()) if of is None else (handles[of][0].view(), model.view(of=handles[of][1]))

    def both(a, b):
        a()
        b()

    check()
    step("add 7", lambda: add(7))
    step("add 1", lambda: add(1))
    step("add 292 (growth)", lambda: add(292))
    assert (model.n, model.cap) == (300, 300)
    step("view A", lambda: view("A"))
    step("add 100 (growth: A stale)", lambda: add(100))
    assert (model.n, model.cap) == (400, 450) and not handles["A"][1].alive
    step("reserve 1000", lambda: both(lambda: _lib.check(_lib.lib().knn_flat_reserve(idx._h, 1000)), lambda: model.reserve(1000)))
    step("view B", lambda: view("B"))
    step("view C of B", lambda: view("C", of="B"))
    step("add 300 (fits)", lambda: add(300))
    assert model.n == 700 and model.cap == 1000 and handles["B"][1].alive and handles["C"][1].alive
    assert handles["B"][0].ntotal == 400 and handles["C"][0].ntotal == 400
    step("normalize_rows", lambda: both(idx.normalize_rows, model.normalize_rows))
    step("add 301 (growth to 1500: B and C stale)", lambda: add(301))
    assert (model.n, model.cap) == (1001, 1500) and not handles["B"][1].alive and not handles["C"][1].alive
    # a view of a stale view is refused (check_stale has tried it on A, B and C; here with the model saying so too)
    with pytest.raises(Refused):
        model.view(of=handles["B"][1])
    with pytest.raises(Knn355Error, match="stale"):
        handles["B"][0].view()
    step("reset", lambda: both(idx.reset, model.reset))
    step("add 257", lambda: add(257))
    step("view D", lambda: view("D"))
    step("free parent (D stale)", lambda: both(lambda: _free_now(idx), model.free))
    assert not handles["D"][1].alive and handles["D"][0].ntotal == 257


# ---- (b) seeded random sequences ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(30))
def test_random_lifecycle(gpu_faiss, oracle, seed):
    rng = np.random.default_rng(7000 + seed)
    d = int(rng.choice([1, 8, 31, 33, 64, 100]))
    metric = int(rng.integers(0, 2))
    model = FlatModel(oracle, d, metric)
    idx = gpu_faiss.IndexFlat(d, metric)
    L = _lib.lib()
    views = []  # (handle, model view)
    ops = []
    what = lambda: f"seed {seed} d {d} metric {metric} ops {ops}"
    try:
        for _ in range(12):
            op = str(rng.choice(["add", "add", "add", "reserve", "reset", "normalize_rows", "view", "view", "view_of_view", "drop"]))
            if op == "add":
                m = int(rng.integers(1, 401))
                if model.n + m > 3000:
                    op, m = "reset", 0
                else:
                    x = (rng.standard_normal((m, d)) * rng.uniform(0.2, 3.0)).astype(np.float32)
                    ops.append(f"add {m}")
                    idx.add(x)
                    model.add(x)
            if op == "reserve":
                n = int(rng.integers(0, model.cap + 600))
                ops.append(f"reserve {n}")
                _lib.check(L.knn_flat_reserve(idx._h, n))
                model.reserve(n)
            elif op == "reset":
                ops.append("reset")
                idx.reset()
                model.reset()
            elif op == "normalize_rows":
                ops.append("normalize_rows")
                idx.normalize_rows()
                model.normalize_rows()
            elif op == "view":
                ops.append("view")
                views.append((idx.view(), model.view()))
            elif op == "view_of_view" and views:
                j = int(rng.integers(0, len(views)))
                ops.append(f"view of view {j} ({'alive' if views[j][1].alive else 'stale'})")
                if views[j][1].alive:
                    views.append((views[j][0].view(), model.view(of=views[j][1])))
                else:
                    with pytest.raises(Refused):
                        model.view(of=views[j][1])
                    with pytest.raises(Knn355Error, match="stale"):
                        views[j][0].view()
            elif op == "drop" and views:
                j = int(rng.integers(0, len(views)))
                ops.append(f"drop view {j}")
                h, v = views.pop(j)
                model.drop(v)
                _free_now(h)
            check_all(idx, model, model.rows, what() + ": parent")
            live = [hv for hv in views if hv[1].alive]
            stale = [hv for hv in views if not hv[1].alive]
            if live:
                h, v = live[int(rng.integers(0, len(live)))]
                check_all(h, model, model.rows_of(v), what() + ": a live view")
            if stale:
                h, v = stale[int(rng.integers(0, len(stale)))]
                check_stale(h, d, what() + ": a stale view")
    except AssertionError:
        raise
    except Exception as e:  # (an error of the library where the model expects none)
        raise AssertionError(f"{what()}: {e!r}") from e


# ---- (c) hostile pool memory --------------------------------------------------------------------------------------------------
def _poison_and_free(gpu_faiss, d, n, metric):
    """an index whose every float is a NaN bit pattern: added to and freed, nothing else"""
    x = np.full((n, d), 0x7FC0DEAD, np.uint32).view(np.float32)
    p = gpu_faiss.IndexFlat(d, metric)
    p.add(x)
    _free_now(p)


POOL_CASES = {
    # name: (poison d, poison rows, victim d, rows reserved first (0: none), rows of each add)
    "padding_and_tail": (33, 1000, 40, 0, (600,)),     # the same dp = 64: padding columns and 400 tail rows; 600 is no multiple of 256
    "tail_only": (64, 1000, 64, 0, (257,)),            # no padding
    "reserve_then_two_adds": (33, 1000, 40, 900, (350, 250)),
}


@pytest.mark.parametrize("case", list(POOL_CASES))
@pytest.mark.parametrize("metric", [IP, L2], ids=["ip", "l2"])
def test_index_in_poisoned_pool_memory(gpu_faiss, oracle, metric, case):
    pd, pn, d, reserve, adds = POOL_CASES[case]
    L = _lib.lib()
    L.knn_trim()
    _poison_and_free(gpu_faiss, pd, pn, metric)
    pooled = L.knn_trim()  # what a poisoned index leaves in the pool
    assert pooled >= pn * ((pd + 31) // 32 * 32) * 4
    _poison_and_free(gpu_faiss, pd, pn, metric)
    rng = np.random.default_rng(31 * d + metric)
    model = FlatModel(oracle, d, metric)
    idx = gpu_faiss.IndexFlat(d, metric)
    if reserve:
        _lib.check(L.knn_flat_reserve(idx._h, reserve))
        model.reserve(reserve)
    for m in adds:
        x = rng.standard_normal((m, d)).astype(np.float32)
        idx.add(x)
        model.add(x)
    request = model.cap * ((d + 31) // 32 * 32) * 4  # the bytes the victim asked the pool for its rows
    assert request >= model.n * ((d + 31) // 32 * 32) * 4
    left = L.knn_trim()
    assert pooled - left >= request, f"the victim's rows did not come from the pool: it held {pooled} bytes, {left} are left, the rows take {request}"
    _poison_and_free(gpu_faiss, pd, pn, metric)  # (the pool again: the victim's scratch buffers come out of it)
    check_all(idx, model, model.rows, f"victim of {case}")
    # a window that is not at the end, a whole self-search, and the rows normalised in place
    _same_knn(idx.search_self(10, 3, 200), model.search_self(model.rows, 3, 200, 10), "search_self [3, 203)")
    _same_knn(idx.search_self(5), model.search_self(model.rows, 0, model.n, 5), "search_self of every row")
    idx.normalize_rows()
    model.normalize_rows()
    check_all(idx, model, model.rows, f"victim of {case}, normalised")


# ---- (d) something between two streaming searches of one shape ----------------------------------------------------------------
NB, D32, NQ, K = 131_072, 32, 32, 10


@pytest.fixture(scope="module")
def stream_rows():
    rng = np.random.default_rng(4242)
    return (rng.standard_normal((NB, D32)).astype(np.float32), rng.standard_normal((1000, D32)).astype(np.float32),
            rng.standard_normal((NQ, D32)).astype(np.float32), rng.standard_normal((NQ, D32)).astype(np.float32))


def _range_within_topk(D, I, metric):
    """a radius that only rows of every query's top-k beat, and the (lims, D, I) it keeps, from the oracle's top-k (D, I)"""
    r = np.float32(D[:, -1].max() if metric == IP else D[:, -1].min())
    lims, Ds, Is = [0], [], []
    for q in range(D.shape[0]):
        keep = (I[q] >= 0) & better(D[q], r, metric)
        o = np.argsort(I[q][keep], kind="stable")
        Is.append(I[q][keep][o])
        Ds.append(D[q][keep][o])
        lims.append(lims[-1] + int(keep.sum()))
    return r, (np.array(lims, np.uint64), np.concatenate(Ds).astype(np.float32), np.concatenate(Is).astype(np.int64))


@pytest.mark.parametrize("flags", [0, KNN_TUNE_ALWAYS_RESET], ids=["default", "always_reset"])
@pytest.mark.parametrize("metric", [IP, L2], ids=["ip", "l2"])
def test_something_between_two_streaming_searches(gpu_faiss, oracle, stream_rows, metric, flags):
    xb, extra, qa, qb = stream_rows
    # the second search's queries score worse everywhere than the first one's: thresholds left over from the first search
    # would throw its hits away
    qb = qb * np.float32(0.25) if metric == IP else qb * np.float32(4.0)
    L = _lib.lib()
    model = FlatModel(oracle, D32, metric)
    idx = gpu_faiss.IndexFlat(D32, metric)
    _lib.check(L.knn_flat_reserve(idx._h, 140_000))
    model.reserve(140_000)
    idx.add(xb)
    model.add(xb)
    idx.set_tuning(0, 0, flags)
    view = idx.view()
    mview = model.view()
    want = {}  # the oracle's answers on the model's current rows (by_add and by_normalize empty it)

    def expect(name, xq, k=K):
        if (name, k) not in want:
            want[name, k] = model.search(model.rows, xq, k)
        return want[name, k]

    def streaming(xq, name, what):
        _same_knn(idx.search(xq, K), expect(name, xq), what)
        return idx.last_seed()["stride"]

    def by_range():
        r, keep = _range_within_topk(*expect("qa", qa), metric)
        _same_range(idx.range_search(qa, r), keep, "the interposed range_search")

    def by_range_self():
        n = model.n
        r, keep = _range_within_topk(*model.search_self(model.rows, n - 40, 40, K), metric)
        _same_range(idx.range_search_self(r, n - 40, 40), keep, "the interposed range_search_self")

    def by_refine():
        lab = np.ascontiguousarray(expect("qa", qa)[1][:, ::-1])
        lab[:, 3], lab[:, 1], lab[:, 0] = -1, lab[:, 2], model.n - 1
        _same_knn(_refine(idx, qa, lab, 5), model.refine(model.rows, qa, lab, 5), "the interposed refine")

    def by_gather():
        cand, offs = _cands(model.n, 5)
        out = np.full(71, SENTINEL, np.float32)
        _gather(idx, qa[:3], cand, offs, out)
        assert np.array_equal(_bits(out), _bits(model.gather(model.rows, qa[:3], cand, offs))), "the interposed gather_distances"

    def by_window():
        n = model.n
        _same_knn(idx.search_self(K, n - 300, 300), model.search_self(model.rows, n - 300, 300, K), "the interposed search_self window")

    def by_seven():
        _same_knn(idx.search(qa[:7], K), model.search(model.rows, qa[:7], K), "the interposed 7-query search")

    def by_k100():
        _same_knn(idx.search(qa, 100), expect("qa", qa, 100), "the interposed k = 100 search")

    def by_add():
        idx.add(extra)
        model.add(extra)
        want.clear()
        assert model.cap == 140_000 and mview.alive and idx.ntotal == NB + 1000

    def by_normalize():
        idx.normalize_rows()
        model.normalize_rows()
        want.clear()

    def by_flags(extra_flags):
        """a search of the very same shape and buffers whose selection does NOT reset the state behind itself"""
        def call():
            idx.set_tuning(0, 0, flags | extra_flags)
            _same_knn(idx.search(qa, K), expect("qa", qa), f"the interposed search under tuning flags {flags | extra_flags}")
            idx.set_tuning(0, 0, flags)
        return call

    def by_view():
        _same_knn(view.search(qb, K), model.search(model.rows_of(mview), qb, K), "the interposed search through a view")

    between = [("nothing", lambda: None), ("range_search", by_range), ("range_search_self", by_range_self), ("knn_flat_refine", by_refine),
               ("knn_gather_distances", by_gather), ("a 300-row search_self window", by_window), ("a 7-query search", by_seven),
               ("a k = 100 search", by_k100), ("the same search without pairs", by_flags(KNN_TUNE_NO_PAIRS)),
               ("the same search with the reset forced", by_flags(KNN_TUNE_ALWAYS_RESET)), ("a search through a view", by_view), ("an add of 1000 rows that fits", by_add),
               ("a search through a view of the rows before the add", by_view), ("normalize_rows", by_normalize)]
    strides = []
    for name, call in between:
        strides.append(streaming(qa, "qa", f"the search before {name}"))
        call()
        strides.append(streaming(qb, "qb", f"the search after {name}"))
    assert strides[0] < 0 and strides[-1] < 0 and all(s < 0 for s in strides), \
        f"the planner did not choose the streaming, self-resetting launch (tile-minimum seed) for {NB} x {D32}, {NQ} queries: seed strides {strides}"
