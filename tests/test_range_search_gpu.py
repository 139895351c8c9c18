"""GPU: IndexFlat.range_search / range_search_self (range.inc) against the CPU oracle, bit for bit.

The expected answer of a query is read off the oracle's full ranking (flat_search with k = nb, FAISS's L2 batch rule
applied by the oracle): the rows whose score beats the radius strictly (IP: score > r, L2: score < r), in ascending
row id.  lims, I and the D bits are compared exactly."""
import threading

import numpy as np
import pytest

import range_reference as rr
from conftest import GOLDEN
from flat_lifecycle_reference import expected_range as _expected  # (lims, D, I) from the oracle's full ranking

pytestmark = pytest.mark.gpu

IP, L2 = 0, 1
NARROW, WIDE, DIFF = "range_scan_q32_d256", "range_scan_q128_d128", "range_scan_q32_d256_diff"


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _better(D, r, metric):
    return D > np.float32(r) if metric == IP else D < np.float32(r)


def _assert_same(got, want):
    lims, D, I = got
    wl, wD, wI = want
    assert lims.dtype == np.uint64 and D.dtype == np.float32 and I.dtype == np.int64
    assert np.array_equal(lims, wl), f"lims differ at {np.flatnonzero(lims != wl)[:5]}"
    assert np.array_equal(I, wI), f"{int((I != wI).sum())} ids differ"
    assert np.array_equal(_bits(D), _bits(wD)), f"{int((_bits(D) != _bits(wD)).sum())} scores differ"


def _radius(oracle, xb, xq, metric, frac):
    """a radius that about `frac` of the (query, row) pairs beat: 0 -> none, 1 -> all"""
    if frac <= 0:
        return np.float32(np.inf) if metric == IP else np.float32(-1.0)
    if frac >= 1:
        return np.float32(-np.inf) if metric == IP else np.float32(np.inf)
    D, I = oracle.flat_search(xb, xq, xb.shape[0], metric)
    v = np.sort(D[I >= 0].ravel())
    return np.float32(v[int((1 - frac) * (len(v) - 1))] if metric == IP else v[int(frac * (len(v) - 1))])


def _data(seed, nb, nq, d):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((nb, d)).astype(np.float32), rng.standard_normal((nq, d)).astype(np.float32)


def _index(gpu_faiss, xb, metric):
    idx = gpu_faiss.IndexFlat(xb.shape[1], metric)
    if xb.shape[0]:
        idx.add(xb)
    return idx


# ---- 1. parity matrix: every tile width, the difference build, radii from none to all -----------------------------
PARITY = [
    # (nb, d, nq, metric, frac, kernel)
    (1, 1, 1, IP, 1.0, NARROW),
    (37, 3, 7, L2, 0.5, DIFF),
    (1000, 100, 19, L2, 0.01, DIFF),
    (1000, 100, 20, L2, 0.01, NARROW),
    (4097, 1024, 32, IP, 0.01, NARROW),
    (4097, 1280, 33, L2, 0.5, NARROW),
    (20000, 100, 129, IP, 0.01, WIDE),
    (20000, 3, 300, L2, 0.01, WIDE),
    (1000, 1280, 300, IP, 0.0, WIDE),
    (4097, 100, 1, L2, 0.0, DIFF),
    (37, 1024, 129, L2, 1.0, WIDE),
    (20000, 1024, 7, IP, 0.5, NARROW),
]


@pytest.mark.parametrize("nb,d,nq,metric,frac,kernel", PARITY)
def test_parity(gpu_faiss, oracle, nb, d, nq, metric, frac, kernel):
    xb, xq = _data(nb * 7 + d + nq, nb, nq, d)
    r = _radius(oracle, xb, xq, metric, frac)
    idx = _index(gpu_faiss, xb, metric)
    got = idx.range_search(xq, r)
    assert idx.last_scan()["kernel"] == kernel
    _assert_same(got, _expected(oracle, xb, xq, r, metric))
    if frac >= 1:
        assert np.array_equal(got[0], np.arange(nq + 1, dtype=np.uint64) * nb)
    if frac <= 0:
        assert got[0][-1] == 0


# ---- 2. strictness -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", [IP, L2])
def test_strict_radius(gpu_faiss, oracle, metric):
    xb, xq = _data(11, 3000, 24, 64)
    D, I = oracle.flat_search(xb, xq, xb.shape[0], metric)
    r = D[5, 40]  # a score query 5 attains at row I[5, 40]
    idx = _index(gpu_faiss, xb, metric)
    lims, Dg, Ig = idx.range_search(xq, r)
    row = I[5, 40]
    got5 = Ig[lims[5]:lims[6]]
    assert row not in set(got5.tolist())
    for q in range(xq.shape[0]):
        want = np.sort(I[q][_better(D[q], r, metric) & (I[q] >= 0)])
        assert np.array_equal(Ig[lims[q]:lims[q + 1]], want)


# ---- 3. the small-batch L2 rule ----------------------------------------------------------------------------------
def test_small_batch_l2_is_the_difference_form(gpu_faiss, oracle):
    rng = np.random.default_rng(3)
    # rows far from the origin and close to each other: the norm formula cancels, the difference form does not
    xb = (100.0 + rng.standard_normal((2000, 48))).astype(np.float32)
    xq = (100.0 + rng.standard_normal((19, 48))).astype(np.float32)
    Dd, _ = oracle.flat_search(xb, xq, xb.shape[0], L2, l2_mode=2)
    r = np.float32(np.median(Dd))
    idx = _index(gpu_faiss, xb, L2)
    got = idx.range_search(xq, r)
    assert idx.last_scan()["kernel"] == DIFF
    want_diff = _expected(oracle, xb, xq, r, L2, l2_mode=0)
    _assert_same(got, want_diff)
    # the norm formula gives different bits for at least one kept pair: the test tells the two builds apart
    Dn, In = oracle.flat_search(xb, xq, xb.shape[0], L2, l2_mode=1)
    lims, D, I = got
    differ = 0
    for q in range(xq.shape[0]):
        ids = I[lims[q]:lims[q + 1]]
        pos = np.empty(xb.shape[0], np.int64)
        pos[In[q]] = np.arange(xb.shape[0])
        differ += int((_bits(Dn[q][pos[ids]]) != _bits(D[lims[q]:lims[q + 1]])).sum())
    assert differ > 0
    # and the rows agree with `search` on the same batch
    Ds, Is = idx.search(xq, 5)
    assert np.array_equal(_bits(Ds), _bits(Dd[:, :5]))


# ---- 4. agreement with search ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def big_rows():
    rng = np.random.default_rng(2024)
    xb = rng.random((1_000_000, 1024), dtype=np.float32)
    xq = rng.random((64, 1024), dtype=np.float32)
    return xb, xq


@pytest.mark.parametrize("nb", [200_000, 1_000_000])
@pytest.mark.parametrize("metric", [IP, L2])
def test_agrees_with_search(gpu_faiss, big_rows, nb, metric):
    xb, xq = big_rows[0][:nb], big_rows[1]
    idx = _index(gpu_faiss, np.ascontiguousarray(xb), metric)
    Ds, Is = idx.search(xq, 100)
    r = Ds[:, 99].max() if metric == IP else Ds[:, 99].min()
    lims, D, I = idx.range_search(xq, r)  # the whole batch at once: the same L2 formula as the search
    assert idx.last_scan()["kernel"] == NARROW
    for q in range(xq.shape[0]):
        keep = _better(Ds[q], r, metric)
        order = np.argsort(Is[q][keep], kind="stable")
        want_I, want_D = Is[q][keep][order], Ds[q][keep][order]
        assert np.array_equal(I[lims[q]:lims[q + 1]], want_I), f"query {q}"
        assert np.array_equal(_bits(D[lims[q]:lims[q + 1]]), _bits(want_D)), f"query {q}"


# ---- 5. large output, overflow redo ------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", [IP, L2])
def test_large_output_and_redo(gpu_faiss, oracle, metric):
    nb, nq, d = 100_000, 300, 32
    xb, xq = _data(5, nb, nq, d)
    idx = _index(gpu_faiss, xb, metric)
    r = np.float32(-np.inf) if metric == IP else np.float32(np.inf)
    lims, D, I = idx.range_search(xq, r)
    assert np.array_equal(lims, np.arange(nq + 1, dtype=np.uint64) * nb)
    ar = np.arange(nb)
    for q in (0, 1, 150, 299):
        assert np.array_equal(I[q * nb:(q + 1) * nb], ar)
    # what the host model of range_search_impl predicts for this shape on this device: every query overflows in every chunk,
    # the 30 M results leave in two runs and each run's queries are rescanned (256 CUs: 167 and 133 queries, 2 x 171 workgroups)
    import torch
    pred = rr.predict(nb, metric, nq, int(torch.cuda.get_device_properties(0).multi_processor_count), rr.keep_all)
    assert idx.last_range() == pred["last_range"] and pred["last_range"]["redos"] >= 2 and pred["last_range"]["redo_queries"] == nq
    scan = idx.last_scan()
    assert {k: scan[k] for k in pred["last_scan"]} == pred["last_scan"]
    sample = np.array([0, 77, 299])
    Do, Io = oracle.flat_search(xb, xq[sample], nb, metric, l2_mode=1)
    for j, q in enumerate(sample):
        want = np.empty(nb, np.float32)
        want[Io[j]] = Do[j]
        assert np.array_equal(_bits(D[q * nb:(q + 1) * nb]), _bits(want)), f"query {q}"


# ---- 6. range_search_self -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", [IP, L2])
def test_range_search_self(gpu_faiss, oracle, metric):
    xb, _ = _data(8, 5000, 1, 100)
    idx = _index(gpu_faiss, xb, metric)
    if metric == IP:
        idx.normalize_rows()
        r = np.float32(0.2)
    else:
        r = np.float32(170.0)
    for row0, nrows in ((0, None), (1234, 300), (4990, 10)):
        n = idx.ntotal - row0 if nrows is None else nrows
        got = idx.range_search_self(r, row0, nrows)
        want = idx.range_search(idx.reconstruct_n(row0, n), r)
        _assert_same(got, want)
        assert got[0][-1] > 0
    # against the oracle, for the normalised index too
    rows = idx.reconstruct_n(0, idx.ntotal)
    _assert_same(idx.range_search_self(r, 100, 40), _expected(oracle, rows, rows[100:140], r, metric))


# ---- 7. edges -----------------------------------------------------------------------------------------------------
def test_edges(gpu_faiss):
    empty = gpu_faiss.IndexFlat(16, L2)
    x = np.ones((3, 16), np.float32)
    lims, D, I = empty.range_search(x, 1.0)
    assert lims.dtype == np.uint64 and np.array_equal(lims, np.zeros(4, np.uint64))
    assert D.dtype == np.float32 and I.dtype == np.int64 and D.size == 0 and I.size == 0
    xb, xq = _data(1, 500, 5, 16)
    idx = _index(gpu_faiss, xb, IP)
    lims, D, I = idx.range_search(np.zeros((0, 16), np.float32), 0.0)
    assert np.array_equal(lims, np.zeros(1, np.uint64)) and D.size == 0 and I.size == 0
    lims, D, I = idx.range_search_self(0.0, 0, 0)
    assert np.array_equal(lims, np.zeros(1, np.uint64))
    for r in (np.inf, np.float32(1e30), np.nan):
        lims, D, I = idx.range_search(xq, r)
        assert np.array_equal(lims, np.zeros(6, np.uint64)) and D.size == 0
    lims, D, I = idx.range_search(xq, -np.inf)
    assert np.array_equal(lims, np.arange(6, dtype=np.uint64) * 500)
    for a in (D, I):
        assert a.flags.c_contiguous and a.flags.writeable and a.ndim == 1
    assert lims.flags.c_contiguous and lims.flags.writeable
    l2 = _index(gpu_faiss, xb, L2)
    assert l2.range_search(xq, np.nan)[0][-1] == 0
    assert l2.range_search(xq, np.inf)[0][-1] == 5 * 500
    assert l2.range_search(xq, -np.inf)[0][-1] == 0
    with pytest.raises(TypeError):
        idx.range_search(xq.astype(np.float64), 0.0)
    with pytest.raises(AssertionError):
        idx.range_search(np.ones((2, 15), np.float32), 0.0)


def test_flatip_and_flatl2_inherit(gpu_faiss, oracle):
    xb, xq = _data(21, 700, 9, 40)
    for cls, metric, r in ((gpu_faiss.IndexFlatIP, IP, 5.0), (gpu_faiss.IndexFlatL2, L2, 60.0)):
        idx = cls(40)
        idx.add(xb)
        _assert_same(idx.range_search(xq, r), _expected(oracle, xb, xq, r, metric))


# ---- 8. golden data ------------------------------------------------------------------------------------------------
def test_golden_pfam_cosine(gpu_faiss, oracle):
    train = np.load(GOLDEN / "pfam-20-10" / "train.npy")
    test = np.load(GOLDEN / "pfam-20-10" / "test.npy")
    hay, qs = train.copy(), test.copy()
    gpu_faiss.normalize_L2(hay)
    gpu_faiss.normalize_L2(qs)
    oh, oq = train.copy(), test.copy()
    oracle.normalize_l2(oh)
    oracle.normalize_l2(oq)
    idx = _index(gpu_faiss, hay, IP)
    got = idx.range_search(qs, 0.9)
    _assert_same(got, _expected(oracle, oh, oq, np.float32(0.9), IP))
    assert got[0][-1] > 0


# ---- 9. a view in one thread, the parent's search in another ----------------------------------------------------------
def test_view_and_threads(gpu_faiss, oracle):
    xb, xq = _data(9, 30000, 40, 128)
    idx = _index(gpu_faiss, xb, IP)
    view = idx.view()
    r = np.float32(25.0)
    out = {}

    def ranged():
        for _ in range(3):
            out["range"] = view.range_search(xq, r)

    t = threading.Thread(target=ranged)
    t.start()
    for _ in range(3):
        out["search"] = idx.search(xq, 10)
    t.join()
    _assert_same(out["range"], _expected(oracle, xb, xq, r, IP))
    Do, Io = oracle.flat_search(xb, xq, 10, IP)
    assert np.array_equal(out["search"][1], Io) and np.array_equal(_bits(out["search"][0]), _bits(Do))


# ---- 10. bounded random batch --------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(50))
def test_random_cases(gpu_faiss, oracle, seed):
    rng = np.random.default_rng(1000 + seed)
    nb = int(rng.integers(1, 3000))
    nq = int(rng.choice([1, 5, 19, 20, 31, 32, 33, 64, 65, 130]))
    d = int(rng.choice([1, 2, 7, 8, 31, 33, 64, 100, 257]))
    metric = int(rng.integers(0, 2))
    frac = float(rng.choice([0.0, 0.001, 0.05, 0.3, 0.9, 1.0]))
    xb = rng.standard_normal((nb, d)).astype(np.float32)
    xq = rng.standard_normal((nq, d)).astype(np.float32)
    r = _radius(oracle, xb, xq, metric, frac)
    idx = _index(gpu_faiss, xb, metric)
    _assert_same(idx.range_search(xq, r), _expected(oracle, xb, xq, r, metric))
