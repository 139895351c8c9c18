"""GPU: the twelve bf16 builds of flat_scan_kernel (query tile 32 / 64 / 128 x inner product / squared L2 x one query tile /
several), which serve the coarse entry indexes of IndexHNSWFlat, against tests/approx16_reference.py -- ids and score bits,
exactly -- through knn_flat_set_approx16 (IndexFlat.set_approx16).

The inputs are integers times one power of two on which every order of the fp32 accumulation gives the same answer; the
reference asserts that precondition on the generated data of every case (approx16_reference.check_precondition, inside
`scores`).  Integer data ties all the time, which is what the selection needs: the lower id must win through lists, compaction,
chunk merge and final selection.  One bounded case on ordinary floats (exponents that differ across a row) closes the file.

Every case prints the build it reached ("bf16 q<tile> <metric> <one|several>")."""
import ctypes
import functools
import math

import numpy as np
import pytest

import approx16_reference as ar
from approx16_reference import IP, L2
from knn_for_homology_amd import _lib
from knn_for_homology_amd._lib import Knn355Error

pytestmark = pytest.mark.gpu

KNN_ERR_UNSUPPORTED = -4
SENTINEL = np.float32(7.25)
ENTRIES = ("host", "stream", "keys")


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(got, want, what):
    (D, I), (wD, wI) = got, want
    assert D.dtype == np.float32 and I.dtype == np.int64 and D.shape == wD.shape and I.shape == wI.shape, what
    if not np.array_equal(I, wI):
        q, j = np.argwhere(I != wI)[0]
        raise AssertionError(f"{what}: {int((I != wI).sum())} ids differ, first at query {q} rank {j}: got {I[q, j]} ({D[q, j]!r}), "
                             f"expected {wI[q, j]} ({wD[q, j]!r})")
    if not np.array_equal(_bits(D), _bits(wD)):
        q, j = np.argwhere(_bits(D) != _bits(wD))[0]
        raise AssertionError(f"{what}: {int((_bits(D) != _bits(wD)).sum())} score bits differ, first at query {q} rank {j}: got {D[q, j]!r}, "
                             f"expected {wD[q, j]!r}")


@functools.lru_cache(maxsize=None)
def _ints(n, d, lim, seed):
    """[n][d] integers in [-lim, lim] as float32; rows n // 2 .. n // 2 + 2 repeat rows 0 .. 2 (whole-row ties -> lower id)"""
    x = np.random.default_rng(seed).integers(-lim, lim + 1, (n, d)).astype(np.float32)
    if n >= 6:
        x[n // 2: n // 2 + 3] = x[:3]
    x.setflags(write=False)
    return x


def _queries(xb, nq, lim, seed):
    xq = np.random.default_rng(seed).integers(-lim, lim + 1, (nq, xb.shape[1])).astype(np.float32)
    m = min(3, nq, xb.shape[0])
    xq[:m] = xb[:m]  # (queries that tie between a row and its duplicate)
    return xq


def _index(faiss, xb, metric):
    idx = faiss.IndexFlat(xb.shape[1], metric)
    idx.set_approx16()
    if xb.shape[0]:
        idx.add(np.ascontiguousarray(xb))
    return idx


def _search(idx, xq, k, entry):
    """the three ways in: knn_flat_search, knn_flat_search_dev on a caller's stream, knn_flat_search_keys_dev (HNSW's entry;
    its packed keys are unpacked on the host)"""
    if entry == "host":
        return idx.search(xq, k)
    import torch
    import merge_reference as mr
    L = _lib.lib()
    dev = torch.device("cuda:0")
    nq = xq.shape[0]
    q = torch.from_numpy(xq).to(dev)
    if entry == "keys":
        keys = torch.empty((nq, k), device=dev, dtype=torch.int64)
        _lib.check(L.knn_flat_search_keys_dev(idx._h, q.data_ptr(), nq, k, 0, keys.data_ptr(), None))
        return mr.unpack(keys.cpu().numpy().view(np.uint64), idx.metric_type)
    Dd = torch.empty((nq, k), device=dev, dtype=torch.float32)
    Id = torch.empty((nq, k), device=dev, dtype=torch.int64)
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        _lib.check(L.knn_flat_search_dev(idx._h, q.data_ptr(), nq, k, Dd.data_ptr(), Id.data_ptr(), ctypes.c_void_p(side.cuda_stream)))
    side.synchronize()
    return Dd.cpu().numpy(), Id.cpu().numpy()


def _build(idx, nq):
    """The build the last launch ran.  The introspection gives the query tile and, through the grid (one workgroup per query
    tile and chunk), the number of query tiles; "bf16" and "one / several" are what pick_scan_kernel makes of the handle's
    approx16 and of nqtiles == 1 -- an inference, the reported kernel name does not carry the template arguments."""
    s = idx.last_scan()
    qt = s["query_tile"]
    assert s["kernel"].startswith(f"flat_scan_q{qt}_d{s['db_tile']}"), s
    assert s["grid"] == s["nchunks"] * math.ceil(nq / qt), (s, nq)
    return f"bf16 q{qt} {'l2' if idx.metric_type else 'ip'} {'one' if nq <= qt else 'several'}"


def _check(idx, xb, xq, k, what, entries=("host",), **ref):
    want = ar.expected(xb, xq, k, idx.metric_type, **ref)
    for entry in entries:
        _same(_search(idx, xq, k, entry), want, f"{what} [{entry}]")
    b = _build(idx, xq.shape[0])
    print(f"{what}: {b}")
    return b


# ---- every build ----------------------------------------------------------------------------------------------------------
TILES = (32, 64, 128)
NQS = (1, 32, 33, 64, 65, 128, 129, 200)
BUILD_CASES = [(qt, metric, nq) for qt in TILES for metric in (IP, L2) for nq in NQS]


def test_the_cases_cover_the_twelve_builds():
    assert len({(qt, metric, nq <= qt) for qt, metric, nq in BUILD_CASES}) == 12


@pytest.mark.parametrize("qt,metric,nq", BUILD_CASES)
def test_every_build_through_every_entry(gpu_faiss, qt, metric, nq):
    xb = _ints(1000, 100, 16, 1)
    xq = _queries(xb, nq, 16, 100 + nq)
    idx = _index(gpu_faiss, xb, metric)
    idx.set_tuning(qt, 0, 0)
    want = f"bf16 q{qt} {'l2' if metric else 'ip'} {'one' if nq <= qt else 'several'}"
    for entry in ENTRIES:
        assert _check(idx, xb, xq, 10, f"qt {qt} nq {nq}", (entry,)) == want
        assert idx.last_scan()["query_tile"] == qt


@pytest.mark.parametrize("metric", [IP, L2])
@pytest.mark.parametrize("nb", [1, 255, 256, 257, 1000, 4097])
def test_row_counts_around_the_database_tile(gpu_faiss, metric, nb):
    xb = _ints(nb, 65, 16, 2)
    idx = _index(gpu_faiss, xb, metric)
    for nq in (5, 33, 200):
        _check(idx, xb, _queries(xb, nq, 16, 200 + nq), 10, f"nb {nb} nq {nq}", ENTRIES)


@pytest.mark.parametrize("metric", [IP, L2])
@pytest.mark.parametrize("nchunks", [1, 4])
def test_several_workgroups_and_a_chunk_merge(gpu_faiss, metric, nchunks):
    xb = _ints(20000, 64, 16, 3)
    idx = _index(gpu_faiss, xb, metric)
    idx.set_tuning(0, nchunks, 0)
    for nq in (8, 200):
        _check(idx, xb, _queries(xb, nq, 16, 300 + nq), 100, f"nb 20000 nchunks {nchunks} nq {nq}", ("host", "keys"))
        assert idx.last_scan()["nchunks"] == nchunks


# ---- row widths around the 64-value K step --------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", [IP, L2])
@pytest.mark.parametrize("d", [1, 8, 63, 64, 65, 100, 128, 1024, 1280])
def test_row_widths_around_the_k_step(gpu_faiss, metric, d):
    """dp = roundup(d, 64): the padding of rows and of queries contributes nothing, and no K step is lost (the last values of
    every row are the largest, so a lost step changes every score)"""
    xb = _ints(600, d, 16, 4).copy()
    xb[:, -1] = np.where(xb[:, -1] >= 0, 16, -16)
    xq = _queries(xb, 40, 16, 400 + d)
    idx = _index(gpu_faiss, xb, metric)
    _check(idx, xb, xq, 10, f"d {d} nq 40", ENTRIES)
    _check(idx, xb, xq[:7], 10, f"d {d} nq 7")


# ---- k ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", [IP, L2])
@pytest.mark.parametrize("k", [1, 10, 100, 301, 1400, 1401, 2048])
def test_k_up_to_2048_with_ties_everywhere(gpu_faiss, metric, k):
    """d = 8 and values in [-2, 2]: a few dozen distinct scores among 3000 rows, so nearly everything ties and the lower id
    must win; 1400 / 1401 is where the candidate lists change their capacity; nb 257 is k > nb from k = 301 on"""
    for nb in (3000, 257):
        xb = _ints(nb, 8, 2, 5)
        idx = _index(gpu_faiss, xb, metric)
        for nq in (3, 70):
            _check(idx, xb, _queries(xb, nq, 2, 500 + nq), k, f"k {k} nb {nb} nq {nq}", ("host", "keys"))


# ---- rounding -----------------------------------------------------------------------------------------------------------------
TIES = np.array([257, 259, 383, 385, 511, 509, 255, 129, 131, 1, 3, 0], np.float32)  # nine-bit odd values are exact ties


def _rounding_data(scale):
    """d = 15, |v| < 512: values that need rounding, exact ties, both signs, 511 -> 512 across a power of two"""
    rng = np.random.default_rng(6)
    xb = rng.integers(-511, 512, (700, 15)).astype(np.float32)
    xq = rng.integers(-511, 512, (40, 15)).astype(np.float32)
    xb[:200] = rng.choice(TIES, (200, 15)) * rng.choice(np.array([-1, 1], np.float32), (200, 15))
    xq[:12] = rng.choice(TIES, (12, 15)) * rng.choice(np.array([-1, 1], np.float32), (12, 15))
    xb[350:353] = xb[:3]
    return xb * np.float32(scale), xq * np.float32(scale)


@pytest.mark.parametrize("metric", [IP, L2])
@pytest.mark.parametrize("scale", [1.0, 0.5, 2.0 ** -20])
def test_copies_are_rounded_to_nearest_even(gpu_faiss, metric, scale):
    xb, xq = _rounding_data(scale)
    idx = _index(gpu_faiss, xb, metric)
    want = ar.expected(xb, xq, 10, metric, scale=scale)
    trunc = ar.expected(xb, xq, 10, metric, scale=scale, rounding=ar.bf16_trunc)
    assert not np.array_equal(_bits(want[0]), _bits(trunc[0])) and not np.array_equal(want[1], trunc[1]), "the case cannot tell truncation from RNE"
    for entry in ENTRIES:
        _same(_search(idx, xq, 10, entry), want, f"rounding scale {scale} [{entry}]")
    _same(_search(idx, xq[:5], 10, "host"), (want[0][:5], want[1][:5]), f"rounding scale {scale} nq 5")
    print(f"rounding scale {scale}: {_build(idx, 5)}")


def test_l2_norms_come_from_the_fp32_values(gpu_faiss):
    xb, xq = _rounding_data(1.0)
    idx = _index(gpu_faiss, xb, L2)
    D, I = idx.search(xq, 10)
    _same((D, I), ar.expected(xb, xq, 10, L2), "fp32 norms")
    rounded = ar.scores(xb, xq, L2, norms="rounded")
    assert (np.take_along_axis(rounded, I, axis=1) != D).any(), "the case cannot tell the norms of the rounded copies from the fp32 ones"
    assert np.array_equal(_bits(idx.reconstruct_n(0, 700)), _bits(xb)), "reconstruct must return the fp32 rows, not the copies"


# ---- lifecycle of the copies --------------------------------------------------------------------------------------------------
def _add_dev(idx, x):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0")
    _lib.check(_lib.lib().knn_flat_add_dev(idx._h, t.data_ptr(), x.shape[0], None))
    torch.cuda.synchronize()


@pytest.mark.parametrize("metric", [IP, L2])
def test_copies_follow_reserve_adds_regrowth_and_reset(gpu_faiss, metric):
    """reserve, device adds of 7 / 300 / 5000 rows that fit it, one that outgrows it (the copies regrow and every row is
    converted again), reset and adds; a search after every step.  d = 15 rounding data: a row left unconverted, converted
    from the wrong range or left over from before the reset changes scores."""
    rng = np.random.default_rng(7)
    pool = rng.integers(-511, 512, (6000, 15)).astype(np.float32)
    xq = rng.integers(-511, 512, (33, 15)).astype(np.float32)
    idx = gpu_faiss.IndexFlat(15, metric)
    idx.set_approx16()
    _lib.check(_lib.lib().knn_flat_reserve(idx._h, 5400))
    n = 0
    for step in (7, 300, 5000, 200, 493):  # (5307 rows fit; 5507 do not)
        _add_dev(idx, pool[n:n + step])
        n += step
        assert idx.ntotal == n
        _check(idx, pool[:n], xq, 10, f"after add_dev -> {n} rows", ("host", "keys"))
    assert np.array_equal(_bits(idx.reconstruct_n(0, n)), _bits(pool[:n]))
    idx.reset()
    assert idx.ntotal == 0
    D, I = idx.search(xq, 3)
    assert (I == -1).all() and (D == (-ar.FLT_MAX if metric == IP else ar.FLT_MAX)).all()
    rows = pool[::-1]  # (other rows at the same places)
    idx.add(np.ascontiguousarray(rows[:300]))
    _check(idx, rows[:300], xq, 10, "after reset + add 300")
    _add_dev(idx, rows[300:1000])
    _check(idx, rows[:1000], xq, 10, "after reset + add 300 + add_dev 700", ("host", "keys"))


def _pow2_norm_rows(n, d, seed):
    """rows whose norm is a power of two: m in {1, 4, 16, 64} entries of +-v, the rest zero; normalised they are +-2^-j"""
    rng = np.random.default_rng(seed)
    x = np.zeros((n, d), np.float32)
    for r in range(n):
        m = (1, 4, 16, 64)[r % 4]
        x[r, rng.choice(d, m, replace=False)] = rng.choice(np.array([-1, 1], np.float32), m) * np.float32((1, 2, 8, 0.5)[(r // 4) % 4])
    x[n // 2] = 0  # (a zero row stays as it is)
    return x


@pytest.mark.parametrize("metric", [IP, L2])
def test_normalize_rows_converts_the_copies_again(gpu_faiss, metric):
    xb = _pow2_norm_rows(700, 100, 8)
    nrm = np.sqrt((xb.astype(np.float64) ** 2).sum(1))
    assert np.array_equal(np.log2(nrm[nrm > 0]) % 1, np.zeros((nrm > 0).sum()))
    unit = (xb / np.where(nrm > 0, nrm, 1)[:, None]).astype(np.float32)  # (exact: a division by a power of two)
    xq = _queries(unit, 33, 16, 800) * np.float32(0.125)
    xq[:3] = unit[:3]
    idx = _index(gpu_faiss, xb, metric)
    _check(idx, xb, xq, 10, "before normalize_rows", scale=0.125)
    idx.normalize_rows()
    assert np.array_equal(_bits(idx.reconstruct_n(0, 700)), _bits(unit))
    _check(idx, unit, xq, 10, "after normalize_rows", ("host", "keys"), scale=0.125)


# ---- the entry points that read rows: served exactly, or refused ---------------------------------------------------------------
@pytest.mark.parametrize("metric", [IP, L2])
def test_self_searches_are_the_searches_of_the_fp32_rows(gpu_faiss, metric):
    """knn_flat_search_self / _self_dev hand the fp32 rows to the same conversion as uploaded queries: the result is that of
    search(reconstruct_n(...)), never the symmetric fp32 scan"""
    import torch
    xb, _ = _rounding_data(1.0)
    idx = _index(gpu_faiss, xb, metric)
    want = ar.expected(xb, xb, 10, metric)
    _same(idx.search_self(10), want, "search_self")
    assert not idx.last_scan()["kernel"].endswith("_sym")
    _same(idx.search_self(10, 650, 50), (want[0][650:], want[1][650:]), "search_self of a window")
    Dd = torch.empty((700, 10), device="cuda:0", dtype=torch.float32)
    Id = torch.empty((700, 10), device="cuda:0", dtype=torch.int64)
    _lib.check(_lib.lib().knn_flat_search_self_dev(idx._h, 10, Dd.data_ptr(), Id.data_ptr()))
    _same((Dd.cpu().numpy(), Id.cpu().numpy()), want, "search_self_dev")


def _refused(call):
    rc = call()
    assert rc == KNN_ERR_UNSUPPORTED, rc
    assert b"not for an approximate (bf16) index" in _lib.lib().knn_last_error()


def test_entry_points_without_a_bf16_form_refuse(gpu_faiss):
    """KNN_ERR_UNSUPPORTED before anything is copied or launched: every output keeps its sentinel"""
    import torch
    L = _lib.lib()
    xb = _ints(300, 20, 16, 9)
    xq = _queries(xb, 5, 16, 900)
    idx = _index(gpu_faiss, xb, L2)
    h = idx._h
    lims = np.full(6, 77, np.uint64)
    _refused(lambda: L.knn_flat_range_search(h, xq.ctypes.data, 5, ctypes.c_float(1e9), lims.ctypes.data))
    _refused(lambda: L.knn_flat_range_search_self(h, 0, 5, ctypes.c_float(1e9), lims.ctypes.data))
    assert (lims == 77).all()
    out = np.full(4, SENTINEL, np.float32)
    cand, offs = np.array([0, 1, 2, 299], np.int64), np.array([0, 4, 4, 4, 4, 4], np.int64)
    _refused(lambda: L.knn_gather_distances(h, xq.ctypes.data, 5, cand.ctypes.data, offs.ctypes.data, out.ctypes.data))
    assert (out == SENTINEL).all()
    ms, nbytes = ctypes.c_float(-3.0), ctypes.c_int64(-3)
    _refused(lambda: L.knn_flat_read_rate(h, 1, ctypes.byref(ms), ctypes.byref(nbytes)))
    assert ms.value == -3.0 and nbytes.value == -3
    D = np.full((5, 2), SENTINEL, np.float32)
    I = np.full((5, 2), -7, np.int64)
    lab = np.zeros((5, 3), np.int64)
    _refused(lambda: L.knn_flat_refine(h, xq.ctypes.data, 5, lab.ctypes.data, 3, 2, D.ctypes.data, I.ctypes.data))
    assert (D == SENTINEL).all() and (I == -7).all()
    lsh = gpu_faiss.IndexLSH(20, 64)  # (the same rows in an LSH base index: the one-call refine takes the flat handle)
    lsh.add(np.ascontiguousarray(xb))
    _refused(lambda: L.knn_lsh_search_refine(lsh._h, h, xq.ctypes.data, 5, 3, 2, D.ctypes.data, I.ctypes.data))
    assert (D == SENTINEL).all() and (I == -7).all()
    v = ctypes.c_void_p()
    _refused(lambda: L.knn_flat_view(h, ctypes.byref(v)))
    assert not v.value
    with pytest.raises(Knn355Error, match="code -4"):
        idx.view()
    with pytest.raises(Knn355Error, match="code -4"):
        idx.range_search(xq, 1.0)
    # the sharded search: on a real one-rank communicator, refused before the collective
    ident = (ctypes.c_uint8 * 128)()
    _lib.check(L.knn_comm_unique_id(ident))
    comm = ctypes.c_void_p()
    _lib.check(L.knn_comm_create(ident, 1, 0, 0, ctypes.byref(comm)))
    try:
        q = torch.from_numpy(xq).to("cuda:0")
        Dd = torch.full((5, 2), float(SENTINEL), device="cuda:0", dtype=torch.float32)
        Id = torch.full((5, 2), -7, device="cuda:0", dtype=torch.int64)
        _refused(lambda: L.knn_sharded_search_dev(h, comm, q.data_ptr(), 5, 2, 0, Dd.data_ptr(), Id.data_ptr(), None))
        torch.cuda.synchronize()
        assert (Dd.cpu().numpy() == SENTINEL).all() and (Id.cpu().numpy() == -7).all()
    finally:
        L.knn_comm_free(comm)
    # the index still serves its searches
    _check(idx, xb, xq, 10, "after the refusals")


def test_set_approx16_keeps_its_preconditions(gpu_faiss):
    L = _lib.lib()
    idx = gpu_faiss.IndexFlat(20, IP)
    idx.add(_ints(10, 20, 16, 10))
    assert L.knn_flat_set_approx16(idx._h) == -1  # the index already holds rows
    s16 = gpu_faiss.IndexFlat(20, IP)
    s16.set_scan16(1)
    assert L.knn_flat_set_approx16(s16._h) == KNN_ERR_UNSUPPORTED
    a16 = gpu_faiss.IndexFlat(20, IP)
    a16.set_approx16()
    assert L.knn_flat_set_scan16(a16._h, 1) == KNN_ERR_UNSUPPORTED
    assert L.knn_flat_set_approx16(None) == -1
    # storage sized with the fp32 row stride (d = 20: 32 values a row, 64 once approximate): refused until it is gone
    res = gpu_faiss.IndexFlat(20, L2)
    _lib.check(L.knn_flat_reserve(res._h, 100))
    assert L.knn_flat_set_approx16(res._h) == -1 and b"already has storage" in L.knn_last_error()
    res.add(_ints(100, 20, 16, 10))  # (still a plain fp32 index)
    assert res.search(_ints(100, 20, 16, 10)[:5], 1)[1][:, 0].tolist() == [0, 1, 2, 3, 4]
    res.reset()
    res.set_approx16()
    xb = _ints(100, 20, 16, 10)
    res.add(xb)
    _check(res, xb, _queries(xb, 33, 16, 1000), 10, "reserve, refused, reset, set_approx16, add")
    # a view uses its parent's rows; the storage index of an HNSW index keeps bf16 copies of its own
    view = gpu_faiss.IndexFlat(20, IP).view()
    assert L.knn_flat_set_approx16(view._h) == -1 and b"a view" in L.knn_last_error()
    hnsw = gpu_faiss.IndexHNSWFlat(20, 8, IP)
    assert L.knn_flat_set_approx16(L.knn_hnsw_storage(hnsw._h)) == KNN_ERR_UNSUPPORTED


# ---- ordinary floats: bounded -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", [IP, L2])
@pytest.mark.parametrize("d", [100, 1024])
def test_ordinary_floats_within_the_accumulation_bound(gpu_faiss, oracle, metric, d):
    """standard_normal rows: exponents differ across a row, which integers cannot reach.  The reference is the float64 dot
    product of the RNE-rounded operands (squared L2: with the float64 norms of the unrounded ones).  The bound rests on
    nothing measured (approx16_reference.float_reference): the products are exact, and a sum of dp fp32 terms in ANY order is
    off by at most dp * 2^-24 * sum|x_i y_i|; squared L2 adds the error of the fp32 norms (the oracle's bits against float64),
    the rounding of nx + ny, twice the dot product's error and the rounding of the fma.
    Scores: every returned score is within the bound of its pair's reference.  Ids, with the bounds of the pairs involved
    (never more than twice the query's largest): a returned row r was not beaten by some row s of the reference's best k, so
    ref(r) is within bound(r) + bound(s) of the reference's k-th; a row m that is missing was beaten by a returned row j that
    is no better than the reference's k-th, so ref(m) is within bound(m) + bound(j) of it -- any row that beats the k-th by
    more must have been returned."""
    rng = np.random.default_rng(11 + d)
    xb = rng.standard_normal((2000, d), dtype=np.float32)
    xq = rng.standard_normal((40, d), dtype=np.float32)
    k, dp = 10, (d + 63) // 64 * 64
    ref, bound = ar.float_reference(xb, xq, metric, dp, oracle.norm_l2sqr(xb), oracle.norm_l2sqr(xq))
    idx = _index(gpu_faiss, xb, metric)
    for entry in ENTRIES:
        D, I = _search(idx, xq, k, entry)
        assert ((I >= 0) & (I < 2000)).all()
        err = np.abs(D.astype(np.float64) - np.take_along_axis(ref, I, axis=1))
        lim = np.take_along_axis(bound, I, axis=1)
        print(f"d {d} metric {metric} [{entry}]: largest score error {err.max():.3e}, its bound {lim[np.unravel_index(err.argmax(), err.shape)]:.3e}")
        assert (err <= lim).all(), f"[{entry}] {int((err > lim).sum())} scores beyond the bound, worst {float((err / lim).max()):.2f} x"
        key = -ref if metric == IP else ref
        best = np.argsort(key, axis=1, kind="stable")[:, :k]
        kth = np.take_along_axis(key, best, axis=1)[:, k - 1]
        b_best = np.take_along_axis(bound, best, axis=1).max(axis=1)  # (s: some row of the reference's best k)
        got_key = np.take_along_axis(key, I, axis=1)
        assert (got_key <= kth[:, None] + lim + b_best[:, None]).all(), f"[{entry}] a returned row is not among the best within the bound"
        must = key < kth[:, None] - bound - lim.max(axis=1)[:, None]  # (j: some returned row)
        have = np.zeros_like(must)
        np.put_along_axis(have, I, True, axis=1)
        assert not (must & ~have).any(), f"[{entry}] a row that beats the k-th by more than the bound is missing"
        assert all(len(set(r)) == k for r in I.tolist())
    print(f"d {d}: {_build(idx, 40)}")
