"""GPU: the tail of the exact 16-bit prefilter (the sliced re-scoring, the exact selection, the gated fallback).

Every search is compared bit for bit with the same index under KNN_TUNE_NO_SCAN16 and with the CPU oracle.  The shapes are
the smallest that reach every branch of the tail: fewer rows than k', about k', many more; one slab of a row, a padded
row, a full 1024-float slab; one query, a few, a full tile; k' = k + 64, 2k and the cap of 2048; windows that fit, windows
that overflow (the device fallback), a query that is not finite; and sequences of searches on one handle, each compared
with a fresh handle, with and without KNN_TUNE_ALWAYS_RESET."""
import functools

import numpy as np
import pytest

from knn_for_homology_amd._lib import KNN_TUNE_ALWAYS_RESET, KNN_TUNE_NO_SCAN16, KNN_TUNE_SCAN16_ANY_NB

pytestmark = pytest.mark.gpu

IP = 0


@functools.lru_cache(maxsize=None)
def _data(kind, nb, d, nq, seed=0):
    """(xb, xq), read-only.  normed: random unit rows (no fallback).  near: a block of rows that fp16 cannot tell from
    query 0 (its window overflows).  const: every row the same (every window overflows).  nanq: normed with a NaN in the
    last query."""
    rng = np.random.default_rng([seed, nb, d, nq])
    xb = rng.standard_normal((nb, d), dtype=np.float32)
    xb /= np.linalg.norm(xb, axis=1, keepdims=True)
    xq = rng.standard_normal((nq, d), dtype=np.float32)
    xq /= np.linalg.norm(xq, axis=1, keepdims=True)
    if kind == "near":
        m = min(nb // 2, 2500)
        xb[7:7 + m] = xq[0] + rng.standard_normal((m, d), dtype=np.float32) * np.float32(1e-7)
    elif kind == "const":
        xb[:] = np.float32(0.37)
    elif kind == "nanq":
        xq[nq - 1, d // 2] = np.nan
    else:
        assert kind == "normed"
    xb.setflags(write=False)
    xq.setflags(write=False)
    return xb, xq


_ORACLE = {}


def _want(oracle, kind, nb, d, nq, k, seed=0):
    key = (kind, nb, d, nq, k, seed)
    if key not in _ORACLE:
        xb, xq = _data(kind, nb, d, nq, seed)
        _ORACLE[key] = oracle.flat_search(xb, xq, k, IP)
    return _ORACLE[key]


def _index(faiss, xb, flags=0):
    idx = faiss.IndexFlat(xb.shape[1], IP)
    idx.set_scan16(1)
    idx.add(xb)
    idx.set_tuning(0, 0, KNN_TUNE_SCAN16_ANY_NB | flags)
    return idx


def _same(a, b):
    return np.array_equal(a[1], b[1]) and np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32))


def _search_both(idx, xq, k, flags=0):
    """(prefiltered result, its info, fp32 result) of one index"""
    idx.set_tuning(0, 0, KNN_TUNE_SCAN16_ANY_NB | flags)
    got = idx.search(xq, k)
    info = idx.last_scan16()
    assert info["used"], info
    assert idx.last_scan()["kernel"] == "flat_scan_q32_d256_f16x", idx.last_scan()
    idx.set_tuning(0, 0, KNN_TUNE_NO_SCAN16 | flags)
    ref = idx.search(xq, k)
    assert not idx.last_scan16()["used"]
    idx.set_tuning(0, 0, KNN_TUNE_SCAN16_ANY_NB | flags)
    return got, info, ref


# Every value of rows, d, nq and k of the list above at least twice, each k with each number of rows.  k = 1984 leaves the
# window k' - k = 64 keys: the bound B_q is about 2^-12 |q| |x| whatever d is, while unit rows' scores crowd as sqrt(d), so at
# d = 1024 such a window overflows on random rows (about 50 rows within 2 B_q of the 1984-th of 4096) and the search falls
# back; at d = 100 and d = 8 it holds under 20.  d = 1024 meets k' = 2048 where 300 rows leave every window open.
SHAPES = [
    (300, 8, 1, 1), (300, 100, 5, 10), (300, 1024, 32, 100), (300, 100, 5, 1000), (300, 8, 32, 1984), (300, 1024, 5, 1984),
    (4096, 100, 1, 1), (4096, 1024, 5, 10), (4096, 8, 5, 100), (4096, 100, 32, 1000), (4096, 100, 1, 1984),
    (20000, 100, 32, 1), (20000, 8, 32, 10), (20000, 100, 1, 100), (20000, 1024, 32, 100), (20000, 1024, 32, 1000),
    (20000, 100, 5, 1984),
]


@pytest.mark.parametrize("nb,d,nq,k", SHAPES)
def test_normalised_rows_no_fallback(gpu_faiss, oracle, nb, d, nq, k):
    xb, xq = _data("normed", nb, d, nq)
    idx = _index(gpu_faiss, xb)
    before = idx.last_scan16()["fallbacks"]
    got, info, ref = _search_both(idx, xq, k)
    assert _same(got, ref), "prefiltered search differs from the fp32 scan"
    assert _same(got, _want(oracle, "normed", nb, d, nq, k)), "prefiltered search differs from the oracle"
    assert info["fallbacks"] == before, info
    assert info["candidates_max"] >= min(k, nb), info


@pytest.mark.parametrize("kind", ["near", "const"])
@pytest.mark.parametrize("nb,d,nq,k", [(4096, 100, 5, 10), (20000, 1024, 32, 100), (20000, 8, 1, 1000), (4096, 1024, 32, 1984)])
def test_overflowing_window_takes_the_fallback(gpu_faiss, oracle, kind, nb, d, nq, k):
    xb, xq = _data(kind, nb, d, nq)
    idx = _index(gpu_faiss, xb)
    before = idx.last_scan16()["fallbacks"]
    got, info, ref = _search_both(idx, xq, k)
    assert _same(got, ref), "fallback differs from the fp32 scan"
    assert _same(got, _want(oracle, kind, nb, d, nq, k)), "fallback differs from the oracle"
    assert info["fallbacks"] == before + 1, info


@pytest.mark.parametrize("nb,d,nq,k", [(300, 8, 1, 10), (4096, 100, 5, 100), (20000, 1024, 32, 1000)])
def test_query_that_is_not_finite(gpu_faiss, nb, d, nq, k):
    xb, xq = _data("nanq", nb, d, nq)
    idx = _index(gpu_faiss, xb)
    before = idx.last_scan16()["fallbacks"]
    got, info, ref = _search_both(idx, xq, k)
    assert _same(got, ref), "fallback differs from the fp32 scan"
    assert info["fallbacks"] == before + 1, info
    xi = xq.copy()
    xi[0, 0] = np.inf
    got, info, ref = _search_both(idx, xi, k)
    assert _same(got, ref)
    assert info["fallbacks"] == before + 2, info


# ---- sequences of searches on one handle: every search returns what a fresh handle returns ----------------------------

A = ("normed", 20000, 100, 32, 100)
B = ("normed", 20000, 100, 5, 1000)   # (its queries and k against A's rows: another k', another number of queries)
F = ("near", 20000, 100, 32, 100)     # (query 0 overflows its window)


def _fresh(faiss, case, flags):
    kind, nb, d, nq, k = case
    xb, xq = _data(kind, nb, d, nq)
    return _index(faiss, xb, flags).search(xq, k)


@pytest.mark.parametrize("flags", [0, KNN_TUNE_ALWAYS_RESET], ids=["default", "always_reset"])
def test_same_shape_three_times(gpu_faiss, oracle, flags):
    xb, xq = _data(*A[:4])
    idx = _index(gpu_faiss, xb, flags)
    want = _want(oracle, *A)
    assert _same(_fresh(gpu_faiss, A, flags), want)
    for _ in range(3):
        got = idx.search(xq, A[4])
        assert idx.last_scan16()["used"] and idx.last_scan16()["fallbacks"] == 0
        assert _same(got, want)


@pytest.mark.parametrize("flags", [0, KNN_TUNE_ALWAYS_RESET], ids=["default", "always_reset"])
def test_shape_a_b_a(gpu_faiss, oracle, flags):
    xb, _ = _data(*A[:4])
    idx = _index(gpu_faiss, xb, flags)  # (A and B: the same rows, other queries and k)
    for case in (A, B, A, B, B, A):
        xq = _data(*case[:4])[1]
        got = idx.search(xq, case[4])
        assert idx.last_scan16()["used"]
        want = oracle.flat_search(xb, xq, case[4], IP)
        assert _same(got, want), case
    assert idx.last_scan16()["fallbacks"] == 0


@pytest.mark.parametrize("flags", [0, KNN_TUNE_ALWAYS_RESET], ids=["default", "always_reset"])
def test_fallback_taken_not_taken_taken(gpu_faiss, oracle, flags):
    """One index, queries of one shape: query 0 of xf sits on a block of near-duplicates, the queries of xn do not."""
    xb, xf = _data(*F[:4])
    xn = _data("normed", 20000, 100, 32, seed=3)[1]
    idx = _index(gpu_faiss, xb, flags)
    k = F[4]
    want_f, want_n = _want(oracle, *F), oracle.flat_search(xb, xn, k, IP)
    assert _same(_index(gpu_faiss, xb, flags).search(xf, k), want_f)
    assert _same(_index(gpu_faiss, xb, flags).search(xn, k), want_n)
    taken = 0
    for xq, want, falls in ((xf, want_f, 1), (xn, want_n, 0), (xf, want_f, 1), (xn, want_n, 0), (xn, want_n, 0), (xf, want_f, 1)):
        got = idx.search(xq, k)
        taken += falls
        info = idx.last_scan16()
        assert info["used"] and info["fallbacks"] == taken, info
        assert _same(got, want)


@pytest.mark.parametrize("flags", [0, KNN_TUNE_ALWAYS_RESET], ids=["default", "always_reset"])
def test_view_between_the_parents_searches(gpu_faiss, oracle, flags):
    xb, xq = _data(*A[:4])
    k = A[4]
    idx = _index(gpu_faiss, xb, flags)
    view = idx.view()
    view.set_tuning(0, 0, KNN_TUNE_SCAN16_ANY_NB | flags)
    want = _want(oracle, *A)
    xq_b, k_b = _data(*B[:4])[1], B[4]
    want_b = oracle.flat_search(xb, xq_b, k_b, IP)
    for who, q, kk, w in ((idx, xq, k, want), (view, xq, k, want), (idx, xq, k, want), (view, xq_b, k_b, want_b), (idx, xq, k, want),
                          (view, xq, k, want)):
        got = who.search(q, kk)
        assert who.last_scan16()["used"]
        assert _same(got, w)


@pytest.mark.parametrize("flags", [0, KNN_TUNE_ALWAYS_RESET], ids=["default", "always_reset"])
def test_both_lanes_alternating(gpu_faiss, oracle, flags):
    """HipShardBackend's two lanes (the index and a view of it, a stream each), searches alternating between them, a
    fallback among them; then the packed keys with a non-zero id base, from the prefiltered search and from the fp32 scan."""
    import torch
    from knn_for_homology_amd.sharded import HipShardBackend
    xb, xf = _data(*F[:4])
    xn = _data("normed", 20000, 100, 32, seed=3)[1]
    k, base = F[4], 70000
    b = HipShardBackend(100, IP)
    b.add(xb)
    want = {id(xf): _want(oracle, *F), id(xn): oracle.flat_search(xb, xn, k, IP)}
    dev = {id(x): torch.from_numpy(x.copy()).cuda() for x in (xf, xn)}
    torch.cuda.synchronize()
    results = []
    for x in (xn, xn, xf, xn, xn, xf, xn, xn):
        index, stream = b.next_lane()
        index.set_tuning(0, 0, KNN_TUNE_SCAN16_ANY_NB | flags)
        with torch.cuda.stream(stream):
            results.append((x, index, b.search(dev[id(x)], k, index=index), b.search_keys(dev[id(x)], k, base, index=index)))
    torch.cuda.synchronize()
    lanes = {id(index): index for _, index, _, _ in results}
    assert len(lanes) == 2
    for x, index, (D, I), keys in results:
        assert index.last_scan16()["used"]
        assert _same((D.cpu().numpy(), I.cpu().numpy()), want[id(x)])
        assert np.array_equal((keys.cpu().numpy() & 0xFFFFFFFF).astype(np.int64) - base, want[id(x)][1])
    assert sum(index.last_scan16()["fallbacks"] for index in lanes.values()) == 4  # (xf twice: D / I and the keys)
    # the keys' score words: those of the fp32 scan
    index = b.index
    with torch.cuda.stream(b.next_lane()[1]):
        index.set_tuning(0, 0, KNN_TUNE_SCAN16_ANY_NB | flags)
        got = b.search_keys(dev[id(xn)], k, base, index=index).cpu().numpy()
        assert index.last_scan16()["used"]
        index.set_tuning(0, 0, KNN_TUNE_NO_SCAN16 | flags)
        ref = b.search_keys(dev[id(xn)], k, base, index=index).cpu().numpy()
        assert not index.last_scan16()["used"]
    assert np.array_equal(got, ref)


# knn_last_scan16_info on three fixed cases: (used, candidates_max) as the commit before the sliced re-scoring reported them
# (recorded once from that commit's library on an MI355X with exactly these inputs)
INFO_CASES = [
    (("normed", 20000, 100, 32, 100), (True, 107)),
    (("normed", 4096, 1024, 5, 10), (True, 13)),
    (("normed", 20000, 1024, 32, 1000), (True, 1130)),
]


@pytest.mark.parametrize("case,recorded", INFO_CASES)
def test_last_scan16_info_as_recorded(gpu_faiss, case, recorded):
    kind, nb, d, nq, k = case
    xb, xq = _data(kind, nb, d, nq)
    idx = _index(gpu_faiss, xb)
    idx.search(xq, k)
    info = idx.last_scan16()
    print(f"scan16 info {case}: {info}")
    assert (info["used"], info["candidates_max"]) == recorded
