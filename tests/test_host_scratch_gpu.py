"""GPU: what the host entries take for one call -- pooled buffers, streams, events -- goes back whichever way the call
returns.  Only pool accounting (knn_trim returns the bytes the pool held, and empties it) and results are checked; nothing
here makes HIP fail.

  (1) steady pool: a second and a third call leave the same bytes in the pool as one another (a buffer that is not
      returned, or returned twice, moves the count), and give the first call's result bit for bit.  knn_flat_read_rate's
      result is a byte count and a measured time: the count is compared, the time only has to be positive.
  (2) knn_pool_ranges_dev refusing a range returns its scratch like a good call, and a good call behind it is right
  (4) an index that reserved its rows and one that grew into them answer alike, and both kill the views made before the
      move.  (An empty index has no storage a view could outlive, so both indexes hold 20 rows when the view is made; the
      first then reserves 200 and takes two adds, the second takes the same two adds and grows at each.)

The two-lane knn_normalize_l2 (more than 64 MiB of rows) is tests/test_flat_gpu.py::test_normalize_l2_in_chunks_matches_oracle."""
import ctypes

import numpy as np
import pytest

import pool_reference as ref
from knn_for_homology_amd import _lib
from knn_for_homology_amd._lib import Knn355Error

pytestmark = pytest.mark.gpu

POOL_ROWS, POOL_D = 40, 8
POOL_STARTS = np.asarray([0, 5, 5, 39, 10], np.int64)
POOL_STOPS = np.asarray([40, 6, 13, 40, 30], np.int64)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def pool_case(gpu_faiss):
    """the rows on the device, and the restated result of the five ranges: computed once, never modified"""
    import torch
    x = ref.residues(POOL_ROWS, POOL_D, 77)
    return torch, torch.from_numpy(x).cuda(), ref.pool_sequential(x, POOL_STARTS, POOL_STOPS)


def _pool_dev(torch, t, starts, stops):
    """knn_pool_ranges_dev on the current stream -> (rc, the pooled rows; untouched rows stay 7.0)"""
    ta, tb = torch.from_numpy(starts).cuda(), torch.from_numpy(stops).cuda()
    out = torch.full((len(starts), POOL_D), 7.0, dtype=torch.float32, device="cuda")
    rc = _lib.lib().knn_pool_ranges_dev(t.data_ptr(), 0, POOL_ROWS, POOL_D, POOL_D, ta.data_ptr(), tb.data_ptr(), len(starts), 0, out.data_ptr(),
                                        ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    return rc, out.cpu().numpy()


def _steady(call, same):
    """call() three times; the pool holds the same bytes behind the second and the third, and their results are the first's"""
    L = _lib.lib()
    L.knn_trim()
    first = call()
    second = call()
    t1 = L.knn_trim()
    third = call()
    t2 = L.knn_trim()
    assert t1 == t2, f"the pool held {t1} bytes behind the second call and {t2} behind the third"
    assert same(second, first) and same(third, first), "a later call's result differs from the first call's"
    return first


def test_steady_pool_normalize_l2(gpu_faiss, oracle):
    x = np.random.default_rng(11).standard_normal((300, 8)).astype(np.float32)
    want = x.copy()
    oracle.normalize_l2(want)

    def call():
        y = x.copy()
        gpu_faiss.normalize_L2(y)
        return y

    first = _steady(call, lambda a, b: np.array_equal(_bits(a), _bits(b)))
    assert np.array_equal(_bits(first), _bits(want))


def test_steady_pool_read_rate(gpu_faiss):
    idx = gpu_faiss.IndexFlat(8)
    idx.add(np.random.default_rng(12).standard_normal((300, 8)).astype(np.float32))

    def call():
        ms, nbytes = ctypes.c_float(-1.0), ctypes.c_int64(-1)
        _lib.check(_lib.lib().knn_flat_read_rate(idx._h, 1, ctypes.byref(ms), ctypes.byref(nbytes)))
        assert ms.value > 0.0
        return nbytes.value

    assert _steady(call, lambda a, b: a == b) == 300 * 32 * 4  # (d = 8 is stored as rows of 32 floats)


def test_steady_pool_pool_ranges_dev(pool_case):
    torch, t, want = pool_case

    def call():
        rc, out = _pool_dev(torch, t, POOL_STARTS, POOL_STOPS)
        assert rc == 0, _lib.lib().knn_last_error()
        return out

    first = _steady(call, lambda a, b: np.array_equal(_bits(a), _bits(b)))
    assert len(ref.bits_differ(first, want)) == 0


def test_refused_pool_ranges_dev_returns_its_scratch(pool_case):
    torch, t, want = pool_case
    L = _lib.lib()
    bad = POOL_STOPS.copy()
    bad[3] = POOL_ROWS + 1
    L.knn_trim()
    rc, _ = _pool_dev(torch, t, POOL_STARTS, POOL_STOPS)
    assert rc == 0, L.knn_last_error()
    after_good = L.knn_trim()
    rc, out = _pool_dev(torch, t, POOL_STARTS, bad)
    assert rc == -1 and b"range 3 " in L.knn_last_error(), L.knn_last_error()
    assert (out[3] == 7.0).all(), "the row of the bad range was written"
    after_refused = L.knn_trim()
    assert after_refused == after_good, f"a refused call left {after_refused} bytes in the pool, a good one {after_good}"
    rc, out = _pool_dev(torch, t, POOL_STARTS, POOL_STOPS)
    assert rc == 0, L.knn_last_error()
    assert len(ref.bits_differ(out, want)) == 0


@pytest.mark.parametrize("metric", [0, 1], ids=["ip", "l2"])
def test_reserve_and_growth_agree(gpu_faiss, oracle, metric):
    rng = np.random.default_rng(13 + metric)
    x = rng.standard_normal((50, 8)).astype(np.float32)
    xq = rng.standard_normal((5, 8)).astype(np.float32)
    reserved, grown = gpu_faiss.IndexFlat(8, metric), gpu_faiss.IndexFlat(8, metric)
    views = []
    for idx in (reserved, grown):
        idx.add(x[:20])
        views.append(idx.view())
        views[-1].search(xq, 3)  # (alive: it searches)
    _lib.check(_lib.lib().knn_flat_reserve(reserved._h, 200))
    for idx in (reserved, grown):
        idx.add(x[20:35])
        idx.add(x[35:])
        assert idx.ntotal == 50
    wD, wI = oracle.flat_search(x, xq, 10, metric)
    for idx, name in ((reserved, "reserved"), (grown, "grown")):
        D, I = idx.search(xq, 10)
        assert np.array_equal(I, wI) and np.array_equal(_bits(D), _bits(wD)), name
        assert np.array_equal(_bits(idx.reconstruct_n(0, 50)), _bits(x)), name
    for v, name in zip(views, ("reserved", "grown")):
        with pytest.raises(Knn355Error, match="this view is stale"):
            v.search(xq, 3)
        assert v.ntotal == 20, name
