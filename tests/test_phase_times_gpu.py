"""GPU: the HIP-event figures behind every knn_*_last_ms / knn_last_*_info getter (PhaseClock, csrc/host_core.inc).  After one
tiny successful call every figure is finite and >= 0, the phases that ran sum to > 0 and a phase that did not run is exactly
0.0; the same holds when a call walks eight slabs or several chunks, whose results are the one-slab results bit for bit; and
a call that is refused with KNN_ERR_INVALID leaves the previous figures byte for byte.  Every entry is called through the C
ABI, so that a refused call is the library's refusal and not the facade's."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

INVALID = -1  # KNN_ERR_INVALID
F32, F64 = 0, 1  # KNN_RANK_F32, KNN_RANK_F64
SLAB = "KNN355_EVAL_SLAB_ROWS"
CHUNK = "KNN355_POOL_CHUNK_ROWS"


@pytest.fixture(scope="module")
def L(gpu_faiss):
    from knn_for_homology_amd import _lib
    return _lib.lib()


def p(a):
    return None if a is None else a.ctypes.data


def floats(n):
    return (ctypes.c_float * n)()


def check_ms(ms, zero=()):
    """the three conditions of one successful call; returns the figures"""
    ms = np.asarray(ms, np.float32)
    assert np.isfinite(ms).all() and (ms >= 0).all(), ms
    assert sum(float(v) for i, v in enumerate(ms) if i not in zero) > 0, ms
    for i in zero:
        assert ms[i] == 0.0, (i, ms)
    return ms


def refused_keeps(read, refuse):
    """a call refused with KNN_ERR_INVALID behind a good one: the figures are the same bytes"""
    before = read().tobytes()
    assert refuse() == INVALID
    assert read().tobytes() == before


# ---- the hit-matrix entries: buckets, hit curve, overlap ---------------------------------------------------------------
class Hits:
    def __init__(self, nq=50, k=20):
        rng = np.random.default_rng(2)
        self.nq, self.k = nq, k
        self.correct = (rng.random((nq, k)) < 0.5).astype(np.uint8)
        self.scores = (self.correct * 0.5 + rng.random((nq, k)) * 0.25).astype(np.float32)
        self.totals = np.full(nq, k, np.int64)
        self.lo = np.linspace(0.0, 0.9, 10)
        self.hi = self.lo + 0.1
        self.hits_a = np.stack([rng.permutation(100)[:k] for _ in range(nq)]).astype(np.int64)
        self.hits_b = np.stack([rng.permutation(100)[:k] for _ in range(nq)]).astype(np.int64)
        self.correct_b = (rng.random((nq, k)) < 0.5).astype(np.uint8)

    def counts(self, L, limit=None):
        count, cor = np.full(10, -7777, np.int64), np.full(10, -7777, np.int64)
        rc = L.knn_eval_bucket_counts(p(self.scores), F32, p(self.correct), self.nq, self.k, self.k if limit is None else limit, p(self.lo), p(self.hi), 10,
                                      p(count), p(cor))
        return rc, count, cor

    def curve(self, L, limit=None):
        mean, rows, cols = np.full(self.k, -7777.25), np.full(self.nq, -7777, np.int64), np.full(self.k, -7777, np.int64)
        rc = L.knn_eval_hit_curve(p(self.correct), self.nq, self.k, self.k if limit is None else limit, p(self.totals), p(mean), p(rows), p(cols))
        return rc, mean, rows, cols

    def overlap(self, L, out=True):
        tp, lead = np.full((self.nq, 3), -7777, np.int32), np.full((self.nq, 3), -7777, np.int32)
        rc = L.knn_eval_overlap(p(self.hits_a), p(self.correct), self.k, p(self.hits_b), p(self.correct_b), self.k, self.nq, p(tp) if out else None,
                                p(lead) if out else None)
        return rc, tp, lead


def buckets_ms(L):
    a, b = floats(3), floats(3)
    assert L.knn_eval_buckets_last_ms(a, b) == 0
    return np.array(list(a) + list(b), np.float32)


def overlap_ms(L):
    a = floats(3)
    assert L.knn_eval_overlap_last_ms(a) == 0
    return np.array(list(a), np.float32)


@pytest.mark.parametrize("slab_rows", [None, "7"])  # "7": eight slabs at 50 rows, every phase the sum of eight intervals
def test_hit_matrix_entries(L, monkeypatch, slab_rows):
    h = Hits()
    monkeypatch.delenv(SLAB, raising=False)
    whole = [h.counts(L), h.curve(L), h.overlap(L)]
    if slab_rows:
        monkeypatch.setenv(SLAB, slab_rows)
    got = [h.counts(L), h.curve(L), h.overlap(L)]
    for a, b in zip(got, whole):
        assert a[0] == 0 and b[0] == 0
        for x, y in zip(a[1:], b[1:]):
            assert x.tobytes() == y.tobytes()  # (the one-slab results, bit for bit)
    ms = buckets_ms(L)
    check_ms(ms[:3])
    check_ms(ms[3:])
    check_ms(overlap_ms(L))
    assert (whole[0][1] >= 0).all() and whole[0][1].sum() > 0 and (whole[2][1] >= 0).all()
    refused_keeps(lambda: buckets_ms(L), lambda: h.counts(L, limit=0)[0])
    refused_keeps(lambda: buckets_ms(L), lambda: h.curve(L, limit=0)[0])
    refused_keeps(lambda: overlap_ms(L), lambda: h.overlap(L, out=False)[0])


# ---- pool_ranges ---------------------------------------------------------------------------------------------------------
def pool_ms(L):
    a, b, c = ctypes.c_float(), ctypes.c_float(), ctypes.c_float()
    assert L.knn_pool_last_ms(ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)) == 0
    return np.array([a.value, b.value, c.value], np.float32)


def pool_case():
    rng = np.random.default_rng(3)
    x = rng.standard_normal((64, 8)).astype(np.float32)
    starts = np.arange(0, 64, 4, dtype=np.int64)  # 16 ranges spread over all the rows
    stops = starts + 4
    return x, starts, stops


def pool_host(L, x, starts, stops, out=True):
    res = np.full((len(starts), x.shape[1]), -7777.25, np.float32)
    return L.knn_pool_ranges(p(x), 0, x.shape[0], x.shape[1], p(starts), p(stops), len(starts), 0, p(res) if out else None), res


@pytest.mark.parametrize("chunk_rows", [None, "16"])  # "16": four chunks of four ranges, two upload buffers taking turns
def test_pool_ranges_host(L, monkeypatch, chunk_rows):
    x, starts, stops = pool_case()
    monkeypatch.delenv(CHUNK, raising=False)
    rc, whole = pool_host(L, x, starts, stops)
    assert rc == 0
    if chunk_rows:
        monkeypatch.setenv(CHUNK, chunk_rows)
    rc, got = pool_host(L, x, starts, stops)
    assert rc == 0 and got.tobytes() == whole.tobytes()
    assert np.allclose(got, x.reshape(16, 4, 8).mean(axis=1), rtol=1e-5, atol=1e-6)
    check_ms(pool_ms(L))
    refused_keeps(lambda: pool_ms(L), lambda: pool_host(L, x, starts, stops, out=False)[0])


def test_pool_ranges_dev(L):
    import torch
    x, starts, stops = pool_case()
    dx, ds, de = torch.from_numpy(x).cuda(), torch.from_numpy(starts).cuda(), torch.from_numpy(stops).cuda()
    out = torch.zeros((16, 8), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()

    def call(out_ptr):
        return L.knn_pool_ranges_dev(dx.data_ptr(), 0, 64, 8, 8, ds.data_ptr(), de.data_ptr(), 16, 0, out_ptr, None)

    assert pool_host(L, x, starts, stops)[0] == 0  # (figures of another call in all three places)
    assert call(out.data_ptr()) == 0
    assert np.allclose(out.cpu().numpy(), x.reshape(16, 4, 8).mean(axis=1), rtol=1e-5, atol=1e-6)
    check_ms(pool_ms(L), zero=(0, 2))  # the device entry moves nothing: upload and download are 0
    refused_keeps(lambda: pool_ms(L), lambda: call(None))
    # refused behind the launches, by the entry's own status word: a range that ends past the rows is skipped by the pooling
    # kernel (test_pool_gpu.py: nothing is read for it) and reported as KNN_ERR_INVALID once the stream has drained -- the
    # figures were measured and must not be committed
    bad = stops.copy()
    bad[5] = 65
    db = torch.from_numpy(bad).cuda()
    torch.cuda.synchronize()
    assert pool_host(L, x, starts, stops)[0] == 0  # (three non-zero figures: a commit of the failed call's would show)
    refused_keeps(lambda: pool_ms(L),
                  lambda: L.knn_pool_ranges_dev(dx.data_ptr(), 0, 64, 8, 8, ds.data_ptr(), db.data_ptr(), 16, 0, out.data_ptr(), None))


# ---- PCA -----------------------------------------------------------------------------------------------------------------
def pca_ms(L):
    a, b = floats(4), ctypes.c_float()
    assert L.knn_pca_last_ms(a, ctypes.byref(b)) == 0
    return np.array(list(a) + [b.value], np.float32)


def test_pca(L, monkeypatch):
    monkeypatch.delenv(SLAB, raising=False)
    x = np.random.default_rng(4).standard_normal((64, 16)).astype(np.float32)
    mean, cov = np.zeros(16, np.float32), np.zeros((16, 16))
    assert L.knn_pca_moments(p(x), 64, 16, p(mean), p(cov)) == 0
    assert np.allclose(mean, x.mean(axis=0), atol=1e-5)
    comp = np.ascontiguousarray(np.eye(16, dtype=np.float32)[:3])

    def project(out):
        return L.knn_pca_project(p(x), 64, 16, p(mean), p(comp), 3, p(out))

    whole = np.zeros((64, 3), np.float32)
    assert project(whole) == 0
    ms = pca_ms(L)
    check_ms(ms[:4])
    check_ms(ms[4:])
    monkeypatch.setenv(SLAB, "7")  # ten slabs: the projection's figure is the sum over them
    got = np.zeros((64, 3), np.float32)
    assert project(got) == 0 and got.tobytes() == whole.tobytes()
    check_ms(pca_ms(L)[4:])
    refused_keeps(lambda: pca_ms(L), lambda: L.knn_pca_moments(p(x), 64, 16, None, p(cov)))
    refused_keeps(lambda: pca_ms(L), lambda: project(None))


# ---- KDE -----------------------------------------------------------------------------------------------------------------
def kde_ms(L):
    a, b = floats(2), floats(3)
    assert L.knn_kde_last_ms(a, b) == 0
    return np.array(list(a) + list(b), np.float32)


def test_kde(L):
    rng = np.random.default_rng(5)
    x = rng.standard_normal((100, 2)).astype(np.float32)
    st = [np.zeros(2) for _ in range(4)]
    assert L.knn_kde_stats(p(x), 0, 100, 2, 2, *[p(s) for s in st]) == 0
    assert np.allclose(st[2], x.astype(np.float64).mean(axis=0))
    grid = np.ascontiguousarray(np.tile(np.linspace(-2.0, 2.0, 16), (2, 1)))
    inv_h, norm = np.full(2, 2.0), np.full(2, 0.01)
    out = np.zeros((2, 16))
    assert L.knn_kde_eval(p(x), 0, 100, 2, 2, p(grid), 16, p(inv_h), p(norm), p(out)) == 0
    assert (out > 0).all()
    ms = kde_ms(L)
    check_ms(ms[:2])
    check_ms(ms[2:])
    refused_keeps(lambda: kde_ms(L), lambda: L.knn_kde_stats(p(x), 0, 100, 2, 2, None, p(st[1]), p(st[2]), p(st[3])))
    refused_keeps(lambda: kde_ms(L), lambda: L.knn_kde_eval(p(x), 0, 100, 2, 2, p(grid), 16, p(inv_h), p(norm), None))


# ---- LayerMix ------------------------------------------------------------------------------------------------------------
def mix_ms(L):
    a, b, c = ctypes.c_float(), ctypes.c_float(), ctypes.c_float()
    assert L.knn_mix_last_ms(ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)) == 0
    return np.array([a.value, b.value, c.value], np.float32)


def test_mix(L, gpu_faiss):
    from knn_for_homology_amd import layers
    rng = np.random.default_rng(6)
    x = [rng.standard_normal((40, 16)).astype(np.float32) for _ in range(2)]
    lm = layers.LayerMix(x)
    mapping = np.repeat(np.arange(10, dtype=np.int32), 4)[:, None]
    ratios = np.array([[1.0, 0.0], [0.5, 0.5], [0.0, 1.0]], np.float32)  # G = 3: every phase the sum of three intervals
    got = lm.sweep(ratios, mapping)
    assert got.counts.shape == (3, 1) and (got.counts >= 0).all() and (got.counts <= 40).all()
    check_ms(mix_ms(L))
    counts = np.full((3, 1), -7777, np.int64)
    refused_keeps(lambda: mix_ms(L), lambda: L.knn_mix_sweep(lm._h, p(ratios), 3, lm._flat._h, 2, None, 1, 1, p(counts), None, None))
    assert (counts == -7777).all()
    assert lm.index((0.25, 0.75)).ntotal == 40
    check_ms(mix_ms(L), zero=(1, 2))  # knn_mix_into neither searches nor scores
    refused_keeps(lambda: mix_ms(L), lambda: L.knn_mix_into(lm._h, None, lm._flat._h, 1))


# ---- refine and the LSH training -------------------------------------------------------------------------------------------
def refine_ms(L, flat):
    a, b = ctypes.c_float(), ctypes.c_float()
    assert L.knn_last_refine_ms(flat._h, ctypes.byref(a), ctypes.byref(b)) == 0
    return np.array([a.value, b.value], np.float32)


def train_ms(L, lsh):
    v = [ctypes.c_float() for _ in range(3)]
    assert L.knn_lsh_last_train_ms(lsh._h, *[ctypes.byref(c) for c in v]) == 0
    return np.array([c.value for c in v], np.float32)


def test_refine_and_lsh_train(L, gpu_faiss):
    from knn_for_homology_amd.lsh import IndexLSH
    rng = np.random.default_rng(7)
    rows = rng.standard_normal((300, 32)).astype(np.float32)
    q = np.ascontiguousarray(rows[:5] + 0.01)
    D, I = np.zeros((5, 4), np.float32), np.zeros((5, 4), np.int64)
    # knn_flat_refine: nq = 5, kb = 8, k = 4
    flat = gpu_faiss.IndexFlat(32, gpu_faiss.METRIC_L2)
    flat.add(rows)
    labels = np.ascontiguousarray(flat.search(q, 8)[1], np.int64)
    assert L.knn_flat_refine(flat._h, p(q), 5, p(labels), 8, 4, p(D), p(I)) == 0
    assert np.array_equal(I[:, 0], np.arange(5))
    check_ms(refine_ms(L, flat))
    refused_keeps(lambda: refine_ms(L, flat), lambda: L.knn_flat_refine(flat._h, p(q), 5, p(labels), 8, 4, None, p(I)))
    # knn_lsh_train: d = 32, 64 bits, 300 rows
    lsh = IndexLSH(32, 64, train_thresholds=True)
    index = gpu_faiss.IndexRefineFlat(lsh)
    index.train(rows)
    check_ms(train_ms(L, lsh))
    refused_keeps(lambda: train_ms(L, lsh), lambda: L.knn_lsh_train(lsh._h, p(rows), 0))
    # knn_lsh_search_refine on a handle of its own (its figures start at zero)
    index.add(rows)
    fresh = index.refine_index
    assert refine_ms(L, fresh).tobytes() == np.zeros(2, np.float32).tobytes()
    assert L.knn_lsh_search_refine(lsh._h, fresh._h, p(q), 5, 8, 4, p(D), p(I)) == 0
    assert (I >= 0).all() and (I < 300).all()
    check_ms(refine_ms(L, fresh))
    refused_keeps(lambda: refine_ms(L, fresh), lambda: L.knn_lsh_search_refine(lsh._h, fresh._h, p(q), 5, 8, 4, None, p(I)))


# ---- rank and windows ------------------------------------------------------------------------------------------------------
def rank_ms(L):
    a, b, t, ms = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int64(), floats(6)
    assert L.knn_last_rank_info(ctypes.byref(a), ctypes.byref(b), ctypes.byref(t), ms) == 0
    return np.array(list(ms), np.float32)


def windows_ms(L):
    a, b, c, ms = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64(), floats(8)
    assert L.knn_last_windows_info(ctypes.byref(a), ctypes.byref(b), ctypes.byref(c), ms) == 0
    return np.array(list(ms), np.float32)


def test_rank(L):
    h = Hits()  # N = 50 * 20 = 1000
    order, cum = np.zeros(1000, np.int64), np.zeros(1000, np.int64)

    def rank(limit):
        return L.knn_eval_rank(p(h.scores), F32, 50, 20, limit, p(h.correct), 1, p(order), p(cum), None, 0, None, None, None, 0, None)

    assert rank(20) == 0
    assert np.array_equal(np.sort(order), np.arange(1000)) and cum[-1] == h.correct.sum()
    ms = rank_ms(L)  # host clock: allocations, packing; HIP events: upload, sort, C(r), look-ups
    check_ms(ms)
    check_ms(ms[2:])
    refused_keeps(lambda: rank_ms(L), lambda: rank(0))


def test_windows(L):
    rng = np.random.default_rng(8)
    n, m, W = 1000, 2, 50
    keys = rng.random(n).astype(np.float32)
    values = (rng.random((m, n)) < 0.5).astype(np.uint8)
    starts = np.arange(0, n, 100, dtype=np.int64)
    stops = starts + 100
    key_means, value_means = np.zeros(n), np.zeros((m, n))
    out = [np.zeros(10, np.int64), np.zeros(10, np.int64), np.zeros((m, 10), np.int64), np.zeros(10, np.float32), np.zeros(10, np.float32)]

    def windows(window, bins):
        return L.knn_eval_windows(p(keys), F32, n, p(values), m, 0, window, p(key_means), p(value_means), None, p(starts) if bins else None,
                                  p(stops) if bins else None, None, 10 if bins else 0, *[p(o) if bins else None for o in out])

    # ms: host clock: allocations; HIP events: upload, sort, gather and scans, chains, means, bins, downloads
    assert windows(W, True) == 0
    assert np.array_equal(out[2].sum(axis=1), values.sum(axis=1)) and np.isclose(key_means[:n - W + 1].mean(), 0.5, atol=0.1)
    ms = check_ms(windows_ms(L))
    check_ms(ms[1:])
    assert windows(W, False) == 0
    check_ms(windows_ms(L)[1:], zero=(5,))  # no bins: a zero bins phase
    assert windows(0, True) == 0
    check_ms(windows_ms(L)[1:], zero=(3, 4))  # no window: zero chains and means phases
    refused_keeps(lambda: windows_ms(L), lambda: windows(0, False))
