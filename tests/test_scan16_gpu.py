"""GPU: the exact 16-bit prefilter (knn_flat_set_scan16) returns the fp32 scan's bits.

Every search is compared bit for bit with the CPU oracle and with the same index under KNN_TUNE_NO_SCAN16; KNN_TUNE_SCAN16_ANY_NB
engages the path on databases small enough for the oracle."""
import numpy as np
import pytest

from knn_for_homology_amd._lib import KNN_TUNE_NO_SCAN16, KNN_TUNE_SCAN16_ANY_NB

pytestmark = pytest.mark.gpu

IP, L2 = 0, 1


def _index(faiss, xb, on=True):
    idx = faiss.IndexFlat(xb.shape[1], IP)
    if on:
        idx.set_scan16(1)
    idx.add(xb)
    return idx


def _same(a, b):
    Da, Ia = a
    Db, Ib = b
    return np.array_equal(Ia, Ib) and np.array_equal(Da.view(np.uint32), Db.view(np.uint32))


def _check(idx, xq, k, oracle=None, xb=None, expect_used=True):
    idx.set_tuning(0, 0, KNN_TUNE_SCAN16_ANY_NB)
    got = idx.search(xq, k)
    info = idx.last_scan16()
    assert info["used"] == expect_used, info
    if expect_used:
        assert idx.last_scan()["kernel"] == "flat_scan_q32_d256_f16x", idx.last_scan()
    idx.set_tuning(0, 0, KNN_TUNE_NO_SCAN16)
    ref = idx.search(xq, k)
    assert not idx.last_scan16()["used"]
    assert idx.last_scan()["kernel"] == "flat_scan_q32_d256", idx.last_scan()
    idx.set_tuning(0, 0, 0)
    assert _same(got, ref), "16-bit prefilter differs from the fp32 scan"
    if oracle is not None:
        assert _same(got, oracle.flat_search(xb, xq, k, IP)), "16-bit prefilter differs from the oracle"
    return info


@pytest.mark.parametrize("d", [32, 40, 100, 1024, 1280])
@pytest.mark.parametrize("nq,k", [(1, 1), (5, 10), (20, 100), (31, 1000), (32, 2048)])
def test_bits_match_fp32_and_oracle(gpu_faiss, oracle, d, nq, k):
    rng = np.random.default_rng(d * 1000 + nq * 10 + k)
    nb = 30011 if d >= 1024 else 60013  # (ragged last tile)
    xb = rng.standard_normal((nb, d), dtype=np.float32)
    xb /= np.linalg.norm(xb, axis=1, keepdims=True)
    xq = rng.standard_normal((nq, d), dtype=np.float32)
    xq /= np.linalg.norm(xq, axis=1, keepdims=True)
    idx = _index(gpu_faiss, xb)
    info = _check(idx, xq, k, oracle, xb, expect_used=k < 2048)  # (k = 2048: k' = k leaves no room for a window)
    if k < 2048:
        assert info["fallbacks"] == 0 and info["candidates_max"] >= k, info


def test_ties_zero_rows_and_magnitudes(gpu_faiss, oracle):
    rng = np.random.default_rng(5)
    xb = rng.standard_normal((40000, 128), dtype=np.float32)
    xb[1000:1100] = xb[7]           # exact duplicates
    xb[2000:2100] = 0.0             # zero rows
    xb[3000:3100] *= np.float32(2.0 ** 40)
    xb[3100:3200] *= np.float32(2.0 ** -40)
    xb[5000:5010, :64] *= np.float32(2.0 ** 20)  # mixed magnitudes inside a row
    xq = rng.standard_normal((20, 128), dtype=np.float32)
    xq[3] = xb[7]
    idx = _index(gpu_faiss, xb)
    _check(idx, xq, 100, oracle, xb)


def test_window_overflow_falls_back_on_device(gpu_faiss, oracle):
    """Near-duplicates of a query that fp16 cannot tell apart: more of them than the tail takes, the fallback runs."""
    rng = np.random.default_rng(9)
    d = 256
    xb = rng.standard_normal((40000, d), dtype=np.float32)
    xb /= np.linalg.norm(xb, axis=1, keepdims=True)
    xq = rng.standard_normal((8, d), dtype=np.float32)
    xq /= np.linalg.norm(xq, axis=1, keepdims=True)
    near = np.repeat(xq[2:3], 600, axis=0) + rng.standard_normal((600, d), dtype=np.float32) * np.float32(1e-6)
    xb[10000:10600] = near
    idx = _index(gpu_faiss, xb)
    before = idx.last_scan16()["fallbacks"]
    info = _check(idx, xq, 10, oracle, xb)
    assert info["fallbacks"] == before + 1, info


def test_nonfinite_row_turns_the_path_off(gpu_faiss):
    rng = np.random.default_rng(3)
    xb = rng.standard_normal((20000, 64), dtype=np.float32)
    xb[123, 5] = np.inf
    xb[456, 7] = np.nan
    xq = rng.standard_normal((4, 64), dtype=np.float32)
    idx = _index(gpu_faiss, xb)
    _check(idx, xq, 10, expect_used=False)
    idx.reset()
    idx.add(np.ones((100, 64), dtype=np.float32))  # (a reset clears the flag: finite rows again)
    idx.set_tuning(0, 0, KNN_TUNE_SCAN16_ANY_NB)
    idx.search(xq, 10)
    assert idx.last_scan16()["used"]


def test_nan_query_takes_the_fallback(gpu_faiss):
    rng = np.random.default_rng(4)
    xb = rng.standard_normal((20000, 64), dtype=np.float32)
    xq = rng.standard_normal((6, 64), dtype=np.float32)
    xq[2, 3] = np.nan
    idx = _index(gpu_faiss, xb)
    before = idx.last_scan16()["fallbacks"]
    info = _check(idx, xq, 10)
    assert info["fallbacks"] == before + 1, info


def test_growth_normalize_and_views(gpu_faiss, oracle):
    rng = np.random.default_rng(6)
    d = 96
    xb = rng.standard_normal((50000, d), dtype=np.float32) * np.float32(3.0)
    xq = rng.standard_normal((12, d), dtype=np.float32)
    idx = gpu_faiss.IndexFlat(d, IP)
    idx.set_scan16(1)
    idx.add(xb[:20000])
    early = idx.view()
    idx.add(xb[20000:])  # past the reservation: storage and copies regrow
    with pytest.raises(Exception):
        early.search(xq, 10)  # a view of the old storage is stale
    _check(idx, xq, 50, oracle, xb)
    idx.normalize_rows()
    xn = xb.copy()
    oracle.normalize_l2(xn)
    _check(idx, xq, 50, oracle, xn)
    v = idx.view()
    v.set_tuning(0, 0, KNN_TUNE_SCAN16_ANY_NB)
    got = v.search(xq, 50)
    assert v.last_scan16()["used"]
    assert _same(got, oracle.flat_search(xn, xq, 50, IP))


def test_refused_for_views_after_add_and_off_switch(gpu_faiss):
    idx = gpu_faiss.IndexFlat(64, IP)
    idx.add(np.ones((10, 64), dtype=np.float32))
    with pytest.raises(Exception):
        idx.set_scan16(1)  # rows already there
    plain = _index(gpu_faiss, np.ones((300, 64), dtype=np.float32), on=False)
    plain.set_tuning(0, 0, KNN_TUNE_SCAN16_ANY_NB)
    plain.search(np.ones((2, 64), dtype=np.float32), 5)
    assert not plain.last_scan16()["used"]


def test_sharded_submit_both_lanes(gpu_faiss, oracle):
    """ShardedFlatIndex turns the copies on: submitted searches on both lanes, with and without a fallback."""
    import torch
    from knn_for_homology_amd.sharded import ShardedFlatIndex
    rng = np.random.default_rng(11)
    d, nb = 128, 300_000
    xb = rng.standard_normal((nb, d), dtype=np.float32)
    xb /= np.linalg.norm(xb, axis=1, keepdims=True)
    xq = rng.standard_normal((32, d), dtype=np.float32)
    xq /= np.linalg.norm(xq, axis=1, keepdims=True)
    xb[777:1777] = xq[5] + rng.standard_normal((1000, d), dtype=np.float32) * np.float32(1e-7)  # query 5 overflows the window
    idx = ShardedFlatIndex(d, IP, rank=0, world=1, row_offset=0)
    idx.add(xb)
    q = torch.from_numpy(xq).cuda()
    want = oracle.flat_search(xb, xq, 100, IP)
    pend = [idx.submit(q, 100) for _ in range(4)]
    for p in pend:
        D, I = p.result()
        assert _same((D.cpu().numpy(), I.cpu().numpy()), want)
    lanes = idx.backend._lanes
    assert all(h.last_scan16()["used"] for h, _ in lanes)
    assert sum(h.last_scan16()["fallbacks"] for h, _ in lanes) == 4


def test_reserve_then_view_then_add(gpu_faiss, oracle):
    """reserve grows the fp16 copies with the rows: a view made after it stays valid through an add that fits."""
    from knn_for_homology_amd import _lib
    rng = np.random.default_rng(13)
    d = 64
    xb = rng.standard_normal((30000, d), dtype=np.float32)
    xq = rng.standard_normal((7, d), dtype=np.float32)
    idx = gpu_faiss.IndexFlat(d, IP)
    idx.set_scan16(1)
    idx.add(xb[:10000])
    old = idx.view()
    _lib.check(_lib.lib().knn_flat_reserve(idx._h, 30000))
    with pytest.raises(Exception):
        old.search(xq, 10)  # the rows and their copies moved
    v = idx.view()
    idx.add(xb[10000:20000])  # fits the reservation: nothing moves
    v.set_tuning(0, 0, KNN_TUNE_SCAN16_ANY_NB)
    got = v.search(xq, 10)
    assert v.last_scan16()["used"]
    assert _same(got, oracle.flat_search(xb[:10000], xq, 10, IP))
    _check(idx, xq, 10, oracle, xb[:20000])


def test_sharded_keys_prefiltered_without_fallback(gpu_faiss, oracle):
    """The packed keys of the all-gather path, from the prefiltered search itself (no fallback)."""
    import torch
    from knn_for_homology_amd.sharded import HipShardBackend
    rng = np.random.default_rng(17)
    d, nb, base = 128, 300_000, 5000
    xb = rng.standard_normal((nb, d), dtype=np.float32)
    xb /= np.linalg.norm(xb, axis=1, keepdims=True)
    xq = rng.standard_normal((32, d), dtype=np.float32)
    xq /= np.linalg.norm(xq, axis=1, keepdims=True)
    b = HipShardBackend(d, IP)
    b.add(xb)
    q = torch.from_numpy(xq).cuda()
    before = b.index.last_scan16()["fallbacks"]
    keys = b.search_keys(q, 100, base).cpu().numpy()
    info = b.index.last_scan16()
    assert info["used"] and info["fallbacks"] == before, info
    b.index.set_tuning(0, 0, KNN_TUNE_NO_SCAN16)
    ref = b.search_keys(q, 100, base).cpu().numpy()
    b.index.set_tuning(0, 0, 0)
    assert np.array_equal(keys, ref)
    _, I = oracle.flat_search(xb, xq, 100, IP)
    assert np.array_equal((keys & 0xFFFFFFFF).astype(np.int64) - base, I)


def test_flagship_shape_10m(gpu_faiss):
    """bench.py's headline shape: 10 M x 1024 normalised rows, 32 queries, k = 100, through the sharded backend."""
    import torch
    free, _ = torch.cuda.mem_get_info()
    if free < 70e9:
        pytest.skip("needs 70 GB of free HBM")
    from knn_for_homology_amd.sharded import HipShardBackend
    d, nb, chunk = 1024, 10_000_000, 500_000
    b = HipShardBackend(d, IP)
    b.reserve(nb)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(23)
    for _ in range(0, nb, chunk):
        x = torch.randn((chunk, d), generator=gen, device="cuda", dtype=torch.float32)
        x /= x.norm(dim=1, keepdim=True)
        b.add_dev(x)
        del x
    q = torch.randn((32, d), generator=gen, device="cuda", dtype=torch.float32)
    q /= q.norm(dim=1, keepdim=True)
    torch.cuda.synchronize()
    keys = b.search_keys(q, 100, 0).cpu().numpy()
    info = b.index.last_scan16()
    print(f"flagship shape: {info}")
    assert info["used"] and info["fallbacks"] == 0, info
    b.index.set_tuning(0, 0, KNN_TUNE_NO_SCAN16)
    ref = b.search_keys(q, 100, 0).cpu().numpy()
    assert np.array_equal(keys, ref)
