"""GPU: the shard key exchange, bit for bit.  knn_flat_search_keys_dev against keys packed on the host from the oracle's
result; knn_merge_keys_dev (list-major select_topk_kernel) against numpy.sort on uint64 (tests/merge_reference.py) on synthetic
all-gather buffers -- every build launch_select can pick for a merge, both sides of every threshold, the memory path, the
status row of sharded.py, a world of 8 at k = 1000 and 2048 -- and the 32-bit range of the global ids.

One GPU serves here, so a world larger than 1 exists only as stacked key lists; that is all the merge ever sees of it."""
import ctypes
import functools

import numpy as np
import pytest

import merge_reference as mr
from merge_reference import IP, KEY_PAD, L2

pytestmark = pytest.mark.gpu

KNN_ERR_INVALID = -1

# ---- (a) the builds of select_topk_kernel a merge can run ---------------------------------------------------------------


def select_build(nq, n):
    """(R, NT) of the select_topk_kernel<R, NT, false> that launch_select (csrc/flat_search.inc) launches for a list-major merge of
    n = nlists * k keys per query -- a mirror of its choice, kept beside the table that must reach every branch of it"""
    if nq >= 512 and n <= 64 * 32:  # one wave per query
        return (8, 64) if n <= 64 * 8 else (32, 64)
    if n <= 256 * 4:
        return (4, 256)
    if n <= 256 * 16:
        return (16, 256)
    if n <= 256 * 32:
        return (32, 256)
    return (32, 1024)


def in_registers(nq, n):
    """the kernel holds its keys in registers up to NT * R of them and re-reads longer arrays on every probe (for_each_mem)"""
    R, NT = select_build(nq, n)
    return n <= R * NT


# (nq, nlists, k, the build the case is there for, registers?)
TABLE = [
    (512, 1, 1, (8, 64), True), (512, 8, 64, (8, 64), True),
    (512, 8, 65, (32, 64), True), (512, 2, 1000, (32, 64), True), (512, 2, 1024, (32, 64), True),
    (512, 3, 683, (16, 256), True),                                   # 2049 keys: past the wave builds
    (5, 1, 1, (4, 256), True), (5, 4, 256, (4, 256), True),
    (5, 5, 205, (16, 256), True), (5, 2, 2048, (16, 256), True),
    (5, 4, 1025, (32, 256), True), (5, 8, 1000, (32, 256), True), (5, 8, 1024, (32, 256), True),
    (5, 8, 1025, (32, 1024), True), (5, 8, 2048, (32, 1024), True), (5, 16, 2048, (32, 1024), True),
    (3, 17, 2048, (32, 1024), False), (3, 33, 1000, (32, 1024), False), (3, 64, 2048, (32, 1024), False),
    (511, 8, 64, (4, 256), True), (513, 8, 64, (8, 64), True),        # the two sides of the wave / workgroup switch
]
# the `short` pattern: one shape per row of the table
SHORT_SHAPES = [(512, 8, 64), (512, 2, 1000), (512, 3, 683), (5, 4, 256), (5, 5, 205), (5, 8, 1000), (5, 8, 2048), (3, 17, 2048)]


def _table_id(case):
    nq, nlists, k = case[:3]
    R, NT = select_build(nq, nlists * k)
    return f"nq{nq}-{nlists}x{k}-R{R}NT{NT}{'' if in_registers(nq, nlists * k) else 'mem'}"


def test_the_table_reaches_every_build_and_both_paths_of_the_widest():
    for nq, nlists, k, build, regs in TABLE:
        assert select_build(nq, nlists * k) == build and in_registers(nq, nlists * k) == regs, (nq, nlists, k)
    reached = {(select_build(nq, nl * k), in_registers(nq, nl * k)) for nq, nl, k, _, _ in TABLE}
    assert reached == {((8, 64), True), ((32, 64), True), ((4, 256), True), ((16, 256), True), ((32, 256), True),
                       ((32, 1024), True), ((32, 1024), False)}
    # both sides of every threshold of n
    sizes = {(nq >= 512, nl * k) for nq, nl, k, _, _ in TABLE}
    assert {(True, 512), (True, 520), (True, 2048), (True, 2049), (False, 1024), (False, 1025), (False, 4096), (False, 4100),
            (False, 8192), (False, 8200), (False, 32768), (False, 33000)} <= sizes
    assert {(select_build(nq, nl * k), in_registers(nq, nl * k)) for nq, nl, k in SHORT_SHAPES} == reached
    assert (8, 1000) in {(nl, k) for _, nl, k, _, _ in TABLE} and (8, 2048) in {(nl, k) for _, nl, k, _, _ in TABLE}


# ---- helpers ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def backs(gpu_faiss):
    """a HipShardBackend per metric with no rows: a merge takes the device and the metric from its handle, nothing else"""
    from knn_for_homology_amd.sharded import HipShardBackend
    return {metric: HipShardBackend(8, metric) for metric in (IP, L2)}


@functools.lru_cache(maxsize=2)
def _exchange(pattern, nlists, nq, k, real=None):
    """(keys, the k best keys per query): generated once per shape, read by both metrics"""
    keys = mr.exchange(pattern, nlists, nq, k, real=real)
    keys.setflags(write=False)
    best = mr.merge_keys(keys, k)
    best.setflags(write=False)
    return keys, best


def _to_dev(keys):
    import torch
    return torch.from_numpy(np.array(keys, np.uint64).view(np.int64)).to(torch.device("cuda", 0))  # (a copy: the cached arrays are read-only)


def _merge(back, keys, k, **kw):
    import torch
    nlists, nq, kk = keys.shape
    assert kk == k
    D, I = back.merge(_to_dev(keys), nlists, nq, k, **kw)
    torch.cuda.synchronize()
    return D.cpu().numpy(), I.cpu().numpy()


def _check_merge(backs, metric, pattern, nq, nlists, k, real=None):
    keys, best = _exchange(pattern, nlists, nq, k, real)
    got = _merge(backs[metric], keys, k)
    mr.assert_same(got, mr.unpack(best, metric), f"{pattern} nq={nq} nlists={nlists} k={k} real={real} metric={metric}")


ALL_CASES = [(c[0], c[1], c[2], pattern, metric) for c in TABLE for pattern in mr.PATTERNS for metric in (IP, L2)]


@pytest.mark.parametrize("nq,nlists,k,pattern,metric", ALL_CASES,
                         ids=[f"{_table_id(c)}-{c[3]}-{'ip' if c[4] == IP else 'l2'}" for c in ALL_CASES])
def test_merge_every_build(backs, nq, nlists, k, pattern, metric):
    _check_merge(backs, metric, pattern, nq, nlists, k)


SHORT_CASES = [(nq, nl, k, i, metric) for nq, nl, k in SHORT_SHAPES for i in range(7) for metric in (IP, L2)]


@pytest.mark.parametrize("nq,nlists,k,which,metric", SHORT_CASES,
                         ids=[f"{_table_id(c)}-real{mr.short_reals(c[2])[c[3]]}-{'ip' if c[4] == IP else 'l2'}" for c in SHORT_CASES])
def test_merge_short_lists(backs, nq, nlists, k, which, metric):
    """exactly `real` keys among nlists * k slots, on both sides of k and of kmax (the early-out of the bracket search)"""
    _check_merge(backs, metric, "short", nq, nlists, k, real=mr.short_reals(k)[which])


# ---- (b) every width of the survivors' sort ------------------------------------------------------------------------------
WIDTH_KS = [1, 31, 32, 33, 51, 52, 102, 103, 204, 205, 409, 410, 819, 820]


def _pow2(n):
    return 1 << max(0, (n - 1).bit_length())


def test_the_widths_reach_every_sort_size():
    assert all(2 * k <= 2048 and select_build(512, 2 * k)[1] == 64 for k in WIDTH_KS)
    # P = next_pow2(survivors) with k <= survivors <= kmax, at least 64
    assert {max(64, _pow2(mr.kmax_of(k))) for k in WIDTH_KS} == {64, 128, 256, 512, 1024, 2048}


@pytest.mark.parametrize("metric", [IP, L2])
@pytest.mark.parametrize("pattern", ["gaussian", "one_word"])
@pytest.mark.parametrize("k", WIDTH_KS)
def test_merge_survivor_widths(backs, k, pattern, metric):
    _check_merge(backs, metric, pattern, 512, 2, k)


# ---- (c) the status row of sharded.py ------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", [IP, L2])
@pytest.mark.parametrize("rows", [512, 8])  # nq + 1: the wave build, a workgroup build
def test_status_row_goes_through_the_merge(backs, rows, metric):
    world, nq, k = 4, rows - 1, 100
    keys = mr.exchange("gaussian", world, nq, k, seed=5)
    stacked = mr.with_status_rows(keys, failed=(1, 3))
    D, I = _merge(backs[metric], stacked, k)
    assert I[nq].tolist() == [1, 3] + [-1] * (k - 2)  # (D[nq] is the float of score word 0, a NaN pattern: not compared)
    mr.assert_same((D[:nq], I[:nq]), mr.merge(keys[[0, 2]], k, metric), "the healthy ranks' keys")
    healthy = mr.with_status_rows(keys, failed=())
    D, I = _merge(backs[metric], healthy, k)
    assert (I[nq] == -1).all()
    mr.assert_same((D[:nq], I[:nq]), mr.merge(keys, k, metric), "all ranks healthy")


# ---- (d) packed keys against the oracle -----------------------------------------------------------------------------------
NB = 3000


@functools.lru_cache(maxsize=None)
def _rows(d):
    rng = np.random.default_rng(1000 + d)
    xb = rng.standard_normal((NB, d), dtype=np.float32)
    xb[2990:2995] = xb[10:15]  # five exact duplicates: ties on the score, the lower id first
    xb.setflags(write=False)
    return xb


def _queries(d, nq):
    """nq queries with a zero query (every inner product is 0.0: only ids order the keys) and a copy of a duplicated row; a single
    query is one or the other"""
    xb = _rows(d)
    q = np.random.default_rng(2000 + d + nq).standard_normal((nq, d), dtype=np.float32)
    if nq == 1:
        return [np.zeros((1, d), np.float32), xb[12:13].copy()]
    q[0] = 0.0
    q[1] = xb[12]
    q[2] = xb[NB - 1]  # (the last row leads this query's result: the largest id there is)
    return [q]


@pytest.fixture(scope="module")
def shard3000(gpu_faiss):
    from knn_for_homology_amd.sharded import HipShardBackend
    made = {}

    def get(d, metric):
        if (d, metric) not in made:
            made[d, metric] = HipShardBackend(d, metric)
            made[d, metric].add(_rows(d))
        return made[d, metric]
    return get


def _search_keys(back, xq, k, id_base):
    import torch
    keys = back.search_keys(torch.from_numpy(xq).to(back.device), k, id_base)
    torch.cuda.synchronize()
    return keys.cpu().numpy().view(np.uint64)


def _assert_keys(got, want, what):
    if not np.array_equal(got, want):
        q, j = np.argwhere(got != want)[0]
        raise AssertionError(f"{what}: {int((got != want).sum())} keys differ, first at query {q} slot {j}: got {int(got[q, j]):#018x}, "
                             f"expected {int(want[q, j]):#018x}")


@pytest.mark.parametrize("metric", [IP, L2])
@pytest.mark.parametrize("k", [1, 100])
@pytest.mark.parametrize("nq", [1, 19, 20, 70])  # (both squared-L2 formulas: fewer than 20 queries, and not)
@pytest.mark.parametrize("d", [64, 100])         # (100: rows padded to the kernel's width)
def test_packed_keys_are_the_oracles_result_packed_on_the_host(shard3000, oracle, d, nq, k, metric):
    back = shard3000(d, metric)
    for xq in _queries(d, nq):
        D, I = oracle.flat_search(_rows(d), xq, k, metric)
        for id_base in (0, 1000, (1 << 32) - NB):  # the last one: the last row's id is exactly 0xFFFFFFFF
            want = mr.pack_keys(D, I, metric, id_base)
            _assert_keys(_search_keys(back, xq, k, id_base), want, f"d={d} nq={nq} k={k} metric={metric} id_base={id_base}")
    if nq > 1:  # what the cases are there for, read off the keys of the last id_base
        base, low = (1 << 32) - NB, np.uint64(0xFFFFFFFF)
        assert int(want[2, 0] & low) == 0xFFFFFFFF
        if k == 100:
            assert (want[1, :2] & low).tolist() == [base + 12, base + 2992], "the duplicated row and its copy, the lower id first"
            if metric == IP:
                assert (want[0] >> np.uint64(32) == 0x80000000).all() and np.array_equal(want[0] & low, np.arange(100) + base)


@pytest.mark.parametrize("metric", [IP, L2])
def test_packed_keys_of_a_shard_smaller_than_k_and_of_an_empty_one(gpu_faiss, oracle, metric):
    from knn_for_homology_amd.sharded import HipShardBackend
    rng = np.random.default_rng(7)
    xb = rng.standard_normal((7, 64), dtype=np.float32)
    xq = rng.standard_normal((20, 64), dtype=np.float32)
    back = HipShardBackend(64, metric)
    got = _search_keys(back, xq, 100, 123)
    assert got.shape == (20, 100) and (got == KEY_PAD).all(), "an index with no rows packs nothing"
    back.add(xb)
    got = _search_keys(back, xq, 100, 123)
    _assert_keys(got, mr.pack_keys(*oracle.flat_search(xb, xq, 100, metric), metric, 123), f"7 rows, metric {metric}")
    assert (got[:, 7:] == KEY_PAD).all() and (got[:, :7] != KEY_PAD).all()


def test_packed_keys_of_the_16_bit_prefilter(gpu_faiss, oracle):
    """the exact 16-bit prefilter (HipShardBackend turns the fp16 copies on; KNN_TUNE_SCAN16_ANY_NB engages it at this size) packs
    the keys of the fp32 scan"""
    from knn_for_homology_amd._lib import KNN_TUNE_NO_SCAN16, KNN_TUNE_SCAN16_ANY_NB
    from knn_for_homology_amd.sharded import HipShardBackend
    xb = _rows(64)
    rng = np.random.default_rng(8)
    xq = rng.standard_normal((20, 64), dtype=np.float32)
    xq[1] = xb[12]
    back = HipShardBackend(64, IP)
    back.add(xb)
    want = mr.pack_keys(*oracle.flat_search(xb, xq, 100, IP), IP, 1000)
    back.index.set_tuning(0, 0, KNN_TUNE_SCAN16_ANY_NB)
    got16 = _search_keys(back, xq, 100, 1000)
    assert back.index.last_scan16()["used"], back.index.last_scan16()
    back.index.set_tuning(0, 0, KNN_TUNE_NO_SCAN16)
    got32 = _search_keys(back, xq, 100, 1000)
    assert not back.index.last_scan16()["used"]
    _assert_keys(got32, want, "fp32 scan")
    _assert_keys(got16, want, "16-bit prefilter")


# ---- (e) a world of 8 at the reference's k --------------------------------------------------------------------------------
SHARD_ROWS = [0, 7, 999, 1000, 1001, 2000, 1994, 2000]  # one shard empty, two with fewer than 1000 rows


@functools.lru_cache(maxsize=None)
def _world8_rows():
    rng = np.random.default_rng(88)
    xb = rng.standard_normal((9001, 64), dtype=np.float32)
    # shard boundaries at rows 7, 1006, 2006, 3007, 5007, 7001: two runs of duplicates, each across a boundary
    xb[1004:1008] = xb[3005:3009]
    xq = rng.standard_normal((33, 64), dtype=np.float32)
    xq[:4] = xb[3005:3009]
    xq[4] = 0.0
    return xb, xq


@pytest.fixture(scope="module")
def world8(gpu_faiss):
    from knn_for_homology_amd.sharded import HipShardBackend
    assert sum(SHARD_ROWS) == 9001
    xb, _ = _world8_rows()
    offs = np.concatenate([[0], np.cumsum(SHARD_ROWS)])
    assert offs[3] == 1006 and offs[5] == 3007
    out = {}
    for metric in (IP, L2):
        shards = []
        for r, rows in enumerate(SHARD_ROWS):
            b = HipShardBackend(64, metric)
            if rows:
                b.add(xb[offs[r]:offs[r + 1]])
            shards.append((b, int(offs[r])))
        out[metric] = shards
    return out


@pytest.mark.parametrize("metric", [IP, L2])
@pytest.mark.parametrize("k", [1000, 2048])
def test_world_of_eight_equals_the_flat_search(world8, oracle, k, metric):
    import torch
    xb, xq = _world8_rows()
    shards = world8[metric]
    q = torch.from_numpy(xq).to(shards[0][0].device)
    parts = [b.search_keys(q, k, lo) for b, lo in shards]
    gathered = torch.stack(parts).contiguous()
    assert gathered.shape == (8, 33, k) and select_build(33, 8 * k) == ((32, 256) if k == 1000 else (32, 1024))
    D, I = shards[3][0].merge(gathered, 8, 33, k)
    torch.cuda.synchronize()
    Do, Io = oracle.flat_search(xb, xq, k, metric)
    assert (Io >= 0).all()  # (9001 rows > k: nothing unfilled)
    mr.assert_same((D.cpu().numpy(), I.cpu().numpy()), (Do, Io), f"world 8, k={k}, metric={metric}")
    assert Io[0, :2].tolist() == [1004, 3005] and Io[3, :2].tolist() == [1007, 3008], "the duplicates across the shard boundaries"
    # and the lists the merge read are the host's packing of each shard's own flat search
    got = gathered.cpu().numpy().view(np.uint64)
    offs = np.concatenate([[0], np.cumsum(SHARD_ROWS)])
    for r in (0, 1, 2, 4):
        want = mr.pack_keys(*oracle.flat_search(xb[offs[r]:offs[r + 1]], xq, k, metric), metric, int(offs[r])) if SHARD_ROWS[r] else KEY_PAD
        _assert_keys(got[r], np.broadcast_to(want, got[r].shape), f"shard {r}")


# ---- (f) merges through different handles and streams ----------------------------------------------------------------------
@pytest.mark.parametrize("metric", [IP, L2])
def test_two_merges_on_two_streams_do_not_interfere(backs, metric):
    import torch
    back = backs[metric]
    nq, nlists, k = 5, 8, 1000
    a, best_a = _exchange("gaussian", nlists, nq, k)
    b = mr.exchange("two_clusters", nlists, nq, k, seed=9)
    want_a, want_b = mr.unpack(best_a, metric), mr.merge(b, k, metric)
    ga, gb = _to_dev(a), _to_dev(b)
    view = back.index.view()
    s1, s2 = torch.cuda.Stream(back.device), torch.cuda.Stream(back.device)
    torch.cuda.synchronize()  # (the uploads ran on the default stream: the two streams below do not wait for it)
    outs = []
    for _ in range(3):  # back to back, no synchronisation in between
        with torch.cuda.stream(s1):
            outs.append((back.merge(ga, nlists, nq, k), want_a))
        with torch.cuda.stream(s2):
            outs.append((back.merge(gb, nlists, nq, k, index=view), want_b))
    torch.cuda.synchronize()
    for i, ((D, I), want) in enumerate(outs):
        mr.assert_same((D.cpu().numpy(), I.cpu().numpy()), want, f"merge {i}")


# ---- (g) argument errors ---------------------------------------------------------------------------------------------------
def test_merge_argument_errors_leave_the_outputs_alone(backs):
    import torch
    from knn_for_homology_amd import _lib
    L = _lib.lib()
    back = backs[L2]
    dev = back.device
    keys = _to_dev(mr.exchange("gaussian", 2, 3, 4))
    D = torch.full((3, 4), 7.0, dtype=torch.float32, device=dev)
    I = torch.full((3, 4), 7, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    h = back.index._h

    def call(keys_ptr, nlists, nq, k):
        return L.knn_merge_keys_dev(h, keys_ptr, nlists, nq, k, D.data_ptr(), I.data_ptr(), None)

    for args in ((keys.data_ptr(), 0, 3, 4), (keys.data_ptr(), 2, 3, 0), (keys.data_ptr(), 2, 3, 2049), (None, 2, 3, 4)):
        assert call(*args) == KNN_ERR_INVALID, args
        assert "merge_keys" in L.knn_last_error().decode()
    assert call(keys.data_ptr(), 2, 0, 4) == 0
    assert call(None, 2, 0, 4) == 0
    torch.cuda.synchronize()
    assert (D == 7.0).all().item() and (I == 7).all().item()
    assert call(keys.data_ptr(), 2, 3, 4) == 0  # (the same call with a good shape writes them)
    assert (I != 7).all().item()


# ---- the 32-bit range of the global ids ------------------------------------------------------------------------------------
def test_an_id_base_that_wraps_is_refused_by_search_keys(shard3000):
    import torch
    from knn_for_homology_amd import _lib
    L = _lib.lib()
    back = shard3000(64, IP)
    q = torch.from_numpy(_queries(64, 19)[0]).to(back.device)
    keys = torch.full((19, 10), 7, dtype=torch.int64, device=back.device)
    torch.cuda.synchronize()
    bad = (1 << 32) - NB + 1  # the last row's id would be 2^32
    rc = L.knn_flat_search_keys_dev(back.index._h, q.data_ptr(), 19, 10, bad, keys.data_ptr(), None)
    msg = L.knn_last_error().decode()
    assert rc == KNN_ERR_INVALID and str(bad) in msg and str(NB) in msg, (rc, msg)
    torch.cuda.synchronize()
    assert (keys == 7).all().item(), "nothing was launched"
    with pytest.raises(_lib.Knn355Error, match=str(bad)):
        back.search_keys(q, 10, bad)
    # Python: ctypes would wrap an id_base outside [0, 2^32) silently
    for out_of_range in (1 << 32, -1, (1 << 32) + 5):
        with pytest.raises(ValueError, match="id_base"):
            back.search_keys(q, 10, out_of_range)
    # an empty shard may sit at the very end of the id range
    from knn_for_homology_amd.sharded import HipShardBackend
    assert (_search_keys(HipShardBackend(64, IP), q.cpu().numpy(), 10, (1 << 32) - 1) == KEY_PAD).all()


def test_an_id_base_that_wraps_is_refused_by_the_in_library_sharded_search(shard3000, oracle):
    """knn_sharded_search_dev on a 1-rank communicator: the rank's local scan refuses, the rank still enters the all-gather (with
    "no rows") and returns the error afterwards -- it does not hang, writes no result, and the communicator serves the next
    search"""
    import torch
    from knn_for_homology_amd import _lib
    L = _lib.lib()
    back = shard3000(64, L2)
    xq = _queries(64, 19)[0]
    ident = (ctypes.c_uint8 * 128)()
    _lib.check(L.knn_comm_unique_id(ident))
    comm = ctypes.c_void_p()
    _lib.check(L.knn_comm_create(ident, 1, 0, 0, ctypes.byref(comm)))
    try:
        dev = back.device
        q = torch.from_numpy(xq).to(dev)
        D = torch.full((19, 10), 7.0, dtype=torch.float32, device=dev)
        I = torch.full((19, 10), 7, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        bad = (1 << 32) - NB + 1
        rc = L.knn_sharded_search_dev(back.index._h, comm, q.data_ptr(), 19, 10, bad, D.data_ptr(), I.data_ptr(), None)
        msg = L.knn_last_error().decode()
        assert rc == KNN_ERR_INVALID and str(bad) in msg and str(NB) in msg, (rc, msg)
        torch.cuda.synchronize()
        assert (D == 7.0).all().item() and (I == 7).all().item()
        ok = (1 << 32) - NB
        _lib.check(L.knn_sharded_search_dev(back.index._h, comm, q.data_ptr(), 19, 10, ok, D.data_ptr(), I.data_ptr(), None))
        torch.cuda.synchronize()
        Do, Io = oracle.flat_search(_rows(64), xq, 10, L2)
        mr.assert_same((D.cpu().numpy(), I.cpu().numpy()), (Do, Io + ok), "the boundary id_base")
        assert I.max().item() <= 0xFFFFFFFF
    finally:
        L.knn_comm_free(comm)
