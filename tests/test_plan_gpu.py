"""GPU: the library plans every case of tests/plan_cases.py as the table says -- the introspection of the last scan launch
after a real search through the entry the case names -- and, for the cases small enough for the CPU oracle (nb <= 2^15),
returns the oracle's ids and score bits.  The bf16 rows of the table run on an index made approximate with set_approx16, over
integer rows, and return the ids and score bits of tests/approx16_reference.py.  The table's literals come from the
library before the planner moved into csrc/plan.h (see plan_cases.py); test_plan_cpu.py checks the same table against the
stand-alone planner.  The same for the symmetric self-search (SYM_CASES up to 16384 rows, through search_self) and the range
scan (RANGE_CASES of 4096 rows, through range_search)."""
import ctypes
import functools

import numpy as np
import pytest

import approx16_reference as ar
import plan_cases as pc

pytestmark = pytest.mark.gpu

D = 32


@functools.lru_cache(maxsize=None)
def _rows(nb):
    xb = np.random.default_rng(nb).standard_normal((nb, D), dtype=np.float32)
    xb[nb // 2: nb // 2 + 3] = xb[:3]  # exact duplicates: ties -> lower id
    return xb


@functools.lru_cache(maxsize=None)
def _rows16(nb):
    """the rows of an approximate (bf16) index: integers in [-16, 16], on which its arithmetic is exact in any order"""
    xb = np.random.default_rng(nb).integers(-16, 17, (nb, D)).astype(np.float32)
    xb[nb // 2: nb // 2 + 3] = xb[:3]
    return xb


_INDEX = {}


@pytest.fixture(scope="module", autouse=True)
def _release_indexes():
    yield
    _INDEX.clear()


def _index(gpu_faiss, nb, metric, approx16=False):
    if (nb, metric, approx16) not in _INDEX:
        if len(_INDEX) >= 4:  # (a few databases stay on the device: the cases of one shape follow each other)
            _INDEX.pop(next(iter(_INDEX)))
        idx = gpu_faiss.IndexFlat(D, metric)
        if approx16:
            idx.set_approx16()
        idx.add(_rows16(nb) if approx16 else _rows(nb))
        _INDEX[(nb, metric, approx16)] = idx
    return _INDEX[(nb, metric, approx16)]


def observe(gpu_faiss, c):
    """runs the case; returns (the tuple of plan_cases.EXPECT, queries, D, I)"""
    from knn_for_homology_amd import _lib
    idx = _index(gpu_faiss, c.nb, c.metric, c.approx16)
    if c.approx16:
        xq = np.random.default_rng(c.nq * 7919 + c.k).integers(-16, 17, (c.nq, D)).astype(np.float32)
        xq[:3] = _rows16(c.nb)[:min(3, c.nq)]
    else:
        xq = np.random.default_rng(c.nq * 7919 + c.k).standard_normal((c.nq, D), dtype=np.float32)
        xq[:3] = _rows(c.nb)[:min(3, c.nq)]  # (queries that tie between a row and its duplicate)
    idx.set_tuning(c.force_qt, c.force_chunks, c.flags)
    idx.set_batch(c.batch)
    try:
        if c.entry == "host":
            Dg, Ig = idx.search(xq, c.k)
        else:
            import torch
            dev = torch.device("cuda:0")
            q = torch.from_numpy(xq).to(dev)
            Dd = torch.empty((c.nq, c.k), device=dev, dtype=torch.float32)
            Id = torch.empty((c.nq, c.k), device=dev, dtype=torch.int64)
            if c.entry == "dev":
                _lib.check(_lib.lib().knn_flat_search_dev(idx._h, q.data_ptr(), c.nq, c.k, Dd.data_ptr(), Id.data_ptr(), None))
            else:
                side = torch.cuda.Stream(dev)
                side.wait_stream(torch.cuda.current_stream(dev))
                with torch.cuda.stream(side):
                    _lib.check(_lib.lib().knn_flat_search_dev(idx._h, q.data_ptr(), c.nq, c.k, Dd.data_ptr(), Id.data_ptr(),
                                                              ctypes.c_void_p(side.cuda_stream)))
                side.synchronize()
            Dg, Ig = Dd.cpu().numpy(), Id.cpu().numpy()
        scan, seed = idx.last_scan(), idx.last_seed()
    finally:
        idx.set_tuning(0, 0, 0)
        idx.set_batch(0)
    got = (scan["kernel"], scan["query_tile"], scan["db_tile"], scan["nchunks"], scan["grid"], seed["stride"], seed["stat_rank"],
           seed["sample_rows"])
    return got, xq, Dg, Ig


@pytest.mark.parametrize("case", pc.CASES, ids=[c.name for c in pc.CASES])
def test_last_launch_is_the_planned_one(gpu_faiss, oracle, case):
    got, xq, Dg, Ig = observe(gpu_faiss, case)
    print(f"{case.name!r}: {got!r},")
    assert got == pc.EXPECT[case.name]
    if case.approx16:
        if case.nb <= 1 << 15:
            Do, Io = ar.expected(_rows16(case.nb), xq, case.k, case.metric)
            assert np.array_equal(Ig, Io), f"{int((Ig != Io).sum())} neighbour ids differ"
            assert np.array_equal(Dg.view(np.uint32), Do.view(np.uint32)), "score bits differ"
    elif case.nb <= 1 << 15:
        # (FAISS's small-batch rule follows the caller's batch: the norm formula under KNN_TUNE_NORM_L2 and for a piece of a larger batch)
        norm = bool(case.flags & pc.NORM_L2) or case.batch >= 20
        Do, Io = oracle.flat_search(_rows(case.nb), xq, case.k, case.metric, l2_mode=1 if norm else 0)
        assert np.array_equal(Ig, Io), f"{int((Ig != Io).sum())} neighbour ids differ"
        assert np.array_equal(Dg.view(np.uint32), Do.view(np.uint32)), "score bits differ"


# ---- the symmetric self-search (plan_self_symmetric, sym_work_table) -------------------------------------------------
SYM_GPU = [c for c in pc.SYM_CASES if c.n <= 16384]
STREAM_MIN_BYTES = 32 << 20  # (knn_flat_search_self: from here on the host entry asks for the copy stream)


@functools.lru_cache(maxsize=None)
def _self_oracle(oracle, n, metric):
    """The oracle's all-vs-all of _rows(n), once per database, with the largest k the table asks of it: the oracle orders a
    query's rows by (score, id), so a smaller k is the first columns."""
    kmax = max(c.k for c in SYM_GPU if c.n == n and c.metric == metric)
    return oracle.flat_search(_rows(n), _rows(n), kmax, metric)


@pytest.fixture(scope="module", autouse=True)
def _release_self_oracles():
    yield
    _self_oracle.cache_clear()


def _search_self_dev(idx, n, k):
    """knn_flat_search_self_dev: the results stay on the device, so no host arrays and no copy stream reach the plan"""
    import torch
    from knn_for_homology_amd import _lib
    dev = torch.device("cuda:0")
    Dd = torch.empty((n, k), device=dev, dtype=torch.float32)
    Id = torch.empty((n, k), device=dev, dtype=torch.int64)
    _lib.check(_lib.lib().knn_flat_search_self_dev(idx._h, k, Dd.data_ptr(), Id.data_ptr()))
    return Dd.cpu().numpy(), Id.cpu().numpy()


def _observe_self(gpu_faiss, c, entry):
    idx = _index(gpu_faiss, c.n, c.metric)
    idx.set_tuning(c.force_qt, 0, c.flags)
    try:
        Dg, Ig = idx.search_self(c.k) if entry == "host" else _search_self_dev(idx, c.n, c.k)
        scan, seed = idx.last_scan(), idx.last_seed()
    finally:
        idx.set_tuning(0, 0, 0)
    got = (scan["kernel"], scan["query_tile"], scan["db_tile"], scan["nchunks"], scan["grid"], seed["stride"], seed["stat_rank"],
           seed["sample_rows"])
    return got, Dg, Ig


def _assert_self(oracle, c, got, Dg, Ig):
    want = pc.SYM_EXPECT[c.name]
    if want is None:
        assert not got[0].endswith("_sym"), got
    else:
        kernel, ts, _tiles, st, S, j, _qcap, _k_sample, _n_expect, _groups, _gstart, first_run, items = want[:13]
        assert got == (kernel, ts, ts, first_run, items, st, j, S)
    Do, Io = _self_oracle(oracle, c.n, c.metric)
    assert np.array_equal(Ig, Io[:, :c.k]), f"{int((Ig != Io[:, :c.k]).sum())} neighbour ids differ"
    assert np.array_equal(Dg.view(np.uint32), Do[:, :c.k].view(np.uint32)), "score bits differ"


@pytest.mark.parametrize("case", SYM_GPU, ids=[c.name for c in SYM_GPU])
def test_self_search_is_the_planned_one(gpu_faiss, oracle, case):
    """search_self through the host entry, whose lease on the copy stream makes can_stream true from 32 MB of result on.  The
    rows that record such a result WITHOUT the copy stream cannot be seen through that entry: they go through the device
    entry, which has no host arrays and must use one group whatever the size."""
    entry = "host" if case.can_stream or case.n * case.k * 12 < STREAM_MIN_BYTES else "dev"
    got, Dg, Ig = _observe_self(gpu_faiss, case, entry)
    print(f"{case.name!r} ({entry}): {got!r},")
    _assert_self(oracle, case, got, Dg, Ig)


def test_self_search_dev_entry_uses_one_group(gpu_faiss, oracle):
    case = next(c for c in pc.SYM_CASES if c.name == "n4096-k10-ip-f0-qt0-s0")
    assert pc.SYM_EXPECT[case.name][9] == 1
    got, Dg, Ig = _observe_self(gpu_faiss, case, "dev")
    _assert_self(oracle, case, got, Dg, Ig)


# ---- the range scan (plan_range) ------------------------------------------------------------------------------------
RANGE_GPU = [c for c in pc.RANGE_CASES if c.n == 4096]


@pytest.mark.parametrize("case", RANGE_GPU, ids=[c.name for c in RANGE_GPU])
def test_range_launch_is_the_planned_one(gpu_faiss, oracle, case):
    import test_range_search_gpu as tr  # (its oracle: the expected lims, ids and score bits of a range search)
    xb = _rows(case.n)
    xq = np.random.default_rng(case.nq * 7919).standard_normal((case.nq, D), dtype=np.float32)
    r = tr._radius(oracle, xb, xq, case.metric, 0.01)  # about 1 % of the (query, row) pairs
    idx = _index(gpu_faiss, case.n, case.metric)
    idx.set_batch(case.batch)
    try:
        got = idx.range_search(xq, r)
        scan = idx.last_scan()
    finally:
        idx.set_batch(0)
    kernel, qt, dt, _nqtiles, nchunks, _tiles_base, _tiles_rem, grid = pc.RANGE_EXPECT[case.name][:8]
    assert (scan["kernel"], scan["query_tile"], scan["db_tile"], scan["nchunks"], scan["grid"]) == (kernel, qt, dt, nchunks, grid)
    assert 0 < got[0][-1] < case.nq * case.n
    # (FAISS's small-batch rule follows the caller's batch: the norm formula for a piece of a larger batch)
    tr._assert_same(got, tr._expected(oracle, xb, xq, r, case.metric, l2_mode=1 if case.batch >= 20 else 0))
