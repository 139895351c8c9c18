"""GPU: the library plans every case of tests/plan_cases.py as the table says -- the introspection of the last scan launch
after a real search through the entry the case names -- and, for the cases small enough for the CPU oracle (nb <= 2^15),
returns the oracle's ids and score bits.  The bf16 rows of the table are left to test_plan_cpu.py: no exported call makes such
an index or reaches its introspection (IndexHNSWFlat keeps its coarse index to itself).  The table's literals come from the
library before the planner moved into csrc/plan.h (see plan_cases.py); test_plan_cpu.py checks the same table against the
stand-alone planner."""
import ctypes
import functools

import numpy as np
import pytest

import plan_cases as pc

pytestmark = pytest.mark.gpu

D = 32


@functools.lru_cache(maxsize=None)
def _rows(nb):
    xb = np.random.default_rng(nb).standard_normal((nb, D), dtype=np.float32)
    xb[nb // 2: nb // 2 + 3] = xb[:3]  # exact duplicates: ties -> lower id
    return xb


_INDEX = {}
FP32_CASES = [c for c in pc.CASES if not c.approx16]


@pytest.fixture(scope="module", autouse=True)
def _release_indexes():
    yield
    _INDEX.clear()


def _index(gpu_faiss, nb, metric):
    if (nb, metric) not in _INDEX:
        if len(_INDEX) >= 4:  # (a few databases stay on the device: the cases of one shape follow each other)
            _INDEX.pop(next(iter(_INDEX)))
        idx = gpu_faiss.IndexFlat(D, metric)
        idx.add(_rows(nb))
        _INDEX[(nb, metric)] = idx
    return _INDEX[(nb, metric)]


def observe(gpu_faiss, c):
    """runs the case; returns (the tuple of plan_cases.EXPECT, queries, D, I)"""
    from knn_for_homology_amd import _lib
    idx = _index(gpu_faiss, c.nb, c.metric)
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


@pytest.mark.parametrize("case", FP32_CASES, ids=[c.name for c in FP32_CASES])
def test_last_launch_is_the_planned_one(gpu_faiss, oracle, case):
    got, xq, Dg, Ig = observe(gpu_faiss, case)
    print(f"{case.name!r}: {got!r},")
    assert got == pc.EXPECT[case.name]
    if case.nb <= 1 << 15:
        # (FAISS's small-batch rule follows the caller's batch: the norm formula under KNN_TUNE_NORM_L2 and for a piece of a larger batch)
        norm = bool(case.flags & pc.NORM_L2) or case.batch >= 20
        Do, Io = oracle.flat_search(_rows(case.nb), xq, case.k, case.metric, l2_mode=1 if norm else 0)
        assert np.array_equal(Ig, Io), f"{int((Ig != Io).sum())} neighbour ids differ"
        assert np.array_equal(Dg.view(np.uint32), Do.view(np.uint32)), "score bits differ"
