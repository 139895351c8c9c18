"""GPU: the HNSW construction compared EXACTLY with a host replay, every list of every level ("How
construction is tested exactly").

With efConstruction >= the number of linked nodes the construction beam never fills: every reachable node is a candidate,
re-scored by the contract's chain (keep == ef), and what follows -- the 127 cut, the selection, the forward lists, the reverse
requests in (node, level, v, from) order, appending or pruning, the entry point -- is deterministic bookkeeping over scores
whose bits the CPU oracle produces.  tests/hnsw_build_reference.py replays every add call batch by batch with the levels the
library drew (read from the exported graph) and must arrive at the library's graph slot for slot.  The cases are those of
tests/hnsw_build_cases.py; tests/test_hnsw_build_reference.py has replayed every one on the CPU with the validity
conditions holding.

M = 2          both metrics, one and three calls, on the host walkers (KNN355_HNSW_HOST_BEAM=1) against the restated walk
from scratch   both metrics, M = 4 / 8, one and three add calls, duplicate rows inside a batch and across batches; by
               default (level 0 linked on the device), with the host's bookkeeping (KNN355_HNSW_HOST_LINKS=1) and with
               host walkers instead of the device beam (KNN355_HNSW_HOST_BEAM=1); a search before the export
host walk      d = 20: rows padded to 32 values, the device beam is off
host upper     more than 127 nodes above level 0, upper-level candidates from the host walkers (KNN355_HNSW_HOST_UPPER=1)
wide lists     M = 16 / 42 / 63 onto an imported starting graph: the selection's 64-, 96- and 128-row builds
one batch      add calls of 1, 31, 32 and 33 rows under the default batch limit, compared after each
efConstruction reads back as set; 2000 (host walkers) builds the graph 1024 builds"""
import numpy as np
import pytest

import hnsw_build_cases as cases
import hnsw_build_reference as ref
from hnsw_reference import expected, level0_tables, reachable

pytestmark = pytest.mark.gpu

ENV = ("KNN355_HNSW_HOST_LINKS", "KNN355_HNSW_HOST_BEAM", "KNN355_HNSW_HOST_UPPER", "KNN355_HNSW_BEAM_FP32", "KNN355_HNSW_ORDER",
       "KNN355_HNSW_COARSE_FP32")


@pytest.fixture(autouse=True)
def _default_settings(monkeypatch):
    for name in ENV:
        monkeypatch.delenv(name, raising=False)


def _new_index(gpu_faiss, case, x, start):
    """the index with efConstruction and the batch limit set before the first add; a starting graph is imported as
    tests/test_hnsw_exact_gpu.py imports its graphs"""
    from knn_for_homology_amd import _lib
    idx = gpu_faiss.IndexHNSWFlat(case.d, case.M, case.metric)
    idx.hnsw.efConstruction = cases.EFC
    assert idx.hnsw.efConstruction == cases.EFC
    if start is not None:
        (levels, _, nbrs, _), entry, max_level = start
        L = _lib.lib()
        rows = np.ascontiguousarray(x[:case.start])
        _lib.check(L.knn_flat_add(L.knn_hnsw_storage(idx._h), rows.ctypes.data, case.start))
        _lib.check(L.knn_hnsw_graph_import(idx._h, case.start, levels.ctypes.data, nbrs.ctypes.data, nbrs.size, int(max_level), int(entry)))
    return idx


def _assert_graph(idx, want, entry, max_level, what):
    got = idx.graph()
    assert np.array_equal(got[0], want[0]), f"{what}: levels differ"
    assert np.array_equal(got[1], want[1]), f"{what}: offsets differ"
    assert np.array_equal(got[3], want[3]), f"{what}: cum differs"
    diff = np.flatnonzero(got[2] != want[2])
    if diff.size:
        node, level, ours, theirs = ref.first_difference(want, got)
        print(f"{what}: first difference at node {node}, level {level}\n  replay  {ours}\n  library {theirs}")
    assert diff.size == 0, f"{what}: {diff.size} of {want[2].size} slots differ"
    assert (idx.hnsw.entry_point, idx.hnsw.max_level) == (entry, max_level), f"{what}: entry point / max level"


def _build_and_compare(gpu_faiss, oracle, case, search=False):
    """one build; after every add call the graph is exported, the call replayed with the levels the export shows for its
    rows, and the two compared.  search: the built index is searched BEFORE the last export"""
    x, _, _, start = cases.start_graph(case, oracle)  # (the starting graph does not depend on the library's levels)
    idx = _new_index(gpu_faiss, case, x, start)
    n0, r = case.start, cases.Replay(case, oracle)
    for c, n in enumerate(case.calls):
        idx.set_walk(max_batch=cases.max_batch(case, c))
        idx.add(x[n0:n0 + n])
        n0 += n
        found = None
        if search and c == len(case.calls) - 1:
            q = np.ascontiguousarray(x[::max(1, n0 // 5)][:5] + np.float32(0.01))
            idx.hnsw.efSearch = n0
            found = (q,) + idx.search(q, n0)
        want, entry, max_level, _ = r.add(idx.graph()[0][n0 - n:n0])
        _assert_graph(idx, want, entry, max_level, f"{case.name}, after add call {c}")
        if found:
            _assert_search(found, x, r.g, case, oracle)
    cases.check_reports(case, r.after)


def _assert_search(found, x, g, case, oracle):
    """the device's master copy of level 0, searched before anything exported it, is the replayed graph: with efSearch = n
    the result is the exact top k of what the REPLAYED level 0 reaches (all rows: it is strongly connected)"""
    q, D, I = found
    n = x.shape[0]
    lists0 = [per_level[0] for per_level in g.lists]
    reach = reachable(*level0_tables(lists0, 2 * case.M), [g.entry])
    assert reach.size == n
    De, Ie = expected(x, q, reach, n, case.metric, oracle)
    assert np.array_equal(I, Ie), "search before the export: ids"
    assert np.array_equal(D.view(np.uint32), De.view(np.uint32)), "search before the export: score bits"


def test_efconstruction_is_not_capped(gpu_faiss, oracle):
    """hnsw.efConstruction reads back as set (it used to be cut to 127).  Above 1024 the device beam is off and host walkers
    find the candidates: with efConstruction >= the linked nodes either way, 2000 builds the graph of the replay too"""
    case = cases.SCRATCH[0]
    assert len(case.calls) == 1
    x = cases.rows(case)
    idx = gpu_faiss.IndexHNSWFlat(case.d, case.M, case.metric)
    for value in (127, 128, 150, 1024, 2000):
        idx.hnsw.efConstruction = value
        assert idx.hnsw.efConstruction == value
    idx.set_walk(max_batch=cases.max_batch(case, 0))
    idx.add(x)
    want, entry, max_level, _ = cases.Replay(case, oracle).add(idx.graph()[0])
    _assert_graph(idx, want, entry, max_level, "efConstruction = 2000")


@pytest.mark.parametrize("case", cases.M2, ids=lambda c: c.name)
def test_m2_on_the_host_walkers(gpu_faiss, oracle, monkeypatch, case):
    for name, value in case.env:
        monkeypatch.setenv(name, value)
    _build_and_compare(gpu_faiss, oracle, case)


@pytest.mark.parametrize("way", list(cases.WAYS))
@pytest.mark.parametrize("case", cases.SCRATCH, ids=lambda c: c.name)
def test_from_scratch(gpu_faiss, oracle, monkeypatch, case, way):
    for name, value in cases.WAYS[way].items():
        monkeypatch.setenv(name, value)
    _build_and_compare(gpu_faiss, oracle, case, search=(way == "default"))


@pytest.mark.parametrize("case", cases.HOST_WALK, ids=lambda c: c.name)
def test_host_walk(gpu_faiss, oracle, case):
    _build_and_compare(gpu_faiss, oracle, case)


@pytest.mark.parametrize("case", cases.HOST_UPPER, ids=lambda c: c.name)
def test_host_upper(gpu_faiss, oracle, monkeypatch, case):
    for name, value in case.env:
        monkeypatch.setenv(name, value)
    _build_and_compare(gpu_faiss, oracle, case)


@pytest.mark.parametrize("case", cases.WIDE, ids=lambda c: c.name)
def test_wide_lists(gpu_faiss, oracle, case):
    _build_and_compare(gpu_faiss, oracle, case)


@pytest.mark.parametrize("case", cases.ONE_BATCH, ids=lambda c: c.name)
def test_one_batch_calls(gpu_faiss, oracle, case):
    _build_and_compare(gpu_faiss, oracle, case)
