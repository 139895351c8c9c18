"""GPU: WHICH level-0 nodes an HNSW search enters at, compared EXACTLY with a host reference, on graphs whose level 0 is
disjoint islands.

tests/test_hnsw_exact_gpu.py pins the level-0 beam; its graphs are connected (or sit at level 0 entirely), so every entry node
reaches the same rows and the entry rule stays invisible.  Here level 0 is rings of a few nodes with no link between them,
and only the levels above 0 link the islands' ports: with efSearch = k = n the result is the exact top k of the union of the
islands of the chosen entry nodes, padded with -1 -- ids and score bits name the entries (tests/hnsw_reference.py: descend,
coarse_entries; the cases: tests/hnsw_entry_cases.py).  tests/test_hnsw_reference.py shows on the CPU, for every case here,
that its expected result differs from what each wrong rule would give (the other rule, no descent, a descent stopped a level
early or started a level late, c - 1 / c + 1 entries, a port table off by one row, the greater id on ties), and that the
real-valued cases keep every comparison four worst-case rounding bounds away from a tie.

a  the 64-port boundary between the two rules
b  the coarse rule: c = 1, 4, 64, bf16 and fp32 scans, several ports per island, a tie at the cut
c  the descent rule: max level 1, 2, 3, local minima, empty lists, holes, equal scores on the path
d  query counts on either side of the host walk's OpenMP and two-halves thresholds
e  set_entry toggled on one index
f  real-valued rows, d = 100 and d = 1028 (the host walk)
g  write_index / read_index
h  knn_hnsw_graph_import refuses an upper-level link to a node without that level"""
import os

import numpy as np
import pytest

import hnsw_entry_cases as cases
from hnsw_reference import assert_output_contract, tables

pytestmark = pytest.mark.gpu

METRICS = cases.METRICS
M = cases.M
SCANS = {"bf16": None, "fp32": "1"}  # KNN355_HNSW_COARSE_FP32


@pytest.fixture(autouse=True)
def _default_settings(monkeypatch):
    for name in [k for k in os.environ if k.startswith("KNN355_HNSW_")]:
        monkeypatch.delenv(name, raising=False)


_EXPECTED = {}


def _expected(c, oracle):
    """(D, I) of all the case's queries under the right rule, computed once"""
    key = (c.name, c.metric)
    if key not in _EXPECTED:
        D, I = cases.grouped_expected(c, list(range(c.q.shape[0])), oracle)
        D.setflags(write=False)
        I.setflags(write=False)
        _EXPECTED[key] = (D, I)
    return _EXPECTED[key]


def _raw_import(idx, levels, nbrs, max_level, entry_point):
    from knn_for_homology_amd import _lib
    L = _lib.lib()
    return L.knn_hnsw_graph_import(idx._h, len(levels), levels.ctypes.data, nbrs.ctypes.data, nbrs.size, int(max_level), int(entry_point))


def _storage(gpu_faiss, c):
    from knn_for_homology_amd import _lib
    idx = gpu_faiss.IndexHNSWFlat(c.x.shape[1], M, c.metric)
    L = _lib.lib()
    _lib.check(L.knn_flat_add(L.knn_hnsw_storage(idx._h), c.x.ctypes.data, c.n))
    return idx


def _import(gpu_faiss, c, scan="bf16", monkeypatch=None):
    """storage rows + knn_hnsw_graph_import, as read_index does for an "IHNf" file.  The coarse scan's precision is read when
    the handle is created: the variable is set before that."""
    from knn_for_homology_amd import _lib
    if SCANS[scan] is not None:
        monkeypatch.setenv("KNN355_HNSW_COARSE_FP32", SCANS[scan])
    idx = _storage(gpu_faiss, c)
    _lib.check(_raw_import(idx, c.levels, c.nbrs, c.max_level, c.entry_point))
    assert idx.ntotal == c.n and idx.hnsw.max_level == c.max_level and idx.hnsw.entry_point == c.entry_point
    idx.hnsw.efSearch = c.n
    if c.spec.entry is not None:
        idx.set_entry(c.spec.entry)
    return idx


def _assert_equal(D, I, De, Ie, what=""):
    rows = np.flatnonzero((I != Ie).any(axis=1))
    assert rows.size == 0, (f"{what}: ids differ in {rows.size} of {len(I)} rows, first query {rows[0]}: got {I[rows[0]][:12].tolist()} "
                            f"want {Ie[rows[0]][:12].tolist()}")
    rows = np.flatnonzero((D.view(np.uint32) != De.view(np.uint32)).any(axis=1))
    assert rows.size == 0, f"{what}: score bits differ in {rows.size} of {len(I)} rows, first query {rows[0]}"


def _check(idx, c, oracle, what="", rows=None):
    rows = np.arange(c.q.shape[0]) if rows is None else np.asarray(rows)
    q = np.ascontiguousarray(c.q[rows])
    D, I = idx.search(q, c.n)
    De, Ie = _expected(c, oracle)
    _assert_equal(D, I, De[rows], Ie[rows], f"{c.name} {what}")
    assert_output_contract(D, I, c.x, q, c.metric, c.n, oracle)
    return D, I


# ---- a. the 64-port boundary ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("name", ("ports63", "ports64"))
def test_port_boundary(gpu_faiss, oracle, name, metric):
    """default set_entry: 63 nodes above level 0 -- the descent's single island comes back; 64 -- the four islands of the
    coarse scan's best ports"""
    c = cases.case(name, metric)
    D, I = _check(_import(gpu_faiss, c), c, oracle)
    filled = (I >= 0).sum(axis=1)
    assert (filled == (8 if name == "ports63" else 32)).all()


# ---- b. the coarse rule --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("scan", tuple(SCANS))
@pytest.mark.parametrize("name", ("coarse-c1", "coarse-c4", "coarse-c64", "coarse-shared", "coarse-tie"))
def test_coarse_rule(gpu_faiss, oracle, monkeypatch, name, scan, metric):
    """the c best ports under (score, lower id), mapped from the coarse index's rows back to node ids; integer rows: the
    bf16 scan and the fp32 scan must give the same bits"""
    c = cases.case(name, metric)
    _check(_import(gpu_faiss, c, scan, monkeypatch), c, oracle, scan)


# ---- c. the descent rule -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("name", ("descent-l1", "descent-l2", "descent-l3", "descent-tie"))
def test_descent_rule(gpu_faiss, oracle, name, metric):
    """set_entry(0) with 96 ports: the greedy descent from (entry_point, max_level), through local minima, empty lists, lists
    with holes and equal scores (the lower id wins; an equal score of lower id replaces the current node)"""
    c = cases.case(name, metric)
    D, I = _check(_import(gpu_faiss, c), c, oracle)
    assert ((I >= 0).sum(axis=1) == 8).all()


# ---- d. query counts -----------------------------------------------------------------------------------------------
COUNTS = (1, 127, 128, 511, 512, 600)  # the host walk uses OpenMP from 128 walkers and runs in two halves from 512


@pytest.mark.parametrize("metric", METRICS)
def test_query_counts_descent(gpu_faiss, oracle, metric):
    """every row equals the single-query result for its query, whatever the batch it was walked in"""
    c = cases.case("descent-counts", metric)
    idx = _import(gpu_faiss, c)
    De, Ie = _expected(c, oracle)
    for nq in COUNTS:
        D, I = idx.search(np.ascontiguousarray(c.q[:nq]), c.n)
        _assert_equal(D, I, De[:nq], Ie[:nq], f"nq = {nq}")
    assert_output_contract(D, I, c.x, c.q, metric, c.n, oracle)
    last = c.q.shape[0] - 1
    _check(idx, c, oracle, "one query alone", rows=[last])


@pytest.mark.parametrize("metric", METRICS)
def test_query_counts_coarse(gpu_faiss, oracle, metric):
    """600 queries cycling over the case's six vectors"""
    c = cases.case("coarse-c4", metric)
    _check(_import(gpu_faiss, c), c, oracle, "nq = 600", rows=np.arange(600) % c.q.shape[0])


# ---- e. toggling ---------------------------------------------------------------------------------------------------
TOGGLE = ((4, "coarse-c4"), (0, "toggle-descent"), (4, "coarse-c4"), (1, "coarse-c1"))


@pytest.mark.parametrize("metric", METRICS)
def test_set_entry_toggled_on_one_index(gpu_faiss, oracle, metric):
    """set_entry 4, 0, 4, 1 on one index: the coarse index is dropped with the first toggle and rebuilt with the second; every
    search equals a fresh index's with that setting (the three cases are one graph and one set of rows)"""
    base = cases.case("coarse-c4", metric)
    idx = _import(gpu_faiss, base)
    for entry, name in TOGGLE:
        c = cases.case(name, metric)
        assert c.spec.entry == entry and np.array_equal(c.x, base.x) and np.array_equal(c.nbrs, base.nbrs) and np.array_equal(c.q, base.q)
        idx.set_entry(entry)
        D, I = _check(idx, c, oracle, f"after set_entry({entry})")
        Df, If = _import(gpu_faiss, c).search(c.q, c.n)
        _assert_equal(D, I, Df, If, f"set_entry({entry}) against a fresh index")


# ---- f. real-valued rows -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("name,scan", (("gauss-coarse", "bf16"), ("gauss-coarse", "fp32"), ("gauss-descent", "bf16"), ("gauss-wide", "bf16")))
def test_real_valued_rows(gpu_faiss, oracle, monkeypatch, name, scan, metric):
    """Gaussian rows: d = 100 (padded rows) under both rules, d = 1028 (wider than the device beam serves: the host walk
    descends and beams, ef = n) under the descent.  The margins are asserted in tests/test_hnsw_reference.py."""
    c = cases.case(name, metric)
    _check(_import(gpu_faiss, c, scan, monkeypatch), c, oracle, scan)


# ---- g. the file round trip ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
def test_file_round_trip(gpu_faiss, oracle, tmp_path, metric):
    c = cases.case("coarse-c4", metric)
    idx = _import(gpu_faiss, c)
    gpu_faiss.write_index(idx, tmp_path / "islands.index", rows=c.x)
    back = gpu_faiss.read_index(tmp_path / "islands.index")
    for a, b in zip(idx.graph(), back.graph()):
        assert np.array_equal(a, b)
    assert back.ntotal == c.n and back.hnsw.efSearch == c.n and back.hnsw.max_level == c.max_level and back.hnsw.entry_point == c.entry_point
    _check(back, c, oracle, "read back, the coarse rule")
    back.set_entry(0)
    _check(back, cases.case("toggle-descent", metric), oracle, "read back, the descent")


# ---- h. upper-level links to nodes without that level --------------------------------------------------------------
def _one_bad_link(c, level):
    """the case's tables with one id added to a level-`level` list: a node whose top level is level - 1"""
    lists = [[list(l) for l in node] for node in c.lists]
    host = next(i for i in c.ports.tolist() if c.levels[i] >= level and -1 not in lists[i][level] and 0 < len(lists[i][level]) < M + 1)
    low = int(np.flatnonzero(c.levels == level - 1)[-1])
    lists[host][level][-1] = low
    return tables(c.levels, lists, M), host, low


@pytest.mark.parametrize("level", (1, 2))
def test_import_refuses_an_upper_link_to_a_node_without_the_level(gpu_faiss, oracle, tmp_path, level):
    from knn_for_homology_amd import _lib
    c = cases.case("descent-l2", 1)
    (levels, offsets, nbrs), host, low = _one_bad_link(c, level)
    assert nbrs.size == c.nbrs.size and (nbrs != c.nbrs).sum() == 1 and c.levels[low] == level - 1
    idx = _storage(gpu_faiss, c)
    assert _raw_import(idx, levels, nbrs, c.max_level, c.entry_point) == -1, "KNN_ERR_INVALID"
    assert b"does not have that level" in _lib.lib().knn_last_error()
    assert idx.ntotal == 0 and idx.hnsw.max_level == -1 and idx.hnsw.entry_point == -1 and idx.graph()[0].size == 0
    # the corrected tables go into the same handle, and the search is the case's
    _lib.check(_raw_import(idx, c.levels, c.nbrs, c.max_level, c.entry_point))
    assert idx.ntotal == c.n
    idx.hnsw.efSearch = c.n
    idx.set_entry(0)
    _check(idx, c, oracle, "after the refused import")
    # and read_index raises for a file that holds the bad table
    good = tmp_path / "good.index"
    gpu_faiss.write_index(idx, good, rows=c.x)
    blob = good.read_bytes()
    at = blob.index(c.nbrs.tobytes())
    bad = tmp_path / "bad.index"
    bad.write_bytes(blob[:at] + nbrs.tobytes() + blob[at + nbrs.nbytes:])
    assert gpu_faiss.read_index(good).ntotal == c.n
    with pytest.raises(RuntimeError, match="does not have that level"):
        gpu_faiss.read_index(bad)
