"""GPU: the HNSW device beam compared EXACTLY with a host reference, on small graphs walked to exhaustion.

With ef >= the number of nodes reachable at level 0 from the entry nodes the beam never fills and nothing is pruned: every
reachable node is scored, with keep == ef every one of them is re-scored by the contract's chain, and the result must be the
exact top k of the reachable set under (score, lower id) -- ids and score bits (tests/hnsw_reference.py).  Imported graphs
(knn_hnsw_graph_import, every node at level 0: the walk starts at entry_point alone) make the reachable set known exactly.

a  imported graphs: ring, two components, holes, self/duplicate links, full lists (M = 4, 42, 63), ties, every row width
   (all kernel builds), beam sizes 64 / 65 / 1000 / 1024, k above what can be reached
b  query counts and walker reuse, eager and lazy clearing of the visited bitmaps, search after search
c  built graphs (strongly connected: asserted), both entry rules
d  the keep / kmin cut between the beam and the exact re-score, k < ef
e  approximate searches: the output contract on the full result (no recall figure: tests/test_hnsw_gpu.py has those)

Left open here: WHICH node a search enters at.  Every graph of this file gives the same result from any entry node, so the
coarse scan and the greedy descent through the upper levels are not checked; tests/test_hnsw_entry_exact_gpu.py pins them,
on graphs whose level 0 is disjoint islands."""
import numpy as np
import pytest

from hnsw_reference import assert_output_contract, expected, level0_tables, reachable, strongly_connected

pytestmark = pytest.mark.gpu

METRICS = (0, 1)
NQ = 6
ENV = ("KNN355_HNSW_BEAM_FP32", "KNN355_HNSW_BEAM_ROWS", "KNN355_HNSW_KEYS_DIRECT", "KNN355_HNSW_CLEAR")


@pytest.fixture(autouse=True)
def _default_settings(monkeypatch):
    for name in ENV:
        monkeypatch.delenv(name, raising=False)


def _rows(n, d, seed):
    return np.random.default_rng(seed).standard_normal((n, d), dtype=np.float32)


def _ring_plus_random(n, extra, seed):
    """node i links to i + 1 (a Hamiltonian ring: connected) and to `extra` other nodes"""
    rng = np.random.default_rng(seed)
    lists = []
    for i in range(n):
        others = rng.choice(n - 1, size=min(extra, n - 2), replace=False)
        others = (others + (others >= i)).tolist()  # (never i itself)
        lists.append([(i + 1) % n] + [j for j in others if j != (i + 1) % n])
    return lists


def _import(gpu_faiss, x, lists, M, metric, entry, ef=None):
    """storage rows + knn_hnsw_graph_import, as read_index does for an "IHNf" file; every node at level 0"""
    from knn_for_homology_amd import _lib
    x = np.ascontiguousarray(x, np.float32)
    n, d = x.shape
    levels, _, nbrs, _ = level0_tables(lists, 2 * M)
    idx = gpu_faiss.IndexHNSWFlat(d, M, metric)
    L = _lib.lib()
    _lib.check(L.knn_flat_add(L.knn_hnsw_storage(idx._h), x.ctypes.data, n))
    _lib.check(L.knn_hnsw_graph_import(idx._h, n, levels.ctypes.data, nbrs.ctypes.data, nbrs.size, 0, int(entry)))
    assert idx.ntotal == n and idx.hnsw.max_level == 0 and idx.hnsw.entry_point == entry
    idx.hnsw.efSearch = n if ef is None else ef
    return idx


def _assert_equal(D, I, De, Ie, what=""):
    rows = np.flatnonzero((I != Ie).any(axis=1))
    assert rows.size == 0, f"{what}: ids differ in {rows.size} of {len(I)} rows, first query {rows[0]}: got {I[rows[0]][:12].tolist()} want {Ie[rows[0]][:12].tolist()}"
    rows = np.flatnonzero((D.view(np.uint32) != De.view(np.uint32)).any(axis=1))
    assert rows.size == 0, f"{what}: score bits differ in {rows.size} of {len(I)} rows, first query {rows[0]}"


def _check(idx, x, q, k, reach, metric, oracle, what=""):
    D, I = idx.search(q, k)
    De, Ie = expected(x, q, reach, k, metric, oracle)
    _assert_equal(D, I, De, Ie, what)
    assert_output_contract(D, I, x, q, metric, x.shape[0], oracle)
    return D, I


# ---- a. imported graphs --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
def test_ring(gpu_faiss, oracle, metric):
    """n = 1000, node i links only to i + 1: 1000 dependent expansions, the entry in the middle of the id range"""
    n, d = 1000, 32
    x, q = _rows(n, d, 1), _rows(NQ, d, 2)
    lists = [[(i + 1) % n] for i in range(n)]
    assert reachable(*level0_tables(lists, 8), [500]).size == n
    idx = _import(gpu_faiss, x, lists, 4, metric, 500)
    _check(idx, x, q, n, np.arange(n), metric, oracle)


@pytest.mark.parametrize("metric", METRICS)
def test_two_components(gpu_faiss, oracle, metric):
    """600 nodes in components of 257 and 343 (ids interleaved): only the entry's component comes back, the tail is padding"""
    n, d, M = 600, 48, 4
    x, q = _rows(n, d, 3), _rows(NQ, d, 4)
    rng = np.random.default_rng(5)
    perm = rng.permutation(n)
    lists = [None] * n
    for comp in (perm[:257], perm[257:]):
        for pos, i in enumerate(comp):
            lists[i] = [int(comp[(pos + 1) % comp.size])] + rng.choice(comp, 3).tolist()
    g = level0_tables(lists, 2 * M)
    for comp in (perm[:257], perm[257:]):
        entry = int(comp[comp.size // 2])
        reach = reachable(*g, [entry])
        assert np.array_equal(reach, np.sort(comp))
        idx = _import(gpu_faiss, x, lists, M, metric, entry)
        D, I = _check(idx, x, q, n, reach, metric, oracle, f"component of {comp.size}")
        assert (I[:, comp.size:] == -1).all() and (I[:, :comp.size] >= 0).all()


@pytest.mark.parametrize("metric", METRICS)
def test_holes(gpu_faiss, oracle, metric):
    """Lists with holes: a list ends at its first -1 (the fill knn_hnsw_graph_import defines).  Nodes 150..199 are named
    only behind holes -- the entry's list among them -- and must not come back."""
    n, d, M = 200, 40, 8
    x, q = _rows(n, d, 6), _rows(NQ, d, 7)
    x[150:] = q[np.arange(50) % NQ] + 0.01 * _rows(50, d, 8)  # (the hidden rows are every query's best rows: a walk that reads past a hole returns them first)
    rng = np.random.default_rng(9)
    lists = []
    for i in range(150):
        l = [(i + 1) % 150] + rng.integers(0, 150, 2).tolist()
        if i % 3 == 0:  # a hole, then real ids: two hidden nodes and a visible one
            l += [-1] + rng.integers(150, 200, 2).tolist() + [int(rng.integers(0, 150))]
        lists.append(l)
    for i in range(150, 200):  # the hidden nodes link among themselves and back into the rest
        lists.append([150 + (i + 1 - 150) % 50, int(rng.integers(0, 150))])
    entry = 75
    assert -1 in lists[entry]
    reach = reachable(*level0_tables(lists, 2 * M), [entry])
    assert np.array_equal(reach, np.arange(150))
    idx = _import(gpu_faiss, x, lists, M, metric, entry)
    D, I = _check(idx, x, q, n, reach, metric, oracle)
    assert (I < 150).all() and (I[:, 150:] == -1).all()
    # the exported graph is the imported one up to each list's fill
    nbrs = idx.graph()[2].reshape(n, 2 * M)
    for i in range(0, 150, 3):
        assert nbrs[i, :3].tolist() == lists[i][:3] and (nbrs[i, 3:] == -1).all()


@pytest.mark.parametrize("metric", METRICS)
def test_self_links_and_duplicate_links(gpu_faiss, oracle, metric):
    """Lists name their own node, the same id several times, and ids their neighbour's list names too (i and i + 1 are
    expanded in the same step and both link to i + 2 and i + 3): the visited bitmap must let every id through once"""
    n, d, M = 300, 24, 8
    x, q = _rows(n, d, 10), _rows(NQ, d, 11)
    rng = np.random.default_rng(12)
    lists = []
    for i in range(n):
        r = int(rng.integers(0, n))
        lists.append([i, (i + 1) % n, (i + 1) % n, (i + 2) % n, r, r, (i + 3) % n, i, (i + 2) % n, r, (i + 1) % n])
    idx = _import(gpu_faiss, x, lists, M, metric, 17)
    _check(idx, x, q, n, np.arange(n), metric, oracle)


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("M", (4, 42, 63))
def test_full_lists(gpu_faiss, oracle, M, metric):
    """every level-0 list holds 2M ids; M = 63 is the largest knn_hnsw_create accepts: 126 ids, more than the 64 a wave
    tests and scores in one go"""
    n, d = 500, 40
    with pytest.raises(RuntimeError):
        gpu_faiss.IndexHNSWFlat(d, 64, metric)
    x, q = _rows(n, d, 13), _rows(NQ, d, 14)
    lists = _ring_plus_random(n, 2 * M - 1, 15 + M)
    assert all(len(l) >= 2 * M - 1 for l in lists)
    lists = [l + [(i + 2) % n] * (2 * M - len(l)) for i, l in enumerate(lists)]  # (the ring link was drawn again: fill the slot)
    assert all(len(l) == 2 * M and -1 not in l for l in lists)
    idx = _import(gpu_faiss, x, lists, M, metric, n // 2)
    _check(idx, x, q, n, np.arange(n), metric, oracle)


@pytest.mark.parametrize("metric", METRICS)
def test_ties(gpu_faiss, oracle, metric):
    """exact duplicate rows at scattered ids (and small-integer rows: many equal scores among different rows too): the
    lower id comes first"""
    n, d, M = 400, 24, 4
    rng = np.random.default_rng(16)
    x = rng.integers(-2, 3, (n, d)).astype(np.float32)
    q = rng.integers(-2, 3, (NQ, d)).astype(np.float32)
    src = rng.choice(n, 60, replace=False)
    x[src[30:]] = x[src[:30]]
    x[src[25:30]] = x[src[0]]  # one row six times
    idx = _import(gpu_faiss, x, _ring_plus_random(n, 3, 17), M, metric, 123)
    D, I = _check(idx, x, q, n, np.arange(n), metric, oracle)
    ties = (D[:, 1:] == D[:, :-1])
    assert ties.sum() > 30 * NQ and (I[:, 1:][ties] > I[:, :-1][ties]).all()


WIDTHS = (20, 100, 256, 257, 520, 1024)  # dp = 32, 128, 256, 288, 544, 1024: one, two and four 16-byte chunks per lane
MODES = {"bf16": {}, "fp32": {"KNN355_HNSW_BEAM_FP32": "1"},
         "rows8": {"KNN355_HNSW_BEAM_ROWS": "8"},
         "fp32_rows8": {"KNN355_HNSW_BEAM_FP32": "1", "KNN355_HNSW_BEAM_ROWS": "8"},
         "direct": {"KNN355_HNSW_KEYS_DIRECT": "1"}}
WIDTH_CASES = ([(d, m) for d in WIDTHS for m in ("bf16", "fp32")] + [(d, "rows8") for d in (100, 520, 1024)] +
               [(d, "fp32_rows8") for d in (100, 257, 520, 1024)] + [(d, "direct") for d in (100, 520)])


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("d,mode", WIDTH_CASES)
def test_row_widths(gpu_faiss, oracle, monkeypatch, d, mode, metric):
    """a random 3-regular graph plus a Hamiltonian ring, at every row width and under every beam build: bf16 rows
    (default), fp32 rows, eight rows in flight (with fp32 rows: the RB = 8 builds), the one-lane-per-pair re-score.  With
    keep == ef the bf16 beam is exact too: its scores only order the expansions"""
    for name, value in MODES[mode].items():
        monkeypatch.setenv(name, value)
    n, M = 300, 4
    x, q = _rows(n, d, 18 + d), _rows(NQ, d, 19 + d)
    idx = _import(gpu_faiss, x, _ring_plus_random(n, 3, 20), M, metric, 150)
    _check(idx, x, q, n, np.arange(n), metric, oracle, f"d = {d}, {mode}")


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("ef", (64, 65, 1000, 1024))
def test_beam_sizes(gpu_faiss, oracle, ef, metric):
    """a connected graph of exactly ef nodes, k = ef: one beam entry per lane, one more than that, and the largest beam"""
    d = 36
    x, q = _rows(ef, d, 21), _rows(NQ, d, 22)
    idx = _import(gpu_faiss, x, _ring_plus_random(ef, 3, 23), 4, metric, ef // 3)
    assert idx.hnsw.efSearch == ef
    _check(idx, x, q, ef, np.arange(ef), metric, oracle)


@pytest.mark.parametrize("metric", METRICS)
def test_k_above_what_can_be_reached(gpu_faiss, oracle, metric):
    """ef = k = 150 < n = 400, but only 90 nodes can be reached: they all come back, the tail is padding"""
    n, d, M = 400, 20, 4
    x, q = _rows(n, d, 24), _rows(NQ, d, 25)
    lists = _ring_plus_random(n, 3, 26)
    comp = np.random.default_rng(27).choice(n, 90, replace=False)
    for pos, i in enumerate(comp):  # a closed component of 90 scattered nodes; the others link into it, not it to them
        lists[i] = [int(comp[(pos + 1) % 90]), int(comp[(pos * 7 + 3) % 90])]
    entry = int(comp[11])
    reach = reachable(*level0_tables(lists, 2 * M), [entry])
    assert np.array_equal(reach, np.sort(comp))
    idx = _import(gpu_faiss, x, lists, M, metric, entry, ef=64)
    for k in (150, 90, 91):
        D, I = _check(idx, x, q, k, reach, metric, oracle, f"k = {k}")
        assert (I[:, :90] >= 0).all() and (I[:, 90:] == -1).all()


# ---- b. query counts and walker reuse ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def walker_graph():
    n, d = 300, 64
    return _rows(n, d, 30), _ring_plus_random(n, 5, 31)


def _query_counts():
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    # 16 walkers per CU at the most: the third count gives some walkers a second query, the fourth gives every walker a
    # second one and some a third
    return (1, 5, 16 * cus + 37, 32 * cus + 5)


@pytest.mark.parametrize("metric", METRICS)
def test_walkers_serve_several_queries_search_after_search(gpu_faiss, oracle, monkeypatch, walker_graph, metric):
    """one walker, one visited bitmap, several queries, and the same index searched again and again -- with the bitmaps
    cleared whole before each walk (eager) and word by word after it (lazy), and going from one mode to the other"""
    x, lists = walker_graph
    n, d = x.shape
    counts = _query_counts()
    q = _rows(max(counts), d, 32)
    De, Ie = expected(x, q, np.arange(n), n, metric, oracle)
    idx = _import(gpu_faiss, x, lists, 4, metric, 7)
    for mode in ("eager", "lazy", "eager", "lazy"):
        monkeypatch.setenv("KNN355_HNSW_CLEAR", mode)
        for nq in counts:
            for rep in range(3):
                D, I = idx.search(q[:nq], n)
                _assert_equal(D, I, De[:nq], Ie[:nq], f"{mode}, nq = {nq}, search {rep}")


# ---- c. built graphs -----------------------------------------------------------------------------------------------
# Squared L2 with M = 8 on Gaussian rows of 48 or 128 dimensions leaves nodes nobody links to (hubs take the sixteen slots):
# not strongly connected at any of the four seeds tried per shape.  Those six shapes take rows of a low intrinsic dimension
# instead (four Gaussian coordinates mapped into d dimensions, plus a little noise), where the built level-0 graph is strongly
# connected.  The build is deterministic, so the precondition the test asserts holds or fails for good.
RANK = {(n, 8, d, 1): 4 for n in (257, 640, 1000) for d in (48, 128)}


def built_rows(n, d, M, metric, rank=None):
    rng = np.random.default_rng(1000 * M + n + d + metric)
    rank = RANK.get((n, M, d, metric)) if rank is None else rank
    if not rank:
        return rng.standard_normal((n, d), dtype=np.float32)
    z = rng.standard_normal((n, rank), dtype=np.float32) @ rng.standard_normal((rank, d), dtype=np.float32)
    return np.ascontiguousarray(z + 0.05 * rng.standard_normal((n, d), dtype=np.float32))


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("d", (48, 128))
@pytest.mark.parametrize("M", (8, 32))
@pytest.mark.parametrize("n", (257, 640, 1000))
def test_built_graphs(gpu_faiss, oracle, n, M, d, metric):
    """idx.add builds the graph; efSearch = k = n.  The level-0 graph is strongly connected (asserted), so whichever node
    an entry rule picks, everything is reached: the result is the flat search over all rows -- from the exact scan of the
    nodes above level 0 (or, with fewer than 64 of them, the greedy descent) and under set_entry(0).  That the rules pick
    the RIGHT nodes is what tests/test_hnsw_entry_exact_gpu.py checks."""
    x, q = built_rows(n, d, M, metric), _rows(NQ, d, 41)
    idx = gpu_faiss.IndexHNSWFlat(d, M, metric)
    idx.add(x)
    idx.hnsw.efSearch = n
    assert strongly_connected(*idx.graph()), "precondition: the built level-0 graph is strongly connected"
    for entries in (4, 0):
        idx.set_entry(entries)
        _check(idx, x, q, n, np.arange(n), metric, oracle, f"set_entry({entries})")


# ---- d. the keep / kmin cut ----------------------------------------------------------------------------------------
def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def planted_rows(k, seed=50):
    """n = 1000 unit rows, 64 unit queries in groups around random centres; each group has exactly k planted rows at
    cosine ~0.96 to every query of the group, everything else is a random unit vector"""
    n, d, nq = 1000, 64, 64
    rng = np.random.default_rng(seed + k)
    groups = min(nq, 400 // k)
    x = _unit(rng.standard_normal((n, d)))
    cent = _unit(rng.standard_normal((groups, d)))
    slots = rng.permutation(n)[:groups * k].reshape(groups, k)
    for g in range(groups):
        x[slots[g]] = _unit(cent[g] + 0.25 * _unit(rng.standard_normal((k, d))))
    q = _unit(cent[np.arange(nq) % groups] + 0.05 * _unit(rng.standard_normal((nq, d))))
    return np.ascontiguousarray(x, np.float32), np.ascontiguousarray(q, np.float32)


@pytest.mark.parametrize("k", (10, 40, 100))
def test_keep_cut_keeps_the_planted_neighbours(gpu_faiss, oracle, monkeypatch, k):
    """k < ef = n: the beam hands its best kmin..keep rows, by ITS scores, to the exact re-score.  Every query has exactly k
    rows at cosine >= 0.9 and the oracle's k-th score exceeds its (k+1)-th by more than 0.25 (checked here, on the inputs):
    far above the scoring error of the fp32 beam (summation order: ~1e-6) and of the bf16 beam (rows rounded to 8 bits:
    ~4e-3 for unit rows), so no cut can be excused for dropping a planted row"""
    x, q = planted_rows(k)
    n = x.shape[0]
    Do, Io = oracle.flat_search(x, q, k + 1, 0)
    assert (Do[:, k - 1] >= 0.9).all() and (Do[:, k - 1] - Do[:, k] > 0.25).all(), "condition on the inputs"
    for fp32 in ("0", "1"):
        monkeypatch.setenv("KNN355_HNSW_BEAM_FP32", fp32)
        idx = gpu_faiss.IndexHNSWFlat(64, 16, 0)
        idx.add(x)
        idx.hnsw.efSearch = n
        assert strongly_connected(*idx.graph()), "precondition: every row can be reached"
        D, I = idx.search(q, k)
        _assert_equal(D, I, Do[:, :k], Io[:, :k], f"KNN355_HNSW_BEAM_FP32={fp32}")
        assert_output_contract(D, I, x, q, 0, n, oracle)


def near_tied_rows(k, seed=60):
    """as planted_rows, one query per group and k + 4 planted rows: k - 4 at cosines spread over 0.93..0.99, then EIGHT at
    cosines 0.92 + j * 1e-6 -- ranks k-3 .. k+4, straddling the cut"""
    n, d, nq = 1000, 64, 16
    rng = np.random.default_rng(seed + k)
    x = _unit(rng.standard_normal((n, d)))
    q = _unit(rng.standard_normal((nq, d)))
    slots = rng.permutation(n)[:nq * (k + 4)].reshape(nq, k + 4)
    cos = np.concatenate([np.linspace(0.99, 0.93, k - 4), 0.92 + 1e-6 * np.arange(8)])
    for g in range(nq):
        u = rng.standard_normal((k + 4, d))
        u = _unit(u - (u @ q[g])[:, None] * q[g][None, :])  # unit, orthogonal to the query
        x[slots[g]] = cos[:, None] * q[g][None, :] + np.sqrt(1.0 - cos ** 2)[:, None] * u
    return np.ascontiguousarray(x, np.float32), np.ascontiguousarray(q, np.float32)


@pytest.mark.parametrize("k", (10, 40))
def test_keep_cut_with_near_ties_across_the_cut(gpu_faiss, oracle, monkeypatch, k):
    """The slack of the cut is there for scores the beam cannot tell apart: the rows of ranks k-3 .. k+4 lie within 1e-4 of
    each other -- below the bf16 beam's error, so its order among them is arbitrary -- and rank k+5 is more than 0.25 away
    (both checked here, on the inputs).  The beam hands on at least k + 8 rows by its own scores (kmin = k + max(k/8, 8)):
    all k + 4 planted rows are among them whatever their order, and the exact re-score must return the oracle's top k."""
    x, q = near_tied_rows(k)
    n = x.shape[0]
    Do, Io = oracle.flat_search(x, q, k + 5, 0)
    assert (Do[:, k - 4] - Do[:, k + 3] < 1e-4).all() and (Do[:, k + 3] - Do[:, k + 4] > 0.25).all(), "condition on the inputs"
    for fp32 in ("0", "1"):
        monkeypatch.setenv("KNN355_HNSW_BEAM_FP32", fp32)
        idx = gpu_faiss.IndexHNSWFlat(64, 16, 0)
        idx.add(x)
        idx.hnsw.efSearch = n
        assert strongly_connected(*idx.graph()), "precondition: every row can be reached"
        D, I = idx.search(q, k)
        _assert_equal(D, I, Do[:, :k], Io[:, :k], f"KNN355_HNSW_BEAM_FP32={fp32}")
        assert_output_contract(D, I, x, q, 0, n, oracle)


# ---- e. approximate searches ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
def test_approximate_searches_keep_the_output_contract(gpu_faiss, oracle, metric):
    n, d, nq, k = 20000, 100, 500, 50
    rng = np.random.default_rng(70)
    cent = rng.standard_normal((200, d), dtype=np.float32)
    x = cent[rng.integers(0, 200, n)] + 0.35 * rng.standard_normal((n, d), dtype=np.float32)
    x[n - 500:] = x[:500]  # (exact duplicates: equal scores inside an approximate result)
    q = np.ascontiguousarray(x[::n // nq][:nq] + 0.05 * rng.standard_normal((nq, d), dtype=np.float32))
    idx = gpu_faiss.IndexHNSWFlat(d, 32, metric)
    idx.add(x)
    for ef in (64, 256):
        idx.hnsw.efSearch = ef
        D, I = idx.search(q, k)
        assert (I >= 0).all(), "20 000 connected rows: every slot is filled"
        assert_output_contract(D, I, x, q, metric, n, oracle)
