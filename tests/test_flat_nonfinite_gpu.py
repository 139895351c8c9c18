"""GPU: non-finite and overflowing scores on the fp32 IndexFlat paths (a "smaller is better" value of
+inf or a NaN never becomes a hit; an inner-product score of +inf is the best hit; +-FLT_MAX keeps its id; a starved query
is padded with (-1, -+FLT_MAX)).

Every case builds its data with tests/nonfinite_cases.poison (poisoned rows at the positions a kernel treats specially,
poisoned queries, near-duplicates that would lead a list), compares the library with the CPU oracle bit for bit (ids and
distance bits), asserts the path it means to cover through last_scan() / last_seed() / last_range(), and asserts on the
ORACLE's answer that it is not vacuous: some query has fewer than k hits, some inner-product hit is +inf, the poisoned copy
of a near-duplicate's query is absent from the list it would lead.  tests/test_nonfinite_reference.py pins the oracle itself
to the hand-derived table.

k never exceeds the library's 2048: the starved-list cases (k = nb - 3) run on 2051 rows.  The poisoned kinds need eight
columns, so the smallest range-search shape is 37 x 8 with 7 queries.

What fails without the library's two guards (run against the parent's library): every test_query_tile_builds case and
test_search_keys_and_merge return (row, +-inf) where the oracle pads -- select_topk_kernel's load did not drop the +inf
keys; test_normalize leaves a row whose norm overflows as it was -- normalize_rows_kernel read the factor 0 as "leave the
row alone".  No NaN reaches a key at any site: each forms its key behind an ordered compare, which a NaN fails."""
import numpy as np
import pytest

import nonfinite_cases as nc
from flat_lifecycle_reference import expected_range
from knn_for_homology_amd._lib import (KNN_TUNE_BIG_TILE, KNN_TUNE_EXACT_SEED, KNN_TUNE_NO_BIG_TILE, KNN_TUNE_NO_SCAN16,
                                       KNN_TUNE_NO_SEED, KNN_TUNE_NO_SYM, KNN_TUNE_NORM_L2, KNN_TUNE_SCAN16_ANY_NB,
                                       KNN_TUNE_STAT_SEED)

pytestmark = pytest.mark.gpu

IP, L2 = 0, 1
FLT_MAX = nc.FLT_MAX


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _assert_same(D, I, Do, Io, what=""):
    bad = np.flatnonzero((I != Io).any(1))
    assert bad.size == 0, (f"{what}: {int((I != Io).sum())} neighbour ids differ, first in query {bad[0]}: got "
                           f"{I[bad[0]][I[bad[0]] != Io[bad[0]]][:6]} / {D[bad[0]][I[bad[0]] != Io[bad[0]]][:6]}, expected "
                           f"{Io[bad[0]][I[bad[0]] != Io[bad[0]]][:6]} / {Do[bad[0]][I[bad[0]] != Io[bad[0]]][:6]}")
    assert np.array_equal(_bits(D), _bits(Do)), f"{what}: {int((_bits(D) != _bits(Do)).sum())} distances differ"


def _not_vacuous(oracle, table, Do, Io, metric, l2_mode=0, rows=None):
    """on the oracle's answer: a starved list, a +inf inner-product hit, the near-duplicates' copies absent where they would lead"""
    k = Io.shape[1]
    assert ((Io >= 0).sum(1) < k).any(), "no query has fewer than k hits"
    pad = -FLT_MAX if metric == IP else FLT_MAX
    assert (Do[Io < 0] == pad).all()
    if metric == IP:
        assert np.isposinf(Do).any(), "no +inf inner-product hit"
    xb = table.xb if rows is None else rows
    for q, r in table.near.items():
        assert r not in Io[q]
        clean = xb.copy()
        clean[r] = table.xq[q]
        assert oracle.flat_search(clean, table.xq[q:q + 1], 1, metric, l2_mode=l2_mode)[1][0, 0] == r, "unpoisoned, the copy leads"


def _problem(seed, nb, nq, d, tile=256, nchunks=1, **kw):
    if nq < 8 and not kw:   # (fewer than 8 queries: one near-duplicate and three poisoned queries)
        kw = dict(near=1, query_kinds=("nan", "pinf", "twin"))
    return nc.poison(np.random.default_rng(seed), nb, nq, d, nc.special_rows(nb, tile, max(nchunks, 1)), **kw)


def _search(gpu_faiss, oracle, xb, xq, table, k, metric, qt=0, nch=0, flags=0, l2_mode=None, idx=None):
    if idx is None:
        idx = gpu_faiss.IndexFlat(xb.shape[1], metric)
        idx.add(xb)
    idx.set_tuning(qt, nch, flags)
    D, I = idx.search(xq, k)
    mode = (1 if flags & KNN_TUNE_NORM_L2 else 0) if l2_mode is None else l2_mode
    Do, Io = oracle.flat_search(xb, xq, k, metric, l2_mode=mode)
    _not_vacuous(oracle, table, Do, Io, metric, l2_mode=1 if (mode == 1 or xq.shape[0] >= 20) else 2)
    _assert_same(D, I, Do, Io, str(idx.last_scan()))
    return idx


# ---- every query-tile build: k = 10 and starved lists (k = nb - 3), one chunk and three, both metrics -----------------------
@pytest.mark.parametrize("metric", [IP, L2])
@pytest.mark.parametrize("nch", [1, 3])
@pytest.mark.parametrize("qt,nq", [(32, 7), (48, 41), (64, 60), (96, 80), (128, 133), (256, 260)])
def test_query_tile_builds(gpu_faiss, oracle, qt, nq, nch, metric):
    dt = 256 if qt in (32, 48, 256) else 128
    for nb, k in ((6000 if qt == 256 else 5000, 10), (2051, 2048)):
        xb, xq, table = _problem(qt * 100 + nch * 10 + metric + nb, nb, nq, 64, dt, nch)
        # (fewer than 20 L2 queries are the difference build's; KNN_TUNE_NORM_L2 keeps them on the norm formula's 32-query build)
        for flags in ((0, KNN_TUNE_NORM_L2) if (metric == L2 and nq < 20) else (0,)):
            idx = _search(gpu_faiss, oracle, xb, xq, table, k, metric, qt, nch, flags)
            sc = idx.last_scan()
            diff = metric == L2 and nq < 20 and not flags
            assert sc["query_tile"] == qt and sc["nchunks"] == nch and sc["db_tile"] == dt, sc
            assert sc["kernel"] == (f"flat_scan_q{qt}_d{dt}" + ("_l2diff" if diff else "")), sc


# ---- the four difference builds; the twin separates the two L2 formulas ------------------------------------------------------
@pytest.mark.parametrize("nq", [8, 12, 16, 19])
def test_difference_builds(gpu_faiss, oracle, nq):
    nb, d, k = 700, 37, 20
    xb, xq, table = _problem(nq, nb, nq, d)
    (qt,), rows = table.queries_of("twin"), table.rows_of("twin")
    idx = _search(gpu_faiss, oracle, xb, xq, table, k, L2)
    assert idx.last_scan()["kernel"] == "flat_scan_q32_d256_l2diff", idx.last_scan()
    D, I = idx.search(xq, k)
    assert list(I[qt, :len(rows)]) == rows and (D[qt, :len(rows)] == 0).all(), "twin against twin: exactly 0 by differences"
    idx = _search(gpu_faiss, oracle, xb, xq, table, k, L2, flags=KNN_TUNE_NORM_L2, idx=idx)
    assert idx.last_scan()["kernel"] == "flat_scan_q32_d256", idx.last_scan()
    Dn, In = idx.search(xq, k)
    assert not np.isin(rows, In[qt]).any(), "twin against twin: +inf by the norm formula"


# ---- streaming regime: paired walk, tile-minimum seed (one key per workgroup / per wave), the parked first tile ---------------
@pytest.mark.parametrize("metric", [IP, L2])
@pytest.mark.parametrize("nq,nb,d,k,qt", [(20, 70001, 64, 10, 32), (36, 70001, 64, 10, 48), (47, 140000, 32, 600, 48)])
def test_streaming_paired_walk_and_tile_minimum_seed(gpu_faiss, oracle, nq, nb, d, k, qt, metric):
    xb, xq, table = _problem(nq + nb + metric, nb, nq, d, 256, 16)
    idx = _search(gpu_faiss, oracle, xb, xq, table, k, metric)
    sc, seed = idx.last_scan(), idx.last_seed()
    # (one query tile and >= 64 tiles: workgroups in pairs, grid = nchunks = 2 npairs; no sample pass: the bound is the k-th
    # published tile minimum, one key per workgroup for k = 10 and one per wave for k = 600)
    assert sc["query_tile"] == qt and sc["nchunks"] == sc["grid"] and sc["nchunks"] % 2 == 0 and sc["nchunks"] >= 64, sc
    assert seed["stride"] == (-1 if k <= 100 else -4) and seed["stat_rank"] == 0, seed   # (keys published per workgroup and query)


# ---- the exact seed's sample pass: poison inside the sample (rows 0 .. 7 belong to every sample) and outside -----------------
@pytest.mark.parametrize("metric", [IP, L2])
def test_exact_seed_sample_pass(gpu_faiss, oracle, metric):
    nb, nq, d, k = 40000, 70, 64, 100
    xb, xq, table = _problem(31 + metric, nb, nq, d, 128, 8)
    idx = _search(gpu_faiss, oracle, xb, xq, table, k, metric, flags=KNN_TUNE_EXACT_SEED)
    seed = idx.last_seed()
    assert seed["stride"] > 1 and seed["stat_rank"] == 0 and seed["sample_rows"] > 0, seed
    assert {0, 3} <= set(table.rows) and any(r >= 8 and (r >> 3) % seed["stride"] != 0 for r in table.rows), "poison on both sides of the sample"


# ---- the statistical seed and its repair: poison on sampled rows (row % 64 == 0, row % 128 == 0) ---------------------------------
@pytest.mark.parametrize("metric", [IP, L2])
@pytest.mark.parametrize("k", [10, 100])
def test_statistical_seed(gpu_faiss, oracle, k, metric):
    nb, nq, d = 16384, 130, 32
    xb, xq, table = _problem(55 + k + metric, nb, nq, d, 128, 4)
    idx = _search(gpu_faiss, oracle, xb, xq, table, k, metric, flags=KNN_TUNE_STAT_SEED)
    seed = idx.last_seed()
    # a starved query fails the estimate's verification (its k-th key does not exist): the search is then repeated without
    # the estimate and last_seed() describes the repeat.  Either way the statistical seed ran; the answer, checked above,
    # may not differ
    assert (seed["stride"] > 0 and 0 < seed["stat_rank"] < k) or seed["stat_redo"] >= 1, seed
    assert {0, 64, 128} <= set(table.rows), "poison on rows of every stride-32 / stride-64 sample"


# ---- 4096-key lists (k in (1536, 2048]): wave_select_mem --------------------------------------------------------------------
@pytest.mark.parametrize("metric", [IP, L2])
@pytest.mark.parametrize("k", [1537, 2048])
@pytest.mark.parametrize("nq", [5, 33])
def test_4096_key_lists(gpu_faiss, oracle, nq, k, metric):
    # (fewer than 8 queries: one near-duplicate and three poisoned queries)
    kw = dict(near=1, query_kinds=("nan", "pinf", "twin")) if nq < 8 else {}
    xb, xq, table = _problem(nq + k + metric, 4100, nq, 32, **kw)
    for flags in (0, KNN_TUNE_NO_SEED):
        idx = _search(gpu_faiss, oracle, xb, xq, table, k, metric, flags=flags)
    assert idx.last_scan()["query_tile"] in (32, 48), idx.last_scan()


# ---- final selection: one wave per query (batch regime), the segment pass over long candidate arrays --------------------------
@pytest.mark.parametrize("metric", [IP, L2])
@pytest.mark.parametrize("k", [40, 301])
def test_one_wave_final_selection(gpu_faiss, oracle, k, metric):
    xb, xq, table = _problem(1000 + k + metric, 16384, 640, 32, 128, 4)
    idx = _search(gpu_faiss, oracle, xb, xq, table, k, metric)
    assert idx.last_seed()["stat_rank"] > 0 or idx.last_seed()["stat_redo"] >= 1, idx.last_seed()   # (see test_statistical_seed)


@pytest.mark.parametrize("metric", [IP, L2])
def test_segment_pass_over_long_candidate_arrays(gpu_faiss, oracle, metric):
    nb, d, nq, k = 300_000, 32, 5, 100
    xb, xq, table = _problem(900 + metric, nb, nq, d, 256, 64, near=1, query_kinds=("nan", "pinf", "huge"))
    idx = _search(gpu_faiss, oracle, xb, xq, table, k, metric, flags=KNN_TUNE_NO_SEED)
    assert idx.last_scan()["nchunks"] * 125 > 32768, idx.last_scan()


# ---- symmetric self-search: both sym builds against the plain launch and the oracle ------------------------------------------
@pytest.mark.parametrize("metric", [IP, L2])
@pytest.mark.parametrize("n,k", [(3000, 11), (4100, 301)])
def test_symmetric_self_search(gpu_faiss, oracle, n, k, metric):
    d = 48
    x, _, table = _problem(n + k + metric, n, 8, d, 128, 4)
    (huge,) = table.rows_of("huge")[:1]
    idx = gpu_faiss.IndexFlat(d, metric)
    idx.add(x)
    Do, Io = oracle.flat_search(x, x, k, metric)
    assert ((Io >= 0).sum(1) < k).any() and (metric == L2 or np.isposinf(Do).any())
    for r in table.rows_of("nan"):   # (a NaN row has no hit as a query and is nobody's hit as a row)
        assert (Io[r] == -1).all() and not (Io == r).any()
    if metric == L2:
        assert (Io[huge] == -1).all(), "the huge row has no hit, not even itself (nrm = +inf, dot = +inf: NaN)"
    for flags, kernel in ((KNN_TUNE_NO_BIG_TILE, "flat_scan_q128_d128_sym"), (KNN_TUNE_BIG_TILE, "flat_scan_q256_d256_sym"),
                          (KNN_TUNE_NO_SYM | KNN_TUNE_NO_BIG_TILE, "flat_scan_q128_d128")):
        idx.set_tuning(0, 0, flags)
        before = idx.last_seed()["stat_redo"]
        D, I = idx.search_self(k)
        # (a row without k hits fails the symmetric launch's verification: the plain launch then repeats the search)
        plain = kernel.replace("_sym", "")
        assert idx.last_scan()["kernel"] == kernel or (idx.last_seed()["stat_redo"] > before and idx.last_scan()["kernel"] == plain), idx.last_scan()
        _assert_same(D, I, Do, Io, kernel)
    idx.set_tuning(0, 0, 0)
    D, I = idx.search_self(k, n - 300, 300)   # a window of own rows that ends at the last (poisoned) row
    _assert_same(D, I, Do[n - 300:], Io[n - 300:], "window")


# ---- the shard key exchange: search_keys on two halves, merge_keys_dev over the two lists -----------------------------------------
@pytest.mark.parametrize("metric", [IP, L2])
def test_search_keys_and_merge(gpu_faiss, oracle, metric):
    import torch
    import merge_reference as mr
    from knn_for_homology_amd.sharded import HipShardBackend
    nb, nq, d, k, cut = 5000, 41, 64, 2048, 2051
    xb, xq, table = _problem(77 + metric, nb, nq, d)
    Do, Io = oracle.flat_search(xb, xq, k, metric)
    q = torch.from_numpy(xq).cuda()
    lists = []
    for lo, hi in ((0, cut), (cut, nb)):
        b = HipShardBackend(d, metric)
        b.add(xb[lo:hi])
        keys = b.search_keys(q, k, lo).cpu().numpy().view(np.uint64)
        Ds, Is = oracle.flat_search(xb[lo:hi], xq, k, metric)
        assert ((Is >= 0).sum(1) < k).any(), "a starved shard list"
        want = mr.pack_keys(Ds, Is, metric, lo)
        assert np.array_equal(keys, want), f"{int((keys != want).sum())} keys differ; every key of a dropped pair is KEY_PAD"
        Dd, Id = b.search(q, k)
        _assert_same(Dd.cpu().numpy(), Id.cpu().numpy(), Ds, Is, "search_dev")
        lists.append(keys)
    gathered = torch.from_numpy(np.stack(lists).view(np.int64)).cuda()
    Dm, Im = b.merge(gathered, 2, nq, k)
    _not_vacuous(oracle, table, Do, Io, metric, l2_mode=1)
    _assert_same(Dm.cpu().numpy(), Im.cpu().numpy(), Do, Io, "merge")


# ---- range_search: three builds and range_search_self; radii -inf, a finite median, +inf, NaN ----------------------------------
@pytest.mark.parametrize("metric", [IP, L2])
@pytest.mark.parametrize("nb,d,nq,kernel", [(37, 8, 7, None), (1000, 100, 20, "range_scan_q32_d256"), (4097, 100, 129, "range_scan_q128_d128")])
def test_range_search(gpu_faiss, oracle, nb, d, nq, kernel, metric):
    kw = dict(near=1, query_kinds=("nan", "pinf", "twin", "huge")) if nq < 8 else {}
    xb, xq, table = _problem(nb + nq + metric, nb, nq, d, **kw)
    if kernel is None:
        kernel = "range_scan_q32_d256_diff" if metric == L2 else "range_scan_q32_d256"
    idx = gpu_faiss.IndexFlat(d, metric)
    idx.add(xb)
    Do, Io = oracle.flat_search(xb, xq, nb, metric)
    _not_vacuous(oracle, table, Do, Io, metric, l2_mode=1 if nq >= 20 else 2)
    med = np.float32(np.median(Do[(Io >= 0) & np.isfinite(Do)]))
    for r in (-np.inf, med, np.inf, np.nan):
        got = idx.range_search(xq, r)
        assert idx.last_scan()["kernel"] == kernel and idx.last_range()["query_blocks"] == 1, idx.last_scan()
        want = expected_range(oracle, xb, xq, r, metric)
        for g, w, name in zip(got, want, ("lims", "D", "I")):
            assert np.array_equal(g.view(np.uint32) if name == "D" else g, w.view(np.uint32) if name == "D" else w), (name, r)
    # every admissible pair and nothing else at the all-keeping radius: a +inf inner-product score is kept, -inf and NaN are not
    allr = -np.inf if metric == IP else np.inf
    lims = idx.range_search(xq, allr)[0]
    assert np.array_equal(np.diff(lims.astype(np.int64)), (Io >= 0).sum(1))
    w0 = max(0, nb - 300)
    got = idx.range_search_self(med, w0, nb - w0)
    want = expected_range(oracle, xb, np.ascontiguousarray(xb[w0:]), med, metric)
    for g, w, name in zip(got, want, ("lims", "D", "I")):
        assert np.array_equal(g.view(np.uint32) if name == "D" else g, w.view(np.uint32) if name == "D" else w), ("self", name)


# ---- knn_gather_distances: candidates pointing at every row kind ---------------------------------------------------------------
def _same_or_both_nan(a, b):
    """equal NaN masks, equal bits elsewhere (a NaN's sign differs between host and device)"""
    na, nb_ = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb_) and np.array_equal(_bits(a)[~na], _bits(b)[~nb_])


@pytest.mark.parametrize("metric", [IP, L2])
def test_gather_distances(gpu_faiss, oracle, metric):
    from knn_for_homology_amd import _lib
    nb, nq, d = 700, 25, 37
    xb, xq, table = _problem(17 + metric, nb, nq, d)
    idx = gpu_faiss.IndexFlat(d, metric)
    idx.add(xb)
    poisoned = np.array(sorted(table.rows), np.int64)
    cand = np.concatenate([np.concatenate([poisoned, np.arange(q, q + 5)]) for q in range(nq)]).astype(np.int64)
    counts = np.full(nq, poisoned.size + 5)
    offs = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    out = np.zeros(offs[-1], np.float32)
    _lib.check(_lib.lib().knn_gather_distances(idx._h, xq.ctypes.data, nq, cand.ctypes.data, offs.ctypes.data, out.ctypes.data))
    want = oracle.pair_distances(xb, xq, np.repeat(np.arange(nq), counts).astype(np.int64), cand, metric)
    assert np.isnan(want).any() and np.isinf(want).any() and set(k.split(":")[-1] for k in table.rows.values()) == set(nc.ROW_KINDS)
    assert _same_or_both_nan(out, want)


# ---- normalize_L2 (host entry) and normalize_rows (the stored rows) ----------------------------------------------------------------
def test_normalize(gpu_faiss, oracle):
    nb, d = 700, 37
    xb, _, table = _problem(11, nb, 8, d)
    xb[9] = 0
    want = xb.copy()
    oracle.normalize_l2(want)
    assert (want[table.rows_of("huge")] == 0).all() and np.isnan(want[table.rows_of("pinf")]).any() and (want[9] == 0).all()
    a = xb.copy()
    gpu_faiss.normalize_L2(a)
    assert _same_or_both_nan(a, want)
    idx = gpu_faiss.IndexFlat(d, IP)
    idx.add(xb)
    idx.normalize_rows()
    assert _same_or_both_nan(idx.reconstruct_n(0, nb), want)


# ---- IndexRefineFlat / knn_flat_refine: labels naming poisoned rows (the guard of refine.inc) -----------------------------------------
def _ref_refine(oracle, xb, xq, labels, k, metric):
    """refine_reference.ref_refine without its refusal of unfilled slots: the labelled rows of a query, ascending, searched by
    the oracle in the difference form; a dropped pair leaves its slot to the pad"""
    D = np.full((xq.shape[0], k), -FLT_MAX if metric == IP else FLT_MAX, np.float32)
    I = np.full((xq.shape[0], k), -1, np.int64)
    for i in range(xq.shape[0]):
        cand = np.sort(labels[i][labels[i] >= 0])
        kk = min(k, cand.size)
        Dl, Il = oracle.flat_search(np.ascontiguousarray(xb[cand]), xq[i:i + 1], kk, metric, l2_mode=2)
        D[i, :kk] = Dl[0]
        I[i, :kk] = np.where(Il[0] >= 0, cand[np.maximum(Il[0], 0)], -1)
    return D, I


@pytest.mark.parametrize("metric", [IP, L2])
def test_refine_labels_naming_poisoned_rows(gpu_faiss, oracle, metric):
    from knn_for_homology_amd import _lib
    nb, nq, d, kb, k = 700, 25, 37, 40, 30
    xb, xq, table = _problem(23 + metric, nb, nq, d)
    poisoned = np.array(sorted(table.rows), np.int64)
    plain = np.setdiff1d(np.arange(nb), poisoned)
    rng = np.random.default_rng(5)
    # per query: every poisoned row, distinct ordinary rows, and a -1 (the base found fewer rows than asked for)
    labels = np.stack([np.concatenate([poisoned, rng.choice(plain, kb - 1 - poisoned.size, replace=False), [-1]]) for _ in range(nq)]).astype(np.int64)
    idx = gpu_faiss.IndexFlat(d, metric)
    idx.add(xb)
    D = np.empty((nq, k), np.float32)
    I = np.empty((nq, k), np.int64)
    _lib.check(_lib.lib().knn_flat_refine(idx._h, xq.ctypes.data, nq, labels.ctypes.data, kb, k, D.ctypes.data, I.ctypes.data))
    Do, Io = _ref_refine(oracle, xb, xq, labels, k, metric)
    assert ((Io >= 0).sum(1) < k).any() and (metric == L2 or np.isposinf(Do).any())
    _assert_same(D, I, Do, Io, "refine")


# ---- the 16-bit prefilter switched on: poisoned queries over finite rows, and over rows with one `huge` --------------------------
@pytest.mark.parametrize("with_huge", [False, True])
def test_scan16_with_poisoned_queries(gpu_faiss, oracle, with_huge):
    rng = np.random.default_rng(40 + with_huge)
    nb, nq, d, k = 20000, 12, 64, 10
    where = [(256, "huge")] if with_huge else []
    xb, xq, table = nc.poison(rng, nb, nq, d, where, near=0, query_kinds=("nan", "pinf", "huge", "twin"))
    idx = gpu_faiss.IndexFlat(d, IP)
    idx.set_scan16(1)
    idx.add(xb)
    Do, Io = oracle.flat_search(xb, xq, k, IP)
    assert ((Io >= 0).sum(1) < k).any() and np.isposinf(Do).any()
    for flags in (KNN_TUNE_SCAN16_ANY_NB, KNN_TUNE_NO_SCAN16):
        idx.set_tuning(0, 0, flags)
        D, I = idx.search(xq, k)
        assert idx.last_scan16()["used"] == (flags == KNN_TUNE_SCAN16_ANY_NB), idx.last_scan16()
        _assert_same(D, I, Do, Io, f"scan16 flags {flags}")
