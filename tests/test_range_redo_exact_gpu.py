"""GPU: the host side of IndexFlat.range_search / range_search_self (range_search_impl, csrc/range.inc) exactly: query blocks,
copy-out runs, staging capacity and the overflow rescan as a strict, scattered subset of a block.

Every case compares lims, I and the bits of D of ALL queries with an expectation worked out on the host, and last_range()
and the last launch of last_scan() with the prediction of the host model (tests/range_reference.py).  The integer cases are
rebuilt from the device's CU count through the model's generators, and the conditions that make them mean something (which
queries overflow where, exact capacity, runs, blocks) are asserted before the search, as tests/test_range_reference.py
asserts them for 256 CUs."""
import numpy as np
import pytest

import range_reference as rr
from flat_lifecycle_reference import expected_range

pytestmark = pytest.mark.gpu

IP, L2 = rr.IP, rr.L2
NARROW, WIDE, DIFF = "range_scan_q32_d256", "range_scan_q128_d128", "range_scan_q32_d256_diff"


@pytest.fixture(scope="module")
def cus(gpu_faiss):
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _assert_same(got, want, what=""):
    lims, D, I = got
    wl, wD, wI = want
    assert lims.dtype == np.uint64 and D.dtype == np.float32 and I.dtype == np.int64
    assert np.array_equal(lims, wl), f"{what}: lims differ first at query {np.flatnonzero(lims != wl)[:5] - 1}"
    bad = np.flatnonzero(I != wI)
    assert not len(bad), f"{what}: {len(bad)} ids differ, first at {bad[:3]} (query {np.searchsorted(wl, bad[:3], side='right') - 1}): {I[bad[:3]]} for {wI[bad[:3]]}"
    bad = np.flatnonzero(_bits(D) != _bits(wD))
    assert not len(bad), f"{what}: {len(bad)} scores differ, first at {bad[:3]} (query {np.searchsorted(wl, bad[:3], side='right') - 1}): {D[bad[:3]]} for {wD[bad[:3]]}"


def _assert_reports(idx, pred, what=""):
    assert idx.last_range() == pred["last_range"], what
    scan = idx.last_scan()
    assert {k: scan[k] for k in pred["last_scan"]} == pred["last_scan"], what


def _index(gpu_faiss, xb_i, metric):
    idx = gpu_faiss.IndexFlat(8, metric)
    idx.add(rr.f32(xb_i))
    return idx


def _search(idx, p, what):
    got = idx.range_search(rr.f32(p.xq_i), p.radius)
    _assert_same(got, p.want, what)
    _assert_reports(idx, p.pred, what)
    return got


def _scratch_reuse(idx, p, first, cus):
    """(f) a small search with another radius and another plan on the same handle, then the large one again"""
    m = min(p.nq, rr.QB)
    sel = np.array([0, 1, 2, m // 2, m - 1, p.nq - 1, 3])
    xs = p.xq_i[sel]
    r2 = np.float32(190.0) if p.metric == IP else np.float32(6.0)  # a part of the own family only
    want = rr.expected(p.xb_i, xs, r2, p.metric)
    large = np.diff(p.want[0].astype(np.int64))[sel]
    assert 0 < want[0][-1] < large.sum() and len(want[2]) and want[0][1] > 0  # it returns something, and something else
    pred = rr.predict(p.nb, p.metric, len(sel), cus, rr.counts_from_result(want[0], want[2]))
    assert pred["last_range"]["redos"] == 0 and pred["blocks"][0]["plan"] != p.pred["blocks"][0]["plan"]
    _assert_same(idx.range_search(rr.f32(xs), r2), want, p.name + " small")
    _assert_reports(idx, pred, p.name + " small")
    again = _search(idx, p, p.name + " again")
    for a, b in zip(first, again):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))


# ---- a. partial overflow, each kernel; f. scratch reuse and a view ----------------------------------------------------------
@pytest.mark.parametrize("name,nb,nq,metric", rr.CASES_A, ids=[c[0] for c in rr.CASES_A])
def test_partial_overflow(gpu_faiss, cus, name, nb, nq, metric):
    p = rr.banded(name, nb, nq, metric, cus)
    pred = rr.check_banded(p)
    assert 0 < pred["last_range"]["redo_queries"] < nq and pred["last_range"]["query_blocks"] == 1
    assert p.plan.kernel == {"wide": WIDE, "narrow": NARROW, "diff": DIFF}[name.split("-")[0]]
    idx = _index(gpu_faiss, p.xb_i, metric)
    first = _search(idx, p, name)
    _scratch_reuse(idx, p, first, cus)
    if name == "wide-ip":  # a view has its own scratch and reports: the same result, the same rescan
        view = idx.view()
        _search(view, p, name + " view")
        _search(idx, p, name + " parent after its view")


# ---- b. copy-out runs ----------------------------------------------------------------------------------------------------
def test_copy_out_runs(gpu_faiss, cus):
    p = rr.two_runs(*rr.CASE_B, cus)
    pred = rr.check_two_runs(p)
    assert len(pred["blocks"][0]["runs"]) == 2 and 0 < pred["last_range"]["redo_queries"] < p.nq
    idx = _index(gpu_faiss, p.xb_i, p.metric)
    _search(idx, p, p.name)


# ---- c. more than one query block, uploaded queries; f. scratch reuse -------------------------------------------------------
@pytest.mark.parametrize("name,nb,metric", rr.CASES_C, ids=[c[0] for c in rr.CASES_C])
def test_two_query_blocks(gpu_faiss, cus, name, nb, metric):
    p = rr.two_blocks(name, nb, metric, cus)
    pred = rr.check_two_blocks(p)
    assert pred["last_range"]["query_blocks"] == 2 and 0 < pred["last_range"]["redo_queries"] < p.nq
    idx = _index(gpu_faiss, p.xb_i, metric)
    first = _search(idx, p, name)
    assert first[0][rr.QB] > 0 and first[0][-1] > first[0][rr.QB]
    _scratch_reuse(idx, p, first, cus)


# ---- d. the small-batch L2 rule is the whole batch's, in every block ---------------------------------------------------------
def test_l2_rule_across_blocks(gpu_faiss, oracle, cus):
    rng = np.random.default_rng(3)
    # rows far from the origin and close to each other: the norm formula cancels, the difference form does not
    xb = (100.0 + rng.standard_normal((300, 48))).astype(np.float32)
    xq = (100.0 + rng.standard_normal((rr.QB + 5, 48))).astype(np.float32)
    Dd, _ = oracle.flat_search(xb, xq[:19], 300, L2, l2_mode=2)
    r = np.float32(np.median(Dd))
    idx = gpu_faiss.IndexFlat(48, L2)
    idx.add(xb)
    want = expected_range(oracle, xb, xq, r, L2)  # (the oracle applies the rule to the whole batch: the norm formula)
    got = idx.range_search(xq, r)
    _assert_same(got, want, "16384 + 5 queries")
    pred = rr.predict(300, L2, rr.QB + 5, cus, rr.counts_from_result(want[0], want[2]))
    assert pred["last_range"]["query_blocks"] == 2 and pred["last_scan"]["kernel"] == NARROW
    _assert_reports(idx, pred)
    # the last five queries, a block of their own: the norm formula's bits, which the difference form does not give
    lims, D, I = got
    lo, hi = int(lims[rr.QB]), int(lims[-1])
    assert hi - lo > 100
    qidx = np.repeat(np.arange(5), np.diff(lims[rr.QB:].astype(np.int64)))
    tail = np.ascontiguousarray(xq[rr.QB:])
    norm = oracle.pair_distances(xb, tail, qidx, I[lo:hi], L2, l2_mode=1)
    diff = oracle.pair_distances(xb, tail, qidx, I[lo:hi], L2, l2_mode=2)
    assert np.array_equal(_bits(D[lo:hi]), _bits(norm))
    assert int((_bits(diff) != _bits(D[lo:hi])).sum()) > 0
    # the mirror image: 5 + 14 queries in one call, no batch announced, stay on the difference build
    idx.set_batch(0)
    q19 = np.ascontiguousarray(np.concatenate([xq[rr.QB:], xq[:14]]))
    want19 = expected_range(oracle, xb, q19, r, L2)
    got19 = idx.range_search(q19, r)
    assert idx.last_scan()["kernel"] == DIFF and idx.last_range() == {"query_blocks": 1, "redos": 0, "redo_queries": 0}
    _assert_same(got19, want19, "5 + 14 queries")
    q19idx = np.repeat(np.arange(19), np.diff(want19[0].astype(np.int64)))
    assert np.array_equal(_bits(got19[1]), _bits(oracle.pair_distances(xb, q19, q19idx, want19[2], L2, l2_mode=2)))
    assert int((_bits(got19[1]) != _bits(oracle.pair_distances(xb, q19, q19idx, want19[2], L2, l2_mode=1))).sum()) > 0


# ---- e. range_search_self over more than one block ---------------------------------------------------------------------------
def _window(want, q0, n):
    """the results of queries [q0, q0 + n) of a result"""
    lims, D, I = want
    lo, hi = int(lims[q0]), int(lims[q0 + n])
    return lims[q0:q0 + n + 1] - lims[q0], D[lo:hi], I[lo:hi]


@pytest.mark.parametrize("metric", [IP, L2])
def test_self_search_two_blocks(gpu_faiss, cus, metric):
    x = rr.self_rows(rr.SELF_ROWS)
    n = len(x)
    r = rr.RADIUS[metric]
    whole = rr.expected(x, x, r, metric)
    per = np.diff(whole[0].astype(np.int64))
    assert per[:rr.QB].min() > 0 and per[rr.QB:].min() > 0 and whole[0][-1] < 2_000_000
    idx = _index(gpu_faiss, x, metric)
    for row0, nrows in ((0, n), (11, rr.QB + 5)):
        want = _window(whole, row0, nrows)  # (the queries are rows row0 .. of the same search)
        pred = rr.predict(n, metric, nrows, cus, rr.counts_from_result(want[0], want[2]))
        assert pred["last_range"]["query_blocks"] == 2
        got = idx.range_search_self(r, row0, nrows)
        _assert_same(got, want, f"self {row0} + {nrows}")
        _assert_reports(idx, pred, f"self {row0} + {nrows}")
        assert got[0][rr.QB] > 0 and got[0][-1] > got[0][rr.QB]
    up = idx.range_search(idx.reconstruct_n(11, rr.QB + 5), r)
    _assert_same(up, want, "uploaded rows 11 + 16389")
    _assert_reports(idx, pred, "uploaded rows 11 + 16389")
