"""GPU: knn_eval_pr_curve (csrc/pr_curve.inc) and knn_eval_sets_matrix (csrc/eval.inc) bit for bit against
tests/pr_curve_reference.py.

pr_curve_kernel gives a workgroup of 256 threads to a block of 256 queries: per query the threads stride over `limit`
cells, a binary search over the thresholds in LDS puts each cell into a bin, a suffix scan runs over the bins 256 at a
time (a shuffle scan per wave, the four wave totals through LDS, a carry between passes), and thread t accumulates the
terms of thresholds t, t + 256, ...; pr_fold_kernel adds the block sums in block order.  The shapes here sit where that
can go wrong: row counts around a block, cell counts around a wave and the workgroup, threshold counts around a wave, one
per thread and several per thread, slabs.  Doubles are compared as uint64 patterns, integers with array_equal; there is no
tolerance anywhere except against the reference's own numpy.mean (the bound of tests/test_pr_curve_reference.py)."""
from pathlib import Path

import numpy as np
import pytest

import pr_curve_reference as ref

pytestmark = pytest.mark.gpu

KNOB = "KNN355_EVAL_SLAB_ROWS"
KNN_ERR_INVALID = -1
S64, S32, S8, SD = -7777, -7777, 0xAB, -7777.25  # what the output arrays hold before a call
FMAX = float(np.finfo(np.float32).max)
ODD_SCORES = np.array([np.nan, np.inf, -np.inf, FMAX, -FMAX, 0.0, -0.0, 1e-45], np.float32)
GOLDEN = Path(__file__).resolve().parent / "golden" / "reference_pr_curve.npz"
CASES = ["small", "wide", "tied", "evalues"]


def _ptr(a):
    return None if a is None else a.ctypes.data


def _last_error():
    from knn_for_homology_amd import _lib
    return _lib.lib().knn_last_error().decode()


def c_pr(correct_, scores_, limit, totals_, thr_, counts=True, **over):
    """the C entry point -> (return code, precision, recall, selected, tp, empty), the outputs pre-filled with the
    sentinels; `over` replaces arguments by name (nq, k, nthr) or drops a pointer (scores=None ...)"""
    from knn_for_homology_amd import _lib
    correct = np.ascontiguousarray(correct_, np.uint8)
    scores = np.ascontiguousarray(scores_, np.float32)
    totals = np.ascontiguousarray(totals_, np.int64)
    thr = np.ascontiguousarray(thr_, np.float64)
    nq, k = scores.shape
    n = max(len(thr), 1)
    a = dict(correct=correct, scores=scores, nq=nq, k=k, totals=totals, thr=thr, nthr=len(thr), precision=np.full(n, SD), recall=np.full(n, SD),
             selected=np.full(n, S64, np.int64) if counts else None, tp=np.full(n, S64, np.int64) if counts else None,
             empty=np.full(n, S64, np.int64) if counts else None)
    outs = [a[name] for name in ("precision", "recall", "selected", "tp", "empty")]
    a.update(over)
    rc = _lib.lib().knn_eval_pr_curve(_ptr(a["correct"]), _ptr(a["scores"]), a["nq"], a["k"], limit, _ptr(a["totals"]), _ptr(a["thr"]),
                                      a["nthr"], _ptr(a["precision"]), _ptr(a["recall"]), _ptr(a["selected"]), _ptr(a["tp"]), _ptr(a["empty"]))
    return (rc, *outs)


def c_matrix(hits_, offsets_, members_, **over):
    """-> (return code, is_correct), pre-filled with the sentinel"""
    from knn_for_homology_amd import _lib
    hits = np.ascontiguousarray(hits_, np.int64)
    offsets = np.ascontiguousarray(offsets_, np.int64)
    members = None if members_ is None else np.ascontiguousarray(members_, np.int64)
    nq, k = hits.shape
    a = dict(hits=hits, nq=nq, k=k, offsets=offsets, members=members if members is not None and members.size else None,
             out=np.full((max(nq, 1), k), S8, np.uint8))
    out = a["out"]
    a.update(over)
    rc = _lib.lib().knn_eval_sets_matrix(_ptr(a["hits"]), a["nq"], a["k"], _ptr(a["offsets"]), _ptr(a["members"]), _ptr(a["out"]))
    return rc, out[:nq]


def c_sets(hits_, offsets_, members_):
    from knn_for_homology_amd import _lib
    hits = np.ascontiguousarray(hits_, np.int64)
    offsets = np.ascontiguousarray(offsets_, np.int64)
    members = np.ascontiguousarray(members_, np.int64)
    nq, k = hits.shape
    lead, tp = np.full(nq, S32, np.int32), np.full(nq, S32, np.int32)
    rc = _lib.lib().knn_eval_sets(_ptr(hits), nq, k, _ptr(offsets), _ptr(members) if members.size else None, _ptr(lead), _ptr(tp))
    return rc, lead, tp


def _same(got, want):
    rc, precision, recall, selected, tp, empty = got
    assert rc == 0, _last_error()
    assert np.array_equal(precision.view(np.uint64), want[0].view(np.uint64)), "precision_out (as bits)"
    assert np.array_equal(recall.view(np.uint64), want[1].view(np.uint64)), "recall_out (as bits)"
    if selected is not None:
        assert np.array_equal(selected, want[2]), "selected_out"
        assert np.array_equal(tp, want[3]), "tp_out"
        assert np.array_equal(empty, want[4]), "empty_out"


def _check(correct, scores, limit, totals, thr):
    want = ref.pr_curve(correct, scores, limit, totals, thr)
    _same(c_pr(correct, scores, limit, totals, thr), want)
    return want


def _pr_case(rng, nq, k, limit, nthr, values=None):
    """thresholds: nthr draws from about nthr / 2 float32 values, sorted (runs of equal values), as doubles; scores: those
    values themselves, one float32 ulp above and one below (strictness on both sides of every threshold), or `values`;
    a fifth of the rows below every threshold, a fifth above every one; the columns from `limit` on hold correct cells
    with huge scores (reading them shows); totals from 1 to 2**40"""
    grid = np.unique(rng.normal(0, 1, max(2, (nthr + 1) // 2)).astype(np.float32))
    thr = np.sort(rng.choice(grid, nthr)).astype(np.float64)
    if values is None:
        values = np.concatenate([grid, np.nextafter(grid, np.float32(np.inf)), np.nextafter(grid, np.float32(-np.inf))])
    scores = rng.choice(values, (nq, k)).astype(np.float32)
    kind = rng.integers(0, 5, nq)
    scores[kind == 0] = np.nextafter(grid[0], np.float32(-np.inf))
    scores[kind == 1] = np.nextafter(grid[-1], np.float32(np.inf))
    correct = (rng.random((nq, k)) < 0.4).astype(np.uint8) * rng.choice(np.array([1, 2, 255], np.uint8), (nq, k))
    scores[:, limit:] = 3e38
    correct[:, limit:] = 1
    totals = rng.choice(np.array([1, 2, 5, 300, 2**40], np.int64), nq)
    return correct, scores, limit, totals, thr


# ---- rows around a block, cells around a wave and the workgroup, thresholds around a wave and one per thread ---------
@pytest.mark.parametrize("nq", [1, 255, 256, 257, 513])
def test_row_counts(gpu_faiss, nq):
    rng = np.random.default_rng(nq)
    want = _check(*_pr_case(rng, nq, 8, 5, 7))
    assert nq < 255 or (0 < want[4][0] < nq and want[2][0] > 0)


@pytest.mark.parametrize("extra", [0, 3])
@pytest.mark.parametrize("limit", [1, 63, 64, 65, 256, 257, 300])
def test_cell_counts(gpu_faiss, limit, extra):
    rng = np.random.default_rng(10 * limit + extra)
    _check(*_pr_case(rng, 5, limit + extra, limit, 9))


@pytest.mark.parametrize("nthr", [1, 2, 63, 64, 65, 255, 256, 257, 301, 4096])
def test_threshold_counts(gpu_faiss, nthr):
    rng = np.random.default_rng(nthr)
    case = _pr_case(rng, 3, 73, 70, nthr)
    assert nthr < 3 or (np.diff(case[4]) == 0).any()
    _check(*case)


def test_rows_cells_and_thresholds_past_one_pass_together(gpu_faiss):
    rng = np.random.default_rng(77)
    _check(*_pr_case(rng, 257, 68, 65, 65))
    _check(*_pr_case(rng, 20, 300, 300, 301))


# ---- scores and thresholds ------------------------------------------------------------------------------------------------
def test_scores_equal_to_thresholds_are_not_selected(gpu_faiss):
    """one row per threshold value t (a float32's double image): the float below t, t itself, the float above"""
    t32 = np.array([-3.5, -1e-30, 0.1, 1.0, 16777216.0, 3e38], np.float32)
    thr = t32.astype(np.float64)
    scores = np.stack([np.nextafter(t32, np.float32(-np.inf)), t32, np.nextafter(t32, np.float32(np.inf))], axis=1)
    correct = np.ones_like(scores, dtype=np.uint8)
    want = _check(correct, scores, 3, np.full(len(t32), 3), thr)
    # at threshold j: every cell of the rows above j, one cell of row j, nothing of the rows below
    assert want[2].tolist() == [3 * (len(t32) - 1 - j) + 1 for j in range(len(t32))]
    # a threshold between two floats: the double 0.1 lies below the float32 0.1
    want = _check([[1]], np.array([[0.1]], np.float32), 1, [1], [0.1, float(np.float32(0.1))])
    assert want[2].tolist() == [1, 0]


def test_odd_scores_and_infinite_thresholds(gpu_faiss):
    rng = np.random.default_rng(5)
    correct, scores, limit, totals, _ = _pr_case(rng, 40, 70, 66, 4, values=ODD_SCORES)
    assert np.isnan(scores[:, :limit]).sum() > 100
    thr = [-np.inf, -np.inf, -FMAX, -1.0, -0.0, 0.0, 0.0, 1e-45, 1.0, FMAX, np.inf, np.inf]
    want = _check(correct, scores, limit, totals, thr)
    assert want[2][-1] == 0 and want[2][0] == int((scores[:, :limit] > -np.inf).sum()) and want[2][4] == want[2][5]


def test_nothing_selected_and_everything_selected(gpu_faiss):
    """row 0: below every threshold (P = 1 at every one, counted in empty_out); row 1: NaN everywhere (the same); row 2: above
    every threshold; row 3: mixed"""
    thr = np.array([0.25, 0.5, 0.5, 0.75])
    scores = np.array([[0.25] * 6, [np.nan] * 6, [0.875] * 6, [0.25, 0.5, 0.625, 0.75, 0.875, 0.125]], np.float32)
    correct = np.array([[1] * 6, [1] * 6, [1, 0, 0, 1, 0, 0], [0, 1, 1, 0, 0, 1]], np.uint8)
    want = _check(correct, scores, 6, [1, 2**40, 2, 3], thr)
    assert want[4].tolist() == [2, 2, 2, 2] and want[2].tolist() == [10, 9, 9, 7] and want[3].tolist() == [4, 3, 3, 2]
    assert want[0].tolist() == [(1 + 1 + 2 / 6 + 2 / 4) / 4, (1 + 1 + 2 / 6 + 1 / 3) / 4, (1 + 1 + 2 / 6 + 1 / 3) / 4, (1 + 1 + 2 / 6 + 0) / 4]


def test_totals_of_one_and_of_two_to_the_forty(gpu_faiss):
    rng = np.random.default_rng(6)
    correct, scores, limit, _, thr = _pr_case(rng, 9, 40, 40, 12)
    for totals in (np.ones(9, np.int64), np.full(9, 2**40, np.int64), np.array([1, 2**40] * 4 + [1], np.int64)):
        want = _check(correct, scores, limit, totals, thr)
    assert want[1].max() > 1  # a total of 1 below the number of correct cells: recall above 1, as the division gives it


def test_block_sums_are_added_in_block_order(gpu_faiss):
    """the hand-worked three-block case of tests/test_pr_curve_reference.py: one running sum over all rows gives
    1 / 513, the contract's order (1 + 2**-51) / 513"""
    correct, scores, totals, _ = ref.three_block_case()
    rc, precision, recall, selected, tp, empty = c_pr(correct, scores, 1, totals, [0.0])
    assert rc == 0 and recall[0] == (1.0 + 2.0 ** -51) / 513.0 and precision[0] == 259.0 / 513.0
    assert (selected[0], tp[0], empty[0]) == (513, 259, 0)


def test_count_outputs_are_optional(gpu_faiss):
    rng = np.random.default_rng(8)
    case = _pr_case(rng, 30, 20, 17, 33)
    want = ref.pr_curve(*case)
    _same(c_pr(*case, counts=False), want)
    got = c_pr(*case, tp=None)  # (the array left out keeps its sentinels: it was never passed)
    _same(got[:3] + (None, None, None), want)
    assert np.array_equal(got[3], want[2]) and np.array_equal(got[5], want[4]) and (got[4] == S64).all()


# ---- slabs ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def slab_case():
    rng = np.random.default_rng(9)
    case = _pr_case(rng, 700, 10, 9, 70)
    return case, ref.pr_curve(*case)


@pytest.mark.parametrize("rows", [None, "1", "256", "300"])
def test_slabs_of_whole_blocks(gpu_faiss, slab_case, monkeypatch, rows):
    """700 rows: the knob is rounded up to a multiple of 256 (1 -> 256, 300 -> 512), so blocks never straddle slabs and the
    bits are those of one slab"""
    case, want = slab_case
    if rows is None:
        monkeypatch.delenv(KNOB, raising=False)
    else:
        monkeypatch.setenv(KNOB, rows)
    _same(c_pr(*case), want)


def test_count_outputs_are_optional_across_slabs(gpu_faiss, slab_case, monkeypatch):
    """700 rows in slabs of 256 (the smallest slab this entry cuts): selected_out / tp_out / empty_out present and absent"""
    case, want = slab_case
    monkeypatch.setenv(KNOB, "256")
    _same(c_pr(*case), want)
    _same(c_pr(*case, counts=False), want)


# ---- the Python facade -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as f:
        return {name: f[name] for name in f.files}


@pytest.mark.parametrize("name", CASES)
def test_facade_on_the_reference_cases(gpu_faiss, golden, name):
    """thresholds=None: the reference's quantiles exactly; its means within the bound of two summation orders
    (tests/test_pr_curve_reference.py); the restatement's bits"""
    from knn_for_homology_amd.evaluation import compute_correctness_array, precision_recall_curve
    g = {key[len(name) + 1:]: golden[key] for key in golden if key.startswith(name + "_")}
    nq = g["scores"].shape[0]
    limit, smoothness = int(g["limit"]), int(g["smoothness"])
    sets = [g["set_members"][g["set_offsets"][q]:g["set_offsets"][q + 1]].tolist()[::-1] for q in range(nq)]
    correct = compute_correctness_array(g["hits"], sets)
    assert correct.dtype == bool and np.array_equal(correct, g["correct"])
    recall, precision, thresholds, (selected, tp, empty) = precision_recall_curve(correct, g["scores"], g["totals"], limit, smoothness,
                                                                                 want_counts=True)
    assert np.array_equal(thresholds, g["thresholds"])
    bound = 2 * nq * 2.0 ** -53 * max(1.0, limit / int(g["totals"].min()))
    dp, dr = np.abs(precision - g["precision"]).max(), np.abs(recall - g["recall"]).max()
    print(f"{name}: |precision - reference| <= {dp:.3e}, |recall - reference| <= {dr:.3e}, bound {bound:.3e}")
    assert dp <= bound and dr <= bound
    want = ref.pr_curve(g["correct"], g["scores"], limit, g["totals"], g["thresholds"])
    _same((0, precision, recall, selected, tp, empty), want)
    assert len(precision_recall_curve(correct, g["scores"], g["totals"], limit, smoothness)) == 3


def test_facade_puts_shuffled_thresholds_back(gpu_faiss):
    from knn_for_homology_amd.evaluation import precision_recall_curve
    rng = np.random.default_rng(10)
    correct, scores, limit, totals, thr = _pr_case(rng, 50, 30, 25, 40)
    want = ref.pr_curve(correct, scores, limit, totals, thr)
    perm = rng.permutation(len(thr))
    recall, precision, thresholds, counts = precision_recall_curve(correct, scores, totals, limit, thresholds=thr[perm], want_counts=True)
    assert np.array_equal(thresholds, thr[perm])
    _same((0, precision, recall, *counts), tuple(w[perm] for w in want))
    # a bool matrix, a list of thresholds, a float64 score matrix that holds float32 values
    recall2, precision2, _ = precision_recall_curve(correct.astype(bool), scores.astype(np.float64), totals.tolist(), limit,
                                                    thresholds=thr[perm].tolist())
    assert np.array_equal(recall2, recall) and np.array_equal(precision2, precision)


def test_facade_refuses_before_the_library_is_called(gpu_faiss):
    from knn_for_homology_amd.evaluation import compute_correctness_array, precision_recall_curve
    correct = np.ones((4, 6), bool)
    scores = np.zeros((4, 6), np.float32)
    totals = np.ones(4, np.int64)
    with pytest.raises(ValueError, match="NaN"):
        precision_recall_curve(correct, scores, totals, 6, thresholds=[0.0, np.nan])
    for limit in (7, 0, -1):
        with pytest.raises(ValueError, match="limit"):
            precision_recall_curve(correct, scores, totals, limit, thresholds=[0.0])
    with pytest.raises(ValueError, match="limit"):
        precision_recall_curve(correct, scores, totals, thresholds=[0.0])  # the default limit of 300 is above k = 6
    for bad_scores in (scores[:, :5], scores[:3], scores.ravel()):
        with pytest.raises(ValueError, match="same shape"):
            precision_recall_curve(correct, bad_scores, totals, 6, thresholds=[0.0])
    for bad_totals in (totals[:3], np.ones((4, 1), np.int64)):
        with pytest.raises(ValueError, match="correct_totals"):
            precision_recall_curve(correct, scores, bad_totals, 6, thresholds=[0.0])
    for bad_totals in ([1, 1, 0, 1], [1, -2, 1, 1]):
        with pytest.raises(ValueError, match="positive"):
            precision_recall_curve(correct, scores, bad_totals, 6, thresholds=[0.0])
    for bad_thr in ([], np.zeros(4097), np.zeros((2, 2))):
        with pytest.raises(ValueError, match="thresholds"):
            precision_recall_curve(correct, scores, totals, 6, thresholds=bad_thr)
    with pytest.raises(ValueError, match="one query"):
        precision_recall_curve(correct[:0], scores[:0], totals[:0], 6, thresholds=[0.0])
    with pytest.raises(ValueError, match="homologous_rows"):
        compute_correctness_array(np.zeros((4, 6), np.int64), [[0]] * 3)
    recall, precision, _ = precision_recall_curve(correct, scores, totals, 6, thresholds=[-1.0, 0.0])
    assert recall.tolist() == [6.0, 0.0] and precision.tolist() == [1.0, 1.0]


# ---- knn_eval_sets_matrix ------------------------------------------------------------------------------------------------------
def _set_case(rng, nq, k, nb=3000):
    """the pattern of the set cases of tests/test_consumers_exact_gpu.py, restated: sets of 0, 1, 2, 5 and 40 sorted rows;
    half of each row's hits drawn from its set, a leading run of them, the rest from [-1, nb]"""
    offsets, members = [0], []
    hits = rng.integers(-1, nb + 1, (nq, k)).astype(np.int64)
    for r in range(nq):
        mine = np.sort(rng.choice(nb, rng.choice([0, 1, 2, 5, 40]), replace=False))
        members += mine.tolist()
        offsets.append(len(members))
        if mine.size:
            pick = rng.random(k) < 0.5
            pick[:rng.integers(0, k + 1)] = True
            pick[rng.integers(0, k)] = r % 2 == 0
            hits[r, pick] = rng.choice(mine, int(pick.sum()))
    return hits, np.asarray(offsets, np.int64), np.asarray(members, np.int64)


@pytest.mark.parametrize("name", CASES)
def test_sets_matrix_on_the_reference_cases(gpu_faiss, golden, name):
    rc, got = c_matrix(golden[f"{name}_hits"], golden[f"{name}_set_offsets"], golden[f"{name}_set_members"])
    assert rc == 0 and np.array_equal(got, golden[f"{name}_correct"].astype(np.uint8))


@pytest.mark.parametrize("k", [1, 64, 65, 300])
def test_sets_matrix_shapes(gpu_faiss, k):
    rng = np.random.default_rng(300 + k)
    for nq in (1, 3, 5, 70):
        hits, offsets, members = _set_case(rng, nq, k)
        want = ref.sets_matrix(hits, offsets, members)
        rc, got = c_matrix(hits, offsets, members)
        assert rc == 0 and np.array_equal(got, want)
        rc, lead, tp = c_sets(hits, offsets, members)
        assert rc == 0 and np.array_equal(got.sum(axis=1), tp)  # the row sums are knn_eval_sets' counts
        assert all(got[r, :lead[r]].all() and (lead[r] == k or not got[r, lead[r]]) for r in range(nq))


def test_sets_matrix_empty_sets_and_negative_hits(gpu_faiss):
    sets = [[], [10], [], [7, 8, 9], [0, 2**40], []]
    offsets = np.concatenate([[0], np.cumsum([len(s) for s in sets])])
    members = np.concatenate([np.asarray(s, np.int64) for s in sets])
    hits = np.array([[10, -1, 0, 7] * 17, [10, -1, 10, 7] * 17, [9, 8, 7, 10] * 17, [-1, 9, 6, 7] * 17, [2**40, 0, -1, 2**32] * 17,
                     [0, 2**40, -1, -2**63] * 17], np.int64)[:, :66]
    want = ref.sets_matrix(hits, offsets, members)
    assert want.sum(axis=1).tolist() == [0, 33, 0, 33, 34, 0]  # (66 columns: sixteen patterns of four and two cells more)
    rc, got = c_matrix(hits, offsets, members)
    assert rc == 0 and np.array_equal(got, want)
    # every set empty, set_members NULL
    rc, got = c_matrix(hits, np.zeros(len(sets) + 1, np.int64), None)
    assert rc == 0 and not got.any()
    # no rows: 0 whatever the pointers are
    assert c_matrix(hits[:0], [0], None, hits=None, offsets=None, out=None)[0] == 0


@pytest.mark.parametrize("rows", ["3", "1", "23"])
def test_sets_matrix_slabs(gpu_faiss, monkeypatch, rows):
    rng = np.random.default_rng(7)
    hits, offsets, members = _set_case(rng, 23, 65)
    want = ref.sets_matrix(hits, offsets, members)
    monkeypatch.setenv(KNOB, rows)
    rc, got = c_matrix(hits, offsets, members)
    assert rc == 0 and np.array_equal(got, want)


# ---- errors: refused on the host, nothing allocated or launched, the outputs as they were ------------------------------
def _refused(got, what):
    rc, precision, recall, selected, tp, empty = got
    assert rc == KNN_ERR_INVALID and what in _last_error(), _last_error()
    assert (precision == SD).all() and (recall == SD).all() and (selected == S64).all() and (tp == S64).all() and (empty == S64).all()


def test_pr_curve_refusals(gpu_faiss):
    correct = np.ones((5, 4), np.uint8)
    scores = np.zeros((5, 4), np.float32)
    totals = np.ones(5, np.int64)
    thr = [0.0, 0.5, 0.5]
    for nq in (0, -1):
        _refused(c_pr(correct, scores, 4, totals, thr, nq=nq), "nq >= 1")
    for k in (0, -3):
        _refused(c_pr(correct, scores, 4, totals, thr, k=k), "k >= 1")
    _refused(c_pr(correct, scores, 4, totals, thr, k=2**31), "k > INT32_MAX")
    for limit in (0, -1, 5):
        _refused(c_pr(correct, scores, limit, totals, thr), "limit")
    for nthr in (0, -1, 4097):
        _refused(c_pr(correct, scores, 4, totals, thr, nthr=nthr), "nthr")
    for name in ("correct", "scores", "totals", "thr", "precision", "recall"):
        _refused(c_pr(correct, scores, 4, totals, thr, **{name: None}), "null pointer")
    for bad in ([1, 1, 0, 1, 1], [1, 1, 1, 1, -5]):
        _refused(c_pr(correct, scores, 4, bad, thr), "total")
    _refused(c_pr(correct, scores, 4, totals, [0.0, 0.5, 0.25]), "thresholds decrease")
    _refused(c_pr(correct, scores, 4, totals, [np.inf, -np.inf]), "thresholds decrease")
    for bad in ([np.nan], [0.0, np.nan, 1.0], [0.0, 1.0, np.nan]):
        _refused(c_pr(correct, scores, 4, totals, bad), "NaN threshold")
    # and the same arguments pass once they are right
    rc, precision, recall, selected, tp, empty = c_pr(correct, scores, 4, totals, [-1.0, 0.0, 0.0])
    assert rc == 0 and precision.tolist() == [1.0, 1.0, 1.0] and recall.tolist() == [4.0, 0.0, 0.0]
    assert selected.tolist() == [20, 0, 0] and tp.tolist() == [20, 0, 0] and empty.tolist() == [0, 5, 5]


def test_sets_matrix_refusals(gpu_faiss):
    hits = np.full((3, 5), 10**6, np.int64)
    members = [1, 2, 3, 4]

    def refused(what, offs, mem, **over):
        rc, out = c_matrix(hits, offs, mem, **over)
        assert rc == KNN_ERR_INVALID and what in _last_error(), _last_error()
        assert (out == S8).all()

    refused("negative set offset", [-1, 2, 3, 4], members)
    refused("set offsets decrease", [0, 3, 2, 4], members)
    refused("set offsets decrease", [0, 2, 4, 3], members)
    refused("set members not sorted", [0, 2, 2, 4], [2, 1, 3, 4])
    refused("set members not sorted", [0, 0, 1, 4], [1, 2, 4, 3])
    refused("bad shape", [0, 2, 3, 4], members, k=0)
    refused("bad shape", [0, 2, 3, 4], members, nq=-1)
    refused("k > INT32_MAX", [0, 2, 3, 4], members, k=2**31)
    for name in ("hits", "offsets", "members", "out"):
        refused("null pointer", [0, 2, 3, 4], members, **{name: None})
    rc, out = c_matrix(hits, [0, 2, 3, 4], members)
    assert rc == 0 and not out.any()
    rc, out = c_matrix(np.array([[4, 4, 5, 9, 3]]), [0, 5], [4, 4, 4, 9, 9])  # repeated members are legal
    assert rc == 0 and out.tolist() == [[1, 1, 0, 1, 0]]
