"""GPU: knn_eval_bucket_counts and knn_eval_hit_curve (csrc/buckets.inc) bit for bit against tests/buckets_reference.py,
through evaluation.py and, for the optional outputs and the argument checks, through the C entries.

bucket_hist_kernel gives a wave to a row: two binary searches over the edges in LDS per cell, packed 64-bit LDS atomics
(KNN355_BUCKET_AGG=1: equal (a, h) pairs merged inside the wave first; both ways are run here), global integer
counters carried across slabs.  hit_terms_kernel takes the row prefix counts by ballot over groups of 64 columns;
hit_fold_kernel adds tiles of 128 rows x 32 columns in row order, the running sums carried across slabs.  The shapes sit
where that can go wrong: cells around a wave, rows around a slab and a tile, columns around a fold workgroup, bucket counts
around the workgroup and at the LDS maximum.  Integers are compared with array_equal, doubles as uint64 patterns."""
from pathlib import Path

import numpy as np
import pytest

import buckets_reference as ref

pytestmark = pytest.mark.gpu

SLAB = "KNN355_EVAL_SLAB_ROWS"
AGG = "KNN355_BUCKET_AGG"
KNN_ERR_INVALID = -1
S64, SD = -7777, -7777.25  # what the output arrays hold before a call
GOLDEN = Path(__file__).resolve().parent / "golden" / "reference_buckets.npz"
CASES = ["cosine", "tied", "gaps", "edges64", "one"]


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as g:
        return {key: g[key] for key in g.files}


@pytest.fixture(params=["merged", "plain"])
def agg(request, monkeypatch):
    if request.param == "merged":
        monkeypatch.setenv(AGG, "1")
    else:
        monkeypatch.delenv(AGG, raising=False)
    return request.param


def case(golden, name):
    return {key[len(name) + 1:]: value for key, value in golden.items() if key.startswith(name + "_")}


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _ptr(a):
    return None if a is None else a.ctypes.data


def c_counts(scores_, correct_, limit, lo_, hi_, **over):
    """the C entry -> (return code, count, correct), the outputs pre-filled with the sentinel; `over` replaces arguments
    by name (nq, k, nb, key_type) or drops a pointer (scores=None ...)"""
    from knn_for_homology_amd import _lib
    scores = np.ascontiguousarray(scores_)
    correct = np.ascontiguousarray(correct_).view(np.uint8)
    lo, hi = np.ascontiguousarray(lo_, np.float64), np.ascontiguousarray(hi_, np.float64)
    nq, k = scores.shape
    n = max(len(lo), 1)
    a = dict(scores=scores, key_type=1 if scores.dtype == np.float64 else 0, correct=correct, nq=nq, k=k, lo=lo, hi=hi, nb=len(lo),
             count=np.full(n, S64, np.int64), right=np.full(n, S64, np.int64))
    outs = a["count"], a["right"]
    a.update(over)
    rc = _lib.lib().knn_eval_bucket_counts(_ptr(a["scores"]), a["key_type"], _ptr(a["correct"]), a["nq"], a["k"], limit, _ptr(a["lo"]), _ptr(a["hi"]),
                                           a["nb"], _ptr(a["count"]), _ptr(a["right"]))
    return (rc, *outs)


def c_curve(correct_, limit, totals_, rows=True, cols=True, **over):
    """the C entry -> (return code, mean, row_correct, column_correct), pre-filled with the sentinels"""
    from knn_for_homology_amd import _lib
    correct = np.ascontiguousarray(correct_).view(np.uint8)
    totals = np.ascontiguousarray(totals_, np.int64)
    nq, k = correct.shape
    a = dict(correct=correct, nq=nq, k=k, totals=totals, mean=np.full(max(limit, 1), SD), rows=np.full(nq, S64, np.int64) if rows else None,
             cols=np.full(max(limit, 1), S64, np.int64) if cols else None)
    outs = a["mean"], a["rows"], a["cols"]
    a.update(over)
    rc = _lib.lib().knn_eval_hit_curve(_ptr(a["correct"]), a["nq"], a["k"], limit, _ptr(a["totals"]), _ptr(a["mean"]), _ptr(a["rows"]), _ptr(a["cols"]))
    return (rc, *outs)


def check_counts(correct, scores, limit, lo, hi):
    """evaluation.bucketed_accuracy against the restatement: counts, precision and sem bits, the reference's two arrays"""
    from knn_for_homology_amd import evaluation
    got = evaluation.bucketed_accuracy(correct, scores, limit=limit, lo=lo, hi=hi)
    count, right = ref.bucket_counts(np.asarray(correct), scores, limit, lo, hi)
    assert np.array_equal(got.count, count)
    assert np.array_equal(got.correct, right)
    precision, sem = ref.precision_sem(count, right)
    assert np.array_equal(bits(got.precision), bits(precision))
    assert np.array_equal(bits(got.sem), bits(sem))
    p, s = got.reference_arrays()
    assert np.array_equal(bits(p), bits(precision[count > 0])) and np.array_equal(bits(s), bits(sem[count > 0]))
    return got


def check_curve(correct, totals, limit):
    """the C entry with every output, then the three evaluation.py functions, against the restatement"""
    from knn_for_homology_amd import evaluation
    mean, rows, cols = ref.hit_curve(np.asarray(correct), totals, limit)
    rc, got_mean, got_rows, got_cols = c_curve(correct, limit, totals)
    assert rc == 0
    assert np.array_equal(bits(got_mean), bits(mean))
    assert np.array_equal(got_rows, rows) and np.array_equal(got_cols, cols)
    rc, only_mean, _, _ = c_curve(correct, limit, totals, rows=False, cols=False)
    assert rc == 0 and np.array_equal(bits(only_mean), bits(mean))
    curve, counted = evaluation.accuracy_over_hits(correct, totals, limit=limit, want_rows=True)
    assert np.array_equal(bits(curve), bits(mean)) and np.array_equal(counted, rows)
    assert np.array_equal(bits(evaluation.recall_per_query(correct, totals, limit=limit)), bits(rows / np.asarray(totals)))
    return mean


# ---- the fixture -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("name", CASES)
def test_fixture_bucket_counts(golden, agg, name, dtype):
    c = case(golden, name)
    if dtype == np.float32 and c["scores"].dtype != np.float32:
        scores = c["scores"].astype(np.float32)  # (the float64 case rounded: other cells, the same contract)
    else:
        scores = c["scores"].astype(dtype)
    from knn_for_homology_amd import evaluation
    limit, smoothness = int(c["limit"]), int(c["smoothness"])
    got = evaluation.bucketed_accuracy(c["correct"], scores, limit=limit, smoothness=smoothness)
    lo, hi = ref.default_edges(smoothness)
    assert np.array_equal(bits(got.lo), bits(lo)) and np.array_equal(bits(got.hi), bits(hi))
    count, right = ref.bucket_counts(c["correct"], scores, limit, lo, hi)
    assert np.array_equal(got.count, count) and np.array_equal(got.correct, right)
    if scores.astype(np.float64).tobytes() == c["scores"].astype(np.float64).tobytes():
        # the reference's own arrays: precision bit for bit; sem is the closed form (tests/test_buckets_reference.py)
        p, s = got.reference_arrays()
        assert np.array_equal(bits(p), bits(c["precision"])) and len(s) == len(c["sem"])


@pytest.mark.parametrize("name", CASES)
def test_fixture_hit_curve(golden, name):
    c = case(golden, name)
    limit = int(c["limit"])
    mean = check_curve(c["correct"], c["totals"], limit)
    if limit >= 2:
        assert np.array_equal(bits(mean), bits(c["accuracy_over_hit"]))
    from knn_for_homology_amd import evaluation
    k = c["correct"].shape[1]
    assert np.array_equal(bits(evaluation.recall_per_query(c["correct"], c["totals"], limit=k)), bits(c["recall_per_query"]))


# ---- edges -------------------------------------------------------------------------------------------------------------
def edge_scores(dtype):
    base = np.array([0, 0.25, 0.5, 0.75, 1.0], np.float32)
    odd = np.array([-0.0, np.inf, -np.inf, np.nan], np.float32)
    values = np.concatenate([base, np.nextafter(base, np.float32(2)), np.nextafter(base, np.float32(-2)), odd])
    rng = np.random.default_rng(5)
    scores = rng.choice(values, (9, 70)).astype(dtype)
    scores[0, :len(values)] = values
    return scores, rng.random(scores.shape) < 0.5


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("smoothness", [300, 7])
def test_scores_on_and_beside_the_default_edges(agg, smoothness, dtype):
    scores, correct = edge_scores(dtype)
    lo, hi = ref.default_edges(smoothness)
    check_counts(correct, scores, 70, lo, hi)
    if dtype == np.float64:
        # and on the double edges themselves, where neighbouring buckets overlap or leave a gap
        pool = np.concatenate([lo, hi, np.nextafter(lo, 2), np.nextafter(hi, -1)])
        on = np.random.default_rng(6).choice(pool, (7, 130))
        check_counts(on > 0.4, on, 129, lo, hi)


def test_user_edges_equal_lower_edges_and_empty_buckets(agg):
    scores, correct = edge_scores(np.float32)
    # every lower edge the same: a cell is in every bucket whose upper edge it does not pass
    check_counts(correct, scores, 70, np.full(6, 0.25), np.array([0.25, 0.5, 0.5, 0.75, 1.0, np.inf]))
    # lo[b] == hi[b]: empty buckets between filled ones; infinite edges
    got = check_counts(correct, scores, 70, np.array([-np.inf, 0.0, 0.5, 0.5, 0.75]), np.array([0.0, 0.0, 0.5, 0.75, np.inf]))
    assert got.count[1] == 0 and got.count[2] == 0 and np.isnan(got.precision[1]) and got.count[0] > 0


@pytest.mark.parametrize("nb", [1, 255, 256, 257, 4096])
def test_bucket_counts_around_the_workgroup(agg, nb):
    rng = np.random.default_rng(nb)
    hi = np.sort(rng.random(nb))
    lo = np.minimum(np.sort(rng.random(nb)) * 0.9, hi)
    scores = rng.random((21, 100)).astype(np.float32)
    scores[:, ::5] = hi[rng.integers(0, nb, (21, 20))].astype(np.float32)
    check_counts(rng.random(scores.shape) < 0.3, scores, 97, lo, hi)


# ---- shapes ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def wide():
    """513 x 300, clustered scores; the unread columns of the limited views get nonsense in the tests"""
    rng = np.random.default_rng(11)
    scores = np.clip(rng.normal(0.6, 0.05, (513, 300)), 0, 1).astype(np.float32)
    correct = rng.random(scores.shape) < scores
    correct[7] = False
    correct[8] = True
    totals = np.maximum(correct.sum(axis=1) + rng.integers(0, 50, 513), 1).astype(np.int64)
    totals[::5] = 1 << 40
    return scores, correct, totals


@pytest.mark.parametrize("limit", [1, 63, 64, 65, 257, 300])
def test_limits_across_slabs(wide, monkeypatch, limit):
    monkeypatch.setenv(SLAB, "256")
    scores, correct, totals = wide
    scores, correct = scores.copy(), correct.view(np.uint8).copy()
    scores[:, limit:] = np.nan  # what must not be read: NaN and 1.0 scores, non-zero bytes
    scores[::2, limit:] = 1.0
    correct[:, limit:] = 0xFF
    lo, hi = ref.default_edges(40)
    check_counts(correct, scores, limit, lo, hi)
    check_curve(correct, totals, limit)


@pytest.mark.parametrize("nq", [1, 257])
def test_rows_around_a_slab(wide, monkeypatch, nq):
    monkeypatch.setenv(SLAB, "256")
    scores, correct, totals = wide
    lo, hi = ref.default_edges(40)
    check_counts(correct[:nq], scores[:nq], 300, lo, hi)
    check_curve(correct[:nq], totals[:nq], 300)


def test_slabs_do_not_change_the_bits(wide, monkeypatch):
    from knn_for_homology_amd import evaluation
    scores, correct, totals = wide
    whole = evaluation.accuracy_over_hits(correct, totals, limit=300)
    counts = evaluation.bucketed_accuracy(correct, scores, limit=300, smoothness=40).count
    for rows in ("1", "100", "512"):
        monkeypatch.setenv(SLAB, rows)
        assert np.array_equal(bits(evaluation.accuracy_over_hits(correct, totals, limit=300)), bits(whole))
        assert np.array_equal(evaluation.bucketed_accuracy(correct, scores, limit=300, smoothness=40).count, counts)


# ---- contention --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", ["one bucket", "two buckets"])
def test_every_cell_in_one_or_two_buckets(agg, pattern):
    lo, hi = ref.default_edges(300)
    scores = np.full((2000, 300), np.float32(0.5017))
    if pattern == "two buckets":
        scores[:, 1::2] = np.float32(0.5042)
    correct = np.random.default_rng(3).random(scores.shape) < 0.25
    got = check_counts(correct, scores, 300, lo, hi)
    assert np.count_nonzero(got.count) == (1 if pattern == "one bucket" else 2) and got.count.sum() == 600000


# ---- hit curve ---------------------------------------------------------------------------------------------------------
def test_hit_curve_bytes_totals_and_rows():
    rng = np.random.default_rng(17)
    correct = (rng.random((300, 70)) < 0.3).astype(np.uint8)
    correct[correct != 0] = rng.choice(np.array([1, 2, 255], np.uint8), int(correct.sum()))  # any non-zero byte is correct
    correct[0] = 0      # an all-false row
    correct[1] = 255    # an all-true row
    correct[2] = 2
    totals = rng.integers(1, 100, 300).astype(np.int64)
    totals[::3] = 1
    totals[1::7] = 1 << 40  # int64 to double
    totals[2] = (1 << 40) + 1
    mean = check_curve(correct, totals, 70)
    assert mean[-1] > 1  # (totals of 1 under many correct hits)
    check_curve(correct, totals, 33)
    check_curve(correct[:5], np.ones(5, np.int64), 1)


# ---- invalid arguments ---------------------------------------------------------------------------------------------------
def test_bucket_counts_invalid_arguments():
    scores = np.random.default_rng(1).random((4, 6)).astype(np.float32)
    correct = scores > 0.5
    lo, hi = np.array([0.0, 0.5]), np.array([0.5, 1.0])
    nan = float("nan")
    bad = [
        dict(over=dict(nq=0)), dict(over=dict(k=0)), dict(over=dict(k=2 ** 31)), dict(limit=0), dict(limit=7),
        dict(over=dict(nb=0)), dict(over=dict(nb=4097)), dict(over=dict(key_type=2)), dict(over=dict(key_type=-1)),
        dict(over=dict(scores=None)), dict(over=dict(correct=None)), dict(over=dict(lo=None)), dict(over=dict(hi=None)),
        dict(over=dict(count=None)), dict(over=dict(right=None)),
        dict(lo=[nan, 0.5]), dict(hi=[0.5, nan]), dict(lo=[0.4, 0.0]), dict(hi=[1.0, 0.5], lo=[0.0, 0.0]), dict(lo=[0.0, 0.75], hi=[0.5, 0.6]),
    ]
    for b in bad:
        rc, count, right = c_counts(scores, correct, b.get("limit", 6), b.get("lo", lo), b.get("hi", hi), **b.get("over", {}))
        assert rc == KNN_ERR_INVALID, b
        assert (count == S64).all() and (right == S64).all(), b
    rc, count, right = c_counts(scores, correct, 6, lo, hi)
    assert rc == 0 and count.sum() == 24


def test_hit_curve_invalid_arguments():
    correct = np.random.default_rng(2).random((4, 6)) < 0.5
    totals = np.array([1, 2, 3, 4], np.int64)
    bad = [
        dict(over=dict(nq=0)), dict(over=dict(k=0)), dict(over=dict(k=2 ** 31)), dict(limit=0), dict(limit=7),
        dict(over=dict(correct=None)), dict(over=dict(totals=None)), dict(over=dict(mean=None)),
        dict(totals=[1, 0, 3, 4]), dict(totals=[1, 2, 3, -4]),
    ]
    for b in bad:
        rc, mean, rows, cols = c_curve(correct, b.get("limit", 6), b.get("totals", totals), **b.get("over", {}))
        assert rc == KNN_ERR_INVALID, b
        assert (mean == SD).all() and (rows == S64).all() and (cols == S64).all(), b
    from knn_for_homology_amd import evaluation
    with pytest.raises(ValueError):
        evaluation.accuracy_over_hits(correct, [1, 0, 3, 4], limit=6)
    with pytest.raises(ValueError):
        evaluation.bucketed_accuracy(correct, correct.astype(np.float32), limit=6, lo=[0.5, 0.0], hi=[0.6, 0.7])


def test_last_buckets_ms():
    from knn_for_homology_amd import evaluation
    correct = np.random.default_rng(2).random((50, 20)) < 0.5
    evaluation.bucketed_accuracy(correct, correct.astype(np.float32) * 0.5, limit=20, smoothness=10)
    evaluation.accuracy_over_hits(correct, np.full(50, 20), limit=20)
    ms = evaluation.last_buckets_ms()
    for call in ("bucket_counts", "hit_curve"):
        assert set(ms[call]) == {"upload_ms", "kernel_ms", "download_ms"} and all(v > 0 for v in ms[call].values())
