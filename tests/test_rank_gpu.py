"""GPU: knn_eval_rank (csrc/rank.inc) and the three functions on top of it (evaluation.ranked_precision_recall,
ranked_cumulative, score_quantiles) bit for bit against tests/rank_reference.py and tests/golden/reference_rank.npz.

The sort is a radix sort with 8-bit digits over tiles of TILE = 2048 elements (RANK_TILE): per pass the tiles' digit
counts, a two-level scan of the [256][tiles] table over blocks of SCAN_BLOCK = 1024 entries (RANK_SCAN_BLOCK) whose
block sums one workgroup scans SCAN_TOP = 256 at a time (RANK_SCAN_TOP), and a scatter with a stable rank inside the
tile; the running count C(r) is the same scan over the N sorted flags.  The sizes here sit where that can go wrong: one
element, a tile less one / exactly / plus one, three tiles and a few, SCAN_TOP * SCAN_BLOCK + 1 elements (the scan of the
flags takes a second step of its top level) and (SCAN_TOP * SCAN_BLOCK / 256 + 1) tiles and a few (the scan of the
table does).  The keys make stability, every pass and every skipped pass show.  Everything is compared exactly: integers
with array_equal, floating point as bit patterns."""
from pathlib import Path

import numpy as np
import pytest

import rank_reference as rr

pytestmark = pytest.mark.gpu

TILE, SCAN_BLOCK, SCAN_TOP = 2048, 1024, 256  # RANK_TILE, RANK_SCAN_BLOCK, RANK_SCAN_TOP of csrc/plan.h
CUM_TOP = SCAN_TOP * SCAN_BLOCK + 1                       # N flags: 257 scan blocks
TABLE_TOP = (SCAN_TOP * SCAN_BLOCK // 256 + 1) * TILE + 5  # 1025 tiles: 256 * 1025 table entries, 257 scan blocks
SIZES = [1, TILE - 1, TILE, TILE + 1, 3 * TILE + 5, CUM_TOP, TABLE_TOP]
KNN_ERR_INVALID = -1
S64, SF = -7777, -7777.25  # what the output arrays hold before a call
GOLDEN = Path(__file__).resolve().parent / "golden" / "reference_rank.npz"


def _ptr(a):
    return None if a is None else a.ctypes.data


def c_rank(scores_, correct_, limit, descending=0, targets=None, ranks=None, want_order=True, want_cum=True, over=None):
    """the C entry point -> (return code, order, cum, idx, cum_at, sorted_at), the outputs pre-filled with the sentinels;
    `over` replaces arguments of the call by name"""
    from knn_for_homology_amd import _lib
    scores = np.ascontiguousarray(scores_)
    assert scores.dtype in (np.float32, np.float64) and scores.ndim == 2
    correct = None if correct_ is None else np.ascontiguousarray(correct_, np.uint8)
    rows, k = scores.shape
    n = rows * limit if 1 <= limit <= k else 1
    targets = np.zeros(0, np.int64) if targets is None else np.ascontiguousarray(targets, np.int64)
    ranks = np.zeros(0, np.int64) if ranks is None else np.ascontiguousarray(ranks, np.int64)
    a = dict(scores=scores, key_type=1 if scores.dtype == np.float64 else 0, rows=rows, k=k, limit=limit, correct=correct, descending=descending,
             order=np.full(n, S64, np.int64) if want_order else None, cum=np.full(n, S64, np.int64) if want_cum else None,
             targets=targets, nt=len(targets), idx=np.full(max(len(targets), 1), S64, np.int64), cum_at=np.full(max(len(targets), 1), S64, np.int64),
             ranks=ranks, nr=len(ranks), sorted_at=np.full(max(len(ranks), 1), SF, scores.dtype))
    outs = (a["order"], a["cum"], a["idx"][:len(targets)], a["cum_at"][:len(targets)], a["sorted_at"][:len(ranks)])
    a.update(over or {})
    rc = _lib.lib().knn_eval_rank(_ptr(a["scores"]), a["key_type"], a["rows"], a["k"], a["limit"], _ptr(a["correct"]), a["descending"],
                                  _ptr(a["order"]), _ptr(a["cum"]), _ptr(a["targets"]), a["nt"], _ptr(a["idx"]), _ptr(a["cum_at"]),
                                  _ptr(a["ranks"]), a["nr"], _ptr(a["sorted_at"]))
    return (rc, *outs)


def info():
    from knn_for_homology_amd import evaluation as ev
    return ev.last_rank_info()


def targets_for(C):
    """0, below 0, repeats, the counts at both ends of every tile boundary, the last count, unreachable ones"""
    n = len(C)
    edge = [int(C[i]) for t in range(TILE, n, TILE) for i in (t - 1, t)][:8]
    return np.array([0, -3, 1, 1, *edge, int(C[-1]), int(C[-1]), int(C[-1]) + 1, 1 << 40, int(C[n // 2])], np.int64)


def ranks_for(n, rng):
    fixed = [0, n - 1, n // 2, min(TILE - 1, n - 1), min(TILE, n - 1), n - 1]
    return np.concatenate([fixed, rng.integers(0, n, 20)]).astype(np.int64)


def check(scores, correct, limit, descending, rng):
    """every output of one call against the restatement"""
    C, order = rr.cumulative(correct, scores, limit, descending)
    n = len(C)
    assert n == scores.shape[0] * limit
    targets, ranks = targets_for(C), ranks_for(n, rng)
    rc, g_order, g_cum, g_idx, g_at, g_sorted = c_rank(scores, correct, limit, int(descending), targets, ranks)
    assert rc == 0
    assert np.array_equal(g_order, order)
    assert np.array_equal(g_cum, C)
    idx, at = rr.lookup(C, targets)
    assert np.array_equal(g_idx, idx) and np.array_equal(g_at, at)
    assert g_idx[0] == 0 and g_idx[1] == 0 and g_idx[-2] == n and g_idx[-3] == n  # t <= 0; unreachable
    flat = scores[:, :limit].reshape(-1)
    assert np.array_equal(rr.bits(g_sorted), rr.bits(flat[order[ranks]]))
    i = info()
    assert i["tiles"] == -(-n // TILE) and i["passes_run"] + i["passes_skipped"] == scores.dtype.itemsize and i["passes_run"] >= 1
    return i


def from_bits(words, dtype):
    return np.asarray(words, {np.float32: np.uint32, np.float64: np.uint64}[dtype]).view(dtype)


def make_keys(kind, n, dtype, rng):
    """-> (keys [n], (passes run, passes skipped) the sort must report, or None)"""
    nbytes = np.dtype(dtype).itemsize
    if kind == "equal":  # stability alone: the order is 0 .. n - 1; one forced pass builds the payloads
        return np.full(n, 1.5, dtype), (1, nbytes - 1)
    if kind == "two":
        return rng.choice(np.array([-1.0, 2.0], dtype), n), None
    if kind == "ints":
        return rng.integers(0, 4, n).astype(dtype), None
    if kind == "odd":
        tiny = np.finfo(dtype).smallest_subnormal
        if dtype == np.float32:
            nans = from_bits([0x7FC00000, 0xFFC00000, 0x7F800001, 0xFF800001, 0x7FFFFFFF, 0xFFFFFFFF, 0x7FC12345], dtype)
        else:
            nans = from_bits([0x7FF8000000000000, 0xFFF8000000000000, 0x7FF0000000000001, 0xFFF0000000000001, 0x7FFFFFFFFFFFFFFF,
                              0xFFFFFFFFFFFFFFFF, 0x7FF8000012345678], dtype)
        pool = np.concatenate([np.array([0.0, -0.0, np.inf, -np.inf, tiny, -tiny, 3 * tiny, -3 * tiny, np.finfo(dtype).tiny, np.finfo(dtype).max,
                                         -np.finfo(dtype).max, 1.0, -1.0], dtype), nans, rng.normal(0, 1, 8).astype(dtype)])
        return pool[rng.integers(0, len(pool), n)], None
    if kind == "low_byte":  # float32: one pass runs, the three above it are skipped
        return from_bits(0x3F800000 | rng.integers(0, 256, n, dtype=np.uint32), np.float32), (1, 3)
    if kind == "high_byte":  # float32, positive: only the top pass runs
        return from_bits(rng.integers(0, 128, n, dtype=np.uint32) << 24, np.float32), (1, 3)
    if kind == "low_word":  # float64: the four low passes run
        return from_bits(np.uint64(0x3FF0000000000000) | rng.integers(0, 1 << 32, n, dtype=np.uint64), np.float64), (4, 4)
    if kind == "high_word":  # float64, positive and finite: the four high passes run
        return from_bits(rng.integers(0, 0x7FF00000, n, dtype=np.uint64) << np.uint64(32), np.float64), (4, 4)
    raise AssertionError(kind)


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("n", SIZES)
def test_sizes_around_every_internal_width(gpu_faiss, n, dtype):
    rng = np.random.default_rng(n)
    # a few distinct values only: long runs of equal keys, whose order is the stability of every pass
    keys = (rng.integers(-40, 40, n) * 0.37).astype(dtype).reshape(n, 1)
    correct = rng.random((n, 1)) < 0.4
    check(keys, correct, 1, False, rng)


KINDS = [("equal", np.float32), ("equal", np.float64), ("two", np.float32), ("two", np.float64), ("ints", np.float32), ("ints", np.float64),
         ("odd", np.float32), ("odd", np.float64), ("low_byte", np.float32), ("high_byte", np.float32), ("low_word", np.float64),
         ("high_word", np.float64)]


@pytest.mark.parametrize("descending", [False, True], ids=["asc", "desc"])
@pytest.mark.parametrize("kind,dtype", KINDS, ids=[f"{k}-{np.dtype(d).name}" for k, d in KINDS])
def test_keys(gpu_faiss, kind, dtype, descending):
    rng = np.random.default_rng(len(kind) * 7 + np.dtype(dtype).itemsize)
    n = 3 * TILE + 5
    keys, passes = make_keys(kind, n, dtype, rng)
    correct = rng.random((n, 1)) < 0.5
    i = check(keys.reshape(n, 1), correct, 1, descending, rng)
    if passes is not None:
        assert (i["passes_run"], i["passes_skipped"]) == passes
    if kind == "equal":
        rc, order, *_ = c_rank(keys.reshape(n, 1), correct, 1, int(descending))
        assert rc == 0 and np.array_equal(order, np.arange(n))


@pytest.mark.parametrize("flags", ["zeros", "ones", "random"])
def test_flags_and_tile_boundary_targets(gpu_faiss, flags):
    rng = np.random.default_rng(5)
    n = 2 * TILE + 1
    keys = rng.permutation(n).astype(np.float32).reshape(n, 1)
    correct = {"zeros": np.zeros((n, 1), bool), "ones": np.ones((n, 1), bool), "random": rng.random((n, 1)) < 0.5}[flags]
    check(keys, correct, 1, False, rng)
    if flags == "ones":  # C(r) = r + 1: a target c is first reached at rank c - 1
        t = np.array([TILE, TILE + 1, 2 * TILE, 2 * TILE + 1, n, n + 1, 0, TILE, TILE], np.int64)
        rc, _, _, idx, at, _ = c_rank(keys, correct, 1, targets=t, want_order=False, want_cum=False)
        assert rc == 0
        assert idx.tolist() == [TILE - 1, TILE, 2 * TILE - 1, 2 * TILE, n - 1, n, 0, TILE - 1, TILE - 1]  # last of a tile, first of the next
        assert at.tolist() == [TILE, TILE + 1, 2 * TILE, 2 * TILE + 1, n, n, 1, TILE, TILE]
    if flags == "zeros":  # nothing is ever reached
        rc, _, _, idx, at, _ = c_rank(keys, correct, 1, targets=[1, 0], want_order=False, want_cum=False)
        assert rc == 0 and idx.tolist() == [n, 0] and at.tolist() == [0, 0]


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
# limit <= k / 2: the host packs the first `limit` columns; above that the whole rows go up and the kernels skip the rest
@pytest.mark.parametrize("rows,k,limit", [(700, 9, 9), (700, 9, 4), (700, 9, 5), (700, 8, 4), (1, 5000, 4999), (5000, 3, 1)])
def test_limit_and_strided_rows(gpu_faiss, rows, k, limit, dtype):
    rng = np.random.default_rng(rows + k + limit)
    scores = rng.integers(0, 50, (rows, k)).astype(dtype)
    scores[:, limit:] = -1e9  # the columns past the limit would all sort first if they were read
    correct = rng.random((rows, k)) < 0.3
    correct[:, limit:] = True
    for descending in (False, True):
        check(scores, correct, limit, descending, rng)


def test_optional_outputs(gpu_faiss):
    """each output only when asked for; correct may be left out when neither C nor a target is wanted"""
    rng = np.random.default_rng(9)
    n = TILE + 7
    keys = rng.integers(0, 9, (n, 1)).astype(np.float64)
    correct = rng.random((n, 1)) < 0.5
    C, order = rr.cumulative(correct, keys)
    rc, g_order, _, _, _, g_sorted = c_rank(keys, None, 1, want_cum=False, ranks=[0, n - 1])
    assert rc == 0 and np.array_equal(g_order, order) and np.array_equal(g_sorted, keys[order[[0, n - 1]], 0])
    rc, _, g_cum, _, _, _ = c_rank(keys, correct, 1, want_order=False)
    assert rc == 0 and np.array_equal(g_cum, C)
    rc, _, _, idx, at, _ = c_rank(keys, correct, 1, want_order=False, want_cum=False, targets=[3])
    assert rc == 0 and (idx.tolist(), at.tolist()) == tuple(a.tolist() for a in rr.lookup(C, [3]))


def test_c_entry_refuses_bad_arguments_and_touches_nothing(gpu_faiss):
    keys = np.arange(12, dtype=np.float32).reshape(4, 3)
    correct = np.ones((4, 3), np.uint8)
    bad = [dict(key_type=2), dict(rows=0), dict(k=0), dict(k=1 << 31), dict(limit=0), dict(limit=4), dict(rows=1 << 30, limit=3, k=3),
           dict(scores=None), dict(nt=-1), dict(nr=-1), dict(nt=1 << 31), dict(idx=None), dict(cum_at=None), dict(targets=None),
           dict(ranks=None), dict(sorted_at=None), dict(correct=None), dict(ranks=np.array([12], np.int64)), dict(ranks=np.array([-1], np.int64))]
    for over in bad:
        args = dict(over)
        rc, order, cum, idx, at, sorted_at = c_rank(keys, correct, args.pop("limit", 3), targets=[1], ranks=[0], over=args)
        assert rc == KNN_ERR_INVALID, over
        assert (order == S64).all() and (cum == S64).all() and (idx == S64).all() and (at == S64).all() and (sorted_at == SF).all(), over
    rc, *_ = c_rank(keys, correct, 3, targets=[1], ranks=[0])
    assert rc == 0


# ---- the three functions ------------------------------------------------------------------------------------------------
def golden_cases():
    g = np.load(GOLDEN)
    return [(str(run), str(label), str(name)) for run in g["runs"] for label in g["sets"] for name in g["names"]]


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.mark.parametrize("run,label,name", golden_cases())
def test_ranked_precision_recall_is_the_reference(gpu_faiss, golden, run, label, name):
    from knn_for_homology_amd import evaluation as ev
    g = golden
    scores, correct = g[f"{run}_{label}_scores"], g[f"{run}_{label}_correct"]
    total, limit = int(g[f"{run}_total"]), int(g[f"{run}_{label}_{name}_limit"])
    recall, precision = ev.ranked_precision_recall(correct, scores, total, limit=limit)
    assert recall.dtype == precision.dtype == np.float64 and recall.shape == precision.shape == (10000,)
    assert np.array_equal(rr.bits(recall), rr.bits(g[f"{run}_{label}_{name}_recall"]))
    assert np.array_equal(rr.bits(precision), rr.bits(g[f"{run}_{label}_{name}_precision"]))


def test_ranked_precision_recall_descending_points_and_ties(gpu_faiss):
    from knn_for_homology_amd import evaluation as ev
    rng = np.random.default_rng(11)
    scores = rng.integers(0, 30, (300, 20)).astype(np.float32) / 8  # ties with both values of `correct`: the stable order decides
    scores[::17, 5] = np.nan
    correct = rng.random((300, 20)) < 0.35
    for descending, limit, points, total in ((False, None, 10000, 1500), (True, 7, 501, int(correct[:, :7].sum())), (True, 20, 1, 10)):
        got = ev.ranked_precision_recall(correct, scores, total, limit=limit, points=points, descending=descending)
        want = rr.precision_recall_direct(correct, scores, total, limit, points, descending)
        assert np.array_equal(rr.bits(got[0]), rr.bits(want[0])) and np.array_equal(rr.bits(got[1]), rr.bits(want[1]))


def test_ranked_cumulative(gpu_faiss, golden):
    from knn_for_homology_amd import evaluation as ev
    rng = np.random.default_rng(12)
    for keys, correct in ((rng.integers(0, 6, 5000).astype(np.float64), rng.random(5000) < 0.5),              # 1-D
                          (golden["never_mmseqs_scores"], golden["never_mmseqs_correct"]),                       # 2-D float64
                          (rng.random((100, 33)).astype(np.float32), (rng.random((100, 33)) < 0.2).astype(np.uint8)),
                          (rng.integers(0, 3, (10, 4)), rng.integers(0, 2, (10, 4)))):                          # integers: as float64
        for descending in (False, True):
            want_c, want_o = rr.cumulative(correct, np.asarray(keys, np.float32 if keys.dtype == np.float32 else np.float64), None, descending)
            cum, order = ev.ranked_cumulative(correct, keys, descending=descending, want_order=True)
            assert cum.dtype == order.dtype == np.int64
            assert np.array_equal(cum, want_c) and np.array_equal(order, want_o)
            assert np.array_equal(ev.ranked_cumulative(correct, keys, descending=descending), want_c)
            assert np.array_equal(want_c, np.asarray(correct).reshape(-1)[want_o].astype(bool).cumsum())


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_score_quantiles_is_numpy_quantile(gpu_faiss, dtype):
    from knn_for_homology_amd import evaluation as ev
    rng = np.random.default_rng(13)
    q = np.concatenate([np.linspace(0, 1, 301), [0.0, 1.0, 0.5, 0.5, 1 / 3], rng.random(20)])
    for scores, limit in ((rng.normal(0, 2, (700, 30)).astype(dtype), None), (rng.normal(0, 2, (700, 30)).astype(dtype), 11),
                          (rng.integers(0, 5, (259, 1)).astype(dtype), None), (rng.normal(0, 1, 6000).astype(dtype), None),
                          (np.full((3, 3), 2.5, dtype), 2), (np.array([[7.0]], dtype), None)):
        got = ev.score_quantiles(scores, q, limit)
        assert got.dtype == np.float64 and got.shape == q.shape
        assert np.array_equal(rr.bits(got), rr.bits(rr.quantiles(scores, q, limit)))
        assert np.array_equal(rr.bits(got), rr.bits(np.quantile(scores if scores.ndim == 1 else scores[:, :limit], q)))
    with_nan = rng.normal(0, 1, (40, 5)).astype(dtype)
    with_nan[3, 2] = np.nan
    assert np.isnan(ev.score_quantiles(with_nan, q)).all()
    assert ev.score_quantiles(with_nan, []).shape == (0,)
    # precision_recall_curve takes them as its thresholds: the same curve as with its own host quantiles
    if dtype == np.float32:
        scores = rng.random((300, 12)).astype(np.float32)
        correct = rng.random((300, 12)) < 0.3
        totals = np.maximum(correct.sum(axis=1), 1)
        thr = ev.score_quantiles(scores, np.linspace(0, 1, 21), 8)
        a = ev.precision_recall_curve(correct, scores, totals, limit=8, smoothness=20)
        b = ev.precision_recall_curve(correct, scores, totals, limit=8, thresholds=thr)
        assert all(np.array_equal(rr.bits(x), rr.bits(y)) for x, y in zip(a, b))


def test_python_error_paths(gpu_faiss):
    from knn_for_homology_amd import evaluation as ev
    c, s = np.zeros((3, 4), bool), np.zeros((3, 4), np.float32)
    for bad in (lambda: ev.ranked_precision_recall(c[:2], s, 5), lambda: ev.ranked_precision_recall(c, s, 5, limit=0),
                lambda: ev.ranked_precision_recall(c, s, 5, limit=5), lambda: ev.ranked_precision_recall(c, s, 0),
                lambda: ev.ranked_cumulative(c, s[:, :3]), lambda: ev.score_quantiles(s, [1.5]), lambda: ev.score_quantiles(s, [-0.5]),
                lambda: ev.score_quantiles(s, [0.5], limit=5),
                lambda: ev.ranked_cumulative(np.broadcast_to(np.zeros(1, bool), (1 << 16, 1 << 15)),
                                             np.broadcast_to(np.zeros(1, np.float32), (1 << 16, 1 << 15)))):
        with pytest.raises(ValueError):
            bad()
    # and the calls still work afterwards
    assert ev.ranked_cumulative(np.array([1, 0, 1]), np.array([3.0, 1.0, 2.0])).tolist() == [0, 1, 2]
