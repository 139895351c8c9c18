"""GPU: knn_eval_rankdata / knn_eval_correlate (csrc/correlate.inc) and evaluation.rankdata / pearsonr / spearmanr /
correlations on top of them, against tests/correlation_reference.py: the doubled ranks and the 128-bit sums exactly, the
five Pearson numbers bit for bit (where both sides are NaN the payload is not compared: the sign and payload of inf - inf
are the processor's choice), and with them the Python statistics.

The sizes sit where each mechanism can break: N = 2, 3 and around one wave (63, 64, 65); around the sort tile and the moment
tile (2047, 2048, 2049); a run of equal keys lying across rank 2048 (two sort tiles) and runs across ranks 1024 and 3072 (scan
blocks); one run of N and N runs of one; N = 262 145, one past the 256 x 1024 entries of one step of the scan's top level and
128 moment tiles plus one term; both mixed type pairs; [rows, k] input with the limit above and at or below k / 2 (as given,
and packed on the host); -0.0 beside +0.0; infinities; a NaN in x, in y, in the last cell.
At N = 262 145 no positive sum reaches 2^64 (N^3 < 2^55), so the case that makes the high words non-zero is the one whose
every u * v is near -N^2 / 4: two tie groups in x against the opposite two in y, Suv near -N^3 / 4, high word all ones."""
import math

import numpy as np
import pytest

import correlation_reference as ref
from test_correlation_reference import GOLDEN, STATISTIC_BOUND

pytestmark = pytest.mark.gpu

KNN_ERR_INVALID = -1
S64, SF, SU = -7777, -7777.25, 0x7777777777777777  # what the output arrays hold before a call


def _ptr(a):
    return None if a is None else a.ctypes.data


def _shape(a, limit):
    rows, k = a.shape if a.ndim == 2 else (a.size, 1)
    return rows, k, k if limit is None else limit


def c_rankdata(a, limit=None, over=None):
    """the C entry point -> (return code, rank2, NaN count), rank2 pre-filled with the sentinel"""
    from ctypes import byref, c_int32
    from knn_for_homology_amd import _lib
    a = np.ascontiguousarray(a)
    assert a.dtype in (np.float32, np.float64)
    rows, k, limit = _shape(a, limit)
    arg = dict(a=a, key_type=1 if a.dtype == np.float64 else 0, rows=rows, k=k, limit=limit, rank2=np.full(max(rows * max(limit, 0), 1), S64, np.int64), nan=c_int32(-5))
    arg.update(over or {})
    rc = _lib.lib().knn_eval_rankdata(_ptr(arg["a"]), arg["key_type"], arg["rows"], arg["k"], arg["limit"], _ptr(arg["rank2"]),
                                      None if arg["nan"] is None else byref(arg["nan"]))
    return rc, arg["rank2"], None if arg["nan"] is None else arg["nan"].value


def c_correlate(x, y, limit=None, what=3, over=None):
    """the C entry point -> (return code, pearson [5], spearman words [6], NaN counts [2]), pre-filled with the sentinels"""
    from knn_for_homology_amd import _lib
    x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
    rows, k, limit = _shape(x, limit)
    arg = dict(x=x, x_type=1 if x.dtype == np.float64 else 0, y=y, y_type=1 if y.dtype == np.float64 else 0, rows=rows, k=k, limit=limit, what=what,
               pearson=np.full(5, SF), spearman=np.full(6, SU, np.uint64), nan=np.full(2, S64, np.int64))
    arg.update(over or {})
    rc = _lib.lib().knn_eval_correlate(_ptr(arg["x"]), arg["x_type"], _ptr(arg["y"]), arg["y_type"], arg["rows"], arg["k"], arg["limit"], arg["what"],
                                       _ptr(arg["pearson"]), _ptr(arg["spearman"]), _ptr(arg["nan"]))
    return rc, arg["pearson"], arg["spearman"], arg["nan"]


def same_bits(got, want):
    got, want = np.ascontiguousarray(got, np.float64), np.ascontiguousarray(want, np.float64)
    nan = np.isnan(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(np.uint64)[~nan], want.view(np.uint64)[~nan])


def same_float(a, b):
    return (math.isnan(a) and math.isnan(b)) or a == b


def expected(x, y, limit=None):
    """the restatement -> (rank2_x, rank2_y, NaN counts, words [6] or None, moments [5], r, rho)"""
    fx, fy = ref.cells(x, limit), ref.cells(y, limit)
    (rx, nx), (ry, ny) = ref.doubled_ranks(fx), ref.doubled_ranks(fy)
    sums = None if nx or ny else ref.spearman_sums_fast(rx, ry)
    w = None if sums is None else np.array([word for s in sums for word in ref.words(s)], np.uint64)
    m = ref.pearson_moments(fx, fy)
    return rx, ry, (nx, ny), w, m, ref.ratio(m[3], m[2], m[4]), math.nan if sums is None else ref.spearman_ratio(*sums)


def check_all(x, y, limit=None):
    """every entry and every facade on one pair of arrays against the restatement; -> what expected() returns"""
    from knn_for_homology_amd import evaluation as ev
    rx, ry, nans, w, m, r, rho = want = expected(x, y, limit)
    for a, rank2, nan in ((x, rx, nans[0]), (y, ry, nans[1])):
        rc, got, count = c_rankdata(a, limit)
        assert rc == 0 and count == nan
        assert np.array_equal(got, rank2) if not nan else (got == S64).all()
        ranks = ev.rankdata(a, limit)
        assert ranks.dtype == np.float64 and (np.array_equal(ranks, rank2 / 2) if not nan else np.isnan(ranks).all())
    rc, pear, words, count = c_correlate(x, y, limit, 3)
    assert rc == 0 and tuple(count) == nans
    assert np.array_equal(words, w) if w is not None else (words == SU).all()
    assert same_bits(pear, m), (pear, m)
    # each statistic alone is the same numbers
    rc, pear1, words1, count1 = c_correlate(x, y, limit, 1)
    assert rc == 0 and same_bits(pear1, m) and (words1 == SU).all() and (count1 == S64).all()
    rc, pear2, words2, count2 = c_correlate(x, y, limit, 2)
    assert rc == 0 and (pear2 == SF).all() and np.array_equal(words2, words) and tuple(count2) == nans
    both = ev.correlations(x, y, limit)
    assert same_float(both[0].statistic, r) and same_float(both[1].statistic, rho)
    assert same_float(ev.pearsonr(x, y, limit).statistic, r) and same_float(ev.spearmanr(x, y, limit).statistic, rho)
    assert same_float(both[0].pvalue, ev.correlation_pvalue("pearson", r, rx.size)) and same_float(both[1].pvalue, ev.correlation_pvalue("spearman", rho, rx.size))
    return want


def draws(n, seed, xt=np.float32, yt=np.float64):
    """cosine-like scores and E-value-like values with repeats, correlated"""
    rng = np.random.default_rng(seed)
    e = np.exp(rng.normal(-12, 10, n))
    e[rng.random(n) < 0.2] = e[rng.integers(0, n)]
    e[rng.random(n) < 0.01] = 0.0
    cos = np.round(0.5 - 0.01 * np.log10(e + 1e-300) + rng.normal(0, 0.1, n), 3)
    return cos.astype(xt), e.astype(yt)


@pytest.mark.parametrize("n", [2, 3, 63, 64, 65, 2047, 2048, 2049])
def test_sizes_around_a_wave_and_a_tile(n):
    x, y = draws(n, n)
    check_all(x, y)


def test_runs_across_the_sort_tile_and_the_scan_blocks():
    rng = np.random.default_rng(1)
    n = 4100
    # in the sorted order of x the ranks 2040 .. 2060 are one run; in that of y the ranks 1020 .. 1030 and 3060 .. 3080
    x = np.arange(n, dtype=np.float32)
    x[2040:2061] = 2040.0
    y = np.arange(n, dtype=np.float64) * 0.5
    y[1020:1031] = y[1020]
    y[3060:3081] = y[3060]
    x, y = x[rng.permutation(n)], y[rng.permutation(n)]
    rx, ry, *_ = check_all(x, y)
    assert (rx == 2040 + 2060 + 2).sum() == 21 and (ry == 1020 + 1030 + 2).sum() == 11 and (ry == 3060 + 3080 + 2).sum() == 21


def test_one_run_of_n_and_n_runs_of_one():
    n = 2500
    const = np.full(n, 0.25, np.float32)
    x, y = draws(n, 7)
    rx, _, _, w, _, r, rho = check_all(const, y)
    assert (rx == n + 1).all() and math.isnan(r) and math.isnan(rho) and w[0] == 0 and w[1] == 0
    rng = np.random.default_rng(2)
    rx, ry, *_ = check_all(rng.permutation(n).astype(np.float32), rng.permutation(n) / 7.0)
    assert len(np.unique(rx)) == n == len(np.unique(ry))


def test_past_the_scans_top_level_step():
    x, y = draws(262145, 3)
    check_all(x, y)


def test_mixed_types_both_ways():
    x, y = draws(3000, 4, np.float64, np.float32)
    check_all(x, y)
    x, y = draws(3000, 5, np.float32, np.float32)
    check_all(x, y)
    x, y = draws(3000, 6, np.float64, np.float64)
    check_all(x, y)


@pytest.mark.parametrize("limit", [10, 7, 5, 4, 1])
def test_rows_with_a_limit(limit):
    x, y = draws(300 * 10, 8)
    x, y = x.reshape(300, 10), y.reshape(300, 10)
    x[7], y[7] = x[3], y[3]  # ties between rows
    # what lies past the limit must not matter
    x2, y2 = x.copy(), y.copy()
    x2[:, limit:], y2[:, limit:] = 99.0, np.nan
    want = check_all(x, y, limit)
    rc, pear, words, count = c_correlate(x2, y2, limit, 3)
    assert rc == 0 and same_bits(pear, want[4]) and np.array_equal(words, want[3]) and not count.any()


def test_negative_zero_ties_with_positive_zero():
    x = np.array([0.0, -0.0, 0.5, -0.0, 0.0, -0.5, 1.0], np.float32)
    y = np.array([-0.0, 2.0, 0.0, -1.0, 0.0, -0.0, 3.0])
    rx, ry, *_ = check_all(x, y)
    assert list(rx) == [7, 7, 12, 7, 7, 2, 14] and list(ry) == [7, 12, 7, 2, 7, 7, 14]


def test_infinities_rank_by_value_and_make_pearson_nan():
    x, y = draws(700, 9)
    x[5], x[6], y[17] = np.inf, -np.inf, np.inf
    rx, ry, _, w, m, r, rho = check_all(x, y)
    assert rx[5] == 2 * 700 and rx[6] == 2 and ry[17] == 2 * 700
    assert math.isnan(r) and np.isnan(m[2:]).all() and not math.isnan(rho) and w is not None


@pytest.mark.parametrize("where", ["x", "y", "last", "both"])
def test_a_nan_is_reported_and_propagates(where):
    from knn_for_homology_amd import evaluation as ev
    x, y = draws(2100, 10)
    if where in ("x", "both"):
        x[11] = np.nan
    if where in ("y", "both"):
        y[2050] = y[3] = np.nan
    if where == "last":
        y[-1] = np.nan
    *_, nans, w, m, r, rho = check_all(x, y)
    assert nans == {"x": (1, 0), "y": (0, 2), "last": (0, 1), "both": (1, 2)}[where] and w is None and math.isnan(r) and math.isnan(rho)
    res = ev.spearmanr(x, y)
    assert math.isnan(res.statistic) and math.isnan(res.pvalue)


def test_monotone_pairs_are_exactly_one():
    from knn_for_homology_amd import evaluation as ev
    x, _ = draws(5000, 12)
    up, down = np.exp(x.astype(np.float64) * 3), -(x.astype(np.float64) ** 3) + 1
    assert ev.spearmanr(x, up).statistic == 1.0 and ev.spearmanr(x, down).statistic == -1.0
    assert ev.spearmanr(x, up).pvalue == 0.0
    *_, rho = check_all(x, up)
    assert rho == 1.0
    *_, rho = check_all(x, down)
    assert rho == -1.0


def test_high_words_of_the_sums():
    n = 262145
    rng = np.random.default_rng(13)
    x = (rng.permutation(n) < n // 2).astype(np.float32)  # two tie groups: |u| near N / 2 everywhere
    y = 1.0 - x.astype(np.float64)                        # the opposite two: every u * v near -N^2 / 4
    *_, w, _, r, rho = check_all(x, y)
    assert w[3] == 0xFFFFFFFFFFFFFFFF and w[1] == 0 and w[5] == 0
    suv = ref.spearman_sums_fast(*[ref.doubled_ranks(a)[0] for a in (x, y)])[1]
    assert -n ** 3 // 4 - n ** 2 <= suv <= -n ** 3 // 4 + n ** 2 and rho == -1.0


def test_golden_fixture_within_the_cpu_tests_bound():
    from knn_for_homology_amd import evaluation as ev
    g = np.load(GOLDEN)
    for name in g["cases"]:
        x, y, logged = g[f"{name}_x"], g[f"{name}_y"], g[f"{name}_logged"]
        assert np.array_equal(ev.rankdata(x), g[f"{name}_rank_x"]) and np.array_equal(ev.rankdata(y), g[f"{name}_rank_y"])
        r, rho = ev.pearsonr(x, logged), ev.spearmanr(x, y)
        print(name, "pearson", abs(r.statistic - g[f"{name}_pearson"][0]), "spearman", abs(rho.statistic - g[f"{name}_spearman"][0]))
        assert abs(r.statistic - g[f"{name}_pearson"][0]) <= STATISTIC_BOUND
        assert abs(rho.statistic - g[f"{name}_spearman"][0]) <= STATISTIC_BOUND
        assert r.statistic == ref.pearson(x, logged) and rho.statistic == ref.spearman(x, y)
        if np.isfinite(y).all():  # cath/cath.py:949-952 from one call
            both = ev.correlations(x, logged)
            assert both[0] == r and both[1] == rho


def test_invalid_arguments_leave_the_outputs_untouched():
    from knn_for_homology_amd import _lib
    x, y = draws(40, 14)
    x2, y2 = x.reshape(10, 4), y.reshape(10, 4)
    bad = [dict(x_type=2), dict(y_type=-1), dict(rows=0), dict(rows=-3), dict(k=0), dict(k=2 ** 31), dict(limit=0), dict(limit=5), dict(x=None), dict(y=None),
           dict(what=0), dict(what=4), dict(what=-1), dict(pearson=None), dict(spearman=None), dict(nan=None), dict(rows=2 ** 31, k=1, limit=1),
           dict(rows=2 ** 29, k=4, limit=4)]
    for over in bad:
        rc, pear, words, count = c_correlate(x2, y2, None, 3, over)
        assert rc == KNN_ERR_INVALID, over
        assert _lib.lib().knn_last_error()
        assert (pear is None or (pear == SF).all()) and (words is None or (words == SU).all()) and (count is None or (count == S64).all()), over
    one = np.ones((1, 1), np.float32)
    assert c_correlate(one, one.astype(np.float64), None, 3)[0] == KNN_ERR_INVALID  # N = 1
    # an output that was not asked for may be null
    assert c_correlate(x2, y2, None, 1, dict(spearman=None, nan=None))[0] == 0
    assert c_correlate(x2, y2, None, 2, dict(pearson=None))[0] == 0
    for over in [dict(key_type=2), dict(rows=0), dict(k=0), dict(limit=0), dict(limit=5), dict(a=None), dict(rank2=None), dict(nan=None), dict(rows=2 ** 31, k=1, limit=1)]:
        rc, rank2, count = c_rankdata(x2, None, over)
        assert rc == KNN_ERR_INVALID, over
        assert (rank2 is None or (rank2 == S64).all()) and count in (None, -5), over
    assert c_rankdata(one)[0] == KNN_ERR_INVALID


def test_two_calls_return_identical_bytes():
    from knn_for_homology_amd import evaluation as ev
    x, y = draws(70000, 15)
    first, second = c_correlate(x, y), c_correlate(x, y)
    assert first[0] == 0 == second[0]
    for a, b in zip(first[1:], second[1:]):
        assert a.tobytes() == b.tobytes()
    assert c_rankdata(y)[1].tobytes() == c_rankdata(y)[1].tobytes()
    ms = ev.last_correlate_ms()
    assert list(ms) == ["alloc_ms", "upload_ms", "sort_ms", "ranks_ms", "moments_ms", "download_ms"]
    assert all(math.isfinite(v) and v >= 0 for v in ms.values()) and ms["sort_ms"] > 0 and ms["ranks_ms"] > 0
    ev.pearsonr(x, y)
    ms = ev.last_correlate_ms()
    assert ms["sort_ms"] == 0 and ms["ranks_ms"] == 0 and ms["moments_ms"] > 0
