"""GPU: knn_eval_windows (csrc/windows.inc) and evaluation.rolling_means / even_bins / edge_bins on top of it, bit for
bit against tests/windows_reference.py.

Integers with array_equal, floating point as bit patterns, with one allowance: where both sides are NaN the payload is not
compared (the sign and payload of inf - inf and of NaN + NaN are the processor's choice, not the contract's).  Where a
NaN comes straight from one key -- W = 1 -- sign and payload are compared too (test_special_keys).

The sizes sit where each mechanism can break: one element; N = 300 with W in {1, 2, 7, 299, 300} (a single output,
i % W == 0 on every output, i - 1 = -1); one past one and two sort tiles with W = 1000 (a short last block, windows over the
tile seam); W around the chain kernel's staging run, read from knn_last_windows_info, with N = 3 runs + 5 (W <= run:
whole blocks share a run; W > run: a chain's sum is carried across restaging); M in {0, 1, 5, 32} with column c of the
32 set where position % (c + 2) == 0, so that a swapped or shifted mask bit changes a count."""
import warnings

import numpy as np
import pytest

import rank_reference as rr
import windows_reference as wr

pytestmark = pytest.mark.gpu

KNN_ERR_INVALID = -1
S64, SF = -7777, -7777.25  # what the output arrays hold before a call


def same_bits(got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return False
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and np.array_equal(rr.bits(got)[~nan], rr.bits(want)[~nan])


def _ptr(a):
    return None if a is None else a.ctypes.data


def c_windows(keys, values=None, window=0, descending=0, want_order=True, starts=None, stops=None, edges=None, over=None):
    """the C entry point -> (return code, dict of the outputs), the outputs pre-filled with the sentinels; `over` replaces
    arguments of the call by name"""
    from knn_for_homology_amd import _lib
    keys = np.ascontiguousarray(keys)
    assert keys.dtype in (np.float32, np.float64) and keys.ndim == 1
    n = keys.size
    values = None if values is None else np.ascontiguousarray(values, np.uint8)
    m = 0 if values is None else values.shape[0]
    nout = max(n - window + 1, 1) if 1 <= window <= n else 1
    nb = len(edges) if edges is not None else (len(starts) if starts is not None else 0)
    a = dict(keys=keys, key_type=1 if keys.dtype == np.float64 else 0, n=n, values=values, m=m, descending=descending, window=window,
             key_means=np.full(nout, SF), value_means=np.full((max(m, 1), nout), SF), order=np.full(n, S64, np.int64) if want_order else None,
             starts=None if starts is None else np.ascontiguousarray(starts, np.int64), stops=None if stops is None else np.ascontiguousarray(stops, np.int64),
             edges=None if edges is None else np.ascontiguousarray(edges, keys.dtype), nbins=nb, start=np.full(max(nb, 1), S64, np.int64),
             stop=np.full(max(nb, 1), S64, np.int64), counts=np.full((max(m, 1), max(nb, 1)), S64, np.int64), key_lo=np.full(max(nb, 1), SF, keys.dtype),
             key_hi=np.full(max(nb, 1), SF, keys.dtype))
    a.update(over or {})
    rc = _lib.lib().knn_eval_windows(_ptr(a["keys"]), a["key_type"], a["n"], _ptr(a["values"]), a["m"], a["descending"], a["window"], _ptr(a["key_means"]),
                                     _ptr(a["value_means"]), _ptr(a["order"]), _ptr(a["starts"]), _ptr(a["stops"]), _ptr(a["edges"]), a["nbins"],
                                     _ptr(a["start"]), _ptr(a["stop"]), _ptr(a["counts"]), _ptr(a["key_lo"]), _ptr(a["key_hi"]))
    return rc, a


def info():
    from knn_for_homology_amd import evaluation as ev
    return ev.last_windows_info()


def untouched(a):
    return all((a[name] == S64).all() for name in ("order", "start", "stop", "counts") if a[name] is not None) and \
        all((a[name] == SF).all() for name in ("key_means", "value_means", "key_lo", "key_hi") if a[name] is not None)


def check_rolling(keys, values, window, descending=False):
    """one call through the C ABI against the restatement: the order, the key's means, every column's means"""
    km, vm, o = wr.rolling_means(keys, values, window, descending)
    rc, a = c_windows(keys, values, window, int(descending))
    assert rc == 0
    assert np.array_equal(a["order"], o)
    assert same_bits(a["key_means"], km), (keys.size, window, np.flatnonzero(rr.bits(a["key_means"]) != rr.bits(km))[:5])
    m = 0 if values is None else len(values)
    if m:
        assert same_bits(a["value_means"], vm), (keys.size, window)
    else:
        assert (a["value_means"] == SF).all()
    assert (a["start"] == S64).all() and (a["key_lo"] == SF).all()
    return a


def mixed_keys(n, dtype, rng):
    """distinct magnitudes over many binades, both signs: the order of the additions shows in the last bits"""
    return (rng.normal(0, 1, n) * np.exp(rng.normal(0, 6, n))).astype(dtype)


def columns(n, m, rng):
    if m == 32:  # column c is set exactly where position % (c + 2) == 0
        return np.stack([np.arange(n) % (c + 2) == 0 for c in range(32)])
    return rng.random((m, n)) < np.linspace(0.1, 0.9, max(m, 1))[:m, None] if m else None


def test_one_element():
    a = check_rolling(np.array([2.5], np.float32), np.array([[1]], bool), 1)
    assert a["key_means"].tolist() == [2.5] and a["value_means"].tolist() == [[1.0]]
    assert info()["run"] > 0


@pytest.mark.parametrize("window", [1, 2, 7, 299, 300])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_small_windows(window, dtype):
    rng = np.random.default_rng(300 + window)
    keys = mixed_keys(300, dtype, rng)
    for descending in (False, True):
        check_rolling(keys, columns(300, 5, rng), window, descending)


@pytest.mark.parametrize("n", [2049, 4097])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_past_the_sort_tiles(n, dtype):
    rng = np.random.default_rng(n)
    keys = mixed_keys(n, dtype, rng)
    check_rolling(keys, columns(n, 5, rng), 1000, False)
    check_rolling(keys, columns(n, 1, rng), 1000, True)
    i = info()
    assert i["blocks_per_run"] == i["run"] // 1000 and i["runs_per_block"] == 1


def test_windows_around_the_staging_run():
    rng = np.random.default_rng(5)
    check_rolling(np.ones(8, np.float64), None, 2)
    run = info()["run"]  # the planner's, not a constant of this file
    n = 3 * run + 5
    keys = mixed_keys(n, np.float64, rng)
    values = columns(n, 5, rng)
    for window, bpr, rpb in ((run - 1, 1, 1), (run, 1, 1), (run + 1, 1, 2), (2 * run + 1, 1, 3)):
        check_rolling(keys, values, window)
        i = info()
        assert (i["blocks_per_run"], i["runs_per_block"]) == (bpr, rpb), (window, i)
    check_rolling(keys.astype(np.float32), values[:1], 2 * run + 1, True)
    # small windows: many blocks share a run, up to the workgroup's 128
    for window in (3, 16, 17, run // 2, run // 2 + 1):
        check_rolling(keys[:2 * run + 3], values[:2, :2 * run + 3], window)


@pytest.mark.parametrize("m", [0, 1, 5, 32])
def test_column_counts(m):
    rng = np.random.default_rng(m)
    n = 1500
    keys = mixed_keys(n, np.float32, rng)
    check_rolling(keys, columns(n, m, rng), 64)
    check_rolling(keys, columns(n, m, rng), 1000, True)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("descending", [False, True])
def test_heavy_ties(dtype, descending):
    rng = np.random.default_rng(7)
    n = 2500
    keys = rng.choice(np.array([-3.5, -1.0, 0.0, 0.25, 1.0, 1e10, 7.0], dtype), n)
    check_rolling(keys, columns(n, 5, rng), 100, descending)  # stability decides which cells a window holds
    check_rolling(keys, columns(n, 32, rng), 7, descending)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_special_keys(dtype):
    rng = np.random.default_rng(11)
    tiny = np.finfo(dtype).smallest_subnormal
    # -0.0 among +0.0: one key for the sort, and a window of -0.0 alone has the mean -0.0
    zeros = np.array([-0.0, 0.0, -0.0, -0.0, 0.0, 0.0, -0.0, -0.0, -0.0, 0.0], dtype)
    for window in (1, 2, 3, 10):
        check_rolling(zeros, columns(10, 1, rng), window)
    a = check_rolling(zeros, None, 1)
    assert np.signbit(a["key_means"]).tolist() == np.signbit(zeros).tolist()
    # sub-normals order by value and add exactly
    sub = (np.arange(-20, 20) * tiny).astype(dtype)
    check_rolling(rng.permutation(sub), columns(40, 5, rng), 7)
    # infinities: the windows that hold one are infinite, no other window is touched
    n, w = 600, 50
    keys = mixed_keys(n, dtype, rng)
    keys[[17, 400]] = np.inf
    keys[[3, 99, 250]] = -np.inf
    a = check_rolling(keys, columns(n, 5, rng), w)
    km = a["key_means"]
    assert (km[:3] == -np.inf).all() and np.isfinite(km[3:n - w - 1]).all() and (km[n - w - 1:] == np.inf).all()
    # three NaNs rank last: only the last windows are NaN, ascending or descending
    keys = mixed_keys(n, dtype, rng)
    keys[[0, 77, 599]] = np.nan
    for descending in (False, True):
        km = check_rolling(keys, columns(n, 5, rng), w, descending)["key_means"]
        assert np.isfinite(km[:n - w - 2]).all() and np.isnan(km[n - w - 2:]).all()
    # a NaN that comes straight from a key (W = 1: widened, divided by 1.0, never added to another NaN) keeps its sign and its
    # payload: here the comparison is bit for bit without the allowance
    quiet = {np.float32: [0x7FC00000, 0xFFC00000, 0x7FC12345, 0xFFC00001], np.float64: [0x7FF8000000000000, 0xFFF8000000000000, 0x7FF8000012345678, 0xFFF8000000000001]}[dtype]
    keys = mixed_keys(40, dtype, rng)
    keys[[1, 9, 22, 39]] = np.array(quiet, {np.float32: np.uint32, np.float64: np.uint64}[dtype]).view(dtype)
    for descending in (False, True):
        km = check_rolling(keys, None, 1, descending)["key_means"]
        want = wr.key_means(keys, 1, descending)
        assert np.isnan(want[-4:]).all() and np.array_equal(rr.bits(km), rr.bits(want))


def test_integer_lengths_through_evaluation():
    from knn_for_homology_amd import evaluation as ev
    rng = np.random.default_rng(13)
    lengths = rng.integers(11, 900, (50, 30))  # 2-D: flattened row by row
    cols = [rng.random((50, 30)) < p for p in (0.2, 0.7)]
    got = ev.rolling_means(lengths, cols, window=100, want_order=True)
    km, vm, o = wr.rolling_means(lengths, cols, 100)
    assert same_bits(got.keys, km) and same_bits(got.values, vm) and np.array_equal(got.order, o)
    assert got.keys.dtype == np.float64 and got.values.shape == (2, 1401)
    got = ev.rolling_means(lengths.astype(np.int32), None, window=1500, descending=True)
    assert got.values.shape == (0, 1) and got.order is None and same_bits(got.keys, wr.key_means(lengths, 1500, True))
    # want_order is ranked_cumulative's order
    keys = rng.choice(np.array([0.5, 1.5, -2.0], np.float32), 700)
    correct = rng.random(700) < 0.5
    for descending in (False, True):
        _, order = ev.ranked_cumulative(correct, keys, descending=descending, want_order=True)
        assert np.array_equal(ev.rolling_means(keys, [correct], window=9, descending=descending, want_order=True).order, order)


def check_bins(got, want, dtype):
    assert np.array_equal(got.start, want["start"]) and np.array_equal(got.stop, want["stop"])
    assert np.array_equal(got.counts, want["counts"]) and got.counts.dtype == np.int64
    assert same_bits(got.mean, want["mean"]) and same_bits(got.stderr, want["stderr"])
    assert got.key_lo.dtype == dtype and same_bits(got.key_lo, want["key_lo"]) and same_bits(got.key_hi, want["key_hi"])


@pytest.mark.parametrize("n", [8, 1000, 2049])
@pytest.mark.parametrize("bins", [1, 7, 10])
def test_even_bins(n, bins):
    from knn_for_homology_amd import evaluation as ev
    rng = np.random.default_rng(n * 31 + bins)
    for dtype, descending, m in ((np.float32, False, 5), (np.float64, True, 32), (np.float64, False, 0)):
        keys = mixed_keys(n, dtype, rng)
        keys[rng.integers(0, n, n // 4)] = keys[0]  # ties
        values = columns(n, m, rng)
        with warnings.catch_warnings():
            warnings.simplefilter("error")  # bins + 1 > N: empty slices are nan, silently
            got = ev.even_bins(keys, values, bins, descending=descending)
        want = wr.even_bins(keys, values, bins, descending)
        check_bins(got, want, dtype)
        assert got.counts.shape == (m, bins)
    if bins + 1 > n:
        empty = got.stop == got.start
        assert empty.any()


def test_even_bins_with_empty_slices():
    from knn_for_homology_amd import evaluation as ev
    keys = np.array([3.0, 1.0, 2.0], np.float32)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        got = ev.even_bins(keys, [np.array([1, 0, 1], bool)], 7)
    check_bins(got, wr.even_bins(keys, [np.array([1, 0, 1], bool)], 7), np.float32)
    empty = got.stop == got.start
    assert empty.any() and (got.counts[0, empty] == 0).all() and np.isnan(got.mean[0, empty]).all() and np.isnan(got.stderr[0, empty]).all()


def test_edge_bins():
    from knn_for_homology_amd import evaluation as ev
    rng = np.random.default_rng(17)
    lengths = rng.permutation(np.arange(1, 401))  # the reference's edges on integer lengths 1 .. 400
    cols = columns(400, 5, rng)
    got = ev.edge_bins(lengths, cols, np.arange(0, 300, 50))
    check_bins(got, wr.edge_bins(lengths, cols, np.arange(0, 300, 50)), np.float64)
    assert (got.stop - got.start).tolist() == [49, 50, 50, 50, 50, 151] and got.key_hi[-1] == np.inf
    for dtype in (np.float32, np.float64):
        tiny = np.finfo(dtype).smallest_subnormal
        keys = rng.choice(np.array([-2.0, -0.0, 0.0, tiny, 0.5, 0.5, 3.0, np.nan, np.inf], dtype), 900)  # NaN keys fall in no bin
        cols = columns(900, 32, rng)
        for edges in ([0.5], [0.0, 0.5, 3.0],     # an edge equal to a tied key; -0.0 keys are >= the edge 0.0
                      [-0.0, tiny, 2 * tiny],     # the edge -0.0 is the edge 0.0; sub-normal edges
                      [-5.0, 0.25], [-1e30],      # an edge below every key
                      [1.0, 1e30], [1e30],        # an edge above every finite key: the last bin holds the infinities only
                      [0.5, 0.5, 0.5]):           # equal edges: empty bins
            with warnings.catch_warnings():
                warnings.simplefilter("error")
                got = ev.edge_bins(keys, cols, edges)
            check_bins(got, wr.edge_bins(keys, cols, edges), dtype)
        assert got.stop[-1] == np.count_nonzero(~np.isnan(keys))
        # an edge above every key: the search runs to the end of the non-NaN keys -- the first NaN, or N without one -- and the
        # last bin starts and stops there, empty: count 0, mean and stderr nan, silently
        for with_nan in (True, False):
            pool = [-2.0, -0.0, 0.0, tiny, 0.5, 0.5, 3.0] + ([np.nan] if with_nan else [])
            keys = rng.choice(np.array(pool, dtype), 900)
            assert np.isnan(keys).any() == with_nan and np.nanmax(keys) == 3.0
            end = np.count_nonzero(~np.isnan(keys))
            for edges in ([4.0], [0.5, 1e30], [3.0, np.nextafter(dtype(3.0), dtype(4.0))], [5.0, 6.0]):
                with warnings.catch_warnings():
                    warnings.simplefilter("error")
                    got = ev.edge_bins(keys, cols, edges)
                check_bins(got, wr.edge_bins(keys, cols, edges), dtype)
                assert got.start[-1] == got.stop[-1] == end and (end == 900) == (not with_nan)
                assert (got.counts[:, -1] == 0).all() and np.isnan(got.mean[:, -1]).all() and np.isnan(got.stderr[:, -1]).all()


def test_bins_through_the_c_entry():
    rng = np.random.default_rng(19)
    n = 700
    keys = mixed_keys(n, np.float64, rng)
    cols = columns(n, 5, rng)
    starts, stops = np.array([0, 0, 5, 699, 700, 350]), np.array([0, 700, 6, 700, 700, 351])
    rc, a = c_windows(keys, cols, 0, 1, starts=starts, stops=stops)
    assert rc == 0
    C, o = wr.running_counts(keys, cols, True)
    assert np.array_equal(a["order"], o) and np.array_equal(a["start"], starts) and np.array_equal(a["stop"], stops)
    assert np.array_equal(a["counts"], wr.counts_in(C, starts, stops))
    assert same_bits(a["key_lo"], keys[o[np.minimum(starts, n - 1)]]) and same_bits(a["key_hi"], keys[o[np.minimum(stops, n - 1)]])
    assert (a["key_means"] == SF).all()
    # a window and bins in one call
    rc, a = c_windows(keys, cols, 33, 0, edges=[-1.0, 0.0, 1.0])
    want = wr.edge_bins(keys, cols, [-1.0, 0.0, 1.0])
    assert rc == 0 and np.array_equal(a["counts"], want["counts"]) and np.array_equal(a["stop"], want["stop"])
    assert same_bits(a["key_means"], wr.key_means(keys, 33))


def test_invalid_arguments_leave_the_outputs_untouched():
    keys = np.arange(10, dtype=np.float32)
    vals = np.ones((2, 10), np.uint8)
    e = np.array([1.0, 2.0], np.float32)
    s, t = np.array([0, 2], np.int64), np.array([2, 10], np.int64)
    bad = [dict(window=2, over=dict(key_type=2)), dict(window=2, over=dict(n=0)), dict(window=2, over=dict(n=2 ** 31)), dict(window=2, over=dict(m=33)),
           dict(window=2, over=dict(m=-1)), dict(window=11), dict(window=-1), dict(window=0), dict(window=2, over=dict(keys=None)),
           dict(window=2, over=dict(values=None)), dict(window=2, over=dict(key_means=None)), dict(window=2, over=dict(value_means=None)),
           dict(window=2, over=dict(nbins=-1)), dict(window=2, over=dict(nbins=2 ** 20 + 1)), dict(window=2, over=dict(starts=s)), dict(window=2, over=dict(edges=e)),
           dict(edges=e, over=dict(start=None)), dict(edges=e, over=dict(counts=None)), dict(edges=e, over=dict(key_hi=None)), dict(edges=e, descending=1),
           dict(edges=e, over=dict(starts=s)), dict(starts=s, stops=t, over=dict(stops=None)), dict(edges=np.array([2.0, 1.0], np.float32)),
           dict(edges=np.array([1.0, np.inf], np.float32)), dict(edges=np.array([np.nan], np.float32)), dict(starts=[-1, 2], stops=[2, 10]),
           dict(starts=[3, 2], stops=[2, 10]), dict(starts=[0, 2], stops=[2, 11])]
    for case in bad:
        rc, a = c_windows(keys, vals, **case)
        assert rc == KNN_ERR_INVALID, case
        assert untouched(a), case
    rc, a = c_windows(keys, vals, 2)  # and the call the cases were cut from is a good one
    assert rc == 0 and not untouched(a)


def test_value_errors_of_the_public_functions():
    from knn_for_homology_amd import evaluation as ev
    k, v = np.zeros(10, np.float32), np.zeros((2, 10), bool)
    for bad in (lambda: ev.rolling_means(k, v, window=0), lambda: ev.rolling_means(k, v, window=11), lambda: ev.even_bins(k, v, 0),
                lambda: ev.rolling_means(k, v[:, :9], window=2), lambda: ev.rolling_means(k, np.zeros((33, 10), bool), window=2),
                lambda: ev.edge_bins(k, v, [0.0, 2.0, 1.0]), lambda: ev.edge_bins(k, v, [0.0, np.inf]), lambda: ev.edge_bins(k, v, []),
                lambda: ev.rolling_means(np.array([1, 2 ** 53], np.int64), None, window=1)):
        with pytest.raises(ValueError):
            bad()
    assert ev.rolling_means(k, v, window=10).values.shape == (2, 1)  # the functions do run here
