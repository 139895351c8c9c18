"""No GPU: tests/windows_reference.py, the host restatement of knn_eval_windows' contract, against what the reference's
own statements produced (tests/golden/reference_windows.npz, made by tests/golden/make_windows_golden.py from
rolling_mean, both hist_evenly and the fixed length bins of cath/cath.py).

Orders.  The reference sorts with numpy's default, unstable, sort, the contract with a stable one.  The inputs `evalue`,
`cosine` and `lengths_distinct` are tie-free -- asserted below -- and everything is compared on them.  `evalue_ties` and
`lengths` have many equal keys: on them only quantities that no permutation inside a group of equal keys can change are
compared, the rolling mean of the keys themselves and the fixed-edge bins (masks over the keys, not orders).

Rolling means.  Each side is a sum of at most W terms plus one rounding of 1 / W or one division, so each is within
(W + 2) * 2^-53 * sum|x| / W of the exact mean, and the two within (2 W + 4) * 2^-53 * sum|x| / W of each other.  The
restatement alone is also held to (W + 2) * 2^-53 against math.fsum.

stderr.  The closed form sqrt((c (1 - p)^2 + (n - c) p^2) / n) / sqrt(n) is not numpy's std() / sqrt(n) bit for bit (numpy
sums the squared deviations pairwise).  The largest relative difference over the fixture, under the numpy the fixture
names, is 3.343e-16 (3.3427e-16 rounded up); the test allows eight times that: other bin sizes land on other pairwise trees."""
import math
import warnings
from pathlib import Path

import numpy as np
import pytest

import rank_reference as rr
import windows_reference as wr

GOLDEN = Path(__file__).resolve().parent / "golden" / "reference_windows.npz"
TIE_FREE = ("evalue", "cosine", "lengths_distinct")
TIED = ("evalue_ties", "lengths")
U = 2.0 ** -53
STDERR_MEASURED = 3.343e-16  # the largest relative difference to numpy's std() / sqrt(n) over the fixture (test_stderr prints it)
STDERR_RTOL = 8 * STDERR_MEASURED


@pytest.fixture(scope="module")
def g():
    return np.load(GOLDEN)


def window_abs_sums(x, w):
    """exact (math.fsum) sums of x and of |x| over every window"""
    x = [float(v) for v in x]
    a = [abs(v) for v in x]
    n = len(x) - w + 1
    return np.array([math.fsum(x[i:i + w]) for i in range(n)]), np.array([math.fsum(a[i:i + w]) for i in range(n)])


def test_fixture_is_what_the_docstring_says(g):
    assert set(g["inputs"]) == set(TIE_FREE + TIED)
    for name in TIE_FREE:
        k = g[f"{name}_keys"]
        assert bool(g[f"{name}_tie_free"]) and len(np.unique(k)) == k.size, name
    for name in TIED:
        k = g[f"{name}_keys"]
        assert not bool(g[f"{name}_tie_free"]) and len(np.unique(k)) < k.size - 100, name
    assert (g["evalue_ties_keys"] == 0).sum() >= 5 and g["cosine_keys"].dtype == np.float32 and (g["cosine_keys"] < 0).any()
    assert g["lengths_keys"].dtype.kind == "i" and g["evalue_keys"].dtype == np.float64
    assert g["evalue_columns"].shape == (3, g["evalue_keys"].size) and g["evalue_columns"].dtype == np.bool_
    assert 1000 in g["windows"]


def test_orders_agree_where_the_reference_has_one(g):
    for name in TIE_FREE:
        k = g[f"{name}_keys"]
        assert np.array_equal(rr.order(wr.as_keys(k)), np.argsort(k))
        assert np.array_equal(rr.order(wr.as_keys(k), None, True), np.argsort(-k))


@pytest.mark.parametrize("name", TIE_FREE + TIED)
@pytest.mark.parametrize("descending", [False, True])
def test_rolling_means_within_the_derived_bound(g, name, descending):
    k, cols = g[f"{name}_keys"], g[f"{name}_columns"]
    tag = f"{name}_{'desc' if descending else 'asc'}"
    for w in (int(v) for v in g["windows"]):
        km, vm, o = wr.rolling_means(k, cols, w, descending)
        x = wr.as_keys(k)[o].astype(np.float64)
        exact, abs_sum = window_abs_sums(x, w)
        ref = g[f"{tag}_w{w}_keys"]
        assert km.shape == ref.shape == (k.size - w + 1,)
        assert (np.abs(km - ref) <= (2 * w + 4) * U * abs_sum / w).all(), (tag, w, float(np.abs(km - ref).max()))
        assert (np.abs(km - exact / w) <= (w + 2) * U * abs_sum / w).all(), (tag, w)
        if name in TIE_FREE:
            refc = g[f"{tag}_w{w}_columns"]
            assert vm.shape == refc.shape
            for c in range(3):
                cum = np.concatenate([[0], np.cumsum(cols[c][o], dtype=np.int64)])
                count = (cum[w:] - cum[:-w]).astype(np.float64)  # exact: the set cells of the window
                assert (np.abs(vm[c] - refc[c]) <= (2 * w + 4) * U * count / w).all(), (tag, w, c)
                assert (np.abs(vm[c] - count / w) <= (w + 2) * U * count / w).all(), (tag, w, c)
                assert np.array_equal(rr.bits(vm[c]), rr.bits(count / w))  # in fact the correctly rounded mean


def test_tied_keys_leave_the_key_means_alone(g):
    """the claim behind the comparison on tied inputs: any order among equal keys gives the same ranked key sequence"""
    k = g["lengths_keys"]
    a = k[np.argsort(k)]
    b = k[rr.order(wr.as_keys(k))]
    assert np.array_equal(a, b)


@pytest.mark.parametrize("name", TIE_FREE)
@pytest.mark.parametrize("descending", [False, True])
def test_even_bins_counts_means_and_keys_equal_bits(g, name, descending):
    k, cols = g[f"{name}_keys"], g[f"{name}_columns"]
    tag = f"{name}_{'desc' if descending else 'asc'}"
    worst = 0.0
    for bins in (int(v) for v in g["bins"]):
        b = wr.even_bins(k, cols, bins, descending)
        n = b["stop"] - b["start"]
        assert b["counts"].shape == (3, bins) and (n > 0).all()
        for which in ("cath", "pfam"):
            y, yerr = g[f"{tag}_b{bins}_{which}_y"], g[f"{tag}_b{bins}_{which}_yerr"]
            assert np.array_equal(rr.bits(b["mean"]), rr.bits(y)), (tag, bins, which)
            assert np.array_equal(b["counts"], np.rint(y * n).astype(np.int64))
            rel = np.abs(b["stderr"] - yerr) / yerr
            worst = max(worst, float(rel.max()))
            assert (rel <= STDERR_RTOL).all(), (tag, bins, which, float(rel.max()))
        # the tick labels print the keys at ranks start and stop: the shortest representation that reads back to the same bits
        lo, hi = b["key_lo"], b["key_hi"]
        if k.dtype.kind == "i":
            lo, hi = lo.astype(np.int64), hi.astype(np.int64)
        assert [f"{a}-{z}" for a, z in zip(lo, hi)] == list(g[f"{tag}_b{bins}_cath_ticks"]), (tag, bins)
        assert [f"{a:0.0E} {z:0.0E}" for a, z in zip(lo, hi)] == list(g[f"{tag}_b{bins}_pfam_ticks"]), (tag, bins)
    print(f"{tag}: stderr differs from numpy's by {worst:.3g} at most (relative)")


@pytest.mark.parametrize("name", ["lengths", "lengths_distinct"])
def test_edge_bins_equal_bits(g, name):
    k, cols = g[f"{name}_keys"], g[f"{name}_columns"]
    b = wr.edge_bins(k, cols, g[f"{name}_edges"])
    y, yerr = g[f"{name}_edge_y"], g[f"{name}_edge_yerr"]
    n = b["stop"] - b["start"]
    assert n.sum() == k.size and b["start"][0] == 0
    assert np.array_equal(rr.bits(b["mean"]), rr.bits(y))  # (nan for an empty bin, on both sides)
    filled = n > 0
    diff, ref = np.abs(b["stderr"] - yerr)[:, filled], yerr[:, filled]  # (a column without a set cell in a bin: 0 on both sides)
    print(f"{name}: edge bins' stderr differs from numpy's by {float((diff[ref > 0] / ref[ref > 0]).max()):.3g} at most (relative)")
    assert (diff <= STDERR_RTOL * ref).all()
    assert np.isnan(b["stderr"][:, ~filled]).all() and np.isnan(yerr[:, ~filled]).all()
    for j, (lo, hi) in enumerate(zip(b["key_lo"], b["key_hi"])):
        inside = (k >= lo) & (k < hi)
        assert n[j] == inside.sum() and np.array_equal(b["counts"][:, j], cols[:, inside].sum(axis=1))


def test_stderr_measured_value_is_the_one_written_down(g):
    """the largest relative difference of the closed form to numpy's std() / sqrt(n) over every bin of the fixture; the
    docstring, DESIGN 4.7k and STDERR_MEASURED carry it (valid for the fixture's numpy: major.minor checked)"""
    assert str(g["numpy_version"]).split(".")[:2] == np.__version__.split(".")[:2], "re-measure under this numpy"
    worst = 0.0
    for name in TIE_FREE:
        k, cols = g[f"{name}_keys"], g[f"{name}_columns"]
        for descending in (False, True):
            o = rr.order(wr.as_keys(k), None, descending)
            for bins in (int(v) for v in g["bins"]):
                b = wr.even_bins(k, cols, bins, descending)
                for c in range(3):
                    for j in range(bins):
                        data = cols[c][o][b["start"][j]:b["stop"][j]]
                        ref = data.std() / np.sqrt(len(data))
                        worst = max(worst, abs(b["stderr"][c, j] - ref) / ref)
    print(f"stderr: largest relative difference {worst:.3g}")
    assert worst <= STDERR_MEASURED


def test_empty_bins_are_nan_without_a_warning():
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        b = wr.even_bins(np.array([3.0, 1.0, 2.0]), [np.array([1, 0, 1], bool)], 7)
    n = b["stop"] - b["start"]
    assert (n == 0).any() and np.isnan(b["mean"][0, n == 0]).all() and np.isnan(b["stderr"][0, n == 0]).all()
    assert (b["counts"][0, n == 0] == 0).all()


def test_chains_by_hand():
    x = np.array([1.0, 2.0, 4.0, 8.0, 16.0, 32.0, 64.0])
    P, S = wr.chains(x, 3)  # blocks [1 2 4] [8 16 32] [64]
    assert P.tolist() == [1, 3, 7, 8, 24, 56, 64] and S.tolist() == [7, 6, 4, 56, 48, 32, 64]
    assert wr.key_means(x, 3).tolist() == [7 / 3, 14 / 3, 28 / 3, 56 / 3, 112 / 3]
    # no subtraction: an infinity stays in its own windows, and a leading -0.0 stays -0.0
    y = np.array([-np.inf, 1.0, 2.0, 3.0, np.inf])
    assert wr.key_means(y, 2).tolist() == [-np.inf, 1.5, 2.5, np.inf]
    z = wr.key_means(np.array([-0.0, -0.0, 0.0]), 1)
    assert np.signbit(z).tolist() == [True, True, False]


def test_python_argument_checks_need_no_gpu():
    from knn_for_homology_amd import evaluation as ev
    k, v = np.zeros(10, np.float32), np.zeros((2, 10), bool)
    for bad in (lambda: ev.rolling_means(k, v, window=0), lambda: ev.rolling_means(k, v, window=11), lambda: ev.even_bins(k, v, 0),
                lambda: ev.rolling_means(k, v[:, :9], window=2), lambda: ev.rolling_means(k, [v[0], v[1][:5]], window=2),
                lambda: ev.rolling_means(k, np.zeros((33, 10), bool), window=2), lambda: ev.even_bins(k, [v[0]] * 33, 3),
                lambda: ev.edge_bins(k, v, [0.0, 2.0, 1.0]), lambda: ev.edge_bins(k, v, [0.0, np.inf]), lambda: ev.edge_bins(k, v, [np.nan]),
                lambda: ev.edge_bins(k, v, []), lambda: ev.rolling_means(np.array([1, 2 ** 53], np.int64), None, window=1),
                lambda: ev.rolling_means(np.zeros((2, 2, 2), np.float32), None, window=1), lambda: ev.rolling_means(np.zeros(0, np.float32), None, window=1),
                lambda: ev.rolling_means(k, v.astype(np.float32), window=2)):
        with pytest.raises(ValueError):
            bad()
