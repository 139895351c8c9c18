"""No GPU: tests/correlation_reference.py, the restatement the correlation kernels are held to bit for bit, against scipy's
own results on the reference's statements (tests/golden/reference_correlation.npz, written by make_correlation_golden.py
from cath/cath.py:949-952 and scipy.stats.rankdata), and the host-side functions of evaluation.py that need no device."""
import math
from pathlib import Path

import numpy as np
import pytest

import correlation_reference as ref
from knn_for_homology_amd import evaluation

GOLDEN = Path(__file__).resolve().parent / "golden" / "reference_correlation.npz"

# max |restatement - scipy| over the fixture's five cases, measured on the build machine (numpy 2.2.6, scipy 1.15.3):
# Pearson 1.11e-16 (case "cath"), Spearman 1.73e-18 (case "f64_f32").  Four times that, for another BLAS's or numpy's
# summation order inside scipy, is 4.4e-16: below the floor of 2^-50, which therefore is the bound.
STATISTIC_BOUND = max(4 * 1.11e-16, 2.0 ** -50)
# the p-value function against scipy's p-values, the same way: max |difference| 4.05e-15 (case "inf", p = 0.26).  scipy
# evaluates Pearson's p through its beta distribution object, not through betainc directly, so the small p-values differ
# relatively: at most 1.42e-13 (case "cath", p = 1.4e-47), which an absolute bound cannot see; both are asserted.
PVALUE_BOUND = max(4 * 4.05e-15, 2.0 ** -50)
PVALUE_RELATIVE_BOUND = 4 * 1.42e-13


@pytest.fixture(scope="module")
def golden():
    g = np.load(GOLDEN)
    return {name: {key: g[f"{name}_{key}"] for key in ("x", "y", "logged", "rank_x", "rank_y", "pearson", "spearman")} for name in g["cases"]}


def test_fixture_covers_what_it_is_for(golden):
    assert sum(c["x"].size for c in golden.values()) < 10000
    assert golden["cath"]["x"].dtype == np.float32 and golden["cath"]["y"].dtype == np.float64
    assert golden["f64_f32"]["x"].dtype == np.float64 and golden["f64_f32"]["y"].dtype == np.float32
    assert (golden["cath"]["y"] == 0).any() and (golden["cath"]["logged"] == -1e9).any()
    assert len(np.unique(golden["cath"]["x"])) < golden["cath"]["x"].size
    t = golden["ties"]
    assert t["x"].ndim == 2 and (t["x"][7] == t["x"][3]).all() and (t["y"][8] == t["y"][3]).all()
    zeros = t["x"][t["x"] == 0]
    assert np.signbit(zeros).any() and not np.signbit(zeros).all()
    assert np.isposinf(golden["inf"]["y"]).sum() == 1
    assert len(np.unique(golden["distinct"]["x"])) == 65 == len(np.unique(golden["distinct"]["y"]))


def test_ranks_are_scipys_bit_for_bit(golden):
    for name, c in golden.items():
        for which in ("x", "y"):
            rank2, nans = ref.doubled_ranks(ref.cells(c[which]))
            assert nans == 0
            assert rank2.min() >= 2 and rank2.max() <= 2 * rank2.size
            assert np.array_equal(rank2 / 2, c[f"rank_{which}"]), (name, which)


def test_ranks_against_scipy_on_fresh_draws():
    stats = pytest.importorskip("scipy.stats")
    rng = np.random.default_rng(5)
    for n, dtype in ((2, np.float32), (3, np.float64), (64, np.float32), (2049, np.float64), (5000, np.float32)):
        v = np.round(rng.normal(0, 1, n), 1).astype(dtype)
        v[rng.integers(0, n)] = -0.0
        v[rng.integers(0, n)] = np.inf
        v[rng.integers(0, n)] = -np.inf
        assert np.array_equal(ref.doubled_ranks(v)[0] / 2, stats.rankdata(v, "average"))


def test_statistics_agree_with_scipy_within_the_measured_bound(golden):
    for name, c in golden.items():
        r, rho = ref.pearson(c["x"], c["logged"]), ref.spearman(c["x"], c["y"])
        print(name, "pearson", abs(r - c["pearson"][0]), "spearman", abs(rho - c["spearman"][0]))
        assert abs(r - c["pearson"][0]) <= STATISTIC_BOUND, name
        assert abs(rho - c["spearman"][0]) <= STATISTIC_BOUND, name
        # ranks do not change under the reference's monotone map: one call on (scores, logged) serves both statements
        # (not with a +inf E-value, which the reference's isinf moves to -1e9 as well)
        if np.isfinite(c["y"]).all():
            assert ref.spearman(c["x"], c["logged"]) == rho


def test_pvalues_agree_with_scipy_within_the_measured_bound(golden):
    pytest.importorskip("scipy.special")
    for name, c in golden.items():
        n = c["x"].size
        p = evaluation.correlation_pvalue("pearson", ref.pearson(c["x"], c["logged"]), n)
        q = evaluation.correlation_pvalue("spearman", ref.spearman(c["x"], c["y"]), n)
        print(name, "pearson p", abs(p - c["pearson"][1]), "spearman p", abs(q - c["spearman"][1]))
        for mine, theirs in ((p, c["pearson"][1]), (q, c["spearman"][1])):
            assert abs(mine - theirs) <= PVALUE_BOUND, name
            assert abs(mine - theirs) <= PVALUE_RELATIVE_BOUND * theirs, name
    assert evaluation.correlation_pvalue("pearson", 1.0, 2) == 1.0
    assert evaluation.correlation_pvalue("spearman", 1.0, 10) == 0.0
    assert math.isnan(evaluation.correlation_pvalue("pearson", math.nan, 10))
    assert math.isnan(evaluation.correlation_pvalue("spearman", math.nan, 10))
    with pytest.raises(ValueError):
        evaluation.correlation_pvalue("kendall", 0.5, 10)


def test_the_facades_statistics_are_the_restatements(golden):
    for c in golden.values():
        x, y = ref.cells(c["x"]), ref.cells(c["logged"])
        m = ref.pearson_moments(x, y)
        assert evaluation.pearson_statistic(m) == ref.ratio(m[3], m[2], m[4])
        sums = ref.spearman_sums_fast(ref.doubled_ranks(x)[0], ref.doubled_ranks(y)[0])
        assert evaluation.spearman_statistic(*sums) == ref.spearman_ratio(*sums)
        for s in sums:
            assert evaluation._wide_sum(*ref.words(s)) == s
    assert evaluation._wide_sum(*ref.words(-(3 << 70))) == -(3 << 70)


def test_exact_sums_two_ways(golden):
    c = golden["cath"]
    rx, ry = ref.doubled_ranks(ref.cells(c["x"]))[0], ref.doubled_ranks(ref.cells(c["y"]))[0]
    assert ref.spearman_sums(rx, ry) == ref.spearman_sums_fast(rx, ry)
    n = rx.size
    assert int(rx.sum()) == n * (n + 1) == int(ry.sum())  # the doubled ranks always add up to N (N + 1)


def test_ordered_sum_is_a_sum_and_its_order_is_fixed():
    rng = np.random.default_rng(11)
    for n in (1, 2, 255, 256, 257, 2047, 2048, 2049, 5000, 2048 * 2048 + 1):
        v = rng.normal(0, 1, n)
        s = ref.ordered_sum(v)
        assert abs(s - math.fsum(v)) <= 1e-12 * max(1.0, math.fsum(np.abs(v)))
        assert ref.ordered_sum(v.copy()) == s
    assert ref.levels(2) == [2, 1] and ref.levels(2048) == [2048, 1] and ref.levels(2049) == [2049, 2, 1]
    assert ref.levels(2 ** 31 - 1) == [2 ** 31 - 1, 2 ** 20, 512, 1]
    # a lane starts from +0.0: a sum of -0.0 alone is +0.0
    assert not np.signbit(ref.ordered_sum(np.full(3, -0.0)))


def test_nan_constant_and_infinite_input():
    x = np.array([0.1, 0.5, 0.3, 0.9], np.float32)
    y = np.array([3.0, 1.0, 2.0, 0.5])
    assert ref.spearman(x, y) == -1.0 and ref.spearman(x, -y) == 1.0
    withnan = y.copy()
    withnan[-1] = np.nan
    assert math.isnan(ref.spearman(x, withnan)) and math.isnan(ref.pearson(x, withnan))
    assert ref.doubled_ranks(withnan)[1] == 1
    const = np.full(4, 0.25)
    assert math.isnan(ref.spearman(x, const)) and math.isnan(ref.pearson(x, const))
    assert (ref.doubled_ranks(const)[0] == 5).all()  # one run of four: ranks 0 .. 3, 0 + 3 + 2
    inf = y.copy()
    inf[0] = np.inf
    assert math.isnan(ref.pearson(x, inf)) and ref.spearman(x, inf) == ref.spearman(x, y)
    zeros = np.array([0.0, -0.0, 1.0, -1.0], np.float32)
    assert list(ref.doubled_ranks(zeros)[0]) == [5, 5, 8, 2]


def test_fewer_than_two_values_raise_as_scipy_does():
    for fn in (evaluation.pearsonr, evaluation.spearmanr, evaluation.correlations):
        with pytest.raises(ValueError, match="two values"):
            fn(np.ones(1, np.float32), np.ones(1))
        with pytest.raises(ValueError, match="same shape"):
            fn(np.ones(3, np.float32), np.ones(4))
        with pytest.raises(ValueError, match="limit"):
            fn(np.ones((3, 2), np.float32), np.ones((3, 2)), limit=3)
    with pytest.raises(ValueError, match="two values"):
        evaluation.rankdata(np.ones((1, 4)), limit=1)
