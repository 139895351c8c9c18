"""CPU: tests/buckets_reference.py (the restatement the GPU tests compare knn_eval_bucket_counts and knn_eval_hit_curve
against) against tests/golden/reference_buckets.npz, the arrays the reference's own statements produced
(tests/golden/make_buckets_golden.py: pfam/proteins.py:692-705, 502-507 and 478 under numpy 2.2.6 and scipy 1.15.3).

Counts, precision, the accuracy-over-hits curve (limit >= 2) and the per-query recall are compared bit for bit.  Two
comparisons carry a tolerance, both measured, not assumed:

  sem       the closed form sqrt(c (n - c) / (n (n - 1))) / sqrt(n) against scipy.stats.sem, whose numpy std sums squared
            deviations pairwise.  Largest relative difference measured: 1.12e-15 over the recorded grid (n from 2 to
            3 000 000, rates from 0 to 1, shuffled cells), 3.6e-16 over the fixture's cases.  Asserted at four times the
            larger, 4.5e-15: numpy's pairwise grouping may differ between builds and the closed form has three roundings
            of its own.  Where scipy gives exactly 0 (all cells equal) or NaN (one cell) the closed form gives the same.
  limit = 1 numpy collapses an [nq, 1] array to one dimension and sums it pairwise, the contract sums in row order.
            Measured on the fixture's case (1000 rows): 4.97e-16 relative; asserted at four times that, 2.0e-15.  (The
            a-priori bound for two summation orders of 1000 positive terms, about 1000 ulp, would be far wider.)
"""
from pathlib import Path

import numpy as np
import pytest

import buckets_reference as ref

GOLDEN = Path(__file__).resolve().parent / "golden" / "reference_buckets.npz"
CASES = ["cosine", "tied", "gaps", "edges64", "one"]
SEM_MEASURED = 1.12e-15
SEM_TOLERANCE = 4 * SEM_MEASURED
ONE_MEASURED = 4.97e-16
ONE_TOLERANCE = 4 * ONE_MEASURED


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as g:
        return {key: g[key] for key in g.files}


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def case(golden, name):
    return {key[len(name) + 1:]: value for key, value in golden.items() if key.startswith(name + "_")}


def relative(got, want):
    return float(np.max(np.abs(got - want) / want)) if len(want) else 0.0


def test_fixture_holds_the_cases(golden):
    assert sorted(golden["cases"].tolist()) == sorted(CASES)
    assert GOLDEN.stat().st_size < 100_000


@pytest.mark.parametrize("name", CASES)
def test_counts_and_precision_bit_for_bit(golden, name):
    c = case(golden, name)
    lo, hi = ref.default_edges(int(c["smoothness"]))
    assert np.array_equal(bits(lo), bits(c["score_buckets"]))
    count, right = ref.bucket_counts(c["correct"], c["scores"], int(c["limit"]), lo, hi)
    keep = count > 0
    assert np.array_equal(count[keep], c["nonempty_count"])
    assert np.array_equal(right[keep], c["nonempty_correct"])
    precision, sem = ref.reference_arrays(count, right)
    assert len(precision) == len(c["precision"])
    assert np.array_equal(bits(precision), bits(c["precision"]))
    # sem: NaN and exact zeros where scipy has them, the rest within the measured tolerance
    want = c["sem"]
    assert np.array_equal(np.isnan(sem), np.isnan(want))
    zero = want == 0
    assert np.array_equal(sem[zero], want[zero])
    rest = ~np.isnan(want) & ~zero
    worst = relative(sem[rest], want[rest])
    print(f"{name}: sem at most {worst:.3e} relative from scipy's, allowed {SEM_TOLERANCE:.3e}")
    assert worst <= SEM_TOLERANCE


def test_range_rule_is_the_definition(golden):
    """bucket_counts walks the buckets h .. a - 1 of each cell; here against every cell times every bucket"""
    for name in ("tied", "edges64"):
        c = case(golden, name)
        lo, hi = ref.default_edges(int(c["smoothness"]))
        fast = ref.bucket_counts(c["correct"][:10], c["scores"][:10], int(c["limit"]), lo, hi)
        slow = ref.bucket_counts_bruteforce(c["correct"][:10], c["scores"][:10], int(c["limit"]), lo, hi)
        assert np.array_equal(fast[0], slow[0]) and np.array_equal(fast[1], slow[1])


def test_sem_closed_form_against_the_recorded_grid(golden):
    n, c, want = golden["sem_grid_n"], golden["sem_grid_c"], golden["sem_grid_sem"]
    assert n.min() == 2 and n.max() == 3_000_000 and (c == 0).any() and (c == n).any()
    _, sem = ref.precision_sem(n, c)
    zero = want == 0
    assert np.array_equal(zero, (c == 0) | (c == n))
    assert np.array_equal(sem[zero], want[zero])
    worst = relative(sem[~zero], want[~zero])
    print(f"sem grid: at most {worst:.3e} relative from scipy's, allowed {SEM_TOLERANCE:.3e}")
    assert worst <= SEM_TOLERANCE
    # one cell: scipy returns NaN, and so does the closed form; no cell: NaN as well
    assert np.isnan(ref.precision_sem([1, 0], [1, 0])[1]).all()


@pytest.mark.parametrize("name", CASES)
def test_hit_curve_and_recall(golden, name):
    c = case(golden, name)
    limit, k = int(c["limit"]), c["correct"].shape[1]
    mean, rows, cols = ref.hit_curve(c["correct"], c["totals"], limit)
    want = c["accuracy_over_hit"]
    if limit >= 2:
        assert np.array_equal(bits(mean), bits(want))
    else:
        # limit = 1: numpy sums the single column pairwise, the contract in row order (module docstring)
        worst = relative(mean, want)
        print(f"{name}: limit = 1 curve {worst:.3e} relative from numpy's pairwise mean, allowed {ONE_TOLERANCE:.3e}")
        assert worst <= ONE_TOLERANCE
    assert np.array_equal(rows, c["correct"][:, :limit].sum(axis=1))
    assert np.array_equal(cols, c["correct"][:, :limit].cumsum(axis=1).sum(axis=0))
    # the reference's recall line reads correct[:, :300]: the whole row of these cases
    assert np.array_equal(bits(ref.recall_per_query(c["correct"], c["totals"], k)), bits(c["recall_per_query"]))
    assert (c["totals"] == 1).any() and (c["totals"] > 10 ** 6).any()


def test_default_edges_overlap_and_leave_gaps(golden):
    """At smoothness 300 the upper edge of a bucket and the lower edge of the next differ in the last bit at 90 places; the
    fixture's float64 case sits on those edges, so tidy edges (hi[b] = lo[b + 1]) could not reproduce its counts."""
    c = case(golden, "edges64")
    lo = c["score_buckets"]
    hi = lo + (1 / 300)
    overlap = np.flatnonzero(hi[:-1] > lo[1:])
    gap = np.flatnonzero(hi[:-1] < lo[1:])
    assert len(overlap) >= 1 and len(gap) >= 1
    assert (len(overlap), len(gap)) == (28, 62)
    scores = c["scores"][:, :int(c["limit"])]
    assert any((scores == hi[b]).any() for b in overlap), "no score on an overlapping edge: in two buckets"
    assert any((scores == lo[b + 1]).any() for b in gap), "no score on a gapped edge: in no bucket"
    count, right = ref.bucket_counts(c["correct"], c["scores"], int(c["limit"]), lo, hi)
    tidy = ref.bucket_counts(c["correct"], c["scores"], int(c["limit"]), lo, np.append(lo[1:], hi[-1]))
    assert not np.array_equal(count, tidy[0])
    assert np.array_equal(count[count > 0], c["nonempty_count"])
    # five dyadic values against twelve buckets: one of them sits in a gap between two buckets ("tied")
    t = case(golden, "tied")
    lo12, hi12 = ref.default_edges(12)
    count12, _ = ref.bucket_counts(t["correct"], t["scores"], int(t["limit"]), lo12, hi12)
    assert 0 < count12.sum() < t["scores"][:, :int(t["limit"])].size
    assert np.array_equal(count12[count12 > 0], t["nonempty_count"])


def test_empty_buckets_are_skipped_by_the_reference(golden):
    c = case(golden, "gaps")
    lo, hi = ref.default_edges(int(c["smoothness"]))
    count, right = ref.bucket_counts(c["correct"], c["scores"], int(c["limit"]), lo, hi)
    empty = np.flatnonzero(count == 0)
    filled = np.flatnonzero(count > 0)
    assert len(empty) and filled.min() < empty[(empty > filled.min())].min() < filled.max(), "no empty bucket in the middle"
    assert len(c["precision"]) == len(filled) < len(lo)
