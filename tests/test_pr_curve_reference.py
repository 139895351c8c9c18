"""CPU: tests/pr_curve_reference.py (the restatement the GPU tests compare knn_eval_sets_matrix and knn_eval_pr_curve
with) against tests/golden/reference_pr_curve.npz, the arrays the reference's own compute_correctness_array and
precision-recall loop (pfam/proteins.py:201-207, 626-648) produced (tests/golden/make_pr_curve_golden.py).

The matrices and the integer outputs are compared exactly.  The reference takes its means with numpy.mean (a pairwise
sum), the contract in blocks of 256 rows: two summation orders of nq non-negative doubles, each term at most
max(1, limit / totals.min()), differ by at most 2 * nq * 2**-53 * that size after the division by nq -- nothing
measured.  The block order itself is checked on a hand-worked case in which the orders differ."""
from pathlib import Path

import numpy as np
import pytest

import pr_curve_reference as ref

GOLDEN = Path(__file__).resolve().parent / "golden" / "reference_pr_curve.npz"
CASES = ["small", "wide", "tied", "evalues"]


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as f:
        return {name: f[name] for name in f.files}


@pytest.fixture(scope="module")
def restated(golden):
    """name -> the restatement's five outputs at the reference's thresholds, computed once"""
    out = {}
    for name in CASES:
        g = {key[len(name) + 1:]: golden[key] for key in golden if key.startswith(name + "_")}
        out[name] = (g, ref.pr_curve(g["correct"], g["scores"], int(g["limit"]), g["totals"], g["thresholds"]))
    return out


def mean_bound(nq, limit, totals):
    return 2 * nq * 2.0 ** -53 * max(1.0, limit / int(np.min(totals)))


def test_fixture_holds_the_cases_of_the_issue(golden):
    assert sorted(golden["cases"].tolist()) == sorted(CASES)
    shapes = {name: (golden[f"{name}_scores"].shape, int(golden[f"{name}_limit"]), int(golden[f"{name}_smoothness"])) for name in CASES}
    assert shapes["small"] == ((37, 12), 7, 10) and shapes["wide"] == ((300, 20), 20, 16) and shapes["tied"][0] == (600, 9)
    thr = golden["tied_thresholds"]
    assert (np.diff(thr) == 0).any(), "tied quantiles: equal thresholds"
    lim = int(golden["tied_limit"])
    assert (golden["tied_scores"][:, :lim] <= thr[0]).all(axis=1).sum() > 10, "rows entirely at or below the lowest threshold"
    assert (golden["evalues_scores"][:, -1] == -1e6).all() and (golden["evalues_scores"][:, 0] > -1).all()
    for name in CASES:
        assert golden[f"{name}_scores"].dtype == np.float32 and golden[f"{name}_thresholds"].dtype == np.float64
        assert (np.diff(golden[f"{name}_thresholds"]) >= 0).all() and (golden[f"{name}_totals"] >= 1).all()
        assert len(golden[f"{name}_thresholds"]) == int(golden[f"{name}_smoothness"]) + 1


@pytest.mark.parametrize("name", CASES)
def test_sets_matrix_equals_the_reference(golden, name):
    got = ref.sets_matrix(golden[f"{name}_hits"], golden[f"{name}_set_offsets"], golden[f"{name}_set_members"])
    want = golden[f"{name}_correct"]
    assert want.dtype == bool and 0.1 < want.mean() < 0.9
    assert np.array_equal(got, want.astype(np.uint8))
    # the totals the reference derives from the same sets
    assert np.array_equal(np.diff(golden[f"{name}_set_offsets"]), golden[f"{name}_totals"])


@pytest.mark.parametrize("name", CASES)
def test_means_within_the_bound_of_two_summation_orders(restated, name):
    g, (precision, recall, _, _, _) = restated[name]
    nq = g["scores"].shape[0]
    bound = mean_bound(nq, int(g["limit"]), g["totals"])
    dp = np.abs(precision - g["precision"]).max()
    dr = np.abs(recall - g["recall"]).max()
    print(f"{name}: |precision - reference| <= {dp:.3e}, |recall - reference| <= {dr:.3e}, bound {bound:.3e}")
    assert dp <= bound and dr <= bound
    assert g["precision"][-1] == 1.0 and g["recall"][-1] == 0.0  # the last threshold is the maximum: nothing is above it


@pytest.mark.parametrize("name", CASES)
def test_integer_outputs_equal_a_direct_count(restated, name):
    g, (_, _, selected, tp, empty) = restated[name]
    limit = int(g["limit"])
    above = g["scores"][:, :limit, None] > g["thresholds"]  # float32 against float64: compared in double
    assert np.array_equal(selected, above.sum(axis=(0, 1)))
    assert np.array_equal(tp, (above & g["correct"][:, :limit, None]).sum(axis=(0, 1)))
    assert np.array_equal(empty, (above.sum(axis=1) == 0).sum(axis=0))
    assert selected[0] > 0 and selected[-1] == 0 and empty[-1] == g["scores"].shape[0]


def test_block_order_by_hand():
    correct, scores, totals, terms = ref.three_block_case()
    assert len(terms) == 513
    running = 0.0
    for x in terms:
        running += x
    assert running == 1.0
    assert ref.block_order_sum(terms) == 1.0 + 2.0 ** -51
    assert ref.block_order_sum(terms[:256]) == 1.0 and ref.block_order_sum(terms[256:512]) == 2.0 ** -52
    precision, recall, selected, tp, empty = ref.pr_curve(correct, scores, 1, totals, [0.0])
    assert recall[0] == (1.0 + 2.0 ** -51) / 513.0 and recall[0] != 1.0 / 513.0
    assert precision[0] == 259.0 / 513.0 and (selected[0], tp[0], empty[0]) == (513, 259, 0)


def test_strictness_nan_and_no_prediction():
    scores = np.array([[0.5, 0.25, np.nan, np.inf], [-np.inf, -np.inf, -np.inf, -np.inf]], np.float32)
    correct = np.array([[1, 0, 1, 1], [1, 1, 1, 1]], np.uint8)
    thr = [-np.inf, 0.25, 0.25, 0.5, np.inf]
    precision, recall, selected, tp, empty = ref.pr_curve(correct, scores, 4, [4, 2], thr)
    # row 0: > -inf: 0.5, 0.25, inf (NaN never); > 0.25: 0.5, inf; > 0.5: inf; > inf: nothing.  Row 1: nothing, ever
    assert selected.tolist() == [3, 2, 2, 1, 0] and tp.tolist() == [2, 2, 2, 1, 0] and empty.tolist() == [1, 1, 1, 1, 2]
    assert precision.tolist() == [(2 / 3 + 1) / 2, 1.0, 1.0, 1.0, 1.0]
    assert recall.tolist() == [0.25, 0.25, 0.25, 0.125, 0.0]
    # limit cuts the columns: the infinity is not read
    assert ref.pr_curve(correct, scores, 2, [4, 2], thr)[2].tolist() == [2, 1, 1, 0, 0]
