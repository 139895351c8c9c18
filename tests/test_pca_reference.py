"""CPU: tests/pca_reference.py (the restatement the GPU tests compare knn_pca_moments / knn_pca_project and
decomposition.PCA with) against tests/golden/reference_pca.npz, what the reference's own PCA statements
(pfam/reverse_evaluate.py:34-36, 100-101) produced under sklearn (tests/golden/make_pca_golden.py).

sklearn and the restatement are both fp32 pipelines with different summation orders, so neither is the other's truth:
both are measured against the float64 truth stored in the fixture (float64 centring, eigh, the same sign rule).  The
transform is measured relative to max |Y_truth|, components_ and the three variance vectors relative to their own
maximum.  The tolerance is not fixed in advance: per kind (transform, components, the variance vectors), the
restatement's deviation must not exceed 8 x the largest deviation of sklearn's own two fits over all cases.  8 x leaves
room for two fp32 pipelines of which either can be about twice the other, and admits no wrong sign, swapped component or
uncentred covariance: those are errors of order 1.

Measured when the fixture was made (sklearn 1.7.2, numpy 2.2.6; largest over the cases): sklearn transform 1.1e-6,
components 7.7e-7, variances 4.0e-7; the restatement 8.0e-7, 3.5e-7, 6.5e-8; the restatement on the input with 1000
added to every entry 4.2e-7, 3.7e-7, 1.4e-7.  The fixture stores every figure (`*_dev_*`)."""
import numpy as np
import pytest

import pca_reference as ref


@pytest.fixture(scope="module")
def golden():
    return ref.load_golden()


case_arrays, case_input, sklearn_bound = ref.case_arrays, ref.case_input, ref.sklearn_bound


@pytest.fixture(scope="module")
def restated(golden):
    """(n, d) -> the restatement's fit of the case, computed once"""
    return {(n, d): ref.fit_reference(case_input(golden, n, d), 2) for n, d in ref.CASES}


def test_fixture_is_what_the_issue_asks_for(golden):
    assert [tuple(c) for c in golden["cases"]] == list(ref.CASES) == [(300, 64), (3000, 128), (700, 1024), (3000, 1024)]
    for n, d in ref.CASES:
        assert float(golden[f"{ref.case_name(n, d)}_gap"]) >= 4
        assert (str(golden[f"{ref.case_name(n, d)}_solver"]) == "randomized") == (d > 1000)
    # the reason two fits are stored: above 1000 columns they differ
    a, b = case_arrays(golden, 3000, 1024, "fit1"), case_arrays(golden, 3000, 1024, "fit2")
    assert not np.array_equal(a["transform"], b["transform"])
    bound = sklearn_bound(golden)
    print("bound per kind:", bound)
    assert all(0 < v < 1e-4 for v in bound.values()), bound  # (sklearn itself is an fp32 pipeline, not a wrong one)


@pytest.mark.parametrize("n,d", ref.CASES)
def test_restatement_within_the_reference_s_own_error(golden, restated, n, d):
    bound = sklearn_bound(golden)
    dev = ref.deviations(restated[(n, d)], case_arrays(golden, n, d, "truth"))
    print(ref.case_name(n, d), "restated:", dev, "bound:", bound)
    # the fixture's record of the same figures (eigh and the oracle's chains are deterministic; the BLAS behind numpy's
    # matmul in the truth is not a party here: the truth is stored)
    stored = dict(zip(ref.QUANTITIES, golden[f"{ref.case_name(n, d)}_dev_restated"]))
    for q in ref.QUANTITIES:
        assert dev[q] == pytest.approx(stored[q], rel=0.5, abs=1e-9), q
    for kind, v in ref.pooled(dev).items():
        assert v <= bound[kind], (kind, v, bound[kind])


def test_offset_input_stays_within_the_bound(golden):
    """1000 added to every entry: the rows are centred before any product is formed, so the covariance does not lose the
    digits the offset takes"""
    n, d = ref.OFFSET_CASE
    X = case_input(golden, n, d) + np.float32(1000.0)
    assert X.dtype == np.float32
    assert np.array_equal(ref.input_digest(X), golden[f"{ref.case_name(n, d)}_offset_digest"])
    dev = ref.deviations(ref.fit_reference(X, 2), case_arrays(golden, n, d, "offset_truth"))
    bound = sklearn_bound(golden)
    print("offset, restated:", dev, "bound:", bound)
    for kind, v in ref.pooled(dev).items():
        assert v <= bound[kind], (kind, v, bound[kind])


def test_group_rule():
    assert ref.group_rows(2) == 4096 and ref.group_rows(4096 * 256) == 4096
    assert ref.group_rows(4096 * 256 + 1) == 8192 and ref.group_rows(1048581) == 8192
    assert len(ref._groups(1048581)) == 129 and len(ref._groups(4099)) == 2 and ref._groups(4099)[1] == (4096, 4099)
    assert len(ref._groups(8192)) == 2 and len(ref._groups(4096 * 256 * 3)) == 256


def test_chain_layout_walks_rows_first_to_last():
    """the permutation inside blocks of 8: the oracle's dot over the laid-out columns is the ascending chain"""
    rng = np.random.default_rng(3)
    cols = rng.standard_normal((2, 21)).astype(np.float32)
    from oracle import knn_oracle as ko
    laid = ref._ascending_chain_layout(cols)
    got = ko.oracle().pair_distances(laid, laid, np.array([0]), np.array([1]), ko.METRIC_INNER_PRODUCT)[0]
    acc = np.float64(0.0)
    for r in range(21):  # fmaf in float64 arithmetic: the product of two float32 is exact, one rounding to float32
        acc = np.float64(np.float32(np.float64(cols[0, r]) * np.float64(cols[1, r]) + acc))
    assert np.float32(acc) == got
