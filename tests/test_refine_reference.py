"""CPU: tests/refine_reference.py::ref_refine, the host restatement the GPU refine tests compare against, checked
against a hand-written example (ties included) and against the float64 truth where the candidates are all rows."""
import numpy as np
import pytest

from refine_reference import FLT_MAX, METRIC_INNER_PRODUCT, METRIC_L2, ref_refine

# d = 8, 6 rows of small integers: every product and sum is exact in fp32.  Rows 1 and 4 are equal (an exact tie at any
# query), rows 0 and 5 tie in inner product with q0 but not in L2.
XB = np.array([[1, 0, 0, 0, 0, 0, 0, 0],
               [0, 2, 0, 0, 0, 0, 0, 1],
               [3, 1, 0, 0, 0, 0, 0, 0],
               [0, 0, 0, 0, 0, 0, 0, 0],
               [0, 2, 0, 0, 0, 0, 0, 1],
               [1, 0, 0, 0, 0, 3, 0, 0]], np.float32)
XQ = np.array([[1, 1, 0, 0, 0, 0, 0, 0],
               [0, 0, 0, 0, 0, 1, 0, 2]], np.float32)
# by hand -- inner products: q0 . rows = 1, 2, 4, 0, 2, 1; q1 . rows = 0, 2, 0, 0, 2, 3
#            squared L2: q0: 1, 3, 4, 2, 3, 10; q1: 6, 6, 15, 5, 6, 9


def test_hand_example_inner_product(oracle):
    labels = np.array([[5, 4, 3, 1, 0, 2], [0, 1, 2, 3, 4, 5]], np.int64)  # (the order of the labels does not matter)
    D, I = ref_refine(oracle, XB, XQ, labels, 4, METRIC_INNER_PRODUCT)
    assert I.tolist() == [[2, 1, 4, 0], [5, 1, 4, 0]]  # ties 1/4, 0/5 and 0/2/3: lower id first
    assert D.tolist() == [[4, 2, 2, 1], [3, 2, 2, 0]]
    assert D.dtype == np.float32 and I.dtype == np.int64


def test_hand_example_l2(oracle):
    labels = np.tile(np.arange(6, dtype=np.int64), (2, 1))
    D, I = ref_refine(oracle, XB, XQ, labels, 6, METRIC_L2)
    assert I.tolist() == [[0, 3, 1, 4, 2, 5], [3, 0, 1, 4, 5, 2]]
    assert D.tolist() == [[1, 2, 3, 3, 4, 10], [5, 6, 6, 6, 9, 15]]


def test_hand_example_subsets_padding_and_duplicates(oracle):
    # q0: candidates {4, 2} only, two -1 entries; q1: no candidate at all
    labels = np.array([[-1, 4, -1, 2], [-1, -1, -1, -1]], np.int64)
    D, I = ref_refine(oracle, XB, XQ, labels, 3, METRIC_L2)
    assert I.tolist() == [[4, 2, -1], [-1, -1, -1]]
    assert D[0, :2].tolist() == [3, 4] and (D[0, 2:] == FLT_MAX).all() and (D[1] == FLT_MAX).all()
    D, I = ref_refine(oracle, XB, XQ, labels, 3, METRIC_INNER_PRODUCT)
    assert I.tolist() == [[2, 4, -1], [-1, -1, -1]]
    assert D[0, :2].tolist() == [4, 2] and (D[0, 2:] == -FLT_MAX).all() and (D[1] == -FLT_MAX).all()
    # a label given twice is scored twice and may come back twice
    labels = np.array([[2, 0, 2, 3], [5, 5, 5, 0]], np.int64)
    D, I = ref_refine(oracle, XB, XQ, labels, 3, METRIC_INNER_PRODUCT)
    assert I.tolist() == [[2, 2, 0], [5, 5, 5]]
    assert D.tolist() == [[4, 4, 1], [3, 3, 3]]


@pytest.mark.parametrize("metric", (METRIC_INNER_PRODUCT, METRIC_L2))
@pytest.mark.parametrize("d", (1, 8, 33, 100))
def test_all_rows_against_float64(oracle, ko, metric, d):
    """cand = every row, in a shuffled order: ids are the float64 truth's (integer rows: every fp32 sum is exact, ties
    are exact ties and go to the lower id on both sides) and the scores are its scores"""
    rng = np.random.default_rng(d * 2 + metric)
    nb, nq, k = 200, 7, 50
    xb = rng.integers(-3, 4, (nb, d)).astype(np.float32)
    xq = rng.integers(-3, 4, (nq, d)).astype(np.float32)
    labels = np.stack([rng.permutation(nb) for _ in range(nq)]).astype(np.int64)
    D, I = ref_refine(oracle, xb, xq, labels, k, metric)
    De, Ie = ko.exact_knn_f64(xb, xq, k, metric)
    assert np.array_equal(I, Ie)
    assert np.array_equal(D.astype(np.float64), De)


def test_all_rows_gaussian_against_float64(oracle, ko):
    """float rows: same ids as the float64 truth up to near-ties, scores within fp32 rounding of it"""
    rng = np.random.default_rng(3)
    nb, nq, k, d = 300, 5, 20, 64
    xb = rng.standard_normal((nb, d)).astype(np.float32)
    xq = rng.standard_normal((nq, d)).astype(np.float32)
    labels = np.tile(np.arange(nb, dtype=np.int64), (nq, 1))
    for metric in (METRIC_INNER_PRODUCT, METRIC_L2):
        D, I = ref_refine(oracle, xb, xq, labels, k, metric)
        ko.compare_tie_tolerant(I, D, xb, xq, metric)
