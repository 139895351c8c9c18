"""CPU: tests/hnsw_reference.py, the host reference the exact HNSW tests compare the device beam with, checked on
hand-written graphs of at most 12 nodes: a list with a hole, a self link, a duplicate link, two components, two rows with
identical vectors -- and the output contract's checker against results that break one clause each."""
import numpy as np
import pytest

from hnsw_reference import (FLT_MAX, METRIC_INNER_PRODUCT, METRIC_L2, assert_output_contract, contract_scores, expected,
                            level0_tables, reachable, strongly_connected)

# 12 nodes, 6 slots per list.  Component A = {0, 1, 2, 3, 4, 9}, component B = {5, 6, 7, 8}; nodes 10 and 11 are named only
# BEHIND the hole of node 2's list, so nothing reaches them (they link into A themselves).
LISTS = [
    [1, 0, 1],            # 0: a self link and the same id twice
    [2, 2, 2, 0],         # 1: a duplicate link
    [3, -1, 10, 11],      # 2: a hole, real ids behind it
    [4, 9],               # 3
    [0],                  # 4: closes the cycle 0 1 2 3 4
    [6],                  # 5
    [7, 5],               # 6
    [8],                  # 7
    [5, 8],               # 8: a self link
    [3],                  # 9
    [0, 11],              # 10
    [10],                 # 11
]
A, B = [0, 1, 2, 3, 4, 9], [5, 6, 7, 8]
G = level0_tables(LISTS, 6)

# d = 8, small integers: every product and sum is exact in fp32.  Rows 1 and 4 are identical, so are rows 6 and 7.
X = np.array([[1, 0, 0, 0, 0, 0, 0, 0],
              [0, 2, 0, 0, 0, 0, 0, 1],
              [3, 1, 0, 0, 0, 0, 0, 0],
              [0, 0, 0, 0, 0, 0, 0, 0],
              [0, 2, 0, 0, 0, 0, 0, 1],
              [1, 0, 0, 0, 0, 3, 0, 0],
              [2, 2, 0, 0, 0, 0, 0, 0],
              [2, 2, 0, 0, 0, 0, 0, 0],
              [0, 0, 1, 0, 0, 0, 0, 0],
              [1, 1, 0, 0, 0, 0, 0, 0],
              [5, 5, 0, 0, 0, 0, 0, 0],
              [9, 9, 9, 0, 0, 0, 0, 0]], np.float32)
Q = np.array([[1, 1, 0, 0, 0, 0, 0, 0],
              [0, 0, 0, 0, 0, 1, 0, 2]], np.float32)
# by hand, component A (rows 0 1 2 3 4 9) -- inner products: q0: 1 2 4 0 2 2; q1: 0 2 0 0 2 0
#                                            squared L2:     q0: 1 3 4 2 3 0; q1: 6 6 15 5 6 7


def test_tables_layout():
    levels, offsets, nbrs, cum = G
    assert levels.tolist() == [0] * 12 and offsets.tolist() == list(range(0, 78, 6)) and cum.tolist() == [0, 6]
    assert nbrs.dtype == np.int32 and nbrs.reshape(12, 6)[2].tolist() == [3, -1, 10, 11, -1, -1]


def test_reachable_stops_at_the_hole_and_ignores_self_and_duplicate_links():
    assert reachable(*G, [0]).tolist() == A
    assert reachable(*G, 2).tolist() == A, "10 and 11 sit behind the hole of node 2's list"
    assert reachable(*G, [3]).tolist() == A
    assert reachable(*G, [9]).tolist() == A


def test_reachable_two_components_and_several_entries():
    for e in B:
        assert reachable(*G, [e]).tolist() == B
    assert reachable(*G, [4, 7, 4]).tolist() == sorted(A + B)
    assert reachable(*G, [10]).tolist() == sorted(A + [10, 11]), "10 reaches A, nothing in A reaches 10"
    assert reachable(*G, []).tolist() == []


def test_strongly_connected():
    assert not strongly_connected(*G)
    ring = level0_tables([[(i + 1) % 7] for i in range(7)], 4)
    assert strongly_connected(*ring) and strongly_connected(*ring, None), "a fifth table (assign_probas) is accepted"
    chain = level0_tables([[i + 1] for i in range(6)] + [[]], 4)
    assert not strongly_connected(*chain), "0 reaches all, nothing reaches 0"
    sink = level0_tables([[1], [0], [0]], 4)
    assert not strongly_connected(*sink), "all reach 0, 0 does not reach 2"
    holed = level0_tables([[1, -1, 2], [0], [0]], 4)
    assert not strongly_connected(*holed), "2 is named only behind a hole"
    assert strongly_connected(*level0_tables([[]], 4))


def test_expected_by_hand_inner_product(oracle):
    D, I = expected(X, Q, reachable(*G, [0]), 8, METRIC_INNER_PRODUCT, oracle)
    assert I.tolist() == [[2, 1, 4, 9, 0, 3, -1, -1], [1, 4, 0, 2, 3, 9, -1, -1]], "identical rows 1 and 4: the lower id first"
    assert D[:, :6].tolist() == [[4, 2, 2, 2, 1, 0], [2, 2, 0, 0, 0, 0]]
    assert (D[:, 6:] == -FLT_MAX).all() and D.dtype == np.float32 and I.dtype == np.int64
    assert_output_contract(D, I, X, Q, METRIC_INNER_PRODUCT, 12, oracle)
    # k below the reachable count, and the other component (identical rows 6 and 7)
    D, I = expected(X, Q, reachable(*G, [7]), 3, METRIC_INNER_PRODUCT, oracle)
    assert I.tolist() == [[6, 7, 5], [5, 6, 7]] and D.tolist() == [[4, 4, 1], [3, 0, 0]]


def test_expected_by_hand_l2(oracle):
    D, I = expected(X, Q, reachable(*G, [4]), 7, METRIC_L2, oracle)
    assert I.tolist() == [[9, 0, 3, 1, 4, 2, -1], [3, 0, 1, 4, 9, 2, -1]]
    assert D[:, :6].tolist() == [[0, 1, 2, 3, 3, 4], [5, 6, 6, 6, 7, 15]] and (D[:, 6] == FLT_MAX).all()
    assert_output_contract(D, I, X, Q, METRIC_L2, 12, oracle)


def test_expected_takes_the_reachable_set_in_any_order(oracle):
    a = expected(X, Q, np.array(A), 6, METRIC_L2, oracle)
    b = expected(X, Q, np.array(A[::-1]), 6, METRIC_L2, oracle)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    with pytest.raises(AssertionError):
        expected(X, Q, np.array([1, 1, 2]), 2, METRIC_L2, oracle)
    D, I = expected(X, Q, np.array([], np.int64), 2, METRIC_INNER_PRODUCT, oracle)
    assert (I == -1).all() and (D == -FLT_MAX).all()


def test_l2_scores_are_the_difference_form(oracle):
    """(x - y)^2 summed in one fp32 chain, not |x|^2 + |y|^2 - 2<x, y>: at rows far from the origin the two differ, and
    the pair scores are the flat search's bits under l2_mode=2"""
    rng = np.random.default_rng(5)
    x = (rng.standard_normal((40, 20)) + 30.0).astype(np.float32)
    q = (rng.standard_normal((3, 20)) + 30.0).astype(np.float32)
    D, I = oracle.flat_search(x, q, 40, METRIC_L2, l2_mode=2)
    qidx = np.repeat(np.arange(3), 40)
    got = contract_scores(x, q, qidx, I.reshape(-1), METRIC_L2, oracle)
    assert np.array_equal(got.view(np.uint32), D.reshape(-1).view(np.uint32))
    norm_form = oracle.pair_distances(x, q, qidx, I.reshape(-1), METRIC_L2)
    assert (norm_form != got).any(), "the shape should tell the two formulas apart"
    truth = ((q[qidx].astype(np.float64) - x[I.reshape(-1)].astype(np.float64)) ** 2).sum(1)
    assert np.allclose(got, truth, rtol=1e-5)
    # and the inner product: the flat search's bits, a zero included (it comes back as -0.0)
    D, I = oracle.flat_search(X, Q, 12, METRIC_INNER_PRODUCT)
    got = contract_scores(X, Q, np.repeat(np.arange(2), 12), I.reshape(-1), METRIC_INNER_PRODUCT, oracle)
    assert np.array_equal(got.view(np.uint32), D.reshape(-1).view(np.uint32))


@pytest.mark.parametrize("metric", (METRIC_INNER_PRODUCT, METRIC_L2))
def test_the_contract_checker_rejects_each_violation(oracle, metric):
    D, I = expected(X, Q, reachable(*G, [0]), 8, metric, oracle)
    assert_output_contract(D, I, X, Q, metric, 12, oracle)

    def broken(edit):
        d, i = D.copy(), I.copy()
        edit(d, i)
        with pytest.raises(AssertionError):
            assert_output_contract(d, i, X, Q, metric, 12, oracle)

    def swap(j0, j1):
        def edit(d, i):
            d[0, [j0, j1]] = d[0, [j1, j0]]
            i[0, [j0, j1]] = i[0, [j1, j0]]
        return edit

    tie = [j for j in range(5) if D[0, j] == D[0, j + 1]][0]
    broken(swap(tie, tie + 1))                                    # equal scores, the higher id first
    broken(swap(0, 5))                                            # scores out of order
    broken(lambda d, i: i.__setitem__((0, 0), 12))                # an id outside [0, n)
    broken(lambda d, i: i.__setitem__((0, 0), -2))
    broken(lambda d, i: i.__setitem__((1, 2), -1))                # a -1 in the middle of a row
    broken(lambda d, i: d.__setitem__((1, 7), 0.0))               # a -1 slot without the pad score
    broken(lambda d, i: (i.__setitem__((0, 1), i[0, 0]), d.__setitem__((0, 1), d[0, 0])))  # an id twice, with its own score
    broken(lambda d, i: d.__setitem__((0, 0), np.nextafter(d[0, 0], np.float32(100.0))))  # one bit off
    # a wrong id paired with a wrong score: row 5 (not reachable) with the score of the row it replaces
    broken(lambda d, i: i.__setitem__((0, 0), 5))
