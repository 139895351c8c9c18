"""CPU: tests/hnsw_reference.py, the host reference the exact HNSW tests compare the device beam with, checked on
hand-written graphs of at most 12 nodes: a list with a hole, a self link, a duplicate link, two components, two rows with
identical vectors -- and the output contract's checker against results that break one clause each.

The entry rules (tables, descend, coarse_entries, margins) are checked on hand-made three-level graphs whose answers are
written out, and every case of tests/test_hnsw_entry_exact_gpu.py (tests/hnsw_entry_cases.py) is shown to tell the right
entry rule from each wrong one on its own inputs."""
import numpy as np
import pytest

import hnsw_entry_cases as cases
import hnsw_reference as ref
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


# ---- the entry rules: tables, descend, coarse_entries, margins ------------------------------------------------------
def test_tables_by_hand_M4():
    """cum = [0, 8, 12, 16]: node 0 (top level 1) owns 12 slots, node 1 (level 0) 8, node 2 (level 2) 16"""
    levels, offsets, nbrs = ref.tables([1, 0, 2], [[[1, 2], [2]], [[0]], [[0, -1, 1], [0], []]], 4)
    e = -1
    assert levels.dtype == np.int32 and offsets.dtype == np.int64 and nbrs.dtype == np.int32
    assert levels.tolist() == [1, 0, 2] and offsets.tolist() == [0, 12, 20, 36]
    assert nbrs.tolist() == [1, 2, e, e, e, e, e, e, 2, e, e, e,
                             0, e, e, e, e, e, e, e,
                             0, e, 1, e, e, e, e, e, 0, e, e, e, e, e, e, e]
    # level 0 is read through the per-node offsets; the id behind the hole of node 2's list is not reached
    cum = np.array([0, 8], np.int32)
    assert reachable(levels, offsets, nbrs, cum, [2]).tolist() == [0, 1, 2]
    assert reachable(levels, offsets, nbrs, cum, [1]).tolist() == [0, 1, 2]
    assert ref.entry_reach(offsets, nbrs, 4, [2]).tolist() == [0, 1, 2]
    assert ref._list(offsets, nbrs, 4, 2, 0).tolist() == [0] and ref._list(offsets, nbrs, 4, 2, 1).tolist() == [0]
    assert ref._list(offsets, nbrs, 4, 2, 2).tolist() == [] and ref._list(offsets, nbrs, 4, 0, 1).tolist() == [2]
    with pytest.raises(AssertionError):
        ref.tables([1], [[[0] * 9, []]], 4)  # nine ids in eight slots
    with pytest.raises(AssertionError):
        ref.tables([1], [[[0]]], 4)          # a level without its list


# Six nodes, levels 0..2, M = 4; every level-0 list is empty (the descent never reads level 0).
#   level 2:  0 <-> 1                       scores: 0: 10   1: 7   2: 6   3: 3   4: 1   5: 0 (level 0 only: never proposed)
#   level 1:  0 -> 2, 3   1 -> 2   2 -> 1   3 -> 4   4 -> 3
HAND_LEVELS = [2, 2, 1, 1, 1, 0]
HAND_UPPER = {0: [[2, 3], [1]], 1: [[2], [0]], 2: [[1]], 3: [[4]], 4: [[3]], 5: []}
HAND_SCORES = {0: 10.0, 1: 7.0, 2: 6.0, 3: 3.0, 4: 1.0, 5: 0.0}


def _hand(upper=None, scores=None, **kw):
    upper = {**HAND_UPPER, **(upper or {})}
    s = {**HAND_SCORES, **(scores or {})}
    levels, offsets, nbrs = ref.tables(HAND_LEVELS, [[[]] + upper[i] for i in range(6)], 4)
    return ref.descend(levels, offsets, nbrs, 4, 0, 2, lambda ids: np.array([s[int(i)] for i in ids], np.float64), **kw)


def test_descend_by_hand_local_minimum():
    """level 2: 0 -> 1 (7 beats 10), 1's list names only 0.  Level 1: 1 -> 2 (6), 2's list names only 1: the walk ends at 2,
    though ports 3 and 4 score better -- they hang off node 0, which the walk left at level 2"""
    trace = []
    assert _hand(trace=trace) == 2
    assert trace == [(0, 1, [0]), (1, 1, [0]), (1, 2, [1]), (2, 2, [1])]
    # the wrong rules the GPU cases are checked against give other answers here
    assert _hand(walk=range(2, 1, -1)) == 1, "stopped at level 1"
    assert _hand(walk=range(1, 0, -1)) == 4, "the top level skipped: 0 -> 3 -> 4"


def test_descend_by_hand_empty_list_at_the_top_level():
    """the entry's level-2 list is empty: a step without improvement, then level 1 from node 0: 0 -> 3 (3 beats 6) -> 4"""
    assert _hand({0: [[2, 3], []]}) == 4


def test_descend_by_hand_ties_go_to_the_lower_id():
    """2 and 3 score the same and node 0 names 3 first: 2 wins, and its list leads nowhere better"""
    assert _hand({0: [[3, 2], []]}, {2: 5.0, 3: 5.0}) == 2
    assert _hand({0: [[3, 2], []]}, {2: 5.0, 3: 5.0}, key=lambda s, i: (s, -i)) == 4, "the greater id: 3, then 4"
    # an equal score of LOWER id replaces the current node (4 -> 3), one of greater id does not (3 stays)
    assert _hand({0: [[4], []]}, {3: 1.0, 4: 1.0}) == 3
    assert _hand({0: [[4], []]}, {3: 1.0, 4: 1.0}, key=lambda s, i: (s, 0)) == 4, "FAISS's strict comparison stays at 4"
    assert _hand({0: [[3], []]}, {3: 1.0, 4: 1.0}) == 3


def test_descend_by_hand_list_with_a_hole():
    """0's level-1 list is 2, -1, 3: only 2 is proposed (read past the hole, the walk would reach 3 and 4)"""
    assert _hand({0: [[2, -1, 3], []]}) == 2
    assert _hand({0: [[-1, 3], []]}) == 0


def test_descend_without_upper_levels_and_at_a_node_without_the_level():
    levels, offsets, nbrs = ref.tables([0, 0], [[[1]], [[0]]], 4)
    assert ref.descend(levels, offsets, nbrs, 4, 1, 0, lambda ids: np.zeros(len(ids))) == 1
    # a level-1 list that names a level-0 node: the reference refuses to walk it (the library refuses the import)
    levels, offsets, nbrs = ref.tables([1, 0], [[[], [1]], [[]]], 4)
    with pytest.raises(AssertionError):
        ref.descend(levels, offsets, nbrs, 4, 0, 1, lambda ids: -np.asarray(ids, np.float64))


def test_coarse_entries_by_hand():
    """70 nodes with the one-dimensional rows i % 10; nodes 3 .. 68 are ports"""
    x = (np.arange(70) % 10).astype(np.float32)[:, None]
    levels = np.zeros(70, np.int32)
    levels[3:69] = 1
    one, zero = np.ones(1, np.float32), np.zeros(1, np.float32)
    assert ref.ports_of(levels).tolist() == list(range(3, 69))
    assert ref.coarse_entries(levels, x, one, 4, METRIC_INNER_PRODUCT).tolist() == [9, 19, 29, 39]
    assert ref.coarse_entries(levels, x, one, 7, METRIC_INNER_PRODUCT).tolist() == [9, 19, 29, 39, 49, 59, 8]
    assert ref.coarse_entries(levels, x, zero, 4, METRIC_L2).tolist() == [10, 20, 30, 40]
    assert ref.coarse_entries(levels, x, one, 4, METRIC_INNER_PRODUCT, shift=1).tolist() == [10, 20, 30, 40]
    assert ref.coarse_entries(levels, x, one, 4, METRIC_INNER_PRODUCT, key=lambda s, i: (s, -i)).tolist() == [59, 49, 39, 29]
    assert ref.coarse_entries(levels, x, one, 100, METRIC_INNER_PRODUCT).size == 66
    levels[66:] = 0  # 63 ports: the descent applies
    assert ref.coarse_entries(levels, x, one, 4, METRIC_INNER_PRODUCT) is None


def test_margins_by_hand():
    x = np.array([[1.0, 0.0], [1.0 - 2.0 ** -19, 0.0], [0.5, 0.0]], np.float32)
    q = np.array([1.0, 0.0], np.float32)
    # fp32 chain, inner product: bound 2 * 2^-24 * |q y| per score; gap 2^-19 over about 2 * 2^-23
    assert ref.margins(x, q, METRIC_INNER_PRODUCT, trace=[(1, 0, [1])]) == pytest.approx(2.0 ** -19 / (2.0 ** -23 * (2 - 2.0 ** -19)))
    assert ref.margins(x, q, METRIC_INNER_PRODUCT, trace=[(1, 0, [1, 2])]) == pytest.approx(8.0, rel=1e-5), "the worst comparison counts"
    assert ref.margins(x, q, METRIC_INNER_PRODUCT, trace=[(2, 0, [2])]) == pytest.approx(0.5 / (2.0 ** -23 * 1.5))
    # the coarse cut: the worst inside against the best outside, bf16 adds 2^-8 of the term sum
    got = ref.margins(x, q, METRIC_INNER_PRODUCT, cut=([0, 1], [2]), bf16=True)
    assert got == pytest.approx((0.5 - 2.0 ** -19) / ((2.0 ** -23 + 2.0 ** -8) * (1.5 - 2.0 ** -19)))
    # squared L2 at the cut: the terms are bounded by (|q_i| + |y_i|)^2 -- 4 for row 0, 2.25 for row 2; gap 0.25
    assert ref.margins(x, q, METRIC_L2, cut=([0], [2])) == pytest.approx(0.25 / (2.0 ** -23 * 6.25))
    assert ref.margins(x, q, METRIC_L2, trace=[(2, 0, [2])]) == pytest.approx(0.25 / (2.0 ** -23 * 0.25)), "the difference form"
    assert ref.margins(x, q, METRIC_L2) == np.inf
    with pytest.raises(AssertionError):
        ref.margins(x, q, METRIC_INNER_PRODUCT, trace=[(0, 2, [0])])  # the "winner" scores worse


# ---- the cases of tests/test_hnsw_entry_exact_gpu.py ----------------------------------------------------------------
ALL_CASES = [(name, metric) for name in cases.SPECS for metric in cases.METRICS]


def _island_of(c, node):
    return tuple(cases.reach(c, [int(node)]).tolist())


@pytest.mark.parametrize("name,metric", ALL_CASES)
def test_entry_cases_are_islands_within_the_limits(name, metric):
    c = cases.case(name, metric)
    sp = c.spec
    assert c.n <= 1000 and c.q.shape[0] <= 600 and sp.d <= 1028 and c.levels.max() == c.max_level == sp.max_level
    assert c.levels[c.entry_point] == c.max_level and c.ports.size == sp.islands * sp.ports_per
    islands = {_island_of(c, i) for i in range(c.n)}
    assert len(islands) == sp.islands and all(len(isl) == sp.size for isl in islands), "level 0: disjoint closed rings"
    assert all(sum(c.levels[list(isl)] >= 1) == sp.ports_per for isl in islands)
    assert (np.diff(c.ports % sp.size) != 0).any() and not np.array_equal(c.ports, np.arange(c.ports.size)), "ports at scattered ids"
    # every upper list names nodes that have the level (what knn_hnsw_graph_import requires)
    for i in c.ports.tolist():
        for l in range(1, int(c.levels[i]) + 1):
            assert all(j == -1 or c.levels[j] >= l for j in c.lists[i][l]), (i, l)
    if sp.family == "int":
        assert sp.d <= 128 and np.abs(c.x).max() <= 8 and np.abs(c.q).max() <= 8
        assert (c.x == np.round(c.x)).all() and (c.q == np.round(c.q)).all()


@pytest.mark.parametrize("name,metric", ALL_CASES)
def test_entry_cases_tell_the_right_rule_from_each_wrong_one(name, metric):
    """the discriminating precondition: for every wrong rule, some query's expected result (k = n: the ids of the reachable
    set) differs from the right rule's"""
    c = cases.case(name, metric)
    truth = cases.reaches(c)
    differs = {}
    for j in range(c.q.shape[0]):
        for rule, ents in cases.wrong_entries(c, j).items():
            differs[rule] = differs.get(rule, 0) + (not np.array_equal(cases.reach(c, ents), truth[j]))
    want = ({"the descent instead", "c + 1 entries", "port table shifted by one"} if cases.rule_of(c) == "coarse" else
            {"the coarse rule instead", "entry_point, no descent", "descent stopped at level 1", "descent skipping the top level"})
    if cases.rule_of(c) == "coarse" and (c.spec.entry or 4) > 1:
        want.add("c - 1 entries")
    if c.spec.tie:
        want.add("the greater id on ties")
    if c.spec.tie == "path":
        want.add("no move on an equal score")
    assert want == set(differs), "every wrong rule is tried"
    assert all(v > 0 for v in differs.values()), f"rules this case cannot tell from the right one: {[r for r, v in differs.items() if not v]}"


@pytest.mark.parametrize("metric", cases.METRICS)
def test_entry_cases_reach_their_branches(metric):
    """each case holds what its name promises"""
    case = lambda name: cases.case(name, metric)  # noqa: E731
    assert cases.rule_of(case("ports63")) == "descent" and case("ports63").ports.size == 63 and case("ports63").n == 504
    assert cases.rule_of(case("ports64")) == "coarse" and case("ports64").ports.size == 64 and case("ports64").n == 512
    for name in ("ports63", "ports64"):
        assert case(name).spec.entry is None and case(name).spec.d == 32 and case(name).max_level == 2 and case(name).q.shape[0] == 6
    for name, count in (("coarse-c1", 1), ("coarse-c4", 4), ("coarse-c64", 64)):
        c = case(name)
        assert c.n == 768 and all(len(cases.entries(c, j)) == count for j in range(6))
        assert all(cases.reach(c, cases.entries(c, j)).size == count * 8 for j in range(6))
    # several ports per island: some query enters one island twice
    c = case("coarse-shared")
    assert min(cases.reach(c, cases.entries(c, j)).size for j in range(6)) < 4 * c.spec.size
    # the tie at the cut: query 0's 4th and 5th ports hold one row, in two islands
    c = case("coarse-tie")
    five = ref.coarse_entries(c.levels, c.x, c.q[0], 5, metric)
    assert np.array_equal(c.x[five[3]], c.x[five[4]]) and five[3] < five[4] and _island_of(c, five[3]) != _island_of(c, five[4])
    # the descents: local minima, empty lists, holes and ties ON THE PATHS walked
    for name in ("descent-l1", "descent-l2", "descent-l3", "descent-tie", "descent-counts", "gauss-descent", "gauss-wide"):
        c = case(name)
        local_minimum = empty = hole = tie_proposals = tie_current = False
        for j in range(c.q.shape[0]):
            trace = []
            end = ref.descend(c.levels, c.offsets, c.nbrs, cases.M, c.entry_point, c.max_level, cases._Scorer(c.x, c.q[j], metric), trace=trace)
            best = c.ports[np.argmin(ref.scores(c.x, c.q[j], c.ports, metric))]
            local_minimum |= end != best
            empty |= any(others == [] for _, _, others in trace)
            for cur, w, others in trace:
                for l in range(1, int(c.levels[cur]) + 1):
                    hole |= -1 in c.lists[cur][l][:-1] and any(v >= 0 for v in c.lists[cur][l][c.lists[cur][l].index(-1):])
                s = ref.scores(c.x, c.q[j], [w] + others, metric)
                tie_proposals |= any(s[1 + t] == s[0] and o != cur and w != cur for t, o in enumerate(others))
                tie_current |= any(s[1 + t] == s[0] and o == cur for t, o in enumerate(others))
        assert local_minimum, name
        assert empty or not c.spec.empty1, f"{name}: no walk meets an empty list"
        assert hole or not c.spec.holes, f"{name}: no walk meets a list with a hole"
        assert (tie_proposals and tie_current) or c.spec.tie != "path", f"{name}: no equal scores on a path"
    assert case("descent-l1").max_level == 1 and case("descent-l2").max_level == 2 and case("descent-l3").max_level == 3
    c = case("descent-l3")
    assert c.lists[c.entry_point][2] == [] and c.lists[c.entry_point][3] != []
    assert case("descent-counts").q.shape[0] == 600 and case("gauss-wide").spec.d == 1028 and case("gauss-coarse").spec.d == 100


@pytest.mark.parametrize("name,metric", [(name, metric) for name in cases.GAUSS_CASES for metric in cases.METRICS])
def test_entry_cases_with_real_rows_keep_their_margins(name, metric):
    """every comparison the applicable rule makes is more than four worst-case rounding bounds from a tie: the fp32 chain
    for the descent's pair scores, the fp32 scan and the bf16 scan for the coarse cut"""
    c = cases.case(name, metric)
    for j in range(c.q.shape[0]):
        if cases.rule_of(c) == "descent":
            trace = []
            ref.descend(c.levels, c.offsets, c.nbrs, cases.M, c.entry_point, c.max_level, cases._Scorer(c.x, c.q[j], metric), trace=trace)
            assert trace and ref.margins(c.x, c.q[j], metric, trace=trace) > 4.0, (name, j)
        else:
            inside = cases.entries(c, j)
            outside = np.setdiff1d(c.ports, inside)
            assert ref.margins(c.x, c.q[j], metric, cut=(inside, outside), bf16=False) > 4.0, (name, j)
            assert ref.margins(c.x, c.q[j], metric, cut=(inside, outside), bf16=True) > 4.0, (name, j)
