"""CPU: tests/hnsw_build_reference.py checked before it judges the library (tests/test_hnsw_build_exact_gpu.py), and every GPU
case replayed to the end with the validity conditions (a)-(c) holding at every batch."""
import numpy as np
import pytest

import hnsw_build_cases as cases
import hnsw_build_reference as ref


def test_mt19937_known_value():
    """the C++ standard's check value: the 10000th output of a default-seeded mt19937"""
    rng = ref.MT19937()
    for _ in range(9999):
        rng()
    assert rng() == 4123659995
    order = ref.call_order(100, 50)
    assert sorted(order) == list(range(100, 150)) and order != sorted(order)
    assert ref.call_order(100, 50) == order and ref.call_order(101, 50) != [i + 1 for i in order]


def test_batch_sizes_worked_by_hand():
    # a quarter of what is linked, one row at least
    assert [ref.batch_size(done, 1000, 0, 16384) for done in (1, 3, 4, 7, 8, 100)] == [1, 1, 1, 1, 2, 25]
    # never more than 1/32 of the call, 32 rows at least
    assert ref.batch_size(1000, 1000, 0, 16384) == 32 and ref.batch_size(10000, 3200, 0, 16384) == 100
    # nor max_batch, nor what is left of the call
    assert ref.batch_size(10000, 3200, 0, 24) == 24 and ref.batch_size(10000, 3200, 3190, 16384) == 10
    # calls of 1, 31 and 32 rows onto 320 linked nodes are one batch, 33 rows are two
    assert [[len(b) for b in ref.call_batches(320, 320, n, 16384)] for n in (1, 31, 32, 33)] == [[1], [31], [32], [32, 1]]
    # an empty graph: the first row alone, then one row at a time until eight are linked
    assert [len(b) for b in ref.call_batches(0, 0, 20, 16384)] == [1] * 8 + [2, 2, 3, 3, 2]
    assert [len(b) for b in ref.call_batches(0, 0, 600, 8)][-3:] == [8, 8, 7] and sum(len(b) for b in ref.call_batches(0, 0, 600, 8)) == 600


# Eight points on a line (squared L2) / on an arc (inner product: unit rows at the angles 0.02 t, so that -cos orders the
# pairs as the distances on the line do).  Row 4 is an exact duplicate of row 1; no other two pairs tie.
T = [0, 10, 21, 33, 10, 9, 12, 14]
LEVELS = [1, 1, 1, 0, 1, 0, 0, 2]
BATCHES = [[1], [2], [3, 4], [5, 6, 7]]  # row 0 is the entry point
# after [1]: 0 <-> 1 on both levels.  after [2]: row 2 keeps 1 only (0 is closer to 1 than to 2); 1 appends 2 on both levels.
# [3, 4]: 3 keeps 2.  4 keeps 1 (v = 0), then 0 and 2 (v(0, 1) == v(0, 4): not smaller, kept); on level 1 the capacity 2 cuts
#   it to [1, 0].  Requests: 0 appends 4 on both levels; 1 appends 4 on level 0; on level 1 [0, 2] + 4 exceeds 2 -> pruned to
#   [4, 0]; 2 appends 4 (v = 11^2) before 3 (v = 12^2).
AFTER_3 = {0: [[1, 4], [1, 4]], 1: [[0, 2, 4], [4, 0]], 2: [[1, 4, 3], [1]], 3: [[2]], 4: [[1, 0, 2], [1, 0]]}
# [5, 6, 7]: 5 keeps 1 (ties with 4: lower id first; 4 then has v(4, 1) = 0) and 0.  6 and 7 keep 1 and 2, 7 on level 1 too
#   (its level 2 is above the graph's max level at the batch's start: no links there).  Requests: 0 appends 5.  1, level 0:
#   [0, 2, 4] + 5, 6, 7 -> pruned to [4, 5, 6] (7 is closer to 6, 0 to 5, 2 to 6).  1, level 1: [4, 0] + 7 -> [4, 7].
#   2, level 0: [1, 4, 3] + 7, 6 -> [7, 3].  2, level 1 appends 7.  Row 7 then takes the entry point at level 2.
FINAL = {0: [[1, 4, 5], [1, 4]], 1: [[4, 5, 6], [4, 7]], 2: [[7, 3], [1, 7]], 3: [[2]], 4: [[1, 0, 2], [1, 0]], 5: [[1, 0]],
         6: [[1, 2]], 7: [[1, 2], [1, 2], []]}


@pytest.mark.parametrize("metric", (0, 1))
def test_hand_worked_graph(oracle, metric):
    t = np.array(T, np.float64)
    x = np.zeros((8, 8), np.float32)
    if metric == ref.METRIC_L2:
        x[:, 0] = t
    else:
        x[:, 0], x[:, 1] = np.cos(0.02 * t), np.sin(0.02 * t)
    assert np.array_equal(x[1], x[4])
    sc = ref.Scores(x, metric, oracle)
    g = ref.Graph(2)
    g.levels = list(LEVELS)
    g.lists = [[[] for _ in range(lv + 1)] for lv in LEVELS]
    g.linked = [True] + [False] * 7
    g.entry, g.max_level = 0, 1
    for batch in BATCHES:
        ref.link_batch(g, sc, batch, 1024)
        if batch == [3, 4]:
            assert {i: g.lists[i] for i in range(5)} == AFTER_3
            assert (g.entry, g.max_level) == (0, 1)
    assert {i: g.lists[i] for i in range(8)} == FINAL
    assert (g.entry, g.max_level) == (7, 2)
    ref.check_invariants(g)
    levels, offsets, nbrs, cum = ref.tables(g)
    assert cum[:4].tolist() == [0, 4, 6, 8] and offsets.tolist() == [0, 6, 12, 18, 22, 28, 32, 36, 44]
    assert nbrs[:6].tolist() == [1, 4, 5, -1, 1, 4] and nbrs[36:].tolist() == [1, 2, -1, -1, 1, 2, -1, -1]


@pytest.mark.parametrize("metric", (0, 1))
def test_restated_walk_on_the_hand_worked_graph(oracle, metric):
    """a ninth row at t = 34 walks the final graph above.  As a level-0 row: nothing on level 2 (row 7 has no links there), on
    level 1 from 7 (20 away) to 2 (13 away; its links 1 and 7 are farther), then everything level 0 reaches from 2, nearest
    first (1 before its duplicate 4).  As a level-1 row: level 1 from the entry 7 -- 0, 1, 2, 4, 7 -- then level 0 from 2"""
    t = np.array(T + [34], np.float64)
    x = np.zeros((9, 8), np.float32)
    if metric == ref.METRIC_L2:
        x[:, 0] = t
    else:
        x[:, 0], x[:, 1] = np.cos(0.02 * t), np.sin(0.02 * t)
    sc = ref.Scores(x, metric, oracle)
    g = ref.Graph(2)
    g.levels = list(LEVELS) + [0]
    g.lists = [[list(l) for l in FINAL[i]] for i in range(8)] + [[[]]]
    g.linked = [True] * 8 + [False]
    g.entry, g.max_level = 7, 2
    assert ref.walk_candidates(g, sc, 8, 0) == {0: [3, 2, 7, 6, 1, 4, 5, 0]}
    g.levels[8], g.lists[8] = 1, [[], []]
    assert ref.walk_candidates(g, sc, 8, 0) == {1: [2, 7, 1, 4, 0], 0: [3, 2, 7, 6, 1, 4, 5, 0]}
    assert ref.walk_candidates(g, sc, 8, 1) == {1: [2, 7, 1, 4, 0]}
    # a level that is NOT connected: without row 2's link to 3, a walk that enters at 2 never sees 3 ... and 3 sees everything
    g.lists[2][0] = [7]
    assert ref.walk_candidates(g, sc, 8, 0)[0] == [2, 7, 6, 1, 4, 5, 0] and ref.reachable_on_level(g, 0, 3) == list(range(8))


def _select_f64(V, cap):
    """the rule, stated over a float64 matrix of the group (member 0 is the centre)"""
    n = V.shape[0]
    order = sorted(range(1, n), key=lambda c: (V[c, 0], c))
    kept = []
    for c in order:
        if len(kept) < cap and all(not (V[c, s] < V[c, 0]) for s in kept):
            kept.append(c)
    return kept


@pytest.mark.parametrize("metric", (0, 1))
@pytest.mark.parametrize("members", (2, 64, 65, 96, 97, 128))
def test_select_against_the_rule_in_float64(oracle, metric, members):
    d = 16
    # well separated: the fp32 scores are within 2e-5 of the float64 ones (asserted below), so a comparison whose sides differ
    # by more than 4e-5 comes out the same in both; the first seed whose group decides every comparison by more than that
    for seed in range(100):
        x = np.random.default_rng(1000 * members + 10 * seed + metric).standard_normal((members, d)).astype(np.float32)
        x64 = x.astype(np.float64)
        V = -(x64 @ x64.T) if metric == 0 else ((x64[:, None, :] - x64[None, :, :]) ** 2).sum(-1)
        gaps = np.abs(V[1:, 1:] - V[1:, :1])[~np.eye(members - 1, dtype=bool)]
        keys = np.sort(V[1:, 0])
        if (gaps.size == 0 or gaps.min() > 4e-5) and (keys.size < 2 or np.diff(keys).min() > 4e-5):
            break
    else:
        raise AssertionError("no well-separated group among a hundred seeds")
    sc = ref.Scores(x, metric, oracle)
    assert np.abs(sc.Vn - V).max() < 2e-5
    ids = list(range(1, members))
    for cap in (2, 8, 126):
        kept, v = ref.select(sc.Vn, 0, ids[::-1], cap)
        assert kept == _select_f64(V, cap)
        assert v == [sc.Vn[c, 0] for c in kept]


def test_select_drops_repeats_and_the_centre(oracle):
    x = np.zeros((4, 8), np.float32)
    x[:, 0] = [0, 1, -2, 4]
    sc = ref.Scores(x, 1, oracle)
    assert ref.select(sc.Vn, 0, [1, 2, 0, 2, 1, 3], 8)[0] == [1, 2]  # (3 is closer to 1 than to 0)


def test_level_table():
    """2M slots at level 0, M at every other level, levels until their probability falls below 1e-9"""
    assert ref.level_table(32).tolist() == [0, 64, 96, 128, 160, 192, 224]
    assert ref.level_table(2)[:3].tolist() == [0, 4, 6]


def test_the_case_table_covers_what_the_gpu_file_promises():
    names = [c.name for c in cases.ALL]
    assert len(set(names)) == len(names) and set(names) == set(cases.PICK), "every case has rows, every entry a case"
    assert all(sum(c.calls) + c.start <= 1024 and c.d <= 64 for c in cases.ALL)
    assert {(c.metric, c.M, len(c.calls)) for c in cases.SCRATCH} == {(m, M, p) for m in (0, 1) for M in (4, 8) for p in (1, 3)}
    assert {(c.metric, len(c.calls)) for c in cases.M2} == {(m, p) for m in (0, 1) for p in (1, 3)} and all(c.M == 2 and c.walk == "all" for c in cases.M2)
    assert all(c.d == 20 for c in cases.HOST_WALK) and {c.metric for c in cases.HOST_WALK} == {0, 1}
    assert all(c.host_upper for c in cases.HOST_UPPER) and cases.HOST_UPPER
    assert {c.M for c in cases.WIDE} == {16, 42, 63}
    # between them the wide cases must report pruning groups in both ranges: the selection's 96- and 128-row builds
    assert sum(c.groups[0] for c in cases.WIDE) >= 1 and sum(c.groups[1] for c in cases.WIDE) >= 1
    assert {c.metric for c in cases.ONE_BATCH} == {0, 1}


@pytest.mark.parametrize("case", cases.ONE_BATCH, ids=lambda c: c.name)
def test_one_batch_calls_are_one_batch(case):
    """from the case's own parameters: calls of 1, 31 and 32 rows are a single batch, 33 rows are cut into 32 + 1"""
    assert case.calls[1:] == (1, 31, 32, 33)
    done = case.start + case.calls[0]
    got = []
    for c in range(1, len(case.calls)):
        got.append([len(b) for b in ref.call_batches(done, done, case.calls[c], cases.max_batch(case, c))])
        done += case.calls[c]
    assert got == [[1], [31], [32], [32, 1]]


@pytest.mark.parametrize("case", cases.ALL, ids=lambda c: c.name)
def test_every_gpu_case_replays_with_the_conditions_holding(oracle, case):
    """levels drawn by the documented law; replay_add asserts (a)-(c) at the start of every batch, replay once more at the
    end; the report shows the device batches and pruning groups the case is there for"""
    levels = cases.draw_levels(case)
    x, start, after, g = cases.replay(case, oracle, levels)
    cases.check_reports(case, after)
    ref.check_invariants(g)
    assert sum(g.linked) == x.shape[0] == len(g.levels)
    # duplicate rows inside one batch and across batches are part of every case
    dup = cases.duplicate_batches(case)
    if dup:
        inside, early, late = dup
        assert (x[inside[1:4]] == x[inside[0]]).all() and (x[late[:3]] == x[early[:3]]).all()
    else:
        assert case in cases.ONE_BATCH, "only the small last calls of the one-batch cases go without planted duplicates"
    # replaying again gives the same graph
    again = cases.replay(case, oracle, levels)[2][-1][0]
    assert all(np.array_equal(a, b) for a, b in zip(after[-1][0], again))


MUTATIONS = {"le": ("closer", lambda a, b: a <= b), "from_before_v": ("request_key", lambda r: (r[0], r[1], r[3], r[2]))}


@pytest.mark.parametrize("mutation", list(MUTATIONS))
@pytest.mark.parametrize("case", cases.ALL, ids=lambda c: c.name)
def test_every_case_tells_the_rule_from_its_two_nearest_mistakes(oracle, monkeypatch, case, mutation):
    """a replay with `<=` for `<` in the heuristic, or with the reverse requests ordered (from, v) for (v, from), ends in
    ANOTHER graph on the case's rows: a library that made either mistake would build that other graph and fail the case's
    slot-for-slot comparison.  `<=` shows only where two scores tie, so it is asked of the cases with planted duplicate rows
    (all but the one-batch cases); the request order of every case."""
    if mutation == "le" and not cases.duplicate_batches(case):
        assert case in cases.ONE_BATCH
        return
    levels = cases.draw_levels(case)
    right = cases.replay(case, oracle, levels)[2][-1][0]
    name, wrong_rule = MUTATIONS[mutation]
    monkeypatch.setattr(ref, name, wrong_rule)
    try:
        wrong = cases.replay(case, oracle, levels)[2][-1][0]
    except AssertionError:  # (the mutated graph may break the conditions: it is another graph all the same)
        return
    assert not np.array_equal(right[2], wrong[2])
