"""GPU: knn_eval_assemble (csrc/assemble.inc) bit for bit against tests/assemble_reference.py.

One workgroup of four waves serves a group: it streams the entries 256 at a time into an LDS buffer of
max(2 * next_pow2(depth), 1024) keys, sorts and cuts the buffer whenever the next 256 would not fit, looks the groups of
the best depth entries up, marks repeats and compacts the survivors across its waves.  The shapes here sit where that
can go wrong: entry counts around one wave, one pass of the workgroup and the buffer's size, depths on both sides of k
and of the entry count, survivors and their repeats in different waves, and groups cut into slabs.  Integers are
compared with array_equal, scores as uint32 patterns; there is no tolerance anywhere."""
import numpy as np
import pytest

import assemble_reference as ref

pytestmark = pytest.mark.gpu

KNOB = "KNN355_EVAL_SLAB_ROWS"
KNN_ERR_INVALID = -1
S64, SBITS = -7777, 0xDEADBEEF  # what the output arrays hold before a call
FMAX = float(np.finfo(np.float32).max)
I64_MIN = -2**63
ODD_SCORES = np.array([np.nan, np.inf, -np.inf, FMAX, -FMAX, 0.0, -0.0, 1.5, -1.5, 2.0, 3.0, 1e-45], np.float32)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _ptr(a):
    return None if a is None else a.ctypes.data


def c_assemble(hits_, scores_, offsets_, row_group_, self_group, depth, k_out, ascending, sources=True, **over):
    """the C entry point -> (return code, groups, score bits, qrow, hit), the outputs pre-filled with the sentinels;
    `over` replaces arguments by name (ns, k, ng, nb) or drops a pointer (hits=None ...)"""
    from knn_for_homology_amd import _lib
    hits = np.ascontiguousarray(hits_, np.int64)
    scores = np.ascontiguousarray(scores_, np.float32)
    offsets = np.ascontiguousarray(offsets_, np.int64)
    row_group = np.ascontiguousarray(row_group_, np.int32)
    self_group = None if self_group is None else np.ascontiguousarray(self_group, np.int32)
    ns, k = hits.shape
    ng = len(offsets) - 1
    shape = (max(ng, 1), max(k_out, 1))
    groups = np.full(shape, S64, np.int64)
    so = np.full(shape, SBITS, np.uint32)
    qrow = np.full(shape, S64, np.int64) if sources else None
    hit = np.full(shape, S64, np.int64) if sources else None
    a = dict(hits=hits, scores=scores, ns=ns, k=k, offsets=offsets, ng=ng, row_group=row_group if row_group.size else None,
             nb=len(row_group), groups=groups, so=so)
    a.update(over)
    rc = _lib.lib().knn_eval_assemble(_ptr(a["hits"]), _ptr(a["scores"]), a["ns"], a["k"], _ptr(a["offsets"]), a["ng"], _ptr(a["row_group"]),
                                      a["nb"], _ptr(self_group), depth, k_out, ascending, _ptr(a["groups"]), _ptr(a["so"]), _ptr(qrow),
                                      _ptr(hit))
    return rc, groups[:ng], so[:ng], (qrow[:ng] if sources else None), (hit[:ng] if sources else None)


def _same(got, want):
    rc, groups, so, qrow, hit = got
    assert rc == 0, _last_error()
    assert np.array_equal(groups, want[0]), "groups_out"
    assert np.array_equal(so, _bits(want[1])), "scores_out (as bits)"
    if qrow is not None:
        assert np.array_equal(qrow, want[2]), "qrow_out"
        assert np.array_equal(hit, want[3]), "hit_out"


def _check(hits, scores, offsets, row_group, self_group, depth, k_out, ascending):
    want = ref.assemble(hits, scores, offsets, row_group, self_group, depth, k_out, ascending)
    _same(c_assemble(hits, scores, offsets, row_group, self_group, depth, k_out, ascending), want)
    return want


def _last_error():
    from knn_for_homology_amd import _lib
    return _lib.lib().knn_last_error().decode()


def _case(rng, sizes, k, nb=97, ndb=23, values=None):
    """rows of random hits from [-2, nb + 2) in no order, scores from a small set (ties are the rule), a table of ndb
    database groups; group g owns sizes[g] rows"""
    ns = int(sum(sizes))
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    hits = rng.integers(-2, nb + 2, (ns, k)).astype(np.int64)
    values = np.arange(-4, 5, dtype=np.float32) / 2 if values is None else values
    scores = rng.choice(values, (ns, k)).astype(np.float32)
    row_group = rng.integers(0, ndb, nb).astype(np.int32)
    return hits, scores, offsets, row_group


# ---- entry counts around a wave, a pass of the workgroup and the buffer ----------------------------------------------
@pytest.mark.parametrize("S, k, depth, k_out", [
    (1, 1, 1, 1),
    (1, 64, 64, 64), (5, 13, 65, 65), (1, 65, 64, 3),
    (4, 64, 256, 256), (1, 257, 257, 256), (257, 1, 256, 200),
    (23, 89, 2048, 2048), (16, 128, 2048, 2048), (3, 683, 2048, 2048), (2049, 1, 2048, 2047),
    (40, 128, 2048, 2048), (40, 128, 7, 7), (40, 128, 7, 2),
])
def test_entry_counts(gpu_faiss, S, k, depth, k_out):
    rng = np.random.default_rng(1000 * S + k)
    # many database groups, so that a deep walk still emits many: 3000 rows, 2500 groups
    hits, scores, offsets, row_group = _case(rng, [0, S, 2], k, nb=3000, ndb=2500)
    for ascending in (0, 1):
        want = _check(hits, scores, offsets, row_group, None, depth, k_out, ascending)
    assert (want[0][1] >= 0).sum() >= min(k_out, S * k) // 2


@pytest.mark.parametrize("k, depth, k_out", [(70, 30, 30), (70, 70, 70), (70, 200, 200), (70, 200, 10), (70, 700, 700), (70, 2048, 1)])
def test_depth_against_k(gpu_faiss, k, depth, k_out):
    """depth below, at and above k; k_out below depth; (70, 700): 9 x 70 = 630 entries, fewer than depth"""
    rng = np.random.default_rng(k + depth)
    hits, scores, offsets, row_group = _case(rng, [9, 1, 3], k, nb=500, ndb=400)
    for ascending in (0, 1):
        _check(hits, scores, offsets, row_group, None, depth, k_out, ascending)


# ---- scores and ids -----------------------------------------------------------------------------------------------------
def test_equal_scores_keep_the_order_of_the_positions(gpu_faiss):
    S, k = 6, 100
    hits = np.random.default_rng(3).permutation(S * k).reshape(S, k).astype(np.int64)
    scores = np.full((S, k), 0.25, np.float32)
    row_group = np.arange(S * k, dtype=np.int32)
    for ascending in (0, 1):
        want = _check(hits, scores, [0, S], row_group, None, 300, 300, ascending)
        assert np.array_equal(want[0][0], hits.reshape(-1)[:300])  # the reference itself: all distinct groups, input order


def test_all_hits_in_one_group_give_one_output(gpu_faiss):
    rng = np.random.default_rng(4)
    hits, scores, offsets, _ = _case(rng, [7], 90, nb=50)
    hits = np.abs(hits) % 50
    want = _check(hits, scores, offsets, np.full(50, 11, np.int32), None, 500, 500, 0)
    assert want[0][0, 0] == 11 and (want[0][0, 1:] == -1).all()


def test_repeats_more_than_a_wave_behind_their_first_occurrence(gpu_faiss):
    """one row of 600 distinct descending scores: ranks are positions.  Ranks 0..99 name groups 0..99, ranks 100..299
    name them again twice over (every repeat 100 or 200 ranks behind its first occurrence, in another wave and, from rank
    256 on, in another pass), ranks 300..599 name new groups: the survivors come from waves 0, 1 and from the second and
    third pass and must close up."""
    k = 600
    hits = np.arange(k, dtype=np.int64)[None, :]
    scores = (1000.0 - np.arange(k, dtype=np.float32))[None, :]
    row_group = np.concatenate([np.arange(100), np.arange(100), np.arange(100), np.arange(300, 600)]).astype(np.int32)
    want = _check(hits, scores, [0, 1], row_group, None, k, 400, 0)
    assert want[0][0].tolist() == list(range(100)) + list(range(300, 600))
    assert want[3][0].tolist() == list(range(100)) + list(range(300, 600))
    want = _check(hits, scores, [0, 1], row_group, None, k, 250, 1)  # ascending: the walk starts at the far end
    assert want[0][0].tolist() == list(range(599, 349, -1))


def test_zeros_nan_infinities(gpu_faiss):
    rng = np.random.default_rng(5)
    hits, scores, offsets, row_group = _case(rng, [3, 11, 0, 2], 75, nb=2000, ndb=1500, values=ODD_SCORES)
    assert np.isnan(scores).sum() > 20 and (_bits(scores) == 0x80000000).sum() > 20
    for depth, k_out in ((75, 75), (400, 400), (2048, 2048)):
        for ascending in (0, 1):
            _check(hits, scores, offsets, row_group, None, depth, k_out, ascending)
    # the two zeros and nothing else: the order is the positions' whatever the signs
    z = rng.choice(np.array([0.0, -0.0], np.float32), (4, 75))
    want = _check(np.arange(300).reshape(4, 75), z, [0, 4], np.arange(300, dtype=np.int32), None, 300, 300, 0)
    assert want[0][0].tolist() == list(range(300)) and np.array_equal(_bits(want[1][0]), _bits(z).reshape(-1))


def test_ids_outside_the_table(gpu_faiss):
    rng = np.random.default_rng(6)
    hits, scores, offsets, row_group = _case(rng, [4, 4], 66, nb=40, ndb=30)
    hits[0, :6] = [-1, 40, 41, I64_MIN, 2**32 + 2, 2**62]  # (2^32 + 2 is not row 2)
    scores[0, :6] = 100.0  # at the head of the order: they use up depth and name nothing
    row_group[5] = -3      # a negative group names nothing either
    want = _check(hits, scores, offsets, row_group, None, 8, 8, 0)
    assert (want[0][0] >= 0).sum() <= 2
    _check(hits, scores, offsets, row_group, None, 264, 264, 1)
    # an empty table: every entry names nothing
    got = c_assemble(hits, scores, offsets, np.zeros(0, np.int32), None, 66, 5, 0)
    assert got[0] == 0 and (got[1] == -1).all() and (got[3] == -1).all() and (got[4] == -1).all()
    assert (got[2] == _bits(np.float32(-FMAX))).all()


# ---- groups and slabs ---------------------------------------------------------------------------------------------------
def test_empty_groups_and_no_groups(gpu_faiss):
    rng = np.random.default_rng(7)
    hits, scores, offsets, row_group = _case(rng, [0, 0, 3, 0, 1, 0, 0, 2, 0], 33)
    # rows in front of the first group and behind the last belong to nobody
    offsets = offsets + 2
    hits = np.concatenate([hits[:2], hits, hits[:3]])
    scores = np.concatenate([scores[:2], scores, scores[:3]])
    for ascending in (0, 1):
        want = _check(hits, scores, offsets, row_group, None, 40, 12, ascending)
    assert (want[0][[0, 1, 3, 5, 6, 8]] == -1).all() and (want[0][[2, 4, 7], 0] >= 0).all()
    rc, groups, so, qrow, hit = c_assemble(hits, scores, [0], row_group, None, 40, 12, 0)
    assert rc == 0 and groups.shape[0] == 0
    rc = c_assemble(hits, scores, [0], row_group, None, 40, 12, 0, hits=None, scores=None, offsets=None, groups=None, so=None)[0]
    assert rc == 0  # ng = 0 returns before any pointer is looked at


def test_self_group_entries_count_toward_depth(gpu_faiss):
    """the query's own protein holds the five best places of a depth of six: one foreign protein is found"""
    hits = np.array([[0, 1, 2, 3, 4, 5, 6, 7]], np.int64)
    scores = np.array([[9, 8, 7, 6, 5, 4, 3, 2]], np.float32)
    row_group = np.array([2, 2, 2, 2, 2, 0, 1, 3], np.int32)
    want = _check(hits, scores, [0, 1], row_group, [2], 6, 4, 0)
    assert want[0].tolist() == [[0, -1, -1, -1]]
    want = _check(hits, scores, [0, 1], row_group, None, 6, 4, 0)
    assert want[0].tolist() == [[2, 0, -1, -1]]
    rng = np.random.default_rng(8)
    hits, scores, offsets, row_group = _case(rng, [2, 5, 0, 1], 80, nb=60, ndb=9)
    _check(hits, scores, offsets, row_group, [3, 0, 1, -1], 100, 9, 0)
    _check(hits, scores, offsets, row_group, [3, 0, 1, 8], 400, 9, 1)


@pytest.mark.parametrize("rows", [1, 3, 4, 10, 11])
def test_slabs_are_cut_at_group_boundaries(gpu_faiss, monkeypatch, rows):
    """group sizes 1, 4, 2, 0, 3; 3 rows per slab: a group larger than a slab, a slab of two groups, a slab boundary on a
    group boundary.  The knob is read on every call."""
    rng = np.random.default_rng(9)
    hits, scores, offsets, row_group = _case(rng, [1, 4, 2, 0, 3], 41, nb=300, ndb=200)
    self_group = [5, 6, 7, 8, 9]
    want = ref.assemble(hits, scores, offsets, row_group, self_group, 60, 50, 0)
    monkeypatch.delenv(KNOB, raising=False)
    whole = c_assemble(hits, scores, offsets, row_group, self_group, 60, 50, 0)
    monkeypatch.setenv(KNOB, str(rows))
    cut = c_assemble(hits, scores, offsets, row_group, self_group, 60, 50, 0)
    _same(whole, want)
    _same(cut, want)
    assert all(np.array_equal(a, b) for a, b in zip(whole[1:], cut[1:]))
    nosrc = c_assemble(hits, scores, offsets, row_group, self_group, 60, 50, 0, sources=False)
    _same(nosrc, want)


@pytest.mark.parametrize("k", [3, 65])
def test_optional_columns_across_slabs(gpu_faiss, monkeypatch, k):
    """5 groups of one row in slabs of 2: self_group and qrow_out / hit_out, each present and absent"""
    rng = np.random.default_rng(90 + k)
    hits, scores, offsets, row_group = _case(rng, [1, 1, 1, 1, 1], k, nb=300, ndb=200)
    row_group[hits[:, 0].clip(0, 299)] = [5, 6, 7, 8, 9]  # every group meets its own: leaving self_group out shows
    monkeypatch.setenv(KNOB, "2")
    for self_group in ([5, 6, 7, 8, 9], None):
        want = ref.assemble(hits, scores, offsets, row_group, self_group, 70, 60, 0)
        for sources in (True, False):
            _same(c_assemble(hits, scores, offsets, row_group, self_group, 70, 60, 0, sources=sources), want)


# ---- a seeded sweep -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(4))
def test_random_sweep(gpu_faiss, seed):
    rng = np.random.default_rng(4242 + seed)
    for _ in range(10):
        ng = int(rng.integers(1, 21))
        k = int(rng.integers(1, 71))
        sizes = rng.integers(0, 13, ng)
        depth = int(rng.choice([1, 2, k, int(rng.integers(1, 2049)), int(rng.integers(1, 200))]))
        k_out = int(rng.integers(1, depth + 1))
        nb = int(rng.integers(1, 400))
        hits, scores, offsets, row_group = _case(rng, sizes, k, nb=nb, ndb=int(rng.integers(1, nb + 1)),
                                                 values=ODD_SCORES if rng.random() < 0.3 else None)
        self_group = rng.integers(-1, 20, ng).astype(np.int32) if rng.random() < 0.5 else None
        _check(hits, scores, offsets, row_group, self_group, depth, k_out, int(rng.integers(0, 2)))


# ---- the Python facade --------------------------------------------------------------------------------------------------
def test_facade_names_and_auc1(gpu_faiss):
    from knn_for_homology_amd.evaluation import assemble, assemble_grouping, auc1_assembled
    slice_proteins = ["a", "a", "b", "c", "c", "c", "a"]
    hits = np.array([[2, 0, 3], [6, 3, 2], [0, 3, 2], [2, 0, 6], [1, 2, -1], [3, 3, 3], [5, 4, 2]], np.int64)
    scores = np.array([[9, 8, 7], [9.5, 6, 5], [3, 2, 1], [1, 2, 3], [6, 5, 4], [0, 0, 0], [1, 1, 1]], np.float32)
    groups, out_scores, names, qrow, hit = assemble(hits, scores, slice_proteins, want_sources=True)
    # database ids: a = 0, b = 1, c = 2.  First "a": 9.5 -> row 6 (a), 9 -> row 2 (b), 8 -> row 0 (a, again); depth 3
    # "c": 6 -> row 1 (a), 5 -> row 2 (b), 4 -> hit -1, which uses up the depth.  Second "a": row 5 (c), row 4 (c again), row 2 (b)
    assert names == ["a", "b", "c", "a"]
    assert groups.tolist() == [[0, 1, -1], [0, 2, 1], [0, 1, -1], [2, 1, -1]]
    assert out_scores.tolist() == [[9.5, 9, -FMAX], [3, 2, 1], [6, 5, -FMAX], [1, 1, -FMAX]]
    assert qrow.tolist() == [[1, 0, -1], [2, 2, 2], [4, 4, -1], [6, 6, -1]]
    assert hit.tolist() == [[6, 2, -1], [0, 3, 2], [1, 2, -1], [5, 2, -1]]
    offsets, _, row_group, self_group, id_to_name = assemble_grouping(slice_proteins)
    want = ref.assemble(hits, scores, offsets, row_group, None, 3, 3, False)
    assert np.array_equal(groups, want[0]) and np.array_equal(_bits(out_scores), _bits(want[1]))
    # without the query's own protein, deeper, shorter, ascending
    g2, s2, _ = assemble(hits, scores, slice_proteins, depth=6, k_out=2, ascending=True, exclude_self=True)
    want = ref.assemble(hits, scores, offsets, row_group, self_group, 6, 2, True)
    assert np.array_equal(g2, want[0]) and np.array_equal(_bits(s2), _bits(want[1]))
    assert g2.tolist() == [[1, 2], [2, 0], [1, 0], [2, 1]]
    # leading correct proteins over the number of homologous ones; -1 ends a run; names outside the database count below the line
    homologous = {"a": {"a", "b"}, "b": {"a", "c", "nowhere"}, "c": set()}
    auc1 = auc1_assembled(groups, names, homologous, id_to_name)
    assert auc1.tolist() == [2 / 2, 2 / 3, 0.0, 0.0]
    assert auc1_assembled(np.array([[-1, 0], [1, -1]]), ["b", "c"], {"b": {"a"}, "c": {"b"}}, id_to_name).tolist() == [0.0, 1.0]


# ---- errors: refused on the host, nothing allocated or launched, the outputs as they were ------------------------------
def _refused(got, what):
    rc, groups, so, qrow, hit = got
    assert rc == KNN_ERR_INVALID and what in _last_error(), _last_error()
    assert (groups == S64).all() and (so == SBITS).all() and (qrow == S64).all() and (hit == S64).all()


def test_refusals(gpu_faiss):
    hits = np.zeros((6, 4), np.int64)
    scores = np.zeros((6, 4), np.float32)
    rg = np.zeros(3, np.int32)
    ok = [0, 2, 6]
    for depth, k_out, what in ((0, 1, "depth"), (2049, 1, "depth"), (-1, 1, "depth"), (4, 0, "k_out"), (4, 5, "k_out"), (4, -2, "k_out")):
        _refused(c_assemble(hits, scores, ok, rg, None, depth, k_out, 0), what)
    _refused(c_assemble(hits, scores, ok, rg, None, 4, 4, 0, k=0), "k >= 1")
    _refused(c_assemble(hits, scores, ok, rg, None, 4, 4, 0, k=-3), "k >= 1")
    _refused(c_assemble(hits, scores, ok, rg, None, 4, 4, 0, k=2**31), "k > INT32_MAX")
    for name in ("ns", "ng", "nb"):
        _refused(c_assemble(hits, scores, ok, rg, None, 4, 4, 0, **{name: -1}), "negative")
    for name in ("hits", "scores", "offsets", "row_group"):
        _refused(c_assemble(hits, scores, ok, rg, None, 4, 4, 0, **{name: None}), "null pointer")
    for name in ("groups", "so"):  # (the array left out keeps its sentinels too: it was never passed)
        _refused(c_assemble(hits, scores, ok, rg, None, 4, 4, 0, **{name: None}), "null pointer")
    _refused(c_assemble(hits, scores, [-1, 2, 6], rg, None, 4, 4, 0), "negative group offset")
    _refused(c_assemble(hits, scores, [0, 3, 2], rg, None, 4, 4, 0), "group offsets decrease")
    _refused(c_assemble(hits, scores, [2, 1, 6], rg, None, 4, 4, 0), "group offsets decrease")
    _refused(c_assemble(hits, scores, [0, 2, 7], rg, None, 4, 4, 0), "past the last row")
    # a group of 2^31 entries: no such array exists here, the check runs before anything is read
    _refused(c_assemble(hits, scores, [0, 2**29, 2**29 + 1], rg, None, 4, 4, 0, ns=2**30), "2^31 entries")
    _refused(c_assemble(hits, scores, [0, 2, 3], rg, None, 4, 4, 0, k=2**30), "2^31 entries")
    # and the same arguments pass once they are right
    got = c_assemble(hits, scores, ok, rg, None, 4, 4, 0)
    assert got[0] == 0 and got[1].tolist() == [[0, -1, -1, -1]] * 2
