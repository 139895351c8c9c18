"""GPU: the four evaluation kernels of csrc/eval.inc, bit for bit against tests/consumers_reference.py.

Each kernel gives a 64-lane wave to a row and four rows to a block, and the host sends the rows through the device in
slabs.  The shapes here are the ones at which that structure can go wrong: k on both sides of one, two and many lane
trips, row counts that leave the last block partly filled, and (with KNN355_EVAL_SLAB_ROWS) slabs of 1, 4 and 7 rows
over 23.  Integers and bytes are compared with array_equal, scores as uint32 patterns; there is no tolerance anywhere.
The C entry points are called directly (_lib) wherever the Python wrapper hides an output."""
import numpy as np
import pytest

import consumers_reference as ref

pytestmark = pytest.mark.gpu

KS = [1, 2, 63, 64, 65, 127, 128, 129, 1000, 1001]
NQS = [1, 3, 5, 70]
SLABS = [1, 4, 7, 23, 24]
KNOB = "KNN355_EVAL_SLAB_ROWS"
KNN_ERR_INVALID = -1
I32_MIN, I32_MAX, I64_MIN = -2**31, 2**31 - 1, -2**63
S64, S32, S8, SBITS = -7777, -7777, 0xAB, 0xDEADBEEF  # what the output arrays hold before a call


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _ptr(a):
    return None if a is None else a.ctypes.data


# ---- the C entry points: -> (return code, outputs), the outputs pre-filled with the sentinels -------------------------
def c_remove(gpu, hits, scores, self_ids, k=None):
    from knn_for_homology_amd import _lib
    nq, kk = hits.shape
    ho = np.full((nq, kk - 1), S64, np.int64)
    so = np.full((nq, kk - 1), SBITS, np.uint32)
    missing = np.full(nq, S32, np.int32)
    rc = _lib.lib().knn_eval_remove_self_hit(_ptr(hits), _ptr(scores), nq, kk if k is None else k, _ptr(self_ids), _ptr(ho), _ptr(so),
                                             _ptr(missing))
    return rc, ho, so, missing


def c_labels(gpu, hits, lq, ldb, matrix=True, k=None):
    from knn_for_homology_amd import _lib
    nq, kk = hits.shape
    ic = np.full((nq, kk), S8, np.uint8) if matrix else None
    lead = np.full(nq, S32, np.int32)
    tp = np.full(nq, S32, np.int32)
    rc = _lib.lib().knn_eval_labels(_ptr(hits), nq, kk if k is None else k, _ptr(lq), _ptr(ldb), 0 if ldb is None else len(ldb), _ptr(ic),
                                    _ptr(lead), _ptr(tp))
    return rc, ic, lead, tp


def c_sets(gpu, hits, offsets, members, k=None):
    from knn_for_homology_amd import _lib
    nq, kk = hits.shape
    lead = np.full(nq, S32, np.int32)
    tp = np.full(nq, S32, np.int32)
    rc = _lib.lib().knn_eval_sets(_ptr(hits), nq, kk if k is None else k, _ptr(offsets), _ptr(members), _ptr(lead), _ptr(tp))
    return rc, lead, tp


def c_levels(gpu, hits, qrows, mapping, k=None):
    from knn_for_homology_amd import _lib
    nq, kk = hits.shape
    out = np.full((nq, mapping.shape[1], kk), S8, np.uint8)
    rc = _lib.lib().knn_eval_levels(_ptr(hits), nq, kk if k is None else k, _ptr(qrows), _ptr(mapping), mapping.shape[0], mapping.shape[1],
                                    _ptr(out))
    return rc, out


def _same_remove(got, want):
    rc, ho, so, missing = got
    assert rc == 0
    assert np.array_equal(ho, want[0]), "hits_out"
    assert np.array_equal(so, _bits(want[1])), "scores_out (as bits)"
    assert np.array_equal(missing, want[2]), "missing_out"


def _same_labels(got, want):
    rc, ic, lead, tp = got
    assert rc == 0
    if ic is not None:
        assert np.array_equal(ic, want[0]), "is_correct_out"
    assert np.array_equal(lead, want[1]), "lead_out"
    assert np.array_equal(tp, want[2]), "tp_out"


def _same_sets(got, want):
    rc, lead, tp = got
    assert rc == 0
    assert np.array_equal(lead, want[0]), "lead_out"
    assert np.array_equal(tp, want[1]), "tp_out"


def _same_levels(got, want):
    rc, out = got
    assert rc == 0 and np.array_equal(out, want)


# ---- random inputs of a given shape --------------------------------------------------------------------------------------
def _remove_case(rng, nq, k):
    """ids from a small range, so that rows hold their self id never, once and several times, and -1 here and there;
    the self ids are a shifted permutation; the scores are random bit patterns (NaNs with payloads, infinities, -0.0)"""
    self_ids = (rng.permutation(nq) + 3).astype(np.int64)
    hits = rng.integers(-1, max(50, 2 * k), (nq, k)).astype(np.int64)
    for r in range(0, nq, 3):
        hits[r, rng.integers(0, k)] = self_ids[r]
    scores = rng.integers(0, 2**32, (nq, k), dtype=np.uint64).astype(np.uint32).view(np.float32)
    scores[0, :2] = [np.nan, -0.0]
    return hits, scores, self_ids


def _label_case(rng, nq, k, nb=37):
    """a leading run of matches of random length per row (0 .. k), then ids from [-2, nb + 2)"""
    ldb = rng.integers(0, 3, nb).astype(np.int32)
    ldb[:3] = [0, 1, 2]
    lq = rng.integers(0, 3, nq).astype(np.int32)
    hits = rng.integers(-2, nb + 2, (nq, k)).astype(np.int64)
    for r in range(nq):
        run = rng.integers(0, k + 1)
        hits[r, :run] = rng.choice(np.flatnonzero(ldb == lq[r]), run)
    return hits, lq, ldb


def _set_case(rng, nq, k, nb=3000):
    """sets of 0, 1, 2, 5 and 40 sorted rows; half of each row's hits drawn from its set, a leading run of them, the
    rest from [-1, nb]"""
    offsets, members = [0], []
    hits = rng.integers(-1, nb + 1, (nq, k)).astype(np.int64)
    for r in range(nq):
        mine = np.sort(rng.choice(nb, rng.choice([0, 1, 2, 5, 40]), replace=False))
        members += mine.tolist()
        offsets.append(len(members))
        if mine.size:
            pick = rng.random(k) < 0.5
            pick[:rng.integers(0, k + 1)] = True
            pick[rng.integers(0, k)] = r % 2 == 0
            hits[r, pick] = rng.choice(mine, int(pick.sum()))
    return hits, np.asarray(offsets, np.int64), np.asarray(members, np.int64)


def _level_case(rng, nq, k, nlevels, n=29):
    mapping = rng.integers(0, 3, (n, nlevels)).astype(np.int32)
    hits = rng.integers(-2, n + 2, (nq, k)).astype(np.int64)
    return hits, rng.integers(0, n, nq).astype(np.int64), mapping


# ---- every k, every row count ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", KS[1:])  # k = 1 has no k - 1 columns to return: an error, tested below
def test_remove_self_hit_shapes(gpu_faiss, k):
    rng = np.random.default_rng(100 + k)
    for nq in NQS:
        hits, scores, self_ids = _remove_case(rng, nq, k)
        _same_remove(c_remove(gpu_faiss, hits, scores, self_ids), ref.remove_self_hit(hits, scores, self_ids))


@pytest.mark.parametrize("k", KS)
def test_label_eval_shapes(gpu_faiss, k):
    rng = np.random.default_rng(200 + k)
    for nq in NQS:
        hits, lq, ldb = _label_case(rng, nq, k)
        want = ref.label_eval(hits, lq, ldb)
        _same_labels(c_labels(gpu_faiss, hits, lq, ldb), want)
        _same_labels(c_labels(gpu_faiss, hits, lq, ldb, matrix=False), want)


@pytest.mark.parametrize("k", KS)
def test_set_eval_shapes(gpu_faiss, k):
    rng = np.random.default_rng(300 + k)
    for nq in NQS:
        hits, offsets, members = _set_case(rng, nq, k)
        _same_sets(c_sets(gpu_faiss, hits, offsets, members), ref.set_eval(hits, offsets, members))


@pytest.mark.parametrize("k", KS)
def test_levels_eval_shapes(gpu_faiss, k):
    rng = np.random.default_rng(400 + k)
    for nq, nlevels in zip(NQS, (4, 1, 5, 4)):
        hits, qrows, mapping = _level_case(rng, nq, k, nlevels)
        _same_levels(c_levels(gpu_faiss, hits, qrows, mapping), ref.levels_eval(hits, qrows, mapping))


# ---- slabs ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def slab_inputs():
    """23 rows at k = 65, every row different from every other (a slab that reads another slab's self ids, labels, set
    offsets or query rows gets another answer), and the reference's results, computed once"""
    rng = np.random.default_rng(7)
    nq, k = 23, 65
    rm = _remove_case(rng, nq, k)
    lb = _label_case(rng, nq, k)
    st = _set_case(rng, nq, k)
    lv = _level_case(rng, nq, k, 5)
    want = (ref.remove_self_hit(*rm), ref.label_eval(*lb), ref.set_eval(*st), ref.levels_eval(*lv))
    assert len(set(np.diff(st[1]).tolist())) > 2 and len(set(want[2][0].tolist())) > 3
    return (rm, lb, st, lv), want


def _all_four(gpu, inputs):
    rm, lb, st, lv = inputs
    return c_remove(gpu, *rm), c_labels(gpu, *lb), c_sets(gpu, *st), c_levels(gpu, *lv)


@pytest.mark.parametrize("rows", SLABS)
def test_slabs(gpu_faiss, slab_inputs, monkeypatch, rows):
    inputs, want = slab_inputs
    monkeypatch.delenv(KNOB, raising=False)
    whole = _all_four(gpu_faiss, inputs)
    monkeypatch.setenv(KNOB, str(rows))
    cut = _all_four(gpu_faiss, inputs)
    for got in (whole, cut):
        _same_remove(got[0], want[0])
        _same_labels(got[1], want[1])
        _same_sets(got[2], want[2])
        _same_levels(got[3], want[3])
    for a, b in zip(whole, cut):
        assert all(np.array_equal(x, y) for x, y in zip(a[1:], b[1:]))


@pytest.mark.parametrize("k", [3, 65])
def test_label_eval_without_the_matrix_across_slabs(gpu_faiss, monkeypatch, k):
    """5 rows in slabs of 2, one lane trip and two: is_correct_out present and absent"""
    hits, lq, ldb = _label_case(np.random.default_rng(500 + k), 5, k)
    want = ref.label_eval(hits, lq, ldb)
    monkeypatch.setenv(KNOB, "2")
    _same_labels(c_labels(gpu_faiss, hits, lq, ldb), want)
    _same_labels(c_labels(gpu_faiss, hits, lq, ldb, matrix=False), want)


@pytest.mark.parametrize("value", ["0", "-4", "", "seven", "7 ", "4x", "99999999999999999999"])
def test_slab_knob_ignores_what_is_no_positive_integer(gpu_faiss, slab_inputs, monkeypatch, value):
    inputs, want = slab_inputs
    monkeypatch.setenv(KNOB, value)
    _same_sets(c_sets(gpu_faiss, *inputs[2]), want[2])
    _same_remove(c_remove(gpu_faiss, *inputs[0]), want[0])


# ---- remove_self_hit -----------------------------------------------------------------------------------------------------
def _self_rows(k):
    """-> (hits, scores, self_ids, position removed per row, missing per row).  Fillers are 0 .. k-1 with a few -1, the
    self ids are far above them and no arange; scores differ in every cell and hold NaN, +-inf and -0.0 around the cuts."""
    places = [[0], [1], [63], [64], [65], [k - 1], [],       # once at each position that starts or ends a lane trip, absent
              [64, 3],                                       # twice, in different lanes: lane 0 finds 64, lane 3 finds 3
              [5, 69],                                       # twice in lane 5: its first trip wins
              [0, 100], [0, k - 1], [1, 65, 129]]            # at the front and again later
    nq = len(places)
    hits = np.tile(np.arange(k, dtype=np.int64), (nq, 1))
    hits[:, [2, 66, k - 2]] = -1
    self_ids = (1000 + 7 * np.arange(nq)[::-1]).astype(np.int64)
    scores = (np.arange(nq * k, dtype=np.float32).reshape(nq, k) + 0.5)
    scores[:, [0, 4, 62, 63, 64, 65, 66, k - 1]] = [np.nan, -0.0, np.inf, -np.inf, -0.0, np.nan, 1e-45, np.inf]
    for r, ps in enumerate(places):
        hits[r, ps] = self_ids[r]
    removed = [ps[0] if ps else k - 1 for ps in [sorted(p) for p in places]]
    return hits, scores, self_ids, removed, [0 if ps else 1 for ps in places]


@pytest.mark.parametrize("k", [130, 1001])
def test_remove_self_hit_positions(gpu_faiss, k):
    hits, scores, self_ids, removed, missing = _self_rows(k)
    want = ref.remove_self_hit(hits, scores, self_ids)
    # the reference itself, against the positions written out above
    for r, p in enumerate(removed):
        keep = [j for j in range(k) if j != p]
        assert np.array_equal(want[0][r], hits[r, keep]) and np.array_equal(_bits(want[1][r]), _bits(scores[r, keep]))
    assert want[2].tolist() == missing
    _same_remove(c_remove(gpu_faiss, hits, scores, self_ids), want)


def test_remove_self_hit_wrapper_prints_the_counts(gpu_faiss, capsys):
    from knn_for_homology_amd.evaluation import remove_self_hit
    k = 130
    hits, scores, self_ids, _, _ = _self_rows(k)
    want = ref.remove_self_hit(hits, scores, self_ids)
    ho, so = remove_self_hit(hits, scores, self_ids)
    assert np.array_equal(ho, want[0]) and np.array_equal(_bits(so), _bits(want[1]))
    misplaced, absent = int((hits[:, 0] != self_ids).sum()), int(want[2].sum())
    assert (misplaced, absent) == (9, 1)
    assert capsys.readouterr().out == f"Fixing {misplaced} misplaced self hits\nThere are {absent} missing self hits\n"
    # self_ids=None: row r's self id is r
    nq = hits.shape[0]
    hits = hits + 1000
    hits[hits == 999] = -1
    for r in range(nq):
        hits[r, hits[r] == self_ids[r] + 1000] = r
    hits[3] = np.arange(2000, 2000 + k)
    want = ref.remove_self_hit(hits, scores, np.arange(nq))
    ho, so = remove_self_hit(hits, scores)
    assert np.array_equal(ho, want[0]) and np.array_equal(_bits(so), _bits(want[1]))
    assert want[2].tolist() == [0, 0, 0, 1, 0, 0, 1, 0, 0, 0, 0, 0]
    assert capsys.readouterr().out == "Fixing 9 misplaced self hits\nThere are 2 missing self hits\n"


# ---- label_eval ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [130, 1001])
def test_label_eval_edges(gpu_faiss, k):
    nb = 12
    ldb = np.array([5, 6, 5, 6, 5, 6, I32_MIN, I32_MAX, I32_MIN, I32_MAX, 5, 5], np.int32)
    same, other = np.array([0, 2, 4, 10, 11]), np.array([1, 3, 5])
    rows, lq, lead, tp = [], [], [], []

    def row(fill, label, changes, want_lead, want_tp):
        h = np.resize(fill, k).astype(np.int64)
        for p, v in changes.items():
            h[p] = v
        rows.append(h), lq.append(label), lead.append(want_lead), tp.append(want_tp)

    row(same, 5, {}, k, k)                                    # every hit matches
    row(other, 5, {}, 0, 0)                                   # none does
    row(same, 7, {}, 0, 0)                                    # the query's label is nowhere in the database
    for p in (0, 63, 64, 65, k - 1):                          # the first foreign hit
        row(same, 5, {p: 1}, p, k - 1)
    row(same, 5, {70: -1}, 70, k - 1)                         # -1 cuts the run and is not counted
    row(same, 5, {64: -1, 3: 1}, 3, k - 2)
    for bad in (nb, nb + 1, -2, I64_MIN, 2**40, 2**32 + 2):   # ids outside the table never match (2^32 + 2: not row 2)
        row(same, 5, {65: bad}, 65, k - 1)
    row([6, 8], I32_MIN, {k - 1: 7}, k - 1, k - 1)            # extreme labels match themselves only
    row([7, 9], I32_MAX, {1: 6, 64: 8}, 1, k - 2)
    hits, lq = np.stack(rows), np.asarray(lq, np.int32)
    want = ref.label_eval(hits, lq, ldb)
    assert want[1].tolist() == lead and want[2].tolist() == tp  # the reference, against the numbers written out above
    _same_labels(c_labels(gpu_faiss, hits, lq, ldb), want)
    _same_labels(c_labels(gpu_faiss, hits, lq, ldb, matrix=False), want)


def test_label_eval_empty_database(gpu_faiss):
    from knn_for_homology_amd.evaluation import label_matches
    hits = np.array([[0, -1, 1] * 22, [5, 0, I64_MIN] * 22, [0] * 66], np.int64)
    lq = np.array([0, 0, I32_MIN], np.int32)
    rc, ic, lead, tp = c_labels(gpu_faiss, hits, lq, None)  # nb = 0, labels_db NULL
    assert rc == 0 and not ic.any() and not lead.any() and not tp.any()
    ic, lead, tp = label_matches(hits, lq, np.zeros(0, np.int32))
    assert ic.dtype == bool and not ic.any() and not lead.any() and not tp.any()
    assert label_matches(hits, lq, np.zeros(0, np.int32), want_matrix=False)[0] is None


# ---- set_eval ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [130, 1001])
def test_set_eval_edges(gpu_faiss, k):
    big = np.arange(0, 3000, 2)                                # 1500 even rows
    sets = [[], [10], [10, 20], big, [], [7, 8, 9], [100, 200], [300, 400, 500], [600, 900]]  # the last one ends members
    offsets = np.concatenate([[0], np.cumsum([len(s) for s in sets])]).astype(np.int64)
    members = np.concatenate([np.asarray(s, np.int64) for s in sets])
    rows = [np.resize([10, 0, -1], k),                         # an empty set at offset 0
            np.resize([10], k),                                # a set of one: all match
            np.resize([20, 10], k),                            # a set of two
            np.resize(big, k),                                 # a set larger than k
            np.resize([7, 2998], k),                           # an empty set between two others: neither's members match
            np.resize([9, 8, 7], k),
            np.resize([200, 100], k),
            np.resize([300, 500, 400], k),
            np.resize([900, 600], k)]
    hits = np.stack(rows).astype(np.int64)
    hits[2, 64] = 15                                           # between the two members
    hits[2, 70] = 0                                            # the big set's first member, below this set's first
    hits[3, [63, 65, 100]] = [1, 2999, -1]                     # odd, past the big set's last member, -1
    hits[5, 65] = 10                                           # below every member: set 2's last-but-one, before this set
    hits[6, 64] = 300                                          # larger than all of this set and the FIRST member of the next
    hits[6, 66] = -1
    hits[7, 63] = 600                                          # the same at the next boundary
    hits[8, [1, 64, k - 1]] = [901, 10**12, 2**62]             # larger than every member of the last set: lo == hi0 == nmem
    lead = [0, k, 64, 63, 0, 65, 64, 63, 1]
    tp = [0, k, k - 2, k - 3, 0, k - 1, k - 2, k - 1, k - 3]
    want = ref.set_eval(hits, offsets, members)
    assert want[0].tolist() == lead and want[1].tolist() == tp
    _same_sets(c_sets(gpu_faiss, hits, offsets, members), want)
    # all sets empty, set_members NULL
    rc, lead, tp = c_sets(gpu_faiss, hits, np.zeros(len(sets) + 1, np.int64), None)
    assert rc == 0 and not lead.any() and not tp.any()


def test_compute_auc1_names_and_sizes(gpu_faiss):
    from knn_for_homology_amd.evaluation import compute_auc1
    k, nb = 65, 200
    target_ids = [f"t{i}" for i in range(nb)]
    queries = ["a", "b", "c", "d", "e"]
    homologous = {"a": {f"t{i}" for i in range(0, 140, 2)},            # 70 members, the row's first 64 hits and its last
                  "b": {"t1", "t3", "not a target", "nor this one"},     # names outside target_ids count in the divisor only
                  "c": set(),                                            # the divisor is 1, not 0
                  "d": {"gone"},
                  "e": {"t199"}}
    hits = np.array([list(range(0, 128, 2)) + [138],
                     [3, 1, 3] + [5] * 62,
                     list(range(65)),
                     [-1] * 65,
                     [199] * 65], np.int64)
    got = compute_auc1(hits, homologous, queries, target_ids)
    assert got.tolist() == [65 / 70, 3 / 4, 0.0, 0.0, 65.0]
    offsets, members = [0], []
    for q in queries:
        members += sorted(int(t[1:]) for t in homologous[q] if t in set(target_ids))
        offsets.append(len(members))
    lead, _ = ref.set_eval(hits, offsets, members)
    assert np.array_equal(got, lead / np.array([70, 4, 1, 1, 1]))


# ---- levels_eval ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nlevels", [1, 4, 5])
def test_levels_eval_layout_and_rows(gpu_faiss, nlevels):
    """k = 65: lane 0 writes columns 0 and 64 of each of the nlevels rows of out[q]; a transposed or mis-strided layout
    moves bytes.  The mapping makes every (level, hit) cell predictable: level l of row i is (i >> l) & 1."""
    from knn_for_homology_amd.evaluation import compute_is_correct
    n, k, nq = 32, 65, 7
    mapping = ((np.arange(n)[:, None] >> np.arange(nlevels)[None, :]) & 1).astype(np.int32)
    rng = np.random.default_rng(nlevels)
    hits = rng.integers(0, n, (nq, k)).astype(np.int64)
    hits[:, 64] = [31, 0, 31, 0, 31, 0, 31]
    hits[0, [0, 63]] = [-1, n]       # outside the table: false at every level
    hits[1, [1, 64]] = [n + 1, -2]
    hits[2, [5, 6]] = [I64_MIN, 2**32]  # 2^32 is not row 0
    qrows = np.array([31, 0, 5, 10, 21, 16, 31], np.int64)  # neither arange nor a prefix of it
    want = ref.levels_eval(hits, qrows, mapping)
    inside = (hits >= 0) & (hits < n)
    for l in range(nlevels):  # the reference, against the closed form
        assert np.array_equal(want[:, l, :], (inside & (((hits >> l) & 1) == ((qrows >> l) & 1)[:, None])).astype(np.uint8))
    assert not want[0, :, [0, 63]].any() and not want[1, :, [1, 64]].any() and not want[2, :, [5, 6]].any()
    _same_levels(c_levels(gpu_faiss, hits, qrows, mapping), want)
    got = compute_is_correct(hits, mapping, qrows)
    assert got.dtype == bool and got.shape == (nq, nlevels, k) and np.array_equal(got, want.astype(bool))
    # query_rows=None: query q is row q
    assert np.array_equal(compute_is_correct(hits, mapping), ref.levels_eval(hits, np.arange(nq), mapping).astype(bool))


def test_compute_is_correct_label_types(gpu_faiss):
    from knn_for_homology_amd.evaluation import compute_is_correct
    rng = np.random.default_rng(5)
    hits = rng.integers(-1, 7, (5, 66)).astype(np.int64)
    qrows = rng.permutation(6)[:5]
    strings = np.array([["3", "3.40", "3.40.50", "x"], ["3", "3.40", "3.40.50", "y"], ["3", "3.4", "3.40.5", "x"],
                        ["2", "3.40", "3.40.50", "x "], ["3", "3.40", "3.40.50", "x"], ["", "3.40", "3.40.50", "X"]])
    # int64 labels that differ only above bit 32: equal as int32, not as labels
    wide = np.array([[5, 1 << 40], [5 + (1 << 32), 1 << 40], [5, (1 << 40) + (1 << 33)], [5 - (1 << 32), 1 << 41], [5, 1 << 40],
                     [1 << 32, 0]], np.int64)
    assert len(set(wide[:, 0].astype(np.int32).tolist())) == 2 and len(set(wide[:, 0].tolist())) == 4
    for mapping in (strings, wide):
        want = ref.levels_eval(hits, qrows, mapping).astype(bool)
        assert 0 < want.mean() < 1
        assert np.array_equal(compute_is_correct(hits, mapping, qrows), want)
    only = compute_is_correct(np.array([[0, 1, 2, 3, 4, 5]]), wide, np.array([0]))
    assert only[0].tolist() == [[True, False, True, False, True, False], [True, True, False, False, True, False]]


# ---- errors: refused on the host, nothing allocated or launched, the outputs as they were ------------------------------
def _untouched(*arrays):
    for a in arrays:
        assert (a == {np.dtype(np.int64): S64, np.dtype(np.int32): S32, np.dtype(np.uint8): S8, np.dtype(np.uint32): SBITS}[a.dtype]).all()


def _last_error():
    from knn_for_homology_amd import _lib
    return _lib.lib().knn_last_error().decode()


@pytest.mark.parametrize("offsets, members, what", [
    ([-1, 2, 3, 4], [1, 2, 3, 4], "negative set offset"),
    ([0, 3, 2, 4], [1, 2, 3, 4], "set offsets decrease"),
    ([0, 2, 4, 3], [1, 2, 3, 4], "set offsets decrease"),
    ([0, 2, 2, 4], [2, 1, 3, 4], "set members not sorted"),
    ([0, 0, 1, 4], [1, 2, 4, 3], "set members not sorted"),
])
def test_set_eval_refuses_bad_sets(gpu_faiss, offsets, members, what):
    """The hits are larger than every member, which keeps a binary search at the upper end of its range whatever the
    offsets are; with the check in place no kernel sees them at all."""
    hits = np.full((3, 5), 10**6, np.int64)
    rc, lead, tp = c_sets(gpu_faiss, hits, np.asarray(offsets, np.int64), np.asarray(members, np.int64))
    assert rc == KNN_ERR_INVALID and what in _last_error()
    _untouched(lead, tp)
    # the same members are fine where a set boundary falls between the two that are out of order
    if what == "set members not sorted" and offsets[1] == 2:
        rc, lead, tp = c_sets(gpu_faiss, hits, np.array([0, 1, 2, 4], np.int64), np.asarray(members, np.int64))
        assert rc == 0 and not lead.any() and not tp.any()


def test_set_eval_accepts_repeated_members(gpu_faiss):
    hits = np.array([[4, 4, 5, 9, 3]], np.int64)
    _same_sets(c_sets(gpu_faiss, hits, np.array([0, 5], np.int64), np.array([4, 4, 4, 9, 9], np.int64)), ([2], [3]))


def test_k_past_int32_is_refused(gpu_faiss):
    """No row of 2^31 hits exists here: the check runs before anything is read, so the one-row buffers are never touched."""
    k = 2**31
    hits, scores = np.zeros((1, 4), np.int64), np.zeros((1, 4), np.float32)
    one32, one64 = np.zeros(1, np.int32), np.zeros(1, np.int64)
    rc, *outs = c_remove(gpu_faiss, hits, scores, one64, k=k)
    assert rc == KNN_ERR_INVALID and "k > INT32_MAX" in _last_error()
    _untouched(*outs)
    rc, *outs = c_labels(gpu_faiss, hits, one32, one32, k=k)
    assert rc == KNN_ERR_INVALID and "k > INT32_MAX" in _last_error()
    _untouched(*outs)
    rc, *outs = c_sets(gpu_faiss, hits, np.array([0, 1], np.int64), one64, k=k)
    assert rc == KNN_ERR_INVALID and "k > INT32_MAX" in _last_error()
    _untouched(*outs)
    rc, *outs = c_levels(gpu_faiss, hits, one64, np.zeros((1, 2), np.int32), k=k)
    assert rc == KNN_ERR_INVALID and "k > INT32_MAX" in _last_error()
    _untouched(*outs)
    rc, *outs = c_remove(gpu_faiss, hits, scores, one64, k=1)
    assert rc == KNN_ERR_INVALID
    _untouched(*outs)


def test_wrappers_refuse_wrong_shapes(gpu_faiss):
    from knn_for_homology_amd import evaluation
    hits = np.arange(12, dtype=np.int64).reshape(3, 4)
    scores = np.zeros((3, 4), np.float32)
    for bad_scores in (scores[:, :3], scores[:2], scores.reshape(4, 3), scores.ravel()):
        with pytest.raises(ValueError, match="same shape"):
            evaluation.remove_self_hit(hits, bad_scores)
    for bad_ids in (np.arange(2), np.arange(4), np.arange(3).reshape(3, 1), np.int64(0)):
        with pytest.raises(ValueError, match="self_ids"):
            evaluation.remove_self_hit(hits, scores, bad_ids)
    for k in (0, 1):
        with pytest.raises(ValueError, match="k >= 2"):
            evaluation.remove_self_hit(hits[:, :k], scores[:, :k])
    ldb = np.zeros(12, np.int32)
    for bad_lq in (np.zeros(2, np.int32), np.zeros(4, np.int32), np.zeros((3, 1), np.int32)):
        with pytest.raises(ValueError, match="labels_q"):
            evaluation.label_matches(hits, bad_lq, ldb)
    mapping = np.zeros((12, 4), np.int64)
    for bad_rows in (np.arange(2), np.arange(4), np.arange(3).reshape(1, 3)):
        with pytest.raises(ValueError, match="query_rows"):
            evaluation.compute_is_correct(hits, mapping, bad_rows)
    # and the right shapes still pass
    assert evaluation.remove_self_hit(hits, scores, [0, 4, 8])[0].tolist() == [[1, 2, 3], [5, 6, 7], [9, 10, 11]]
    assert evaluation.label_matches(hits, [0, 0, 1], ldb)[1].tolist() == [4, 4, 0]
    assert evaluation.compute_is_correct(hits, mapping, [0, 1, 2]).all()
