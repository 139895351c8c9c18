"""CPU: the contract of the four evaluation passes as tests/consumers_reference.py states it -- hand-worked rows with
the expected arrays written out, agreement with the reference's loops (oracle/consumers_oracle.py) wherever every id
is inside its table, and the one place where the two part: a loop that indexes a Python list or an array with the
"no hit" id -1 reads the last element, the contract says -1 matches nothing."""
import numpy as np

from consumers_reference import label_eval, levels_eval, remove_self_hit, set_eval

NAN_PAYLOAD = np.array([0x7FC12345], np.uint32).view(np.float32)[0]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- by hand ---------------------------------------------------------------------------------------------------------
def test_remove_self_hit_by_hand():
    hits = np.array([[7, 1, 2, 3],      # self first
                     [1, 2, 8, 3],      # self in the middle
                     [1, 2, 3, 9],      # self last
                     [1, 2, 3, 4],      # self absent: the last element goes, counted missing
                     [5, 6, 5, 5],      # self three times: only the first occurrence goes
                     [-1, 4, -1, 0]],   # no-hit ids are ordinary elements
                    np.int64)
    scores = np.arange(24, dtype=np.float32).reshape(6, 4)
    scores[1, 0], scores[1, 1], scores[1, 3] = NAN_PAYLOAD, -0.0, -np.inf
    self_ids = np.array([7, 8, 9, 10, 5, 4], np.int64)
    ho, so, missing = remove_self_hit(hits, scores, self_ids)
    assert ho.dtype == np.int64 and so.dtype == np.float32 and missing.dtype == np.int32
    assert ho.tolist() == [[1, 2, 3], [1, 2, 3], [1, 2, 3], [1, 2, 3], [6, 5, 5], [-1, -1, 0]]
    assert missing.tolist() == [0, 0, 0, 1, 0, 0]
    assert so[0].tolist() == [1, 2, 3] and so[2].tolist() == [8, 9, 10] and so[3].tolist() == [12, 13, 14]
    assert so[4].tolist() == [17, 18, 19] and so[5].tolist() == [20, 22, 23]
    assert _bits(so[1]).tolist() == [0x7FC12345, 0x80000000, 0xFF800000]  # payload, sign of zero and -inf moved as bits
    assert np.array_equal(hits[0], [7, 1, 2, 3]), "the inputs are left alone"
    # k = 2: one element survives
    ho, so, missing = remove_self_hit(np.array([[3, 0], [0, 3], [1, 2]]), np.array([[1, 2], [3, 4], [5, 6]], np.float32), [0, 0, 0])
    assert ho.tolist() == [[3], [3], [1]] and so.tolist() == [[1], [4], [5]] and missing.tolist() == [0, 0, 1]


def test_label_eval_by_hand():
    labels_db = np.array([5, 5, 6, 5, -2147483648, 2147483647], np.int32)
    labels_q = np.array([5, 5, 6, 5, -2147483648, 2147483647, 5], np.int32)
    hits = np.array([[0, 1, 3, 0],      # every hit matches: lead == k
                     [2, 0, 1, 3],      # first hit foreign: lead 0, tp 3
                     [2, 2, 0, 2],      # foreign at 2
                     [0, -1, 1, 3],     # -1 cuts the run and is not counted
                     [4, 4, 5, 4],      # INT32_MIN matches itself only
                     [5, 4, 5, 5],
                     [6, 7, -2, -9223372036854775808]],  # nb, nb + 1, -2, INT64_MIN: nothing matches
                    np.int64)
    ic, lead, tp = label_eval(hits, labels_q, labels_db)
    assert ic.dtype == np.uint8 and lead.dtype == np.int32 and tp.dtype == np.int32
    assert ic.tolist() == [[1, 1, 1, 1], [0, 1, 1, 1], [1, 1, 0, 1], [1, 0, 1, 1], [1, 1, 0, 1], [1, 0, 1, 1], [0, 0, 0, 0]]
    assert lead.tolist() == [4, 0, 2, 1, 2, 1, 0]
    assert tp.tolist() == [4, 3, 3, 3, 3, 3, 0]
    # an empty database: nothing can match
    ic, lead, tp = label_eval(np.array([[0, -1, 1]]), np.array([0], np.int32), np.zeros(0, np.int32))
    assert ic.tolist() == [[0, 0, 0]] and lead.tolist() == [0] and tp.tolist() == [0]


def test_set_eval_by_hand():
    #            set 0     set 1 (empty)  set 2   set 3 (last; 9 is the largest member)
    members = np.array([2, 4, 6,          6, 7,   1, 9], np.int64)
    offsets = np.array([0, 3, 3, 5, 7], np.int64)
    hits = np.array([[2, 6, 4, 7],      # 7 is past set 0's end and is set 2's second member: no match
                     [2, 6, 4, 7],      # empty set
                     [6, 7, 6, 1],      # a repeated hit counts again; 1 belongs to the next set only
                     [9, 1, 10, -1]],   # 10 is larger than every member of the last set; -1 is no member
                    np.int64)
    lead, tp = set_eval(hits, offsets, members)
    assert lead.dtype == np.int32 and tp.dtype == np.int32
    assert lead.tolist() == [3, 0, 3, 2] and tp.tolist() == [3, 0, 3, 2]
    # a hit larger than all of set 0 and equal to the first member of set 1
    lead, tp = set_eval(np.array([[1, 5], [5, 1]]), np.array([0, 2, 3]), np.array([0, 1, 5]))
    assert lead.tolist() == [1, 1] and tp.tolist() == [1, 1]
    # all sets empty
    lead, tp = set_eval(np.array([[0, 1], [2, 3]]), np.zeros(3, np.int64), np.zeros(0, np.int64))
    assert lead.tolist() == [0, 0] and tp.tolist() == [0, 0]


def test_levels_eval_by_hand():
    mapping = np.array([[1, 10, 100],
                        [1, 10, 101],
                        [1, 11, 100],   # level 2 equal to row 0 although level 1 differs: levels are independent
                        [2, 10, 100]], np.int32)
    hits = np.array([[0, 1, 2, 3, -1, 4],
                     [3, 2, 1, 0, 5, -7]], np.int64)
    out = levels_eval(hits, np.array([0, 3]), mapping)
    assert out.dtype == np.uint8 and out.shape == (2, 3, 6)  # [q][l][j]
    assert out[0].tolist() == [[1, 1, 1, 0, 0, 0],
                               [1, 1, 0, 1, 0, 0],
                               [1, 0, 1, 1, 0, 0]]
    assert out[1].tolist() == [[1, 0, 0, 0, 0, 0],
                               [1, 0, 1, 1, 0, 0],
                               [1, 1, 0, 1, 0, 0]]
    # the query's row is query_rows[q], not q
    assert levels_eval(np.array([[1]]), np.array([1]), mapping).tolist() == [[[1], [1], [1]]]
    assert levels_eval(np.array([[1]]), np.array([0]), mapping).tolist() == [[[1], [1], [0]]]


# ---- against the reference's loops, every id inside its table ----------------------------------------------------------
def _inside_hits(rng, nq, k, nb):
    return rng.integers(0, nb, (nq, k)).astype(np.int64)


def test_remove_self_hit_agrees_with_the_loops():
    from oracle import consumers_oracle as co
    rng = np.random.default_rng(10)
    nq, k, nb = 60, 9, 12  # few ids: rows hold their self id never, once and several times
    hits = _inside_hits(rng, nq, k, nb)
    scores = rng.standard_normal((nq, k)).astype(np.float32)
    self_ids = rng.integers(0, nb, nq).astype(np.int64)
    hits[::5, 0] = self_ids[::5]
    ho, so, missing = remove_self_hit(hits, scores, self_ids)
    oh, os_, bogus = co.remove_self_hit(hits, scores, self_ids)
    assert np.array_equal(ho, oh) and np.array_equal(_bits(so), _bits(os_))
    assert 0 < bogus == int(missing.sum()) < nq
    assert (missing == [s not in row for s, row in zip(self_ids, hits.tolist())]).all()


def _family_tables(rng, nq, nb, nfam):
    ldb = rng.integers(0, nfam, nb).astype(np.int32)
    ldb[:nfam] = np.arange(nfam)  # every family has a member: the loops divide by its size
    lq = rng.integers(0, nfam, nq).astype(np.int32)
    train_ids = [f"t{i}" for i in range(nb)]
    test_ids = [f"q{i}" for i in range(nq)]
    fam = {f"t{i}": f"F{ldb[i]}" for i in range(nb)}
    fam.update({f"q{i}": f"F{lq[i]}" for i in range(nq)})
    size = np.bincount(ldb, minlength=nfam)[lq]
    return lq, ldb, train_ids, test_ids, fam, size


def test_label_eval_agrees_with_the_loops():
    from oracle import consumers_oracle as co
    rng = np.random.default_rng(11)
    nq, k, nb, nfam = 50, 12, 40, 3
    lq, ldb, train_ids, test_ids, fam, size = _family_tables(rng, nq, nb, nfam)
    hits = _inside_hits(rng, nq, k, nb)
    hits[0] = np.flatnonzero(ldb == lq[0])[0]  # one row of matches only
    ic, lead, tp = label_eval(hits, lq, ldb)
    assert lead[0] == k and tp[0] == k and 0 in lead and (lead < tp).any()
    auc1s, tps = co.evaluate(fam, train_ids, test_ids, hits)
    assert auc1s == [int(a) / int(s) for a, s in zip(lead, size)]
    assert tps == [int(t) / int(s) for t, s in zip(tp, size)]
    want = co.compute_tps_comulative(fam, train_ids, test_ids, hits)
    assert np.array_equal((ic.astype(bool).cumsum(axis=1) / size.repeat(k).reshape(nq, k)).mean(axis=0), want)


def _homology(rng, hits, nb):
    nq = hits.shape[0]
    target_ids = [f"t{i}" for i in range(nb)]
    queries = [f"q{i}" for i in range(nq)]
    homologous, offsets, members = {}, [0], []
    for i in range(nq):
        rows = set(rng.choice(nb, rng.integers(0, 8), replace=False).tolist()) | set(hits[i, :rng.integers(0, 5)].tolist())
        homologous[queries[i]] = {target_ids[j] for j in rows}
        members += sorted(rows)
        offsets.append(len(members))
    return target_ids, queries, homologous, np.asarray(offsets, np.int64), np.asarray(members, np.int64)


def test_set_eval_agrees_with_the_loops():
    from oracle import consumers_oracle as co
    rng = np.random.default_rng(12)
    nq, k, nb = 50, 10, 30
    hits = _inside_hits(rng, nq, k, nb)
    target_ids, queries, homologous, offsets, members = _homology(rng, hits, nb)
    lead, tp = set_eval(hits, offsets, members)
    sizes = np.maximum(np.diff(offsets), 1)
    assert np.array_equal(lead / sizes, co.compute_auc1(hits, homologous, queries, target_ids))
    assert (lead > 0).any() and (lead == 0).any() and (tp > lead).any()
    assert tp.tolist() == [sum(target_ids[h] in homologous[q] for h in row) for q, row in zip(queries, hits.tolist())]


def test_levels_eval_agrees_with_the_loops():
    from oracle import consumers_oracle as co
    rng = np.random.default_rng(13)
    nq, k, n = 25, 7, 25
    mapping = rng.integers(0, 3, (n, 4)).astype(np.int32)
    hits = _inside_hits(rng, nq, k, n)
    out = levels_eval(hits, np.arange(nq), mapping)
    want = co.compute_is_correct(hits, mapping)
    assert want.shape == (nq, 4, k) and np.array_equal(out.astype(bool), want) and 0 < out.mean() < 1


# ---- where the loops and the contract part ---------------------------------------------------------------------------
def test_remove_self_hit_has_no_table_to_index():
    """remove_self_hit compares ids and indexes nothing with them: rows of -1 are where the loops and the contract could
    part and do not -- a -1 is an element like any other, a self id of -1 included."""
    from oracle import consumers_oracle as co
    hits = np.array([[-1, 2, -1, 0], [3, -1, 1, -1], [-1, -1, -1, -1]], np.int64)
    scores = np.arange(12, dtype=np.float32).reshape(3, 4)
    self_ids = np.array([0, 1, -1], np.int64)
    ho, so, missing = remove_self_hit(hits, scores, self_ids)
    assert ho.tolist() == [[-1, 2, -1], [3, -1, -1], [-1, -1, -1]]
    assert so.tolist() == [[0, 1, 2], [4, 5, 7], [9, 10, 11]] and missing.tolist() == [0, 0, 0]
    oh, os_, bogus = co.remove_self_hit(hits, scores, self_ids)
    assert np.array_equal(ho, oh) and np.array_equal(so, os_) and bogus == 0


def test_label_eval_parts_from_the_loops_at_minus_one():
    from oracle import consumers_oracle as co
    train_ids, test_ids = ["t0", "t1", "t2"], ["q0"]
    fam = {"t0": "A", "t1": "B", "t2": "A", "q0": "A"}
    hits = np.array([[0, -1, 2, 1]], np.int64)
    auc1s, tps = co.evaluate(fam, train_ids, test_ids, hits)
    assert auc1s == [3 / 2] and tps == [3 / 2]  # train_ids[-1] is t2, family A: three "matches" in a family of two
    ic, lead, tp = label_eval(hits, np.array([0], np.int32), np.array([0, 1, 0], np.int32))
    assert ic.tolist() == [[1, 0, 1, 0]] and lead.tolist() == [1] and tp.tolist() == [2]


def test_set_eval_parts_from_the_loops_at_minus_one():
    from oracle import consumers_oracle as co
    target_ids = ["t0", "t1", "t2"]
    hits = np.array([[0, -1, 2, 1]], np.int64)
    assert co.compute_auc1(hits, {"q0": {"t0", "t2"}}, ["q0"], target_ids).tolist() == [3 / 2]  # target_ids[-1] is t2
    lead, tp = set_eval(hits, np.array([0, 2]), np.array([0, 2]))
    assert lead.tolist() == [1] and tp.tolist() == [2]


def test_levels_eval_parts_from_the_loops_at_minus_one():
    from oracle import consumers_oracle as co
    mapping = np.array([[1, 5], [2, 6], [1, 6]], np.int32)
    hits = np.array([[-1, 2], [2, -1], [-1, -1]], np.int64)
    # mapping[-1] is row 2
    assert co.compute_is_correct(hits, mapping).astype(int).tolist() == [[[1, 1], [0, 0]], [[0, 0], [1, 1]], [[1, 1], [1, 1]]]
    assert levels_eval(hits, np.arange(3), mapping).tolist() == [[[0, 1], [0, 0]], [[0, 0], [1, 0]], [[0, 0], [0, 0]]]
