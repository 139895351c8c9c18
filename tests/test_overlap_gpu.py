"""GPU: knn_eval_overlap (csrc/overlap.inc) exactly against tests/overlap_reference.py.

One workgroup of four waves serves a query row: a minimum over the workgroup gives the two lead lengths, (id, membership
bits) pairs are sorted over next_pow2(ka + kb) slots in LDS, the bits of a run of equal ids are OR-ed towards its head
by doubling, and the heads are counted into six classes.  The shapes here sit where that can go wrong: widths around one
wave, one pass of the workgroup and the powers of two of the sort, repeats in other waves and passes than their first
occurrence and runs of every length up to 4096, ids that differ in one half of the word only, rows cut into slabs.
Everything is compared with array_equal; there is no tolerance anywhere."""
from pathlib import Path

import numpy as np
import pytest

import overlap_reference as ref

pytestmark = pytest.mark.gpu

KNOB = "KNN355_EVAL_SLAB_ROWS"
KNN_ERR_INVALID = -1
S32 = -5555  # what the output arrays hold before a call
I64_MIN, I64_MAX = -2**63, 2**63 - 1
GOLDEN = Path(__file__).resolve().parent / "golden" / "reference_overlap.npz"


def _ptr(a):
    return None if a is None else a.ctypes.data


def _last_error():
    from knn_for_homology_amd import _lib
    return _lib.lib().knn_last_error().decode()


def c_overlap(hits_a_, correct_a_, hits_b_, correct_b_, want_tp=True, want_lead=True, **over):
    """the C entry point -> (return code, tp, lead), the outputs pre-filled with the sentinel (None: not asked for);
    `over` replaces arguments by name (ka, kb, nq) or drops a pointer (hits_a=None ...)"""
    from knn_for_homology_amd import _lib
    hits_a = np.ascontiguousarray(hits_a_, np.int64)
    hits_b = np.ascontiguousarray(hits_b_, np.int64)
    correct_a = np.ascontiguousarray(correct_a_, np.uint8)
    correct_b = np.ascontiguousarray(correct_b_, np.uint8)
    nq, ka = hits_a.shape
    tp = np.full((max(nq, 1), 3), S32, np.int32) if want_tp else None
    lead = np.full((max(nq, 1), 3), S32, np.int32) if want_lead else None
    a = dict(hits_a=hits_a, correct_a=correct_a, ka=ka, hits_b=hits_b, correct_b=correct_b, kb=hits_b.shape[1], nq=nq, tp=tp, lead=lead)
    a.update(over)
    rc = _lib.lib().knn_eval_overlap(_ptr(a["hits_a"]), _ptr(a["correct_a"]), a["ka"], _ptr(a["hits_b"]), _ptr(a["correct_b"]), a["kb"],
                                     a["nq"], _ptr(a["tp"]), _ptr(a["lead"]))
    return rc, (tp[:nq] if want_tp else None), (lead[:nq] if want_lead else None)


def _same(got, want):
    rc, tp, lead = got
    assert rc == 0, _last_error()
    if tp is not None:
        assert np.array_equal(tp, want[0]), "tp_out"
    if lead is not None:
        assert np.array_equal(lead, want[1]), "lead_out"


def _check(hits_a, correct_a, hits_b, correct_b):
    want = ref.overlap(hits_a, correct_a, hits_b, correct_b)
    _same(c_overlap(hits_a, correct_a, hits_b, correct_b), want)
    return want[0].tolist(), want[1].tolist()


FLAG_VALUES = np.array([0, 1, 1, 2, 0x80, 0xFF], np.uint8)  # non-zero means set, whatever the value


def _case(rng, nq, ka, kb, nids=None, p_set=0.7):
    """rows of random ids from [-2, nids) in no order (repeats and shared ids are the rule) under random flag bytes; the
    rows' leading runs are made to differ: row 0 as drawn (short runs), the others with flags set up to a random column"""
    nids = max(3, (ka + kb) // 2) if nids is None else nids
    hits_a = rng.integers(-2, nids, (nq, ka)).astype(np.int64)
    hits_b = rng.integers(-2, nids, (nq, kb)).astype(np.int64)
    correct_a = np.where(rng.random((nq, ka)) < p_set, rng.choice(FLAG_VALUES[1:], (nq, ka)), 0).astype(np.uint8)
    correct_b = np.where(rng.random((nq, kb)) < p_set, rng.choice(FLAG_VALUES[1:], (nq, kb)), 0).astype(np.uint8)
    for q in range(1, nq):
        ca, cb = int(rng.integers(0, ka + 1)), int(rng.integers(0, kb + 1))
        correct_a[q, :ca] = rng.choice(FLAG_VALUES[1:], ca)
        correct_b[q, :cb] = rng.choice(FLAG_VALUES[1:], cb)
    return hits_a, correct_a, hits_b, correct_b


# ---- widths around a wave, a pass of the workgroup and the powers of two of the sort -----------------------------------
# sums: 2 | 64, 65, 66 | 127, 128, 129 | 256, 257 | 511, 512, 513 | 1024, 1025 | 2047, 2048, 2049 | 4095, 4096 | and uneven pairs
SHAPES = [(1, 1), (63, 1), (1, 64), (1, 65), (63, 64), (64, 64), (65, 64), (255, 1), (1, 256), (255, 256), (256, 256), (257, 256),
          (257, 767), (257, 768), (1024, 1023), (1023, 1025), (2048, 1), (1, 2048), (2048, 2047), (2048, 2048), (65, 255), (257, 63)]


@pytest.mark.parametrize("ka, kb", SHAPES)
def test_shapes(gpu_faiss, ka, kb):
    """few ids (long runs of equal keys), about as many ids as slots, and ids that hardly ever repeat"""
    rng = np.random.default_rng(1000 * ka + kb)
    for nids in (3, max(3, (ka + kb) // 2), 50 * (ka + kb)):
        _check(*_case(rng, 4, ka, kb, nids=nids))


# ---- repeats --------------------------------------------------------------------------------------------------------------
def test_repeats_in_another_wave_and_another_pass_and_across_the_lists(gpu_faiss):
    """A holds ids 0..99 three times over (every repeat 100 or 200 columns behind its first occurrence: in another wave
    and, from column 256 on, in another pass of the workgroup); only the LAST occurrence of an id is flagged in A, so its
    membership of TA must travel to the head of its run.  B repeats 50..149 across the lists, flagged in its first
    occurrence only."""
    ids_a = np.concatenate([np.arange(100), np.arange(100), np.arange(100)])[None, :]
    flags_a = np.concatenate([np.zeros(200), np.ones(100)])[None, :]
    ids_b = np.concatenate([np.arange(50, 150), np.arange(50, 150), np.arange(300, 400)])[None, :]
    flags_b = np.concatenate([np.ones(100), np.zeros(200)])[None, :]
    tp, lead = _check(ids_a, flags_a, ids_b, flags_b)
    assert tp == [[50, 50, 50]] and lead == [[0, 0, 100]]
    tp, lead = _check(ids_b, flags_b, ids_a, flags_a)  # the lists swapped
    assert tp == [[50, 50, 50]] and lead == [[100, 0, 0]]
    # flags set throughout: the runs are the whole lists, repeats and all
    tp, lead = _check(ids_a, np.ones_like(ids_a), ids_b, np.ones_like(ids_b))
    assert tp == lead == [[50, 50, 150]]


@pytest.mark.parametrize("ka, kb", [(5, 3), (300, 300), (2048, 2048)])
def test_one_id_throughout_and_all_ids_distinct(gpu_faiss, ka, kb):
    """one id in every slot is one run as long as the row -- at 2048 + 2048 the longest there is, every doubling step
    taken -- with a single flagged entry at its far end; then no two slots alike"""
    n = ka + kb
    one_a, one_b = np.full((3, ka), 7, np.int64), np.full((3, kb), 7, np.int64)
    fa, fb = np.zeros((3, ka), np.uint8), np.zeros((3, kb), np.uint8)
    fa[0, -1] = 1              # row 0: flagged in A's last column only
    fb[1, -1] = 3              # row 1: in B's last column only
    fa[2], fb[2] = 1, 1        # row 2: everywhere
    fb[2, -1] = 0              #        but B's last column: B's run stops there, and still holds the id
    tp, lead = _check(one_a, fa, one_b, fb)
    assert tp == [[1, 0, 0], [0, 0, 1], [0, 1, 0]]
    assert lead == [[1, 0, 0] if ka == 1 else [0, 0, 0], [0, 0, 1] if kb == 1 else [0, 0, 0], [0, 1, 0] if kb > 1 else [1, 0, 0]]
    rng = np.random.default_rng(ka)
    ids = np.stack([rng.permutation(n), rng.permutation(n)]).astype(np.int64)
    flags = np.ones((2, n), np.uint8)
    flags[1, ka // 2] = 0      # row 1: A's run ends half way, B's never
    tp, lead = _check(ids[:, :ka], flags[:, :ka], ids[:, ka:], flags[:, ka:])
    assert tp == [[ka, 0, kb], [ka - 1, 0, kb]] and lead == [[ka, 0, kb], [ka // 2, 0, kb]]


@pytest.mark.parametrize("run", [2, 3, 64, 65, 255, 256, 257, 1000, 2049])
def test_runs_of_every_length_carry_their_last_entrys_flag(gpu_faiss, run):
    """ka + kb = 4096 slots cut into runs of `run` equal ids (the last one short); in A only the last entry of a run is
    flagged, in B none: every head must learn of a flag `run - 1` slots away, through every doubling step up to there"""
    ids = (np.arange(4096) // run).astype(np.int64)
    rng = np.random.default_rng(run)
    flags = np.zeros(4096, np.uint8)
    last = np.r_[ids[1:] != ids[:-1], True]
    flags[last] = 1                        # (the sort puts a flagged entry behind the unflagged ones of its id)
    # the flagged entries (2048 at the most) go to A's first columns, the rest follows in no order
    order = np.concatenate([np.flatnonzero(last), rng.permutation(np.flatnonzero(~last))])
    ids, flags = ids[order], flags[order]
    tp, _ = _check(ids[None, :2048], flags[None, :2048], ids[None, 2048:], flags[None, 2048:])
    assert tp == [[-(-4096 // run), 0, 0]]


# ---- id values --------------------------------------------------------------------------------------------------------------
def test_ids_are_whole_int64_values(gpu_faiss):
    """ids that differ in the high half only, in the low half only; 0 and 2^63 - 1 are ordinary ids; negative ids, the most
    negative one among them, are no entries whatever their flags"""
    ha = np.array([[2**32 + 5, 5, 2**33 + 5, 6, 0, I64_MAX, -1, I64_MIN, 2**62]], np.int64)
    hb = np.array([[5, 2**32 + 6, 2**32 + 5, I64_MAX, I64_MIN + 1, 0, 2**62 + 1, -3]], np.int64)
    fa = np.ones_like(ha)
    fb = np.ones_like(hb)
    tp, lead = _check(ha, fa, hb, fb)
    assert tp == lead == [[3, 4, 2]]  # both: 2^32 + 5, 5, 0, 2^63 - 1
    fa[0, 6], fa[0, 7], fb[0, 4] = 0, 0, 0  # zero flags under entries that do not exist end no run
    assert _check(ha, fa, hb, fb) == (tp, lead)
    rng = np.random.default_rng(6)
    low = rng.integers(0, 40, (3, 300)).astype(np.int64)
    high = rng.integers(0, 3, (3, 300)).astype(np.int64) << 32
    ha, ca, hb, cb = _case(rng, 3, 300, 213)
    _check(low + high, ca, (low + high)[:, :213][:, ::-1], cb)  # equal low halves, three high halves
    _check(ha << 40, ca, hb << 40, cb)                          # nothing in the low 40 bits (negative ids stay negative)
    _check(np.where(ha >= 0, I64_MAX - ha, ha), ca, np.where(hb >= 0, I64_MAX - hb, hb), cb)  # the top of the range


def test_rows_without_entries(gpu_faiss):
    rng = np.random.default_rng(8)
    ha, ca, hb, cb = _case(rng, 6, 70, 45)
    ha[0], hb[1] = -1, I64_MIN   # nothing in A; nothing in B
    ha[2], hb[2] = -2, -1        # nothing in both
    ha[3, 1:] = -1               # a single entry each
    hb[3, :-1] = -1
    tp, lead = _check(ha, ca, hb, cb)
    assert tp[0][:2] == [0, 0] and tp[1][1:] == [0, 0] and tp[2] == lead[2] == [0, 0, 0] and sum(tp[3]) <= 2


# ---- flags ------------------------------------------------------------------------------------------------------------------
def test_flags(gpu_faiss):
    rng = np.random.default_rng(9)
    ha, _, hb, _ = _case(rng, 2, 300, 213, nids=200)
    zeros_a, zeros_b = np.zeros(ha.shape, np.uint8), np.zeros(hb.shape, np.uint8)
    tp, lead = _check(ha, zeros_a, hb, zeros_b)               # all zero
    assert tp == lead == [[0, 0, 0]] * 2
    tp, lead = _check(ha, zeros_a + 1, hb, zeros_b + 1)       # all set: the TP sets are the runs
    assert tp == lead and all(row[1] > 0 for row in tp)
    for value in (2, 0x80, 0xFF):                             # values other than 1
        assert _check(ha, zeros_a + value, hb, zeros_b + value) == (tp, lead)
    assert _check(ha, zeros_a + 1, hb, zeros_b)[0] == [[row[0] + row[1], 0, 0] for row in tp]  # flagged in A, not in B
    # an id repeated in one list with mixed flags is in the set; the run takes it only as far as the walk gets
    tp, lead = _check([[3, 3, 4, 3]], [[0, 1, 1, 2]], [[4, 4, 9]], [[7, 0, 1]])
    assert tp == [[1, 1, 1]] and lead == [[0, 0, 1]]


# ---- leading runs -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ka, kb", [(7, 9), (300, 213), (2048, 2048)])
def test_leading_runs(gpu_faiss, ka, kb):
    """the run ends at column 0, at the last column, never; behind an entry that does not exist; with such entries inside"""
    rng = np.random.default_rng(ka)
    ids = np.stack([rng.permutation(ka + kb) for _ in range(6)]).astype(np.int64)  # all distinct: the sizes are the lengths
    ha, hb = ids[:, :ka].copy(), ids[:, ka:].copy()
    ca, cb = np.ones((6, ka), np.uint8), np.ones((6, kb), np.uint8)
    ca[0, 0] = 0                    # row 0: A ends at column 0, B never
    ca[1, -1], cb[1, -1] = 0, 0     # row 1: both end at the last column
    ha[2, 0], ca[2, 0] = -1, 0      # row 2: a missing entry with a zero flag in front: A's run goes on behind it ...
    ca[2, ka // 2 + 1] = 0          #        ... to past the middle
    hb[2, 0], cb[2, 1] = -5, 0      #        B: a missing entry, then the end: an empty run behind a missing entry
    ha[3, 1:ka - 1] = -1            # row 3: missing entries inside the run; it reaches the last column
    cb[3, 2:] = 0                   #        B: two entries long
    ca[4, 1::2] = 0                 # row 4: every other flag zero behind column 0 ...
    ha[4, 1::2] = -1                #        ... under entries that do not exist: the run never ends
    cb[5] = 0                       # row 5: B empty from the start, A whole
    tp, lead = _check(ha, ca, hb, cb)
    mid = ka // 2 + 1
    assert lead[0] == [0, 0, kb] and lead[1] == [ka - 1, 0, kb - 1]
    assert lead[2] == [mid - 1, 0, 0]
    assert lead[3] == [min(ka, 2), 0, min(kb, 2)]
    assert lead[4] == [(ka + 1) // 2, 0, kb] and lead[5] == [ka, 0, 0]


# ---- slabs ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [1, 3, 100])
def test_slabs(gpu_faiss, monkeypatch, rows):
    """7 rows in slabs of 1, 3 and more than there are rows: the results equal the uncut call's.  The knob is read on
    every call."""
    rng = np.random.default_rng(9)
    case = _case(rng, 7, 70, 45)
    want = ref.overlap(*case)
    monkeypatch.delenv(KNOB, raising=False)
    whole = c_overlap(*case)
    monkeypatch.setenv(KNOB, str(rows))
    cut = c_overlap(*case)
    _same(whole, want)
    _same(cut, want)
    assert np.array_equal(whole[1], cut[1]) and np.array_equal(whole[2], cut[2])
    # either output left out: the other is still right, slab by slab
    _same(c_overlap(*case, want_tp=False), want)
    _same(c_overlap(*case, want_lead=False), want)


# ---- a seeded sweep -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(4))
def test_random_sweep(gpu_faiss, seed):
    rng = np.random.default_rng(4343 + seed)
    for _ in range(10):
        nq = int(rng.integers(1, 9))
        ka, kb = (int(rng.choice([1, 2, int(rng.integers(1, 130)), int(rng.integers(1, 700))])) for _ in range(2))
        _check(*_case(rng, nq, ka, kb, nids=int(rng.integers(1, 2 * (ka + kb) + 1)), p_set=float(rng.choice([0.1, 0.7, 0.98]))))


# ---- the Python layer -------------------------------------------------------------------------------------------------------
def test_python_layer_on_the_reference_fixture(gpu_faiss):
    from knn_for_homology_amd.evaluation import HitOverlap, auc1_optimal, compare_hits, last_overlap_ms, tp_overlap_fractions
    g = np.load(GOLDEN)
    got = compare_hits(g["hits_a"], g["correct_a"], g["hits_b"], g["correct_b"])
    assert isinstance(got, HitOverlap) and got.tp.dtype == got.lead.dtype == np.int32 and got.tp.shape == got.lead.shape == (40, 3)
    assert np.array_equal(got.tp, g["tp"]) and np.array_equal(got.lead, g["lead"])
    nq = len(g["hits_a"])
    want = [int(t) / (10 * nq) for t in g["tp_totals"]]  # the expressions of pfam.py:367-369 on the reference's totals
    fractions = tp_overlap_fractions(got)
    assert np.array_equal(np.array(fractions, np.float64).view(np.uint64), np.array(want, np.float64).view(np.uint64))
    auc1 = auc1_optimal(got, g["family_sizes"])
    assert auc1.dtype == np.float64 and np.array_equal(auc1.view(np.uint64), g["auc1s_optimal"].view(np.uint64))
    # A's flags from elsewhere (bool): the sets follow each list's own flags
    alt = compare_hits(g["hits_a"], g["correct_a_alt"].astype(bool), g["hits_b"], g["correct_b"])
    assert np.array_equal(alt.tp, g["tp_alt"])
    assert tp_overlap_fractions(alt, per_query=7) == tuple(int(t) / (7 * nq) for t in g["tp_alt_totals"])
    ms = last_overlap_ms()
    assert sorted(ms) == ["download_ms", "kernel_ms", "upload_ms"] and all(v >= 0 for v in ms.values())


def test_python_layer_checks_its_arguments(gpu_faiss):
    from knn_for_homology_amd.evaluation import auc1_optimal, compare_hits
    ha, hb = np.zeros((3, 4), np.int32), np.ones((3, 5), np.int64)  # (any integer type: converted to int64)
    ca, cb = np.ones((3, 4), bool), np.ones((3, 5), np.float32)      # (any type: non-zero means set)
    got = compare_hits(ha, ca, hb, cb)
    assert got.tp.tolist() == got.lead.tolist() == [[1, 0, 1]] * 3
    assert auc1_optimal(got, [2, 4, 8]).tolist() == [1.0, 0.5, 0.25]
    with pytest.raises(ValueError):
        compare_hits(ha, ca[:, :-1], hb, cb)
    with pytest.raises(ValueError):
        compare_hits(ha, ca, hb[:-1], cb[:-1])
    with pytest.raises(ValueError):
        compare_hits(ha[0], ca[0], hb[0], cb[0])
    with pytest.raises(ValueError):
        auc1_optimal(got, [2, 4])
    with pytest.raises(RuntimeError):
        compare_hits(np.zeros((1, 2049), np.int64), np.zeros((1, 2049), bool), hb[:1], cb[:1])


# ---- errors: refused on the host, nothing allocated or launched, the outputs as they were --------------------------------
def _refused(got, what):
    rc, tp, lead = got
    assert rc == KNN_ERR_INVALID and what in _last_error(), _last_error()
    assert (tp is None or (tp == S32).all()) and (lead is None or (lead == S32).all())


def test_refusals(gpu_faiss):
    ha, hb = np.zeros((3, 4), np.int64), np.ones((3, 5), np.int64)
    ca, cb = np.ones((3, 4), np.uint8), np.ones((3, 5), np.uint8)
    for k in (0, -1, 2049):
        _refused(c_overlap(ha, ca, hb, cb, ka=k), "ka outside")
        _refused(c_overlap(ha, ca, hb, cb, kb=k), "kb outside")
    _refused(c_overlap(ha, ca, hb, cb, nq=-1), "negative nq")
    for name in ("hits_a", "correct_a", "hits_b", "correct_b"):
        _refused(c_overlap(ha, ca, hb, cb, **{name: None}), "null " + name)
    _refused(c_overlap(ha, ca, hb, cb, want_tp=False, want_lead=False), "tp_out and lead_out")
    # nq = 0 returns before any pointer is looked at
    assert c_overlap(ha, ca, hb, cb, nq=0, hits_a=None, correct_a=None, hits_b=None, correct_b=None, want_tp=False, want_lead=False)[0] == 0
    got = c_overlap(ha, ca, hb, cb, nq=0)
    assert got[0] == 0 and (got[1] == S32).all() and (got[2] == S32).all()
    # and the same arguments pass once they are right
    got = c_overlap(ha, ca, hb, cb)
    assert got[0] == 0 and got[1].tolist() == got[2].tolist() == [[1, 0, 1]] * 3
