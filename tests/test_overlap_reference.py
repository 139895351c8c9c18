"""CPU: tests/overlap_reference.py (the restatement of knn_eval_overlap's contract that the GPU tests compare against)
gives exactly what the reference's own loops gave (tests/golden/reference_overlap.npz, written by make_overlap_golden.py
from pfam/pfam.py:349-363 and 602-622), per query and in totals, and does what the contract says where the fixture cannot
go: negative ids other than -1, flags other than 0 and 1, rows without entries in both lists."""
from pathlib import Path

import numpy as np
import pytest

import overlap_reference as ref

GOLDEN = Path(__file__).resolve().parent / "golden" / "reference_overlap.npz"


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def test_tp_overlap_is_the_reference_loop(golden):
    g = golden
    tp, _ = ref.overlap(g["hits_a"], g["correct_a"], g["hits_b"], g["correct_b"])
    assert tp.dtype == np.int32 and np.array_equal(tp, g["tp"])
    assert np.array_equal(tp.sum(axis=0, dtype=np.int64), g["tp_totals"])
    # flags of A that disagree with B's about shared ids, and among an id's repeats
    tp_alt, _ = ref.overlap(g["hits_a"], g["correct_a_alt"], g["hits_b"], g["correct_b"])
    assert np.array_equal(tp_alt, g["tp_alt"]) and not np.array_equal(tp_alt, tp)
    assert np.array_equal(tp_alt.sum(axis=0, dtype=np.int64), g["tp_alt_totals"])


def test_leading_runs_are_the_reference_loop(golden):
    g = golden
    _, lead = ref.overlap(g["hits_a"], g["correct_a"], g["hits_b"], g["correct_b"])
    assert lead.dtype == np.int32 and np.array_equal(lead, g["lead"])
    auc1 = lead.sum(axis=1, dtype=np.int64) / g["family_sizes"]
    assert auc1.dtype == np.float64 and np.array_equal(auc1.view(np.uint64), g["auc1s_optimal"].view(np.uint64))


def test_fixture_holds_the_cases(golden):
    g = golden
    ha, hb, ca, cb = g["hits_a"], g["hits_b"], g["correct_a"], g["correct_b"]
    assert ha.shape == (40, 30) and hb.shape == (40, 40)
    assert ((ha < 0).any(axis=1) & (ha[:, -1] < 0)).sum() > 10 and (ha < 0).all(axis=1).any() and (hb < 0).all(axis=1).any()
    assert any(len(set(a[a >= 0]) & set(b[b >= 0])) > 5 for a, b in zip(ha, hb))                    # ids shared between the lists
    assert any(len(set(a[a >= 0])) < (a >= 0).sum() for a in ha)                                     # repeats inside a list
    assert (g["tp"].sum(axis=1) == 0).sum() >= 4                                                     # rows with no true positive
    whole = [(a >= 0).any() and (c[a >= 0] != 0).all() for a, c in zip(ha, ca)]
    assert sum(whole) >= 4                                                                           # the run is the whole list
    first = [int(np.flatnonzero(b >= 0)[0]) if (b >= 0).any() else -1 for b in hb]
    assert sum(f >= 0 and c[f] == 0 for f, c in zip(first, cb)) >= 4                                 # the run is empty
    assert any((a >= 0).any() and a[0] < 0 for a in ha)                                              # no entry in front of the run
    assert any(b[1] < 0 and b[0] >= 0 and b[2] >= 0 and c[0] and c[2] for b, c in zip(hb, cb))       # no entry inside the run
    assert ((ha < 0) & (ca != 0)).any()                                                              # a set flag under no entry


# ---- hand-typed rows ----------------------------------------------------------------------------------------------------
def _one(hits_a, correct_a, hits_b, correct_b):
    tp, lead = ref.overlap(np.array([hits_a], np.int64), np.array([correct_a], np.uint8), np.array([hits_b], np.int64),
                           np.array([correct_b], np.uint8))
    return tp[0].tolist(), lead[0].tolist()


def test_an_id_is_in_the_sets_its_own_lists_flags_put_it_in():
    # 5 is flagged in A only, 6 in both, 7 in B only; 8 is in both lists and flagged in neither
    tp, lead = _one([5, 6, 8], [1, 1, 0], [5, 6, 7, 8], [0, 1, 1, 0])
    assert tp == [1, 1, 1] and lead == [2, 0, 0]  # A's run is 5, 6; B's ends at column 0
    # a repeat with mixed flags is in the set; in the run only as far as the walk gets
    tp, lead = _one([3, 3, 4, 3], [0, 1, 1, 2], [4, 4, 9], [7, 0, 1])
    assert tp == [1, 1, 1] and lead == [0, 0, 1]


def test_entries_that_do_not_exist():
    m = -2**63
    # -1, -2 and the most negative id are no entries: they end no run and are in no set, whatever their flags
    tp, lead = _one([-1, 2, m, 3, 4], [0, 1, 0, 1, 0], [2, -2, 5], [9, 1, 1])
    assert tp == [1, 1, 1] and lead == [1, 1, 1]
    assert _one([-1, -1], [1, 1], [4, 4], [1, 1]) == ([0, 0, 1], [0, 0, 1])
    assert _one([4, 5], [1, 1], [-1], [0]) == ([2, 0, 0], [2, 0, 0])
    assert _one([-1], [1], [-7], [1]) == ([0, 0, 0], [0, 0, 0])
    # id 0 and the largest id are ordinary ids; ids that differ in one half only are different ids
    tp, lead = _one([0, 2**63 - 1, 2**32 + 1, 1], [1] * 4, [2**63 - 1, 1, 2**33 + 1, 0], [1] * 4)
    assert tp == [1, 3, 1] and lead == [1, 3, 1]
