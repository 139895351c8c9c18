"""knn_eval_overlap's contract (include/knn355.h) restated in plain Python sets, one row at a time: what the GPU tests
compare against with array_equal, and what tests/test_overlap_reference.py holds against the reference's own loops.
Nothing here is fast and nothing has a tolerance."""
import numpy as np


def tp_set(hits_row, correct_row):
    """the distinct ids of the existing entries (id >= 0) whose flag is non-zero"""
    return {int(h) for h, c in zip(hits_row, correct_row) if h >= 0 and c != 0}


def lead_set(hits_row, correct_row):
    """the distinct ids walked in column order up to, and without, the first existing entry whose flag is zero; an entry
    that does not exist is stepped over"""
    out = set()
    for h, c in zip(hits_row, correct_row):
        if h < 0:
            continue
        if c == 0:
            break
        out.add(int(h))
    return out


def split(a, b):
    return [len(a - b), len(a & b), len(b - a)]


def overlap(hits_a, correct_a, hits_b, correct_b):
    """-> (tp int32 [nq, 3], lead int32 [nq, 3])"""
    hits_a, hits_b = np.asarray(hits_a, np.int64), np.asarray(hits_b, np.int64)
    correct_a, correct_b = np.asarray(correct_a), np.asarray(correct_b)
    assert hits_a.ndim == 2 and hits_a.shape == correct_a.shape and hits_b.shape == correct_b.shape and len(hits_a) == len(hits_b)
    nq = len(hits_a)
    tp = np.zeros((nq, 3), np.int32)
    lead = np.zeros((nq, 3), np.int32)
    for q in range(nq):
        ha, ca, hb, cb = hits_a[q].tolist(), correct_a[q].tolist(), hits_b[q].tolist(), correct_b[q].tolist()
        tp[q] = split(tp_set(ha, ca), tp_set(hb, cb))
        lead[q] = split(lead_set(ha, ca), lead_set(hb, cb))
    return tp, lead
