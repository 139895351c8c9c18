"""The contracts of knn_eval_sets_matrix and knn_eval_pr_curve (include/knn355.h), restated in plain Python.

Written from the header, one query at a time with Python floats and ints (a Python float is an IEEE double, `/` on two
of them is the correctly rounded division, `+` the correctly rounded sum); numpy only carries the arrays in and out and
turns a float32 score into its double.  Nothing is shared with the library.  Used by tests/test_pr_curve_reference.py
(CPU, against what the reference's own code produced) and tests/test_pr_curve_gpu.py (bit for bit)."""
import math

import numpy as np

BLOCK = 256  # queries per block of the summation order


def sets_matrix(hits, offsets, members):
    """-> uint8 [nq, k]: 1 where hits[r][j] is one of members[offsets[r] : offsets[r + 1]]"""
    hits = np.asarray(hits, np.int64)
    nq, k = hits.shape
    assert len(offsets) == nq + 1
    out = np.zeros((nq, k), np.uint8)
    for r in range(nq):
        mine = set(int(m) for m in members[int(offsets[r]):int(offsets[r + 1])])
        for j in range(k):
            out[r, j] = 1 if int(hits[r, j]) in mine else 0
    return out


def query_terms(correct_row, score_row, total, thresholds):
    """one query -> per threshold (n, tp, P, R); the rows are already cut to `limit` cells"""
    cells = [(float(s), bool(c)) for s, c in zip(score_row, correct_row)]  # float(): the float32's double, exactly
    out = []
    for t in thresholds:
        picked = [c for s, c in cells if s > t]  # strict, in double; False for a NaN score
        n, tp = len(picked), sum(picked)
        out.append((n, tp, (float(tp) / float(n)) if n else 1.0, float(tp) / float(total)))
    return out


def block_order_sum(terms):
    """the contract's sum of one term per query: blocks of 256 consecutive queries, each block from +0.0 in row order,
    then the block sums from +0.0 in block order"""
    s = 0.0
    for b0 in range(0, len(terms), BLOCK):
        bs = 0.0
        for x in terms[b0:b0 + BLOCK]:
            bs = bs + x
        s = s + bs
    return s


def pr_curve(correct, scores, limit, totals, thresholds):
    """-> (precision float64 [nthr], recall float64 [nthr], selected int64, tp int64, empty int64)"""
    correct = np.asarray(correct)
    scores = np.asarray(scores, np.float32)
    nq, k = scores.shape
    thresholds = [float(t) for t in thresholds]
    nthr = len(thresholds)
    assert correct.shape == scores.shape and nq >= 1 and 1 <= limit <= k and len(totals) == nq and 1 <= nthr <= 4096
    assert all(int(t) >= 1 for t in totals)
    assert not any(math.isnan(t) for t in thresholds) and all(a <= b for a, b in zip(thresholds, thresholds[1:]))
    per_query = [query_terms(correct[q, :limit], scores[q, :limit], int(totals[q]), thresholds) for q in range(nq)]
    precision = np.empty(nthr, np.float64)
    recall = np.empty(nthr, np.float64)
    selected = np.empty(nthr, np.int64)
    tps = np.empty(nthr, np.int64)
    empty = np.empty(nthr, np.int64)
    for j in range(nthr):
        precision[j] = block_order_sum([per_query[q][j][2] for q in range(nq)]) / float(nq)
        recall[j] = block_order_sum([per_query[q][j][3] for q in range(nq)]) / float(nq)
        selected[j] = sum(per_query[q][j][0] for q in range(nq))
        tps[j] = sum(per_query[q][j][1] for q in range(nq))
        empty[j] = sum(1 for q in range(nq) if per_query[q][j][0] == 0)
    return precision, recall, selected, tps, empty


def three_block_case():
    """513 queries of one cell, one threshold, every cell selected.  Recall terms: row 0 is 1.0; rows 1 .. 257 are
    2**-53 (one correct hit of 2**53 homologues); rows 258 .. 511 are 0; row 512 is 2**-53.
    Block sums in row order: block 0 is 1.0 (1.0 + 2**-53 is a tie and rounds to the even 1.0, 255 times over), block 1
    is 2 * 2**-53 = 2**-52, block 2 is 2**-53.  Block order: 1.0 + 2**-52 is exact; adding 2**-53 is a tie between
    1 + 2**-52 (odd) and 1 + 2**-51 (even): 1 + 2**-51.  One running sum over all rows stays at 1.0."""
    nq = 513
    correct = np.ones((nq, 1), np.uint8)
    correct[258:512] = 0
    totals = np.full(nq, 2**53, np.int64)
    totals[0] = 1
    scores = np.ones((nq, 1), np.float32)
    terms = [1.0] + [2.0 ** -53] * 257 + [0.0] * 254 + [2.0 ** -53]
    return correct, scores, totals, terms
