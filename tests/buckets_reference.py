"""The contracts of knn_eval_bucket_counts and knn_eval_hit_curve (include/knn355.h), restated in plain Python.

Loops, Python floats (IEEE doubles) and `bisect` only: no vectorised shortcut that could hide an edge rule.  The GPU
tests compare the library against these functions bit for bit; tests/test_buckets_reference.py compares these functions
against what the reference's own code produced (tests/golden/reference_buckets.npz).
"""
import math
from bisect import bisect_left

import numpy as np


def default_edges(smoothness):
    """the reference's own expressions (pfam/proteins.py:692, 697-699)"""
    lo = np.linspace(0, 1 - (1 / smoothness), smoothness)
    return lo, lo + (1 / smoothness)


def bucket_counts(correct, scores, limit, lo, hi):
    """-> (count, correct) int64 [nb].  Cell s is in bucket b iff lo[b] < float(s) and float(s) <= hi[b].

    With lo and hi sorted and lo <= hi the buckets of a cell are h .. a - 1, a = #{i : lo[i] < s}, h = #{i : hi[i] < s};
    the two counts are taken with bisect and every bucket of the range is then re-checked against the definition."""
    lo = [float(x) for x in lo]
    hi = [float(x) for x in hi]
    nb = len(lo)
    count = [0] * nb
    right = [0] * nb
    for q in range(len(scores)):
        for c in range(limit):
            s = float(scores[q][c])
            if s != s:
                continue  # NaN: in no bucket
            a = bisect_left(lo, s)  # the number of entries below s
            h = bisect_left(hi, s)
            for b in range(h, a):
                assert lo[b] < s and s <= hi[b]
                count[b] += 1
                if correct[q][c] != 0:
                    right[b] += 1
            assert not any(lo[b] < s <= hi[b] for b in (h - 1, a) if 0 <= b < nb)
    return np.asarray(count, np.int64), np.asarray(right, np.int64)


def bucket_counts_bruteforce(correct, scores, limit, lo, hi):
    """the definition itself, every cell against every bucket (for small cases: checks bucket_counts' range rule)"""
    nb = len(lo)
    count = [0] * nb
    right = [0] * nb
    for q in range(len(scores)):
        for c in range(limit):
            s = float(scores[q][c])
            for b in range(nb):
                if float(lo[b]) < s and s <= float(hi[b]):
                    count[b] += 1
                    right[b] += 1 if correct[q][c] != 0 else 0
    return np.asarray(count, np.int64), np.asarray(right, np.int64)


def precision_sem(count, right):
    """-> (precision, sem) float64 [nb]: c / n, NaN for n = 0; sqrt(c (n - c) / (n (n - 1))) / sqrt(n), NaN for n < 2"""
    precision, sem = [], []
    for n, c in zip((int(x) for x in count), (int(x) for x in right)):
        precision.append(float(c) / float(n) if n else math.nan)
        if n < 2:
            sem.append(math.nan)
        else:
            # every operand is an integer below 2^53 for the sizes in use, each operation one rounding
            sem.append(math.sqrt(float(c) * float(n - c) / (float(n) * float(n - 1))) / math.sqrt(float(n)))
    return np.asarray(precision, np.float64), np.asarray(sem, np.float64)


def reference_arrays(count, right):
    """(precision, sem) of the non-empty buckets, in order: what the reference's loop appends"""
    precision, sem = precision_sem(count, right)
    keep = np.asarray(count) > 0
    return precision[keep], sem[keep]


def hit_curve(correct, totals, limit):
    """-> (mean float64 [limit], row_correct int64 [nq], column_correct int64 [limit]); S(j) adds t(q, j) in row order"""
    nq = len(correct)
    sums = [0.0] * limit
    rows = [0] * nq
    cols = [0] * limit
    for q in range(nq):
        total = float(int(totals[q]))
        c = 0
        for j in range(limit):
            if correct[q][j] != 0:
                c += 1
            sums[j] = sums[j] + float(c) / total
            cols[j] += c
        rows[q] = c
    return (np.asarray([s / float(nq) for s in sums], np.float64), np.asarray(rows, np.int64), np.asarray(cols, np.int64))


def recall_per_query(correct, totals, limit):
    """the row counts over the totals, numpy's own division (pfam/proteins.py:478)"""
    return hit_curve(correct, totals, limit)[1] / np.asarray(totals)
