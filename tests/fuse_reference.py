"""A plain per-row restatement of knn_eval_fuse's contract (include/knn355.h), for the tests.

Written from the contract, one row at a time, with Python lists, sets and a stable sort; nothing here is shared with the
library.  Scores travel as their 64-bit patterns, so that "the input's bits" can be checked for NaN payloads and the
two zeros as well."""
import math

import numpy as np

PREFIX_FILL, SORTED_UNION = 0, 1
DBL_MAX = float(np.finfo(np.float64).max)


def row_entries(hits_a, keep_a, hits_b):
    """the existing entries of one row as (position, id) in order of position"""
    ka = len(hits_a)
    out = [(j, int(hits_a[j])) for j in range(ka) if hits_a[j] >= 0 and (keep_a is None or keep_a[j])]
    return out, [(ka + j, int(hits_b[j])) for j in range(len(hits_b)) if hits_b[j] >= 0]


def union_order(entries, scores, ascending):
    """the entries of one row in the contract's order; scores is the row's concatenated float64 scores by position"""
    def sort_key(e):
        s = float(scores[e[0]])
        if math.isnan(s):
            return (1, 0.0)
        return (0, (s if ascending else -s) + 0.0)  # Python compares -0.0 == 0.0: the zeros tie
    return sorted(entries, key=sort_key)  # sorted() is stable: equal keys stay in order of position


def fuse(hits_a, scores_a, keep_a, hits_b, scores_b, mode, ascending, k_out):
    """-> (hits int64 [nq][k_out], scores float64, source int32, filled int32 [nq])"""
    hits_a = np.asarray(hits_a, np.int64)
    hits_b = np.asarray(hits_b, np.int64)
    scores = np.concatenate([np.asarray(scores_a, np.float64), np.asarray(scores_b, np.float64)], axis=1)
    bits = np.ascontiguousarray(scores).view(np.uint64)
    nq = hits_a.shape[0]
    hits = np.full((nq, k_out), -1, np.int64)
    out_bits = np.full((nq, k_out), np.float64(DBL_MAX if ascending else -DBL_MAX).view(np.uint64), np.uint64)
    source = np.full((nq, k_out), -1, np.int32)
    filled = np.zeros(nq, np.int32)
    for q in range(nq):
        ea, eb = row_entries(hits_a[q], None if keep_a is None else keep_a[q], hits_b[q])
        if mode == PREFIX_FILL:
            in_a = set(h for _, h in ea)
            walk = ea + [e for e in eb if e[1] not in in_a]
        else:
            assert mode == SORTED_UNION
            seen, walk = set(), []
            for e in union_order(ea + eb, scores[q], ascending):
                if e[1] not in seen:
                    seen.add(e[1])
                    walk.append(e)
        walk = walk[:k_out]
        for at, (pos, h) in enumerate(walk):
            hits[q, at] = h
            out_bits[q, at] = bits[q, pos]
            source[q, at] = pos
        filled[q] = len(walk)
    return hits, out_bits.view(np.float64), source, filled


def with_padding(hits, scores, filled, pad_hit, pad_score):
    """the library's padding behind `filled` replaced, as evaluation.merge_hits does on the host"""
    hits, scores = hits.copy(), scores.copy()
    for q in range(len(filled)):
        hits[q, filled[q]:] = pad_hit
        scores[q, filled[q]:] = pad_score
    return hits, scores
