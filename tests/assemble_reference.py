"""A plain per-group restatement of knn_eval_assemble's contract (include/knn355.h), for the tests.

Written from the contract, one group at a time, with Python lists and a stable sort; nothing here is shared with the
library.  For each group: build the positions p, sort them stably with NaN last and the two zeros equal, cut the list
at depth, walk it."""
import math

import numpy as np

FLT_MAX = float(np.finfo(np.float32).max)


def group_order(scores, ascending):
    """positions p of one group's flattened scores in the contract's order"""
    def sort_key(p):
        s = float(scores[p])
        if math.isnan(s):
            return (1, 0.0)
        return (0, (s if ascending else -s) + 0.0)  # Python compares -0.0 == 0.0: the zeros tie
    return sorted(range(len(scores)), key=sort_key)  # sorted() is stable: equal keys stay in order of p


def assemble(hits, scores, group_offsets, row_group, self_group, depth, k_out, ascending):
    """-> (groups int64 [ng][k_out], scores float32, qrow int64, hit int64)"""
    hits = np.asarray(hits, np.int64)
    scores = np.asarray(scores, np.float32)
    k = hits.shape[1]
    ng = len(group_offsets) - 1
    nb = len(row_group)
    groups = np.full((ng, k_out), -1, np.int64)
    out_scores = np.full((ng, k_out), FLT_MAX if ascending else -FLT_MAX, np.float32)
    qrow = np.full((ng, k_out), -1, np.int64)
    hit_out = np.full((ng, k_out), -1, np.int64)
    for g in range(ng):
        lo, hi = int(group_offsets[g]), int(group_offsets[g + 1])
        flat_hits = hits[lo:hi].reshape(-1)
        flat_scores = scores[lo:hi].reshape(-1)
        picked = []
        for p in group_order(flat_scores, ascending)[:depth]:
            h = int(flat_hits[p])
            if h < 0 or h >= nb:
                continue
            grp = int(row_group[h])
            if grp < 0:
                continue
            if self_group is not None and grp == int(self_group[g]):
                continue
            if grp in picked:
                continue
            if len(picked) == k_out:
                break
            at = len(picked)
            picked.append(grp)
            groups[g, at] = grp
            out_scores[g, at] = flat_scores[p]
            qrow[g, at] = lo + p // k
            hit_out[g, at] = h
    return groups, out_scores, qrow, hit_out


def bare_reference(hits, scores, group_offsets, row_group, k_out):
    """The reference's loop as it stands (numpy.argsort(-scores), cut at k, skip picked): only for inputs whose scores
    are all distinct, finite and whose hits are all inside the table.  -> groups [ng][k_out], -1 = unfilled"""
    k = hits.shape[1]
    out = np.full((len(group_offsets) - 1, k_out), -1, np.int64)
    for g in range(len(group_offsets) - 1):
        lo, hi = group_offsets[g], group_offsets[g + 1]
        h = hits[lo:hi].flatten()
        s = scores[lo:hi].flatten()
        h = h[np.argsort(-s)]
        picked = []
        for hit in h[:k]:
            if row_group[hit] in picked:
                continue
            picked.append(row_group[hit])
        out[g, :len(picked[:k_out])] = picked[:k_out]
    return out
