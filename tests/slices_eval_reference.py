"""A plain restatement of knn_eval_slice_annotate's and knn_eval_slices' contract (include/knn355.h), for the tests.

Written from the contract with Python sets and lists, one slice and one hit at a time; nothing here is shared with the
library.  The arguments are the integer tables of the C entry points."""
import numpy as np


def slice_sets(slice_protein, slice_start, slice_stop, domain_offsets, domain_family, domain_start, domain_stop):
    """-> (matching, intersecting): per slice the set of family codes with a domain inside / merely intersecting"""
    matching, intersecting = [], []
    for p, s0, s1 in zip(slice_protein, slice_start, slice_stop):
        inside, touching = set(), set()
        if p >= 0:
            for d in range(int(domain_offsets[p]), int(domain_offsets[p + 1])):
                f, d0, d1 = int(domain_family[d]), int(domain_start[d]), int(domain_stop[d])
                if s0 <= d0 and d1 <= s1:
                    inside.add(f)
                elif s0 < d1 and d0 < s1:
                    touching.add(f)
        matching.append(inside)
        intersecting.append(touching)
    return matching, intersecting


def annotate(slice_protein, slice_start, slice_stop, domain_offsets, domain_family, domain_start, domain_stop, nfam):
    """-> (match_count int32 [ns], annotation int32 [ns], family_sizes int64 [nfam])"""
    matching, _ = slice_sets(slice_protein, slice_start, slice_stop, domain_offsets, domain_family, domain_start, domain_stop)
    match_count = np.asarray([len(m) for m in matching], np.int32).reshape(len(matching))
    annotation = np.asarray([next(iter(m)) if len(m) == 1 else -1 for m in matching], np.int32).reshape(len(matching))
    family_sizes = np.zeros(nfam, np.int64)
    for m in matching:
        for f in m:
            family_sizes[f] += 1
    return match_count, annotation, family_sizes


def evaluate(hits, query_family, slice_protein, slice_start, slice_stop, domain_offsets, domain_family, domain_start, domain_stop,
             ignore_unannotated):
    """-> (is_correct uint8 [nq][k], is_ignore uint8 [nq][k], lead int32 [nq], tp int32 [nq], column_correct int64 [k])"""
    hits = np.asarray(hits, np.int64)
    nq, k = hits.shape
    ns = len(slice_protein)
    matching, intersecting = slice_sets(slice_protein, slice_start, slice_stop, domain_offsets, domain_family, domain_start, domain_stop)
    is_correct = np.zeros((nq, k), np.uint8)
    is_ignore = np.zeros((nq, k), np.uint8)
    lead = np.zeros(nq, np.int32)
    tp = np.zeros(nq, np.int32)
    for q in range(nq):
        a = int(query_family[q])
        if a < 0:
            continue
        for j in range(k):
            h = int(hits[q, j])
            if 0 <= h < ns:
                is_correct[q, j] = a in matching[h]
                is_ignore[q, j] = a in intersecting[h] or (bool(ignore_unannotated) and len(matching[h]) == 0)
        run = 0
        for j in range(k):
            if is_correct[q, j]:
                run += 1
            elif is_ignore[q, j]:
                continue
            else:
                break
        lead[q] = run
        tp[q] = int(is_correct[q].sum())
    return is_correct, is_ignore, lead, tp, is_correct.sum(axis=0, dtype=np.int64)
