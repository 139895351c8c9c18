"""Host statement of the four evaluation passes of include/knn355.h (knn_eval_*), for tests/test_consumers_exact_gpu.py.

remove_self_hit  out row = in row without the FIRST occurrence of the row's self id; a row that does not hold it loses
                 its last element and is counted missing.  Scores move as 32-bit patterns: a NaN payload, an infinity
                 and -0.0 arrive unchanged.
label_eval       hit j of row r matches iff 0 <= hit < nb and labels_db[hit] == labels_q[r]; lead = matches before the
                 first hit that does not match, tp = matches anywhere
set_eval         hit j of row r matches iff it is one of members[offsets[r] : offsets[r + 1]]; lead and tp as above
levels_eval      out[q][l][j] = 0 <= hit < n and mapping[hit][l] == mapping[query_rows[q]][l]

These state the contract of the C ABI, not the indexing of the Python loops they replace (oracle/consumers_oracle.py
restates those): a loop that writes train_ids[hit] reads the LAST element for the "no hit" id -1; here -1, every other
negative id and every id at or past the table's end match nothing.  On inputs whose ids are all inside the table the two
agree exactly (tests/test_consumers_reference.py).

Plain loops over rows and hits, nothing shared with the kernels' lane / slab structure; small inputs only."""
import numpy as np


def remove_self_hit(hits, scores, self_ids):
    """-> (hits_out int64 [nq, k-1], scores_out float32 [nq, k-1], missing int32 [nq])"""
    hits = np.asarray(hits, np.int64)
    bits = np.ascontiguousarray(scores, np.float32).view(np.uint32)
    nq, k = hits.shape
    assert k >= 2 and bits.shape == hits.shape and len(self_ids) == nq
    ho = np.empty((nq, k - 1), np.int64)
    so = np.empty((nq, k - 1), np.uint32)
    missing = np.zeros(nq, np.int32)
    for r in range(nq):
        index = k - 1
        for j in range(k):
            if hits[r, j] == self_ids[r]:
                index = j
                break
        else:
            missing[r] = 1
        ho[r] = np.concatenate([hits[r, :index], hits[r, index + 1:]])
        so[r] = np.concatenate([bits[r, :index], bits[r, index + 1:]])
    return ho, so.view(np.float32), missing


def _lead_tp(ok):
    """ok bool [nq, k] -> (leading run of True per row, count of True per row), both int32"""
    nq, k = ok.shape
    lead = np.empty(nq, np.int32)
    for r in range(nq):
        bad = np.flatnonzero(~ok[r])
        lead[r] = bad[0] if bad.size else k
    return lead, ok.sum(axis=1).astype(np.int32)


def label_eval(hits, labels_q, labels_db):
    """-> (is_correct uint8 [nq, k], lead int32 [nq], tp int32 [nq])"""
    hits = np.asarray(hits, np.int64)
    nq, k = hits.shape
    nb = len(labels_db)
    assert len(labels_q) == nq
    ok = np.zeros((nq, k), bool)
    for r in range(nq):
        for j in range(k):
            h = int(hits[r, j])
            ok[r, j] = 0 <= h < nb and int(labels_db[h]) == int(labels_q[r])
    lead, tp = _lead_tp(ok)
    return ok.astype(np.uint8), lead, tp


def set_eval(hits, offsets, members):
    """-> (lead int32 [nq], tp int32 [nq])"""
    hits = np.asarray(hits, np.int64)
    nq, k = hits.shape
    assert len(offsets) == nq + 1
    ok = np.zeros((nq, k), bool)
    for r in range(nq):
        mine = set(int(m) for m in members[int(offsets[r]):int(offsets[r + 1])])
        for j in range(k):
            ok[r, j] = int(hits[r, j]) in mine
    return _lead_tp(ok)


def levels_eval(hits, query_rows, mapping):
    """-> uint8 [nq, nlevels, k]"""
    hits = np.asarray(hits, np.int64)
    mapping = np.asarray(mapping)
    nq, k = hits.shape
    n, nlevels = mapping.shape
    assert len(query_rows) == nq
    out = np.zeros((nq, nlevels, k), np.uint8)
    for q in range(nq):
        mine = mapping[int(query_rows[q])]
        for j in range(k):
            h = int(hits[q, j])
            if 0 <= h < n:
                for l in range(nlevels):
                    out[q, l, j] = mapping[h, l] == mine[l]
    return out
