"""Exact host restatement of IndexRefineFlat's second stage, for tests/test_refine_gpu.py and tests/test_refine_reference.py.

ref_refine   per query: the candidate labels without the -1 entries, sorted ascending, are scored by the CPU oracle's flat
             search over exactly those rows (``l2_mode=2``: the sum of squared differences at every batch size, what
             FAISS's compute_distance_subset computes); the oracle's local ids are mapped back through the sorted
             labels -- sorted, so the oracle's lower-id tie rule is the global one -- and short rows are padded with
             -1 and -FLT_MAX (inner product) / +FLT_MAX (L2).  A label that occurs twice is a row that occurs twice.
             allow_unfilled: candidates may be poisoned rows (tests/nonfinite_cases.py); a pair the oracle drops leaves
             its slot to the pad, which is what DESIGN.md section 2 asks of the library

The labels come from a host restatement of the base index (tests/lsh_reference.py::ref_search) or are hand-made: nothing
here touches the library under test."""
import numpy as np

FLT_MAX = np.float32(np.finfo(np.float32).max)
METRIC_INNER_PRODUCT, METRIC_L2 = 0, 1


def ref_refine(orc, xb, xq, labels, k, metric, allow_unfilled=False):
    """orc: oracle.knn_oracle.oracle(); xb [nb, d], xq [nq, d] float32; labels int64 [nq, kb] with -1 = no candidate
    -> (D float32 [nq, k], I int64 [nq, k])"""
    xb = np.ascontiguousarray(xb, np.float32)
    xq = np.ascontiguousarray(xq, np.float32)
    labels = np.asarray(labels, np.int64)
    nq = xq.shape[0]
    assert labels.shape[0] == nq and labels.ndim == 2
    D = np.full((nq, k), -FLT_MAX if metric == METRIC_INNER_PRODUCT else FLT_MAX, np.float32)
    I = np.full((nq, k), -1, np.int64)
    for i in range(nq):
        cand = np.sort(labels[i][labels[i] >= 0])
        kk = min(k, cand.size)
        if kk == 0:
            continue
        Dl, Il = orc.flat_search(np.ascontiguousarray(xb[cand]), xq[i:i + 1], kk, metric, l2_mode=2)
        assert allow_unfilled or (Il[0] >= 0).all(), "refine_reference: the oracle left a slot unfilled (a score that is not finite?)"
        D[i, :kk] = Dl[0]
        I[i, :kk] = np.where(Il[0] >= 0, cand[np.maximum(Il[0], 0)], -1)
    return D, I
