"""GPU: the batched host searches of different index types share one set of copy pipes per device and one double-buffered
result download (ResultPipe in host_core.inc).  Whoever holds the pipes downloads batch b - 1 while batch b runs; the others
run their batches one after the other on their own streams.  Three index types searched at once on one device -- a holder
of one type beside non-holders of the others -- must each return what they return alone, bit for bit.

The rows are small integers (lsh_reference.int_rows) and the LSH rotation is +-1, so every score is exact in fp32
whichever formula a path takes."""
import threading

import numpy as np
import pytest

from lsh_reference import int_rows, pm1_rotation

pytestmark = pytest.mark.gpu

QB = 16384  # queries per batch of every host search


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_three_index_types_searched_at_once(gpu_faiss, oracle):
    """16384 + 5 queries, k = 4: two batches, the last one ragged -- the smallest shape that takes the piped path"""
    d, nb, nq, k = 16, 2000, QB + 5, 4
    rng = np.random.default_rng(355)
    jobs = []
    R = pm1_rotation(rng, 64, d)  # (exact projections: every code bit has one right answer)
    for make in (lambda: gpu_faiss.IndexFlatL2(d), lambda: gpu_faiss.IndexHNSWFlat(d, 32), lambda: gpu_faiss.IndexLSH(d, 64, _rotation=R)):
        xb, xq = int_rows(rng, nb, d), int_rows(rng, nq, d)
        idx = make()
        idx.add(xb)
        jobs.append((idx, xb, xq))
    seq = [idx.search(xq, k) for idx, _, xq in jobs]
    for D, I in seq:
        assert D.shape == I.shape == (nq, k)
    # the flat index against the oracle: the first and last rows of both batches
    rows = np.array([0, QB - 1, QB, nq - 1])
    assert rows.tolist() == [0, 16383, 16384, 16388]
    _, xb, xq = jobs[0]
    Do, Io = oracle.flat_search(xb, xq[rows], k, 1)
    assert np.array_equal(seq[0][1][rows], Io) and np.array_equal(_bits(seq[0][0][rows]), _bits(Do))

    out, errs = [None] * len(jobs), []
    start = threading.Barrier(len(jobs))

    def run(j):
        try:
            start.wait()
            out[j] = jobs[j][0].search(jobs[j][2], k)
        except Exception as e:  # pragma: no cover
            errs.append(e)

    threads = [threading.Thread(target=run, args=(j,)) for j in range(len(jobs))]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errs, errs
    for j, name in enumerate(("IndexFlatL2", "IndexHNSWFlat", "IndexLSH")):
        (D, I), (Ds, Is) = out[j], seq[j]
        assert np.array_equal(I, Is), f"{name}: {int((I != Is).sum())} ids differ from the sequential search"
        assert np.array_equal(_bits(D), _bits(Ds)), f"{name}: {int((_bits(D) != _bits(Ds)).sum())} distances differ from the sequential search"
