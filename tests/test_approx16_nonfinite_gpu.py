"""GPU: the twelve bf16 builds of flat_scan_kernel (query tile 32 / 64 / 128 x inner product / squared L2 x one query tile /
several) on non-finite and overflowing rows and queries, through IndexFlat.set_approx16, against
approx16_reference.expected_nonfinite -- ids and score bits, exactly.  DESIGN.md section 2: a "smaller is better" value of +inf
or a NaN never becomes a hit, an inner-product +inf is the best hit, a starved query is padded with (-1, -+FLT_MAX).

The data is nonfinite_cases.poison_ints (small integers, on which the bf16 scan has one right answer, with the poisoned kinds of
that file at nonfinite_cases.special_rows of both database tiles); tests/test_approx16_nonfinite_reference.py pins the
reference by hand, among it the one kind whose outcome the rounding changes (`fltmax`: bf16(FLT_MAX) is +inf).  Every case
asserts the build it reached and, on the REFERENCE's answer, that it is not vacuous."""
import math

import numpy as np
import pytest

import approx16_reference as ar
import nonfinite_cases as nc
from approx16_reference import IP, L2, FLT_MAX

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(got, want, what):
    (D, I), (wD, wI) = got, want
    assert D.dtype == np.float32 and I.dtype == np.int64 and D.shape == wD.shape and I.shape == wI.shape, what
    if not np.array_equal(I, wI):
        q, j = np.argwhere(I != wI)[0]
        raise AssertionError(f"{what}: {int((I != wI).sum())} ids differ, first at query {q} rank {j}: got {I[q, j]} ({D[q, j]!r}), "
                             f"expected {wI[q, j]} ({wD[q, j]!r})")
    if not np.array_equal(_bits(D), _bits(wD)):
        q, j = np.argwhere(_bits(D) != _bits(wD))[0]
        raise AssertionError(f"{what}: {int((_bits(D) != _bits(wD)).sum())} score bits differ, first at query {q} rank {j}: got {D[q, j]!r}, "
                             f"expected {wD[q, j]!r}")


def _build(idx, nq):
    """the build the last launch ran (tests/test_approx16_exact_gpu.py::_build)"""
    s = idx.last_scan()
    qt = s["query_tile"]
    assert s["kernel"].startswith(f"flat_scan_q{qt}_d{s['db_tile']}"), s
    assert s["grid"] == s["nchunks"] * math.ceil(nq / qt), (s, nq)
    return f"bf16 q{qt} {'l2' if idx.metric_type else 'ip'} {'one' if nq <= qt else 'several'}"


def _not_vacuous(xb, xq, table, Do, Io, metric):
    """on the reference's answer: a starved list, a +inf inner-product hit, the near-duplicates' copies absent where they would lead"""
    k = Io.shape[1]
    assert ((Io >= 0).sum(1) < k).any(), "no query has fewer than k hits"
    assert (Do[Io < 0] == (-FLT_MAX if metric == IP else FLT_MAX)).all()
    if metric == IP:
        assert np.isposinf(Do).any(), "no +inf inner-product hit"
    for q, r in table.near.items():
        assert r not in Io[q]
        clean = xb.copy()
        clean[r] = xq[q]
        assert ar.expected_nonfinite(clean, xq[q:q + 1], 1, metric)[1][0, 0] == r, "unpoisoned, the copy leads"


CASES = [(qt, metric, nq) for qt in (32, 64, 128) for metric in (IP, L2) for nq in (qt - 3, qt + 9)]


def test_the_cases_cover_the_twelve_builds():
    assert len({(qt, metric, nq <= qt) for qt, metric, nq in CASES}) == 12


@pytest.mark.parametrize("qt,metric,nq", CASES)
def test_every_build_on_poisoned_rows_and_queries(gpu_faiss, qt, metric, nq):
    """k = 10 on 1000 rows, and starved lists: k = nb - 3 on 2051 rows (more than three rows are never hits, for every query)"""
    for nb, k in ((1000, 10), (2051, 2048)):
        where = sorted(set(nc.special_rows(nb, 128)) | set(nc.special_rows(nb, 256)))
        xb, xq, table = nc.poison_ints(np.random.default_rng(qt * 100 + metric * 10 + nq + nb), nb, nq, 64, where)
        assert set(v.split(":")[-1] for v in table.rows.values()) == set(nc.ROW_KINDS)
        want = ar.expected_nonfinite(xb, xq, k, metric, table)
        _not_vacuous(xb, xq, table, want[0], want[1], metric)
        if k == 2048:
            assert ((want[1] >= 0).sum(1) < k).all(), "every query is starved"
        idx = gpu_faiss.IndexFlat(64, metric)
        idx.set_approx16()
        idx.add(xb)
        idx.set_tuning(qt, 0, 0)
        got = idx.search(xq, k)
        build = _build(idx, nq)
        print(f"qt {qt} nq {nq} nb {nb} k {k}: {build}")
        assert build == f"bf16 q{qt} {'l2' if metric else 'ip'} {'one' if nq <= qt else 'several'}" and idx.last_scan()["query_tile"] == qt
        _same(got, want, f"qt {qt} metric {metric} nq {nq} nb {nb} k {k}")
