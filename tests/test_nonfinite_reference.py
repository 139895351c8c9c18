"""CPU: the oracle on non-finite and overflowing inputs, against the hand-derived outcomes of tests/nonfinite_cases.py.
DESIGN.md section 2: a "smaller is better" value of +inf or a NaN never becomes a hit; under inner product a +inf score
is the best hit; a +-FLT_MAX score keeps its id; a starved query is padded with (-1, -+FLT_MAX).  The oracle is what the
GPU tests (test_flat_nonfinite_gpu.py) compare the library with bit for bit, so this file is the ground truth under it."""
import numpy as np
import pytest

import nonfinite_cases as nc
from nonfinite_cases import IP, L2, FLT_MAX, C_INF, C_NAN, ROW_KINDS

NB, D = 40, 16
BATCHES = [(5, ("nan", "pinf", "twin")), (5, ("huge", "fltmax+", "fltmax-")), (25, nc.QUERY_KINDS)]
CODE = {"never": 0, "hit": 1, "best": 2, "zero": 3}


def _problem(kind, nq, qk, seed=0):
    rng = np.random.default_rng(1000 * nq + seed + len(qk))
    pos = [0, 3, 15, 16, 17, 31, NB - 1]
    where = pos if kind == "mix" else [(p, kind) for p in pos[:4]] + [(NB - 1, kind)]
    if kind == "mix":
        where = where + [(20 + i, k) for i, k in enumerate(ROW_KINDS)]  # every kind at least twice
    return nc.poison(rng, NB, nq, D, where, query_kinds=qk, near=1 if nq < 8 else 2)


@pytest.mark.parametrize("nq,qk", BATCHES)
@pytest.mark.parametrize("metric", [IP, L2])
@pytest.mark.parametrize("kind", ROW_KINDS + ("mix",))
def test_oracle_flat_search_follows_the_table(oracle, kind, metric, nq, qk):
    xb, xq, table = _problem(kind, nq, qk)
    form = nc.form_of(metric, nq)
    out = table.outcome(form)
    Dg, Ig = oracle.flat_search(xb, xq, NB, metric)
    pad = -FLT_MAX if metric == IP else FLT_MAX
    for q in range(nq):
        want = np.flatnonzero(out[q] > 0)
        n = want.size
        assert (Ig[q, :n] >= 0).all() and (Ig[q, n:] == -1).all(), (q, table.queries.get(q), "count of hits")
        assert sorted(Ig[q, :n]) == list(want), (q, table.queries.get(q), "ids present")
        assert (Dg[q, n:] == pad).all(), "pad slots: -FLT_MAX (inner product) / +FLT_MAX (L2)"
        assert np.isfinite(Dg[q, :n][out[q][Ig[q, :n]] != 2]).all()
        best = np.flatnonzero(out[q] == 2)     # +inf inner-product scores lead the list, in ascending id
        assert list(Ig[q, :best.size]) == list(best) and (Dg[q, :best.size] == np.inf).all()
        zero = np.flatnonzero(out[q] == 3)     # exact zeros of the difference form lead theirs
        assert list(Ig[q, :zero.size]) == list(zero) and (Dg[q, :zero.size] == 0).all()
        # sorted best first among the finite hits
        fin = Dg[q, best.size:n]
        assert (np.diff(fin) <= 0).all() if metric == IP else (np.diff(fin) >= 0).all()
    # the poisoned queries of the issue's last row
    for q in table.queries_of("nan"):
        assert (Ig[q] == -1).all() and (Dg[q] == pad).all()
    if metric == L2:
        for q in table.queries_of("pinf"):
            assert (Ig[q] == -1).all() and (Dg[q] == pad).all()
    # a near-duplicate's poisoned copy is absent from the list it would lead
    for q, r in table.near.items():
        assert r not in Ig[q]
        clean = xb.copy()
        clean[r] = xq[q]
        assert oracle.flat_search(clean, xq[q:q + 1], 1, metric)[1][0, 0] == r, "unpoisoned, the copy leads"


@pytest.mark.parametrize("nq,qk", BATCHES)
def test_classify_agrees_with_the_table_as_written(nq, qk):
    """the order-independent rules of nonfinite_cases.classify reproduce every cell of ISSUE_TABLE / ISSUE_PAIRS"""
    xb, xq, table = _problem("mix", nq, qk)
    seen = set()
    for form in nc.FORMS:
        out = table.outcome(form)
        for r, kind in table.rows.items():
            kind = kind.split(":")[-1]
            cell = nc.ISSUE_TABLE[kind][form]
            for q in table.ordinary_queries():
                c = cell
                if isinstance(c, dict):
                    c = c[1 if xq[q, C_INF if kind == "pinf" else 0] > 0 else -1]
                allowed = c if isinstance(c, tuple) else (c,)
                assert out[q, r] in [CODE[a] for a in allowed], (form, kind, q, r, out[q, r])
                seen.add((kind, form))
            for qkind in table.queries.values():
                if (qkind, kind) in nc.ISSUE_PAIRS:
                    for q in table.queries_of(qkind):
                        assert out[q, r] == CODE[nc.ISSUE_PAIRS[(qkind, kind)][form]], (form, qkind, kind)
        for q in table.queries_of("nan"):
            assert (out[q] == 0).all()
        if form != "ip":
            for q in table.queries_of("pinf"):
                assert (out[q] == 0).all()
    assert seen == {(k, f) for k in ROW_KINDS for f in nc.FORMS}


def test_both_l2_formulas_on_the_twin(oracle):
    """twin against twin: +inf by the norm formula (3.24e38 + 3.24e38), exactly 0 by differences -- whatever the batch size"""
    xb, xq, table = _problem("twin", 25, nc.QUERY_KINDS)
    (q,) = table.queries_of("twin")
    rows = table.rows_of("twin")
    for nq, mode, present in ((25, 0, False), (25, 2, True), (25, 1, False)):
        Dg, Ig = oracle.flat_search(xb, xq[:nq], NB, L2, l2_mode=mode)
        assert np.isin(rows, Ig[q]).all() == present
        if present:
            assert list(Ig[q, :len(rows)]) == rows and (Dg[q, :len(rows)] == 0).all()
    with np.errstate(over="ignore"):
        assert (FLT_MAX > np.float32(1.8e19) * np.float32(1.8e19)) and np.isinf(np.float32(3.24e38) + np.float32(3.24e38))


def test_fltmax_scores_keep_their_ids(oracle):
    xb, xq, table = _problem("fltmax", 25, nc.QUERY_KINDS)
    rows = table.rows_of("fltmax")
    Dg, Ig = oracle.flat_search(xb, xq, NB, IP)
    (qp,), (qm,) = table.queries_of("fltmax+"), table.queries_of("fltmax-")
    assert list(Ig[qp, :len(rows)]) == rows and (Dg[qp, :len(rows)] == FLT_MAX).all()
    n = int((table.outcome("ip")[qm] > 0).sum())   # (the near-duplicates' poisoned copies are no hits)
    assert 0 < n < NB and (Ig[qm, :n] >= 0).all() and (Ig[qm, n:] == -1).all()
    assert list(Ig[qm, n - len(rows):n]) == rows and (Dg[qm, n - len(rows):] == -FLT_MAX).all(), "-FLT_MAX with a real id, then the pads"


def test_oracle_pair_distances_and_normalize(oracle):
    xb, xq, table = _problem("mix", 25, nc.QUERY_KINDS)
    nq = xq.shape[0]
    qi, ri = (a.ravel().astype(np.int64) for a in np.meshgrid(np.arange(nq), np.arange(NB), indexing="ij"))
    for metric, mode, form in ((IP, 0, "ip"), (L2, 0, "l2n"), (L2, 2, "l2d")):
        got = oracle.pair_distances(xb, xq, qi, ri, metric, l2_mode=mode).reshape(nq, NB)
        out = table.outcome(form)
        assert np.isfinite(got[(out == 1) | (out == 3)]).all() and (got[out == 3] == 0).all()
        assert (got[out == 2] == np.inf).all()
        never = got[out == 0]
        assert (np.isnan(never) | (never == (-np.inf if metric == IP else np.inf))).all()
    x = xb.copy()
    x[7] = 0
    before = x.copy()
    oracle.normalize_l2(x)
    bits = lambda a: np.ascontiguousarray(a).view(np.uint32)
    assert (x[7] == 0).all(), "the zero row is untouched"
    for r in table.rows_of("huge"):
        assert (x[r] == 0).all(), "nrm = +inf: every entry times 1 / sqrt(inf) = 0"
    for r in table.rows_of("pinf"):
        assert np.isnan(x[r, C_INF]) and (np.delete(x[r], C_INF) == 0).all(), "inf * 0 = NaN, the rest 0"
    for r in table.rows_of("nan"):
        assert np.isnan(x[r, C_NAN]) and np.array_equal(bits(x[r]), bits(before[r])), "nrm = NaN is not > 0: the row stays as it is"
    for r in table.rows_of("both"):
        assert np.isnan(x[r]).sum() == 2
    for r in table.rows_of("twin"):
        assert abs(float(x[r, 0]) - 1.0) < 1e-6 and (x[r, 1:] == 0).all()
    plain = [r for r in range(NB) if r not in table.rows and r != 7]
    assert np.allclose(np.linalg.norm(x[plain].astype(np.float64), axis=1), 1.0, atol=1e-6)
