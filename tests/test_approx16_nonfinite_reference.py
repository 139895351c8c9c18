"""CPU: the bf16 scan's reference on non-finite and overflowing inputs (tests/approx16_reference.py: classify16, TABLE16,
expected_nonfinite), pinned to hand-derived values.  tests/test_approx16_nonfinite_gpu.py compares the library with it bit for
bit, so this file is the ground truth under it."""
import numpy as np
import pytest

import approx16_reference as ar
import nonfinite_cases as nc
from approx16_reference import IP, L2, FLT_MAX
from nonfinite_cases import C_INF, ROW_KINDS

NB, D = 40, 16
CODE = {"never": 0, "hit": 1, "best": 2, "zero": 3}
INF = np.float32(np.inf)


def _problem(nq=25, seed=0):
    rng = np.random.default_rng(seed + nq)
    pos = [0, 3, 15, 16, 17, 31, NB - 1]
    where = pos + [(20 + i, k) for i, k in enumerate(ROW_KINDS)]   # every kind at least twice
    return nc.poison_ints(rng, NB, nq, D, where)


def _cell(table, kind, form, q, xq):
    c = table[kind][form]
    if isinstance(c, dict):
        c = c[1 if xq[q, C_INF if kind == "pinf" else 0] > 0 else -1]
    return c if isinstance(c, tuple) else (c,)


def test_classify16_agrees_with_the_table_as_written():
    xb, xq, table = _problem()
    seen = set()
    for form in ar.FORMS16:
        out = ar.classify16(xq, xb, form)
        for r, kind in table.rows.items():
            kind = kind.split(":")[-1]
            for q in table.ordinary_queries():
                assert out[q, r] in [CODE[a] for a in _cell(ar.TABLE16, kind, form, q, xq)], (form, kind, q, r, out[q, r])
                seen.add((kind, form))
            for qkind in table.queries.values():
                if (qkind, kind) in ar.PAIRS16:
                    for q in table.queries_of(qkind):
                        assert out[q, r] == CODE[ar.PAIRS16[(qkind, kind)][form]], (form, qkind, kind)
        for q in table.queries_of("nan"):
            assert (out[q] == 0).all()
        if form != "ip":
            for q in table.queries_of("pinf"):
                assert (out[q] == 0).all()
    assert seen == {(k, f) for k in ROW_KINDS for f in ar.FORMS16}


def test_every_kind_that_rounding_changes_has_its_own_row():
    """the kinds whose outcome differs between the fp32 rules and the rules on the rounded operands, found on the data and
    not by reading the table: exactly ROUNDING_CHANGES, each with a TABLE16 row that differs from the fp32 table's"""
    xb, xq, table = _problem()
    changed = set()
    for form in ar.FORMS16:
        a, b = nc.classify(xq, xb, form), ar.classify16(xq, xb, form)
        for r, kind in table.rows.items():
            if (a[:, r] != b[:, r]).any():
                changed.add(kind.split(":")[-1])
    missing = changed - set(ar.ROUNDING_CHANGES)
    assert not missing, f"rounding changes the outcome of {sorted(missing)}, which the table does not list"
    assert changed == set(ar.ROUNDING_CHANGES) == {"fltmax"}
    for kind in ROW_KINDS:
        same = all(ar.TABLE16[kind][f] == nc.ISSUE_TABLE[kind][f] for f in ar.FORMS16)
        assert same == (kind not in ar.ROUNDING_CHANGES), kind
    assert all(set(ar.TABLE16[k]) == set(ar.FORMS16) for k in ROW_KINDS) and set(ar.TABLE16) == set(ROW_KINDS)


# a hand problem, d = 8.  bf16(1.8e19) = T = 0x5F7A0000 = 250 * 2^56; bf16(3e19) = H = 0x5FD00000 = 208 * 2^57; bf16(FLT_MAX) = +inf
T, H = np.float32(250 * 2.0 ** 56), np.float32(208 * 2.0 ** 57)
HAND_XB = np.array([[3, 1, 0, 2, 1, 1, 0, 0],            # 0  ordinary
                    [1.8e19, 0, 0, 0, 0, 0, 0, 0],        # 1  twin
                    [FLT_MAX, 0, 0, 0, 0, 0, 0, 0],       # 2  fltmax
                    [3e19] * 8,                            # 3  huge
                    [1, np.inf, 1, 1, 1, 1, 1, 1],         # 4  pinf
                    [1, 1, np.nan, 1, 1, 1, 1, 1],         # 5  nan
                    [-3, -1, 0, 2, 1, 1, 0, 0],            # 6  ordinary
                    [0, 0, 0, 0, 0, 0, 0, 0]], np.float32)  # 7  zero
HAND_XQ = np.array([[1, 2, 0, 1, 1, 1, 0, 0],             # q0: positive at 0 and at C_INF
                    [-1, -2, 0, 1, 1, 1, 0, 0],            # q1: negative at both
                    [1.8e19, 0, 0, 0, 0, 0, 0, 0]], np.float32)  # q2: the twin query


def test_expected_by_hand():
    assert ar.bf16_rne(np.array([1.8e19, 3e19], np.float32)).tolist() == [T, H]
    # inner product.  q0: fltmax (1 * inf) and pinf (2 * inf) are +inf, ids ascending; then huge H * 6, twin T * 1, row 0: 3 + 2 + 2 + 1 + 1 = 9,
    # row 6: -3 - 2 + 2 + 1 + 1 = -1, zero row: 0 (returned as -0.0) sorts before -1; nan never
    D, I = ar.expected_nonfinite(HAND_XB, HAND_XQ, 8, IP)
    assert I[0].tolist() == [2, 4, 3, 1, 0, 7, 6, -1]
    assert D[0].tolist() == [INF, INF, np.float32(H * 6), T, 9, -0.0, -1, -FLT_MAX] and np.signbit(D[0, 5])
    # q1: fltmax, pinf -inf: never; nan never; row 6: 3 + 2 + 2 + 1 + 1 = 9; zero 0; row 0: -3 - 2 + 2 + 1 + 1 = -1; twin -T; huge H * 0 = 0 (id 3 before id 7)
    assert I[1].tolist() == [6, 3, 7, 0, 1, -1, -1, -1]
    assert D[1].tolist()[:5] == [9, -0.0, -0.0, -1, -T] and (D[1, 5:] == -FLT_MAX).all()
    # q2, the twin: fltmax +inf; huge H * T overflows: +inf; twin T * T = 62500 * 2^112, finite; row 0: T * 3; zero 0; row 6: -3 T;
    # pinf: the query's 0 at C_INF times inf is a NaN: never
    assert I[2].tolist() == [2, 3, 1, 0, 7, 6, -1, -1]
    assert D[2].tolist()[:6] == [INF, INF, np.float32(62500 * 2.0 ** 112), np.float32(3 * float(T)), -0.0, np.float32(-3 * float(T))]
    # squared L2 (norms of the fp32 values): fltmax, huge, pinf, nan: norm +inf or NaN: never.  q0 (norm 8): row 0 (16): 24 - 18 = 6;
    # zero row: 8; row 6 (16): 24 + 2 = 26; twin: N = fl(1.8e19^2), N + 8 = N, N - 2 T = N (2 T is far below half an ulp of N)
    N = np.float32(1.8e19) * np.float32(1.8e19)
    D, I = ar.expected_nonfinite(HAND_XB, HAND_XQ, 8, L2)
    assert I[0].tolist() == [0, 7, 6, 1, -1, -1, -1, -1] and D[0].tolist() == [6, 8, 26, N] + [FLT_MAX] * 4
    assert I[1].tolist() == [6, 7, 0, 1, -1, -1, -1, -1] and D[1].tolist() == [6, 8, 26, N] + [FLT_MAX] * 4
    # the twin query: N + 16 = N and N - 2 * 3 T: 6 T = 1500 * 2^56 against ulp(N) = 2^104 -- nothing; twin against twin: N + N = +inf: never
    assert I[2].tolist() == [0, 6, 7, -1, -1, -1, -1, -1] and D[2].tolist() == [N, N, N] + [FLT_MAX] * 5
    assert ar._f32_of_int(2 ** 24 + 1) == 2 ** 24 and ar._f32_of_int(2 ** 24 + 3) == 2 ** 24 + 4 and ar._f32_of_int(-(2 ** 128)) == -INF
    assert ar._f32_of_int(int(FLT_MAX) + 2 ** 102) == FLT_MAX and ar._f32_of_int(int(FLT_MAX) + 2 ** 103) == INF


@pytest.mark.parametrize("metric", [IP, L2])
def test_finite_data_gives_the_exact_reference(metric):
    rng = np.random.default_rng(7)
    xb, xq, table = nc.poison_ints(rng, 300, 20, 24, [], query_kinds=(), near=0)
    want = ar.expected(xb, xq, 10, metric)
    got = ar.expected_nonfinite(xb, xq, 10, metric, table)
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32))
    got = ar.expected_nonfinite(xb, xq, 10, metric)
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32))


@pytest.mark.parametrize("metric", [IP, L2])
def test_ranking_follows_the_rule(metric):
    xb, xq, table = _problem()
    form = "ip" if metric == IP else "l2n"
    out = ar.classify16(xq, xb, form)
    D, I = ar.expected_nonfinite(xb, xq, NB, metric, table)
    full = ar.expected_nonfinite(xb, xq, NB, metric)
    assert np.array_equal(I, full[1]) and np.array_equal(D.view(np.uint32), full[0].view(np.uint32)), "classifying only the poisoned pairs"
    pad = -FLT_MAX if metric == IP else FLT_MAX
    for q in range(xq.shape[0]):
        want = np.flatnonzero(out[q] > 0)
        n = want.size
        assert sorted(I[q, :n]) == list(want) and (I[q, n:] == -1).all() and (D[q, n:] == pad).all()
        best = np.flatnonzero(out[q] == 2)
        assert list(I[q, :best.size]) == list(best) and (D[q, :best.size] == np.inf).all()
        assert np.isfinite(D[q, best.size:n]).all()
        fin = D[q, best.size:n]
        assert (np.diff(fin) <= 0).all() if metric == IP else (np.diff(fin) >= 0).all()
    assert ((I >= 0).sum(1) < NB).all() and (metric == L2 or np.isposinf(D).any())
    for q, r in table.near.items():
        assert r not in I[q]
        clean = xb.copy()
        clean[r] = xq[q]
        assert ar.expected_nonfinite(clean, xq[q:q + 1], 1, metric)[1][0, 0] == r, "unpoisoned, the copy leads"


def test_the_reference_refuses_what_depends_on_the_order():
    xb = np.array([[1.8e19, 1, 0, 0, 0, 0, 0, 0]], np.float32)
    with pytest.raises(ar.PreconditionError):
        ar.expected_nonfinite(xb, HAND_XQ[:1], 1, IP)
    xb = np.array([[4000] * 8], np.float32)
    with pytest.raises(ar.PreconditionError):
        ar.expected_nonfinite(xb, xb * 2, 1, IP)
