"""CPU: the LSH references on non-finite and overflowing inputs, pinned to hand-derived values.  They are what
tests/test_lsh_nonfinite_gpu.py compares the library with bit for bit, so this file is the ground truth under it:
the code bit as FAISS computes it (float32 projection - threshold >= 0), the median over columns that hold infinities,
and the generator of poisoned rows with its order-independent rules (tests/lsh_nonfinite_cases.py)."""
import numpy as np
import pytest

import lsh_nonfinite_cases as lc
from lsh_reference import (faiss_bits, int_rows, pack_bits, pm1_rotation, projections32, ref_codes, ref_search,
                           zero_projection_rows)
from lsh_thresholds_reference import ref_codes_thr, ref_projections, ref_thresholds, ref_train, thresholds_of, unpack_bits

INF, NAN = np.float32(np.inf), np.float32(np.nan)
FLT_MAX = np.float32(np.finfo(np.float32).max)
B = lc.BIG

# d = 6; the base row's projections: 2, 0, 6, -8
R6 = np.array([[+1, +1, +1, +1, +1, +1],
               [+1, -1, +1, +1, -1, -1],
               [-1, +1, -1, -1, -1, +1],
               [-1, -1, +1, -1, +1, +1]], np.float32)
BASE = np.array([1, 3, -1, 1, -3, 1], np.float32)
# kind: (projections onto the four bits, bits without thresholds) -- derived by hand from R6 and BASE:
#   pinf: +inf at column 1, R6[:, 1] = + - + -;  both: +inf at column 3 (R6[:, 3] = + + - -), -inf at column 4 (R6[:, 4] = + - - +):
#   bit 0 inf - inf, bit 1 inf + inf, bit 2 -inf + inf, bit 3 -inf - inf;  p127 / m127: +-2^127 at column 0, R6[:, 0] = + + - -
HAND = {
    "base": ([2, 0, 6, -8], [1, 1, 1, 0]),
    "nan": ([NAN, NAN, NAN, NAN], [0, 0, 0, 0]),
    "pinf": ([INF, -INF, INF, -INF], [1, 0, 1, 0]),
    "ninf": ([-INF, INF, -INF, INF], [0, 1, 0, 1]),
    "both": ([NAN, INF, NAN, -INF], [0, 1, 0, 0]),
    "p127": ([B, B, -B, -B], [1, 1, 0, 0]),
    "m127": ([-B, -B, B, B], [0, 0, 1, 1]),
    "zero": ([0, 0, 0, 0], [1, 1, 1, 1]),
}


def _hand_rows():
    kinds = list(HAND)
    x = np.stack([BASE if k == "base" else lc.make_row(k, BASE) for k in kinds])
    return kinds, x


def _same_floats(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(a)].view(np.uint32), b[~np.isnan(b)].view(np.uint32))


def test_every_kind_by_hand():
    kinds, x = _hand_rows()
    assert set(lc.KINDS) <= set(kinds)
    want_p = np.array([HAND[k][0] for k in kinds], np.float32)
    want_b = np.array([HAND[k][1] for k in kinds], bool)
    assert _same_floats(lc.classify(x, R6), want_p), "the rules"
    assert _same_floats(projections32(x, R6), want_p), "the float64 products, rounded once"
    assert np.array_equal(faiss_bits(want_p), want_b)
    assert np.array_equal(unpack_bits(ref_codes(x, R6), 4), want_b)
    assert np.array_equal(unpack_bits(lc.expected_codes(x, R6), 4), want_b)
    assert np.array_equal(ref_codes(x, R6), np.array([[0b0111], [0], [0b0101], [0b1010], [0b0010], [0b0011], [0b1100], [0b1111]], np.uint8))


# thresholds +inf, -inf, finite, against projections +inf, -inf, finite, NaN: FAISS's float32 (p - t >= 0)
#              p = +inf                 -inf                  3 (finite)          NaN
BIT_TABLE = {INF: (0, 0, 0, 0),       # inf - inf = NaN      -inf                -inf                NaN
             -INF: (1, 0, 1, 0),      # +inf                 -inf + inf = NaN    +inf                NaN
             np.float32(3): (1, 0, 1, 0),
             np.float32(3.5): (1, 0, 0, 0)}


def test_the_bit_against_infinite_thresholds_by_hand():
    p = np.array([INF, -INF, 3, NAN], np.float32)
    for t, want in BIT_TABLE.items():
        assert list(faiss_bits(p, t).astype(int)) == list(want), t
    # `p >= t` is the same predicate except where p and t are the same infinity
    with np.errstate(invalid="ignore"):
        for t in BIT_TABLE:
            differs = (p >= t) != faiss_bits(p, t)
            assert list(differs) == [t == INF, t == -INF, False, False], t
    # through the codes: the hand rows against t = (+inf, -inf, +inf, -inf); projections of HAND
    kinds, x = _hand_rows()
    t = np.array([INF, -INF, INF, -INF], np.float32)
    want = {"base": [0, 1, 0, 1], "nan": [0, 0, 0, 0], "pinf": [0, 0, 0, 0], "ninf": [0, 1, 0, 1], "both": [0, 1, 0, 0],
            "p127": [0, 1, 0, 1], "m127": [0, 1, 0, 1], "zero": [0, 1, 0, 1]}
    got = unpack_bits(ref_codes_thr(x, R6, t), 4)
    for i, k in enumerate(kinds):
        assert list(got[i].astype(int)) == want[k], k
    assert np.array_equal(ref_codes_thr(x, R6, t), lc.expected_codes(x, R6, t))


def _ge_codes(x, R, t):
    """ref_codes_thr as it was: (x . R[j] >= t[j]) in float64"""
    bits = (np.asarray(x, np.float64) @ np.asarray(R, np.float64).T) >= np.broadcast_to(np.asarray(t, np.float64), (R.shape[0],))
    return np.packbits(bits, axis=1, bitorder="little")


@pytest.mark.parametrize("nbits,d,n", [(7, 33, 2), (64, 100, 3), (65, 1024, 127), (200, 33, 129), (777, 100, 1000), (65, 1, 1001)])
def test_finite_inputs_keep_their_codes(nbits, d, n):
    """the data of test_lsh_thresholds_gpu.py (_rows: integer rows, an all-zero row, rows with an exact zero projection; the
    trained thresholds, rows that sit on them) and of test_lsh_exact_gpu.py: the restated bit gives the codes `>=` gave"""
    rng = np.random.default_rng(nbits * 7919 + d * 31 + n)
    R = pm1_rotation(rng, nbits, d)
    x = int_rows(rng, n, d)
    if n >= 3:
        x[n // 2] = 0
    if d % 2 == 0 and n >= 4:
        x[: n // 4] = zero_projection_rows(rng, R, n // 4)[0]
    t = ref_thresholds(x, R)
    assert n == 2 or (ref_projections(x, R) == t).any(), "no row sits on a threshold"
    for thr in (t, 0.0, np.float32(-2.5)):
        assert np.array_equal(ref_codes_thr(x, R, thr), _ge_codes(x, R, thr))
    assert np.array_equal(ref_codes(x, R), _ge_codes(x, R, 0.0))
    xf = rng.standard_normal((n, d)).astype(np.float32)
    assert np.array_equal(ref_codes(xf, R), _ge_codes(xf, R, 0.0))


def test_median_over_columns_with_infinities_by_hand():
    F = FLT_MAX
    odd = np.array([[1, INF, -INF, -0.0, F],
                    [2, INF, -INF, -0.0, F],
                    [3, INF, -INF, -0.0, F],
                    [INF, INF, -INF, -0.0, F],
                    [INF, 1, 5, 1, 1],
                    [-INF, 2, 6, 2, 2],
                    [0, 3, 7, -1, 3]], np.float32)
    # sorted columns: (-inf 0 1 [2] 3 inf inf), (1 2 3 [inf] ...), (-inf x4: [-inf] ...), (-1 0 0 [0] 0 1 2), (1 2 3 [F] F F F)
    t = thresholds_of(odd)
    assert _same_floats(t, [2, INF, -INF, 0.0, F]) and t.view(np.uint32)[3] == 0, "-0.0 counts as +0.0"
    even = np.array([[1, 1, F, -INF, -INF, 2.0 ** 127],
                     [2, 2, F, -INF, -INF, 2.0 ** 127],
                     [3, 3, F, -INF, -INF, 2.0 ** 127],
                     [4, INF, F, -INF, -INF, 2.0 ** 127],
                     [INF, INF, F, INF, 1, 2.0 ** 127],
                     [INF, INF, 1, INF, 2, 0],
                     [INF, INF, 2, INF, 3, 1],
                     [-INF, 0, 3, INF, 4, 2]], np.float32)
    # middles: (3, 4) -> 3.5; (3, inf) -> inf; (F, F) -> F + F = inf in float32; (-inf, inf) -> NaN; (-inf, 1) -> -inf;
    # (2^127, 2^127) -> 2^128 = inf in float32
    t = thresholds_of(even)
    assert _same_floats(t, [3.5, INF, INF, NAN, -INF, INF])


@pytest.mark.parametrize("n", [7, 8, 1029, 1030])
def test_training_outcomes(n):
    x, R = lc.train_case(n, "few")
    what, t = ref_train(x, R)
    assert what == "ok" and np.isfinite(t).all(), "fewer than half of the rows infinite: a finite median"
    x, R = lc.train_case(n, "middle")
    what, t = ref_train(x, R)
    # odd n: s[n/2] is infinite; even n: (finite + inf) / 2 on the +1 bits, (-inf + finite) / 2 on the -1 bits
    assert what == "ok" and t[0] == INF and t[1] == -INF and np.isinf(t).all()
    assert np.array_equal(t, np.where(R[:, lc.C_INF] > 0, INF, -INF))
    x, R = lc.train_case(n, "most_big")
    what, t = ref_train(x, R)
    if n % 2:
        assert what == "ok" and t[0] == B and t[1] == -B
    else:
        assert what == "ok" and t[0] == INF and t[1] == -INF, "(2^127 + 2^127) / 2 overflows in float32"
    assert ref_train(*lc.train_case(n, "nan")) == ("projection", 0)
    if n % 2 == 0:
        assert ref_train(*lc.train_case(n, "around")) == ("median", 0)
    # the projections the medians were taken of are the rules', for every case
    for case in ("few", "middle", "most_big", "nan") + (("around",) if n % 2 == 0 else ()):
        x, R = lc.train_case(n, case)
        assert _same_floats(ref_projections(x, R), lc.classify(x, R) + np.float32(0)), case


@pytest.mark.parametrize("nbits,d,n", [(128, 33, 257), (200, 100, 383), (256, 37, 129)])
def test_generator_and_rules_agree_with_the_float64_restatement(nbits, d, n):
    rng = np.random.default_rng(nbits + d + n)
    R = pm1_rotation(rng, nbits, d)
    x, kinds = lc.poison_rows(rng, n, d)
    assert set(kinds.values()) == set(lc.KINDS) and {0, 127, 128, n - 1} <= set(kinds)
    p = lc.classify(x, R)
    assert _same_floats(p, projections32(x, R))
    for t in (0.0, np.where(np.arange(nbits) % 3 == 0, INF, np.where(np.arange(nbits) % 3 == 1, -INF, 2)).astype(np.float32)):
        assert np.array_equal(lc.expected_codes(x, R, t), ref_codes_thr(x, R, t))
    bits = unpack_bits(ref_codes(x, R), nbits)
    for r, kind in kinds.items():
        if kind == "nan":
            assert not bits[r].any()
        elif kind == "pinf":
            assert np.array_equal(bits[r], R[:, lc.C_INF] > 0), "the bit is the sign of the rotation's entry"
        elif kind == "both":
            assert np.array_equal(bits[r], (R[:, lc.C_B1] > 0) & (R[:, lc.C_B2] < 0))
        elif kind in ("p127", "m127"):
            assert np.array_equal(bits[r], (R[:, lc.C_BIG] > 0) == (kind == "p127")), "decided by the single huge term"
        else:
            assert bits[r].all()
    # a NaN row is at distance popcount(query code) from everything: the search over the codes is an ordinary one
    D, I = ref_search(ref_codes(x, R), ref_codes(x[:40], R), 5)
    assert (I >= 0).all() and (D[:, 0] == 0).all()


def test_the_rules_refuse_what_depends_on_the_order():
    x = np.zeros((1, 6), np.float32)
    x[0, :2] = B
    with pytest.raises(AssertionError, match="more than one huge term"):
        lc.classify(x, R6)
    x[0, :2] = 0.5
    with pytest.raises(AssertionError, match="no small integers"):
        lc.classify(x, R6)
