"""CPU: tests/approx16_reference.py (the host reference of the approximate bf16 flat scan) against values typed in by hand,
and against the fp32 oracle on inputs that are already representable in bf16, where the two arithmetics coincide."""
import numpy as np
import pytest

import approx16_reference as ar
from approx16_reference import IP, L2, FLT_MAX


def _f32(*v):
    return np.array(v, np.float32)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_rne_rounds_nine_bit_integers_to_the_even_neighbour():
    # 257 = 1.00000001b x 2^8: a tie between 256 and 258, 256 has the even significand; 259: a tie between 258 and 260
    got = ar.bf16_rne(_f32(257, 259, 383, -257, -259, -383))
    assert got.tolist() == [256.0, 260.0, 384.0, -256.0, -260.0, -384.0]
    # not ties: 513 and 515 lie below / above the middle of their neighbours 512 and 516
    assert ar.bf16_rne(_f32(513, 515, 511, -511)).tolist() == [512.0, 516.0, 512.0, -512.0]


def test_truncation_is_another_function():
    assert ar.bf16_trunc(_f32(257, 259, 383, -257, -259, -383)).tolist() == [256.0, 258.0, 382.0, -256.0, -258.0, -382.0]


def test_rne_with_a_scale():
    # 255.5 = 511 halves: nine significant bits, a tie between 255 and 256 -> 256 (even), i.e. 512 halves
    r = ar.bf16_rne(_f32(255.5, -255.5, 127.75))
    assert r.tolist() == [256.0, -256.0, 128.0]
    assert ar.units(r, 0.5).tolist() == [512.0, -512.0, 256.0]
    assert ar.units(_f32(255.5), 0.5).tolist() == [511.0]
    with pytest.raises(ar.PreconditionError):
        ar.units(_f32(255.5), 1.0)
    with pytest.raises(ar.PreconditionError):
        ar.units(_f32(3.0), 3.0)


def test_representable_values_and_zeros_pass_unchanged():
    x = _f32(1.5, 96.0, -0.3125, 255.0, 2.0 ** -20, 0.0, -0.0)
    assert np.array_equal(_bits(ar.bf16_rne(x)), _bits(x))
    assert np.array_equal(_bits(ar.bf16_trunc(x)), _bits(x))
    assert _bits(ar.bf16_rne(_f32(-0.0)))[0] == 0x80000000 and _bits(ar.bf16_rne(_f32(0.0)))[0] == 0


def test_scores_by_hand():
    xb = _f32(257, 3, 0, 1, 2, 2).reshape(3, 2)
    xq = _f32(259, -1).reshape(1, 2)
    # rounded: rows (256, 3), (0, 1), (2, 2); query (260, -1)
    assert ar.scores(xb, xq, IP).tolist() == [[256 * 260 - 3, -1.0, 518.0]]
    # squared L2: the norms of the UNROUNDED values: 259^2 + 1 = 67082; 257^2 + 9 = 66058, 1, 8
    assert ar.scores(xb, xq, L2).tolist() == [[67082 + 66058 - 2 * (256 * 260 - 3), 67082 + 1 + 2, 67082 + 8 - 2 * 518]]
    # ... of the rounded values: 260^2 + 1 = 67601; 256^2 + 9 = 65545
    assert ar.scores(xb, xq, L2, norms="rounded").tolist()[0][0] == 67601 + 65545 - 2 * (256 * 260 - 3)
    assert ar.scores(xb, xq, IP, rounding=ar.bf16_trunc).tolist()[0][0] == 256 * 258 - 3


def test_l2_is_clamped_at_zero():
    # a pair whose rounded product overshoots the unrounded norms: 383 -> 384 on both sides, 2 * 383^2 - 2 * 384^2 = -1534 -> 0
    s = ar.scores(_f32(383).reshape(1, 1), _f32(383).reshape(1, 1), L2)
    assert _bits(s)[0, 0] == 0


def test_equal_scores_go_by_id_and_short_databases_are_padded():
    xb = _f32(1, 2, 1, 1, 2).reshape(5, 1)
    xq = _f32(1, -1).reshape(2, 1)
    D, I = ar.expected(xb, xq, 7, IP)
    assert I.tolist() == [[1, 4, 0, 2, 3, -1, -1], [0, 2, 3, 1, 4, -1, -1]]
    assert D[0].tolist() == [2.0, 2.0, 1.0, 1.0, 1.0, -FLT_MAX, -FLT_MAX]
    D, I = ar.expected(xb, xq, 7, L2)
    assert I.tolist() == [[0, 2, 3, 1, 4, -1, -1], [0, 2, 3, 1, 4, -1, -1]]
    assert D.tolist() == [[0.0, 0.0, 0.0, 1.0, 1.0, FLT_MAX, FLT_MAX], [4.0, 4.0, 4.0, 9.0, 9.0, FLT_MAX, FLT_MAX]]
    assert D.dtype == np.float32 and I.dtype == np.int64
    D3, I3 = ar.expected(xb, xq, 3, IP)
    assert I3.tolist() == [[1, 4, 0], [0, 2, 3]]


def test_the_sign_of_a_zero_score():
    # inner product: the key holds (-dot) + 0 = +0.0 and the result is its negation; squared L2: the clamp's +0.0
    D, _ = ar.expected(_f32(1, -1).reshape(1, 2), _f32(-1, -1).reshape(1, 2), 1, IP)
    assert _bits(D)[0, 0] == 0x80000000
    D, _ = ar.expected(_f32(1, -1).reshape(1, 2), _f32(1, -1).reshape(1, 2), 1, L2)
    assert _bits(D)[0, 0] == 0


def test_precondition_violations_are_caught():
    ok = np.full((1, 1280), 16, np.float32)
    assert ar.check_precondition(ok, ok) == 4 * 1280 * 256
    with pytest.raises(ar.PreconditionError):
        ar.check_precondition(np.full((1, 16400), 16, np.float32), np.full((1, 16400), 16, np.float32))  # 4 * 16400 * 256 >= 2^24
    big = np.full((1, 16), 511, np.float32)  # rounds to 512: 4 * 16 * 512^2 = 2^24 exactly
    with pytest.raises(ar.PreconditionError):
        ar.check_precondition(big, big)
    assert ar.check_precondition(big[:, :15], big[:, :15]) == 4 * 15 * 512 * 512
    with pytest.raises(ar.PreconditionError):
        ar.expected(_f32(0.3).reshape(1, 1), _f32(1).reshape(1, 1), 1, IP)  # no integer
    # one bad pair among good ones
    xb = np.ones((5, 16), np.float32)
    xb[3] = 511
    with pytest.raises(ar.PreconditionError):
        ar.scores(xb, big, IP)


@pytest.mark.parametrize("metric", [IP, L2])
@pytest.mark.parametrize("d", [7, 100])
def test_reference_is_the_oracle_on_representable_inputs(oracle, metric, d):
    """Integers of at most 8 significant bits are their own bf16 copies: the approximate scan and the fp32 chain of the oracle
    (norm formula) then compute the same exact integers, and the two rankings must agree bit for bit, ties included.  A zero
    inner product is -0.0 in both: the scans negate a key that holds v + 0."""
    rng = np.random.default_rng(1600 + d)
    xb = rng.integers(-16, 17, (300, d)).astype(np.float32)
    xq = rng.integers(-16, 17, (25, d)).astype(np.float32)
    xb[150:153] = xb[:3]
    xq[:3] = xb[:3]
    assert np.array_equal(ar.bf16_rne(xb), xb) and np.array_equal(ar.bf16_rne(xq), xq)
    for k in (1, 10, 303):
        D, I = ar.expected(xb, xq, k, metric)
        Do, Io = oracle.flat_search(xb, xq, k, metric, l2_mode=1)
        assert np.array_equal(I, Io), f"k {k}: {int((I != Io).sum())} ids differ"
        assert np.array_equal(_bits(D), _bits(Do)), f"k {k}: score bits differ"
    # the same at a scale: the oracle sees the scaled floats
    Ds, Is = ar.expected(xb * np.float32(0.25), xq * np.float32(0.25), 10, metric, scale=0.25)
    Do, Io = oracle.flat_search(xb * np.float32(0.25), xq * np.float32(0.25), 10, metric, l2_mode=1)
    assert np.array_equal(Is, Io) and np.array_equal(_bits(Ds), _bits(Do))


def test_bf16_rne_on_non_finite_and_overflowing_values():
    """NaN -> NaN (every payload, both signs), +-inf -> +-inf, finite values above the largest bf16 -> +-inf (FLT_MAX), and
    the `twin` of tests/nonfinite_cases.py (1.8e19) stays finite: 0x5F79CCD9 rounds to 0x5F7A0000 = 1.8014e19, whose square
    3.245e38 is still below FLT_MAX -- the bf16 scan's twin-against-twin inner product is a finite hit, as in fp32"""
    nan_bits = np.array([0x7FC00000, 0x7F800001, 0x7FFFFFFF, 0xFFFFFFFF, 0xFF800001, 0x7F808000, 0x7FBF8000], np.uint32)
    assert np.isnan(ar.bf16_rne(nan_bits.view(np.float32))).all()
    inf = np.float32(np.inf)
    fmax = np.float32(np.finfo(np.float32).max)
    x = np.array([inf, -inf, fmax, -fmax, 1.8e19, -1.8e19, 3e19], np.float32)
    r = ar.bf16_rne(x)
    assert list(r[:4]) == [inf, -inf, inf, -inf]
    assert np.float32(1.8e19).view(np.uint32) == 0x5F79CCD9 and r[4].view(np.uint32) == 0x5F7A0000 and r[5] == -r[4]
    assert np.isfinite(r[4:]).all() and float(r[4]) ** 2 < float(fmax) and (r.view(np.uint32) & 0xFFFF == 0).all()
    # the edge: the largest bf16 stays, the midpoint to 2^128 (a tie: the even neighbour is 2^128) and everything above go to inf
    edge = np.array([0x7F7F0000, 0x7F7F7FFF, 0x7F7F8000, 0x7F7F8001], np.uint32).view(np.float32)
    assert list(ar.bf16_rne(edge).view(np.uint32)) == [0x7F7F0000, 0x7F7F0000, 0x7F800000, 0x7F800000]
    assert list(ar.bf16_trunc(np.array([fmax, inf], np.float32)).view(np.uint32)) == [0x7F7F0000, 0x7F800000]
