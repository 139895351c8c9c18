"""CPU: the host restatement of IndexLSH's trained thresholds (tests/lsh_thresholds_reference.py) on hand-computed cases.
The GPU tests compare against it bit for bit -- against this restatement of FAISS 1.7.2's IndexLSH::train, not against
FAISS: no FAISS binary exists here."""
import numpy as np

from lsh_reference import int_rows, pm1_rotation, ref_codes
from lsh_thresholds_reference import median64, ref_codes_thr, ref_projections, ref_thresholds, threshold_tol, unpack_bits

EYE2 = np.eye(2, dtype=np.float32)


def _bits(a):
    return np.asarray(a, np.float32).view(np.uint32).tolist()


def _col(*values):
    """training rows whose projections onto the identity are (values, -values)"""
    v = np.asarray(values, np.float32)
    return np.ascontiguousarray(np.stack([v, -v], axis=1))


def test_n_1_to_4():
    assert _bits(ref_thresholds(_col(5), EYE2)) == _bits([5, -5])
    assert _bits(ref_thresholds(_col(5, 2), EYE2)) == _bits([3.5, -3.5])
    assert _bits(ref_thresholds(_col(5, -7, 2), EYE2)) == _bits([2, -2])  # sorted -7 2 5 -> s[1]
    assert _bits(ref_thresholds(_col(9, 5, -7, 2), EYE2)) == _bits([3.5, -3.5])  # sorted -7 2 5 9 -> (2 + 5) / 2


def test_all_rows_equal():
    x = np.repeat(np.array([[3, -1]], np.float32), 6, axis=0)
    assert _bits(ref_thresholds(x, EYE2)) == _bits([3, -1])
    assert _bits(ref_thresholds(x[:5], EYE2)) == _bits([3, -1])
    # every row sits on its threshold: every bit is 1
    assert ref_codes_thr(x, EYE2, ref_thresholds(x, EYE2)).reshape(-1).tolist() == [3] * 6


def test_middle_values_one_apart_give_a_half_integer():
    t = ref_thresholds(_col(1, 4, 3, 0), EYE2)  # sorted 0 1 3 4 -> 2; negated -4 -3 -1 0 -> -2
    assert _bits(t) == _bits([2, -2])
    t = ref_thresholds(_col(1, 4, 2, 0), EYE2)  # sorted 0 1 2 4 -> 1.5
    assert _bits(t) == _bits([1.5, -1.5])
    assert t.dtype == np.float32


def test_negative_zero_in_the_middle_is_positive_zero():
    nz = np.float32(-0.0)
    x = np.array([[-1, nz], [nz, nz], [0.0, 0.0], [2, 1]], np.float32)
    R = np.array([[1, 0], [0, 1], [-1, 0]], np.float32)  # the third projection turns +0.0 into -0.0 as well
    t = ref_thresholds(x, R)
    assert _bits(t) == [0, 0, 0]
    assert _bits(ref_thresholds(x[:3], R)) == [0, 0, 0]
    assert _bits(ref_projections(np.array([[nz, nz]], np.float32), R)[0]) == [0, 0, 0]
    # and a row at +-0.0 is on the threshold: bit set
    assert unpack_bits(ref_codes_thr(x[1:3], R, t), 3).all()


def test_zero_thresholds_are_the_plain_codes():
    rng = np.random.default_rng(0)
    for nbits, d in ((1, 1), (7, 33), (65, 32), (200, 100)):
        R = pm1_rotation(rng, nbits, d)
        x = int_rows(rng, 300, d, values=(-2, -1, 0, 1, 2))
        assert np.array_equal(ref_codes_thr(x, R, 0), ref_codes(x, R))
        assert np.array_equal(ref_codes_thr(x, R, np.zeros(nbits, np.float32)), ref_codes(x, R))


def test_codes_against_thresholds_by_hand():
    x = _col(9, 5, -7, 2)  # thresholds 3.5, -3.5
    c = ref_codes_thr(x, EYE2, ref_thresholds(x, EYE2))
    # bit 0: 9, 5 >= 3.5; bit 1: 7, -2 >= -3.5
    assert c.reshape(-1).tolist() == [1, 1, 2, 2]


def test_the_half_integer_case_of_the_gpu_test():
    """d = 33, nbits = 65, n = 128, rows half from (-2, 0, 2) and half from (-3, -1, 1, 3): some thresholds are half-integers
    and many rows sit on their threshold (the GPU test relies on both)"""
    rng = np.random.default_rng(3)
    R = pm1_rotation(rng, 65, 33)
    x = np.concatenate([int_rows(rng, 64, 33, values=(-2, 0, 2)), int_rows(rng, 64, 33)])
    x = np.ascontiguousarray(rng.permutation(x))
    t = ref_thresholds(x, R)
    assert (t != np.rint(t)).sum() >= 1 and ((2 * t) == np.rint(2 * t)).all()
    assert (ref_projections(x, R) == t).any(axis=1).sum() >= 1
    ones = unpack_bits(ref_codes_thr(x, R, t), 65).sum(0)
    assert (ones >= 64).all()


def test_float64_medians_and_tolerance():
    rng = np.random.default_rng(1)
    x = rng.standard_normal((101, 16)).astype(np.float32)
    R = rng.standard_normal((9, 16)).astype(np.float32)
    t = ref_thresholds(x, R)
    m = median64(x, R)
    tol = threshold_tol(x, R, t)
    assert tol.shape == (9,) and (tol > 0).all() and (tol < 1e-4).all()
    assert (np.abs(t - m) <= tol).all()
