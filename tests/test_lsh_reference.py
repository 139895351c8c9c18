"""CPU: the exact IndexLSH restatement of tests/lsh_reference.py on hand-computed cases, and its comparison helpers'
verdicts on results that are wrong in the ways a kernel goes wrong (a tie out of order, a flipped bit, wrong padding)."""
import numpy as np
import pytest

from lsh_reference import (FLT_MAX, codes_diff, hamming, int_rows, pm1_rotation, rand_codes, ref_codes, ref_search,
                           search_diff, zero_projection_rows)


def test_ref_codes_by_hand():
    x = np.array([[1, -2], [0, 0], [-1, -1], [2, -2]], np.float32)
    R = np.array([[1, 0], [0, 1], [1, 1]], np.float32)
    # projections: (1, -2, -1), (0, 0, 0), (-1, -1, -2), (2, -2, 0): bit j set where >= 0, bit j -> byte j >> 3, bit j & 7
    assert ref_codes(x, R).tolist() == [[0b001], [0b111], [0b000], [0b101]]
    # nine bits: two bytes, the seven bits above nbits stay zero
    assert ref_codes(np.ones((1, 1), np.float32), np.ones((9, 1), np.float32)).tolist() == [[0xFF, 0x01]]
    assert ref_codes(-np.ones((1, 1), np.float32), np.ones((9, 1), np.float32)).tolist() == [[0x00, 0x00]]
    # bit 8 alone: byte 1, bit 0
    R9 = -np.ones((9, 1), np.float32)
    R9[8] = 1
    assert ref_codes(np.ones((1, 1), np.float32), R9).tolist() == [[0x00, 0x01]]


def test_ref_codes_zero_projection_rows():
    rng = np.random.default_rng(0)
    R = pm1_rotation(rng, 40, 10)
    x, js = zero_projection_rows(rng, R, 30)
    assert np.array_equal((x.astype(np.float64) @ R.T.astype(np.float64))[np.arange(30), js], np.zeros(30))
    bits = np.unpackbits(ref_codes(x, R), axis=1, bitorder="little")
    assert (bits[np.arange(30), js] == 1).all(), "x . R[j] == 0 is a 1 bit"
    with pytest.raises(ValueError):
        zero_projection_rows(rng, pm1_rotation(rng, 4, 3), 1)


def test_rand_codes_padding():
    c = rand_codes(np.random.default_rng(1), 500, 13)
    assert c.shape == (500, 2) and (c[:, 1] < 32).all() and c[:, 1].max() == 31


def test_ref_search_by_hand():
    db = np.array([[0b0000], [0b0011], [0b0001], [0b0001], [0b1111]], np.uint8)
    q = np.array([[0b0000], [0b1111]], np.uint8)
    D, I = ref_search(db, q, 3)
    assert D.dtype == np.float32 and I.dtype == np.int64
    assert D.tolist() == [[0, 1, 1], [0, 2, 3]] and I.tolist() == [[0, 2, 3], [4, 1, 2]]
    D, I = ref_search(db, q, 7)
    assert I.tolist() == [[0, 2, 3, 1, 4, -1, -1], [4, 1, 2, 3, 0, -1, -1]]
    assert D[:, :5].tolist() == [[0, 1, 1, 2, 4], [0, 2, 3, 3, 4]] and (D[:, 5:] == FLT_MAX).all()
    D, I = ref_search(db[:0], q, 2)
    assert (I == -1).all() and (D == FLT_MAX).all()
    # a code of 9 bytes: the ninth lands in the second uint64 word, zero-padded
    db9 = np.zeros((2, 9), np.uint8)
    db9[1, 8] = 0xFF
    D, I = ref_search(db9, np.zeros((1, 9), np.uint8), 2)
    assert D.tolist() == [[0, 8]] and I.tolist() == [[0, 1]]


@pytest.mark.parametrize("nbytes,nb,k", [(1, 300, 50), (3, 1000, 999), (16, 2000, 2048), (256, 700, 100), (9, 5000, 1)])
def test_ref_search_equals_a_full_stable_sort(nbytes, nb, k):
    rng = np.random.default_rng(nbytes * 100 + k)
    db = rng.integers(0, 256, (nb, nbytes), dtype=np.uint8)
    db[rng.integers(0, nb, nb // 3)] = db[0]  # duplicated rows: tie groups
    q = rng.integers(0, 256, (17, nbytes), dtype=np.uint8)
    q[0] = db[5]
    D, I = ref_search(db, q, k, max_elems=3 * nb)  # (several query chunks)
    dist = hamming(db, q).astype(np.int64)
    assert np.array_equal(dist, np.unpackbits(db[None] ^ q[:, None], axis=2).sum(axis=2))
    order = np.argsort(dist, axis=1, kind="stable")[:, :k]
    kk = min(k, nb)
    assert np.array_equal(I[:, :kk], order) and np.array_equal(D[:, :kk], np.take_along_axis(dist, order, 1).astype(np.float32))
    assert (I[:, kk:] == -1).all() and (D[:, kk:] == FLT_MAX).all()


def test_exact_inputs_stay_integral():
    """rows from {-3, -1, 1, 3} against a +-1 rotation: |x . r| <= 3 d, far below 2^24 at d = 1024"""
    rng = np.random.default_rng(2)
    x = int_rows(rng, 50, 1024)
    assert set(np.unique(x).tolist()) == {-3.0, -1.0, 1.0, 3.0}
    R = pm1_rotation(rng, 64, 1024)
    assert set(np.unique(R).tolist()) == {-1.0, 1.0}
    p32 = x @ R.T
    assert np.array_equal(p32.astype(np.float64), x.astype(np.float64) @ R.T.astype(np.float64))


def _expected():
    db = np.array([[0b0000], [0b0001], [0b0001], [0b0011]], np.uint8)
    return ref_search(db, np.zeros((1, 1), np.uint8), 6)  # I = [0, 1, 2, 3, -1, -1]


def test_search_diff_accepts_equal_results():
    D, I = _expected()
    assert search_diff(D.copy(), I.copy(), D, I) is None


def test_search_diff_rejects_swapped_tied_ids():
    D, I = _expected()
    I2 = I.copy()
    I2[0, [1, 2]] = I2[0, [2, 1]]  # ids 1 and 2 are tied at distance 1
    msg = search_diff(D, I2, D, I)
    assert msg is not None and "query 0 position 1" in msg and "got id 2" in msg and "expected id 1" in msg


def test_search_diff_rejects_a_flipped_distance_bit():
    D, I = _expected()
    D2 = D.copy()
    D2[0, 3] = np.float32(3)
    assert search_diff(D2, I, D, I) is not None
    D2 = D.copy()
    D2[0, 0] = np.float32(-0.0)  # the same value, other bits
    assert search_diff(D2, I, D, I) is not None


def test_search_diff_rejects_wrong_padding():
    D, I = _expected()
    for pad in (np.inf, 0.0, np.finfo(np.float32).max / 2):
        D2 = D.copy()
        D2[0, 4] = pad
        assert search_diff(D2, I, D, I) is not None, pad


def test_search_diff_rejects_a_missing_minus_one():
    D, I = _expected()
    I2 = I.copy()
    I2[0, 5] = 0
    msg = search_diff(D, I2, D, I)
    assert msg is not None and "position 5" in msg


def test_search_diff_rejects_wrong_shapes_and_dtypes():
    D, I = _expected()
    assert search_diff(D[:, :5], I[:, :5], D, I) is not None
    assert search_diff(D.astype(np.float64), I, D, I) is not None
    assert search_diff(D, I.astype(np.int32), D, I) is not None


def test_codes_diff_rejects_one_flipped_bit():
    c = rand_codes(np.random.default_rng(3), 20, 777)
    assert codes_diff(c.copy(), c) is None
    c2 = c.copy()
    c2[13, 97] ^= 1 << 5
    msg = codes_diff(c2, c)
    assert msg is not None and "row 13 byte 97" in msg and f"code bit {97 * 8 + 5}" in msg
    c3 = c.copy()
    c3[0, -1] |= 0x80  # a set padding bit (777 = 97 * 8 + 1)
    assert codes_diff(c3, c) is not None
    assert codes_diff(c[:, :-1], c) is not None
