"""Non-finite and overflowing rows for IndexLSH: the generator and the rule-derived projection of every (row, bit) pair.
Shared by tests/test_lsh_nonfinite_reference.py (CPU: pins the references) and tests/test_lsh_nonfinite_gpu.py (GPU: compares
the library with them).  Plain numpy, nothing of the library under test.

The rows are lsh_reference.int_rows (small odd integers) against a rotation in {-1, +1} (lsh_reference.pm1_rotation), with
single entries poisoned.  Kinds of poisoned rows (columns are fixed, d >= 5):

  nan    NaN at column C_NAN                 every projection is a NaN: every bit is 0, whatever the threshold
  pinf   +inf at column C_INF                projection +inf where R[j][C_INF] = +1, -inf where it is -1: without thresholds
                                             the bit is the sign of the rotation's entry
  ninf   -inf at column C_INF                the mirror image of pinf.  Not among KINDS (poison_rows does not cycle through
                                             it): train_case uses it to put -inf and +inf into one column
  both   +inf at C_B1, -inf at C_B2          the two infinite terms are R[j][C_B1] * inf and -R[j][C_B2] * inf: a NaN where
                                             the two rotation entries are equal, +inf / -inf where they differ
  p127   +2^127 at column C_BIG              one term of +-2^127 among small integers whose sum is far below its ulp
  m127   -2^127 at column C_BIG              (2^104): the projection is exactly that term in every summation order
  zero   the all-zero row                    every projection is +0.0: bit 1 without thresholds (0 - 0 >= 0)

Rows of MANY huge entries are left out on purpose: their partial sums overflow in one summation order and not in another.

`classify` derives the float32 projection of ANY (row, bit) pair from its terms alone, by rules that hold for every order
of an fp32 accumulation (one rounding per step), as nonfinite_cases.classify does for the flat scan:
  * a NaN term, or terms of +inf and -inf together, make the projection a NaN;
  * otherwise an infinite term makes it that infinity (the finite terms are bounded by 2^127 + 2^24: no overflow);
  * finite terms that are integers with an absolute sum below 2^24 give their exact sum (every partial sum is an integer
    below 2^24);
  * ONE term of magnitude >= 2^100 beside such integers is the projection (adding less than half an ulp changes nothing);
  * anything else would depend on the order: the generator makes no such row, and classify raises if it meets one.
The code bit then follows as FAISS computes it (lsh_reference.faiss_bits): float32 (projection - threshold) >= 0."""
import numpy as np

from lsh_reference import faiss_bits, int_rows, pack_bits, pm1_rotation

C_BIG, C_INF, C_NAN, C_B1, C_B2 = 0, 1, 2, 3, 4
KINDS = ("nan", "pinf", "both", "p127", "m127", "zero")
BIG = np.float32(2.0 ** 127)


def make_row(kind, base):
    v = np.array(base, np.float32, copy=True)
    if kind == "nan":
        v[C_NAN] = np.nan
    elif kind == "pinf":
        v[C_INF] = np.inf
    elif kind == "ninf":
        v[C_INF] = -np.inf
    elif kind == "both":
        v[C_B1], v[C_B2] = np.inf, -np.inf
    elif kind == "p127":
        v[C_BIG] = BIG
    elif kind == "m127":
        v[C_BIG] = -BIG
    elif kind == "zero":
        v[:] = 0
    else:
        raise ValueError(kind)
    return v


def special_rows(n):
    """row positions the encoder treats specially (clipped to n, distinct, ascending): the first and last row of a 128-row
    tile, the rows of the last (ragged) tile, and in a wave's accumulators both 32-row blocks (rows 0..31 / 32..63 of a
    64-row band) and both halves of the lanes (row % 8 < 4 / >= 4), in both bands"""
    last = (n - 1) // 128 * 128
    pos = {0, 1, 5, 33, 37, 66, 70, 98, 102, 127, 128, 129, 133, 255, 256, last, last + 1, n - 2, n - 1}
    return sorted(p for p in pos if 0 <= p < n)


def poison_rows(rng, n, d, where=None):
    """(x float32 [n][d], kinds {row: kind}): int_rows with row where[i] made kind KINDS[i % 6] (`where`: positions, default
    special_rows(n); or (row, kind) pairs)"""
    assert d >= 5
    x = int_rows(rng, n, d)
    kinds = {}
    for i, w in enumerate(special_rows(n) if where is None else where):
        r, kind = w if isinstance(w, tuple) else (int(w), KINDS[i % len(KINDS)])
        assert 0 <= r < n and r not in kinds
        x[r] = make_row(kind, x[r])
        kinds[r] = kind
    return x, kinds


def train_case(n, case, nbits=9, d=7, seed=0):
    """training rows over a +-1 rotation: m rows with +inf at C_INF (projection +inf on the bits whose rotation entry is +1,
    -inf on the others), spread over the rows"""
    rng = np.random.default_rng(seed + n)
    R = pm1_rotation(rng, nbits, d)
    R[0, C_INF], R[1, C_INF] = 1, -1
    R[0, C_BIG], R[1, C_BIG] = 1, -1
    m = {"few": (n - 1) // 2, "middle": n // 2 + 1 if n % 2 else n // 2, "most_big": n // 2 + 1, "around": n // 2, "nan": 1}[case]
    kind = {"few": "pinf", "middle": "pinf", "most_big": "p127", "around": "pinf", "nan": "nan"}[case]
    rows = [int(r) for r in np.linspace(0, n - 1, m).round()] if m > 1 else [n // 2]
    assert len(set(rows)) == m
    where = [(r, kind) for r in rows]
    if case == "around":  # +inf and -inf around the middle of an even n: every other row is -inf
        where += [(r, "ninf") for r in range(n) if r not in rows]
    return poison_rows(rng, n, d, where)[0], R


def classify(x, R, chunk=64):
    """float32 [n][nbits]: the projection of every row onto every rotation row, by the rules of the header; raises
    AssertionError on a pair whose value would depend on the summation order"""
    x = np.asarray(x, np.float32).astype(np.float64)
    R = np.asarray(R, np.float32).astype(np.float64)
    out = np.empty((x.shape[0], R.shape[0]), np.float32)
    for i in range(0, x.shape[0], chunk):
        with np.errstate(all="ignore"):
            T = x[i:i + chunk, None, :] * R[None, :, :]
            nan = np.isnan(T).any(-1)
            pinf = (T == np.inf).any(-1)
            ninf = (T == -np.inf).any(-1)
            fin = np.where(np.isfinite(T), T, 0.0)
            big = np.abs(fin) >= 2.0 ** 100
            small = np.where(big, 0.0, fin)
            if not np.array_equal(small, np.rint(small)) or not (np.abs(small).sum(-1) < 2 ** 24).all():
                raise AssertionError("finite terms that are no small integers: the projection depends on the summation order")
            if (big.sum(-1) > 1).any():
                raise AssertionError("more than one huge term: the partial sums can overflow in one order and not in another")
            p = np.where(big.any(-1), np.where(big, fin, 0.0).sum(-1), small.sum(-1))
            p = np.where(pinf, np.inf, p)
            p = np.where(ninf, -np.inf, p)
            p = np.where(nan | (pinf & ninf), np.nan, p)
            out[i:i + chunk] = p.astype(np.float32)  # (an integer below 2^24, +-2^127, an infinity or a NaN: exact)
    return out


def expected_codes(x, R, t=0.0):
    """uint8 [n][(nbits + 7) // 8]: the codes by the rules (classify) and FAISS's bit (faiss_bits)"""
    return pack_bits(faiss_bits(classify(x, R), t))
