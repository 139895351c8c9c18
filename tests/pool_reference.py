"""The CPU restatement of the pooling contract above knn_pool_ranges in include/knn355.h, and the inputs the pooling
tests share.

pool_sequential is the contract in explicit loops: per range one float32 accumulator row that starts as the first row
and takes one float32 add per further row in ascending order, then one float32 division by (float)L.  The normalizing
variant is the oracle's normalize_l2 (oracle/knn_oracle.c: the restatement of faiss.normalize_L2 every other test uses)
on a float32 copy, followed by the same loops.  pool_pairwise is NOT the contract: a balanced tree over the rows, kept
to show that the order-sensitive case tells the two apart."""
import numpy as np

GRID_L = (1, 2, 7, 8, 9, 127, 128, 129, 1000)
GRID_D = (2, 8, 20, 1024, 3072)


def pool_sequential(x, starts, stops):
    """float32 [n, d]; x float32 or float16 [rows, d] (float16 converts exactly)"""
    x = np.asarray(x)
    out = np.empty((len(starts), x.shape[1]), np.float32)
    with np.errstate(all="ignore"):
        for o, (a, b) in enumerate(zip(starts, stops)):
            a, b = int(a), int(b)
            assert 0 <= a < b <= x.shape[0] and b - a < 1 << 24
            acc = x[a].astype(np.float32)
            for r in range(a + 1, b):
                acc = acc + x[r].astype(np.float32)
            assert acc.dtype == np.float32
            out[o] = acc / np.float32(b - a)
    return out


def pool_normalized(x, starts, stops, oracle):
    """knn_normalize_l2 (the oracle's) on a float32 copy of x, then the plain pooling"""
    y = np.ascontiguousarray(x, np.float32).copy()
    with np.errstate(all="ignore"):
        oracle.normalize_l2(y)
    return pool_sequential(y, starts, stops)


def pool_pairwise(x, starts, stops):
    """a balanced binary tree over the rows of each range: what a kernel that splits a range by rows would compute"""
    def tree(rows):
        if len(rows) == 1:
            return rows[0]
        h = len(rows) // 2
        return tree(rows[:h]) + tree(rows[h:])
    x = np.asarray(x, np.float32)
    with np.errstate(all="ignore"):
        return np.stack([tree(list(x[int(a):int(b)])) / np.float32(int(b) - int(a)) for a, b in zip(starts, stops)])


def bits_differ(a, b):
    """positions where a and b differ: NaN-ness by position, bits elsewhere (tests/nonfinite_cases.py's rule for scores)"""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    assert a.shape == b.shape, (a.shape, b.shape)
    na, nb = np.isnan(a), np.isnan(b)
    return np.argwhere((na != nb) | (~na & (a.view(np.uint32) != b.view(np.uint32))))


# ---- shared inputs ------------------------------------------------------------------------------
RANGE_LENGTHS = (1, 2, 8, 9, 63, 64, 65, 129, 1000)


def residues(rows, d, seed, dtype=np.float32):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((rows, d), dtype=np.float32) * np.float32(0.7) + rng.uniform(-1, 1, d).astype(np.float32)
    return x.astype(dtype)


def ranges(rows, seed):
    """(starts, stops): every length of RANGE_LENGTHS at a seeded place, overlapping and unordered, one duplicate, one
    range over all rows, the first and the last row alone"""
    rng = np.random.default_rng(seed)
    pairs = []
    for L in RANGE_LENGTHS:
        if L <= rows:
            a = int(rng.integers(0, rows - L + 1))
            pairs.append((a, a + L))
    pairs += [(0, rows), (0, 1), (rows - 1, rows), pairs[3]]
    for _ in range(6):
        a = int(rng.integers(0, rows))
        pairs.append((a, int(rng.integers(a + 1, min(rows, a + 200) + 1))))
    order = rng.permutation(len(pairs))
    starts = np.asarray([pairs[i][0] for i in order], np.int64)
    stops = np.asarray([pairs[i][1] for i in order], np.int64)
    return starts, stops


def order_sensitive(rows=1024, d=8):
    """columns of [1e8, 1, -1e8, 1, ...] patterns at different phases: the running sum swings between 1e8, where a 1 is
    below half an ulp and is lost, and small values, where it counts -- a tree over the same rows loses other ones"""
    pattern = np.asarray([1e8, 1.0, -1e8, 1.0], np.float32)
    x = np.empty((rows, d), np.float32)
    for c in range(d):
        x[:, c] = np.roll(pattern, c % 4)[np.arange(rows) % 4] * np.float32(1 + c // 4)
    return x


def special_values(rows=200, d=20, seed=5):
    """a first row of -0.0, subnormal entries, +-inf and NaN entries in known places"""
    x = residues(rows, d, seed)
    x[0] = np.float32(-0.0)
    x[1, 0] = np.float32(-0.0)
    x[10:20, 3] = np.float32(1e-41)    # subnormal
    x[10:20, 4] = np.float32(-3e-45)   # the smallest subnormals
    x[15, 4] = np.float32(1.4e-45)
    x[30:33, :] = np.float32(1e-40)    # whole subnormal rows: their sum and mean stay subnormal
    x[40, 5] = np.inf
    x[41, 6] = -np.inf
    x[42, 7] = np.nan
    x[43, 8], x[44, 8] = np.inf, -np.inf  # inf - inf
    starts = np.asarray([0, 0, 1, 10, 30, 30, 35, 35, 40, 43, 0, 100], np.int64)
    stops = np.asarray([1, 2, 2, 20, 33, 31, 41, 50, 45, 45, rows, 180], np.int64)
    return x, starts, stops


def normalize_edge_rows(rows=150, d=20, seed=9):
    """a zero row, a row whose norm overflows (factor 0: the row becomes +-0, or NaN where it holds an infinity), a row
    with a NaN (its norm is NaN: not > 0, used as it is), a subnormal row whose norm underflows to 0"""
    x = residues(rows, d, seed)
    x[5] = 0.0
    x[17] = np.float32(3e19)
    x[18, 2] = np.inf
    x[40, 1] = np.nan
    x[60] = np.float32(1e-30)
    starts = np.asarray([0, 5, 4, 17, 10, 18, 40, 35, 60, 55, 0], np.int64)
    stops = np.asarray([10, 6, 7, 18, 30, 19, 41, 45, 61, 70, rows], np.int64)
    return x, starts, stops
