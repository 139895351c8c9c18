"""The contract of knn_eval_rankdata / knn_eval_correlate (include/knn355.h) in numpy and Python integers: the bit-for-bit
yardstick of csrc/correlate.inc.  Nothing here runs on a device and nothing is imported from the package.

  key_image        rank.inc's order-preserving unsigned image of a float (-0.0 -> +0.0, every NaN -> all ones)
  doubled_ranks    stable argsort of the images, runs of equal images, s + e + 2 for every member of a run at ranks s .. e
  spearman_sums    the exact integers sum u*u, sum u*v, sum v*v over u = rank2_x - (N + 1), v = rank2_y - (N + 1)
  ordered_sum      one float64 sum in plan_correlate's order: tiles of 2048, 256 lanes of 8 strided terms, a halving tree
  pearson_moments  mean_x, mean_y, Sxx, Sxy, Syy in that order, two passes
  plan             plan_correlate's sizes and levels
"""
import math

import numpy as np

TILE, LANES, MAX_LEVELS, TIE_GRID = 2048, 256, 3, 65536  # CORR_TILE, CORR_LANES, CORR_MAX_LEVELS, CORR_GRID of csrc/plan.h
RANK_TILE, SCAN_BLOCK = 2048, 1024                       # RANK_TILE, RANK_SCAN_BLOCK
PEARSON, SPEARMAN = 1, 2


def cells(a, limit=None):
    """a[:, :limit] flattened row by row (a 1-D array is one column), in its own float type"""
    a = np.asarray(a)
    if a.ndim == 1:
        a = a.reshape(-1, 1)
    a = a if a.dtype == np.float32 else a.astype(np.float64)
    return np.ascontiguousarray(a[:, :limit]).reshape(-1)


def key_image(v):
    """uint32 / uint64 per value: ascending images order the values, -0.0 equals +0.0, every NaN is the largest"""
    v = np.asarray(v)
    u = v.view(np.uint32 if v.dtype == np.float32 else np.uint64).copy()
    top = u.dtype.type(1) << u.dtype.type(8 * u.dtype.itemsize - 1)
    u[u == top] = 0
    img = np.where(u & top, ~u, u | top)
    img[np.isnan(v)] = ~u.dtype.type(0)
    return img


def doubled_ranks(v):
    """-> (rank2 int64 [N], NaN cells): rank2[p] = s + e + 2 over the run s .. e of equal images that holds cell p"""
    img = key_image(v)
    n = img.size
    order = np.argsort(img, kind="stable")
    s = img[order]
    head = np.ones(n, bool)
    head[1:] = s[1:] != s[:-1]
    run = np.cumsum(head) - 1                      # 0-based run number of every rank
    start = np.append(np.flatnonzero(head), n)     # first rank of every run, and N behind the last
    rank2 = np.empty(n, np.int64)
    rank2[order] = start[run] + (start[run + 1] - 1) + 2
    return rank2, int(np.isnan(np.asarray(v)).sum())


def spearman_sums(rank2_x, rank2_y):
    """exact Python integers (Suu, Suv, Svv)"""
    n = len(rank2_x)
    u = [int(r) - (n + 1) for r in rank2_x]
    v = [int(r) - (n + 1) for r in rank2_y]
    return sum(a * a for a in u), sum(a * b for a, b in zip(u, v)), sum(b * b for b in v)


def spearman_sums_fast(rank2_x, rank2_y):
    """the same integers for large N: int64 products (each below 2^62) summed in chunks that cannot overflow, the chunks
    as Python integers"""
    n = len(rank2_x)
    u, v = np.asarray(rank2_x, np.int64) - (n + 1), np.asarray(rank2_y, np.int64) - (n + 1)
    out = []
    for a, b in ((u, u), (u, v), (v, v)):
        prod = a * b
        hi, lo = prod >> 31, prod & ((1 << 31) - 1)  # prod = hi * 2^31 + lo; |hi| < 2^31, so 2^31 terms of either fit int64
        out.append((int(hi.sum()) << 31) + int(lo.sum()))
    return tuple(out)


def words(value):
    """a Python integer as the (lo, hi) uint64 words of its 128-bit two's complement"""
    value &= (1 << 128) - 1
    return value & ((1 << 64) - 1), value >> 64


def levels(n):
    """[N, ceil(N / 2048), ..., 1]"""
    out = [n]
    while out[-1] > 1:
        out.append(-(-out[-1] // TILE))
    return out


def ordered_sum(terms):
    """float64: the sum of float64 terms in plan_correlate's order"""
    t = np.asarray(terms, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        while True:
            tiles = -(-t.size // TILE)
            padded = np.zeros(tiles * TILE)          # (+0.0 added to a lane's sum, which starts at +0.0, changes nothing)
            padded[:t.size] = t
            steps = padded.reshape(tiles, TILE // LANES, LANES)
            lane = np.zeros((tiles, LANES))
            for i in range(TILE // LANES):           # lane j: terms j, j + 256, ... of its tile, in that order
                lane = lane + steps[:, i, :]
            off = LANES // 2
            while off:                               # lane[j] = lane[j] + lane[j + off], j < off
                lane = lane[:, :off] + lane[:, off:2 * off]
                off //= 2
            t = lane[:, 0]
            if t.size == 1:
                return float(t[0])


def pearson_moments(x, y):
    """float64 [5]: mean_x, mean_y, Sxx, Sxy, Syy"""
    x, y = np.asarray(x).astype(np.float64), np.asarray(y).astype(np.float64)
    n = x.size
    with np.errstate(invalid="ignore", over="ignore"):
        mx, my = ordered_sum(x) / np.float64(n), ordered_sum(y) / np.float64(n)
        dx, dy = x - mx, y - my
        return np.array([mx, my, ordered_sum(dx * dx), ordered_sum(dx * dy), ordered_sum(dy * dy)])


def ratio(sab, saa, sbb):
    """sab / (sqrt(saa) * sqrt(sbb)) clipped to [-1, 1]; NaN for a zero or NaN denominator"""
    sab, saa, sbb = float(sab), float(saa), float(sbb)
    den = math.sqrt(saa) * math.sqrt(sbb) if saa >= 0 and sbb >= 0 else math.nan
    if den == 0 or den != den or sab != sab:
        return math.nan
    r = sab / den
    return r if r != r else max(-1.0, min(1.0, r))


def spearman_ratio(suu, suv, svv):
    """ratio() of the exact integers; where they say |rho| = 1 -- Suv^2 = Suu Svv, both sides not 0 -- exactly +-1, which
    the product of two rounded square roots may miss by an ulp"""
    if suu and svv and suv * suv == suu * svv:
        return 1.0 if suv > 0 else -1.0
    return ratio(suv, suu, svv)


def pearson(x, y, limit=None):
    m = pearson_moments(cells(x, limit), cells(y, limit))
    return ratio(m[3], m[2], m[4])


def spearman(x, y, limit=None):
    (rx, nx), (ry, ny) = doubled_ranks(cells(x, limit)), doubled_ranks(cells(y, limit))
    if nx or ny:
        return math.nan
    return spearman_ratio(*spearman_sums_fast(rx, ry))


def rank_plan(rows, k, limit, key_bytes):
    """plan_rank(rows, k, limit, key_bytes, no flags, running count, no wide) -> scores, keys, pay, table, partial, hist bytes"""
    n = rows * limit
    dev_k = limit if 2 * limit <= k else k
    ntiles = -(-n // RANK_TILE)
    table = 256 * ntiles
    return {"scores": rows * dev_k * key_bytes, "keys": n * key_bytes, "pay": n * 4, "table": table * 4,
            "partial": max(-(-table // SCAN_BLOCK), -(-n // SCAN_BLOCK)) * 4, "hist": key_bytes * 1024}


def plan(rows, k, limit, x_bytes, y_bytes, what):
    """plan_correlate as the line `correlate_check plan` prints, or "refused" """
    n = rows * limit
    if (rows < 1 or k < 1 or not 1 <= limit <= k or k > 2 ** 31 - 1 or not 2 <= n <= 2 ** 31 - 1 or x_bytes not in (4, 8) or not 0 <= what <= 3
            or (what == 0) != (y_bytes == 0) or (y_bytes and y_bytes not in (4, 8))):
        return "refused"
    rx, ry = rank_plan(rows, k, limit, x_bytes), rank_plan(rows, k, limit, y_bytes or x_bytes)
    wide = ry if y_bytes > x_bytes else rx
    sorts = what != PEARSON
    lv = levels(n)
    level_n = lv + [1] * (MAX_LEVELS + 1 - len(lv))
    entry = 3 * (16 if what & SPEARMAN else 8)
    shared = [wide[name] if sorts else 0 for name in ("keys", "pay", "table", "partial", "hist")]
    run, start = (n * 4, (n + 1) * 4) if sorts else (0, 0)
    rank2, buffers, nan = (n * (4 if what else 8), 2 if what else 1, 16) if sorts else (0, 0, 0)
    ma, mb = (level_n[1] * entry, level_n[2] * entry) if what else (0, 0)
    xb, yb = rx["scores"], ry["scores"] if y_bytes else 0
    resident = xb + yb + 2 * shared[0] + 2 * shared[1] + sum(shared[2:]) + run + start + buffers * rank2 + nan + ma + mb
    fields = [n, len(lv) - 1, *level_n, min(TIE_GRID, -(-n // 256)), xb, yb, *shared, run, start, rank2, buffers, nan, ma, mb, resident]
    return " ".join(map(str, fields))
