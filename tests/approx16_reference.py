"""Host reference of the approximate (bf16) flat scan: flat_scan_kernel<..., BF16> behind knn_flat_set_approx16 and the coarse
entry indexes of IndexHNSWFlat.

The kernel multiplies bf16 copies (round to nearest even) of rows and queries on v_mfma_f32_32x32x16_bf16: every product of
two 8-bit significands is exact in fp32, the accumulation is fp32 in an order nobody has documented.  So there is no bit
contract for general inputs, but there is one for inputs on which every order gives the same answer:

  rows and queries are integers times one power of two (`scale`), and for every (query, row) pair
      nrm(x) + nrm(y) + 2 * sum |x_i * y_i|  <  2^24      (in units of scale^2; `check_precondition`)

Then every partial sum of the dot product, the fp32 norms of the UNROUNDED rows and queries (the kernel takes its norms from
the fp32 copies) and fma(-2, dot, nx + ny) are integers below 2^24: exact in fp32 in any order.  The expected result is plain
integer arithmetic (`expected`), compared bit for bit.  The integers are carried in float64 (exact below 2^53) so that the
products run on BLAS.

`float_reference` is the bounded comparison for ordinary floats (exponents that differ across a row).

Non-finite and overflowing inputs (a "smaller is better" value of +inf or a NaN never becomes a hit, an
inner-product score of +inf is the best hit, a starved query is padded) -- `classify16`, `expected_nonfinite`.  The data is
tests/nonfinite_cases.poison_ints: small integers with the poisoned kinds of that file.  The scan multiplies the ROUNDED
operands and takes its norms from the fp32 values, and it has no difference build, so there are two forms, "ip" and "l2n",
and nonfinite_cases.classify's term rules are applied to the rounded vectors' products and the unrounded vectors' norms.
Rounding changes the outcome of ONE kind, `fltmax`: bf16_rne(FLT_MAX) is +inf, so its single term is q[0] * inf -- the best
hit for a query that is positive there, none for one that is negative -- where fp32 has a finite +-FLT_MAX.  `huge` (3e19)
and `twin` (1.8e19) stay finite and keep their fp32 outcome.  TABLE16 / PAIRS16 state every cell; ROUNDING_CHANGES names the
kinds whose row differs from nonfinite_cases.ISSUE_TABLE.

A finite score has one right answer here too: every vector is small integers (unit 1) or small-integer multiples of ONE
huge bf16 value (the rounded 3e19 of `huge`, 1.8e19 of `twin`; 8 significant bits), so a dot product is
unit_q * unit_b * sum(c_q c_b) with integer coefficients, and every partial sum is exact in fp32 as long as
bits(unit_q unit_b) + bits(sum |c_q c_b|) <= 24, which `expected_nonfinite` asserts pair by pair.  The L2 value is
max(0, fma(-2, dot, nx + ny)): nx + ny is one fp32 addition of two fp32 numbers, the fma rounds the exact integer
nx + ny - 2 dot once (`_f32_of_int`)."""
import numpy as np

import nonfinite_cases as nc

IP, L2 = 0, 1
FLT_MAX = np.float32(3.4028234663852886e38)
LIMIT = 1 << 24


class PreconditionError(AssertionError):
    """the inputs are not ones on which every summation order gives the same fp32 answer"""


def bf16_rne(x):
    """float32 -> the nearest bf16 (ties to the even significand), returned as float32.  +-inf stay +-inf, a finite value
    beyond the largest bf16 (0x7F7F0000, 3.39e38) plus half its last place rounds to +-inf -- FLT_MAX does; 1.8e19 (the `twin`
    of tests/nonfinite_cases.py) stays finite -- and a NaN stays a NaN whatever its payload (the increment alone would carry
    some payloads into the infinity's pattern, or out of the word)"""
    x = np.ascontiguousarray(x, np.float32)
    u = x.view(np.uint32).astype(np.uint64)
    u = (u + np.uint64(0x7FFF) + ((u >> np.uint64(16)) & np.uint64(1))) & np.uint64(0xFFFF0000)
    return np.where(np.isnan(x), np.float32(np.nan), (u & np.uint64(0xFFFFFFFF)).astype(np.uint32).view(np.float32))


def bf16_trunc(x):
    """float32 -> bf16 by dropping the low 16 bits (what the kernel must NOT do), returned as float32"""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32) & np.uint32(0xFFFF0000)
    return u.view(np.float32)


def units(x, scale=1.0):
    """x / scale as exact integers (float64); raises PreconditionError if some value is no integer multiple of scale"""
    m, e = np.frexp(float(scale))
    if m != 0.5:
        raise PreconditionError(f"scale {scale!r} is no power of two")
    u = np.asarray(x, np.float64) / float(scale)
    if not np.all(np.isfinite(u)) or not np.array_equal(u, np.rint(u)):
        raise PreconditionError("a value is no integer multiple of the scale")
    return u


def check_precondition(xb, xq, scale=1.0, rounding=bf16_rne):
    """Asserts nrm(x) + nrm(y) + 2 sum|x_i y_i| < 2^24 for every pair, in units of scale^2, with the norms the larger of the
    unrounded and the rounded values' and the products those of the rounded values.  Returns the largest value met."""
    xb, xq = np.ascontiguousarray(xb, np.float32), np.ascontiguousarray(xq, np.float32)
    ub, uq, rb, rq = units(xb, scale), units(xq, scale), units(rounding(xb), scale), units(rounding(xq), scale)
    nb_ = np.maximum((ub * ub).sum(1), (rb * rb).sum(1))
    nq_ = np.maximum((uq * uq).sum(1), (rq * rq).sum(1))
    worst = 0.0
    for q0 in range(0, xq.shape[0], 256):
        t = nq_[q0:q0 + 256, None] + nb_[None, :] + 2.0 * (np.abs(rq[q0:q0 + 256]) @ np.abs(rb).T)
        worst = max(worst, float(t.max())) if t.size else worst
    if not worst < LIMIT:
        raise PreconditionError(f"nrm(x) + nrm(y) + 2 sum|x_i y_i| reaches {worst:.0f} >= 2^24: fp32 sums would depend on their order")
    return worst


def scores(xb, xq, metric, scale=1.0, rounding=bf16_rne, norms="fp32"):
    """[nq][nb] float32 scores of the approximate scan: the dot product of the rounded operands; for squared L2
    max(0, nx + ny - 2 dot) with the norms of the UNROUNDED values (norms="fp32": what the kernel does) or of the rounded
    ones (norms="rounded": what it must not do).  Checks the precondition first."""
    check_precondition(xb, xq, scale, rounding)
    xb, xq = np.ascontiguousarray(xb, np.float32), np.ascontiguousarray(xq, np.float32)
    rb, rq = units(rounding(xb), scale), units(rounding(xq), scale)
    dot = rq @ rb.T
    if metric == IP:
        s = dot
    else:
        nb_, nq_ = (rb, rq) if norms == "rounded" else (units(xb, scale), units(xq, scale))
        s = np.maximum(0.0, (nq_ * nq_).sum(1)[:, None] + (nb_ * nb_).sum(1)[None, :] - 2.0 * dot)
    assert np.all(np.abs(s) < LIMIT)
    out = (s * (float(scale) * float(scale))).astype(np.float32)  # (an integer below 2^24 times a power of two: exact)
    if metric == IP:
        # the scan's key holds v + 0 with v = -dot (so that -0.0 and +0.0 are one key) and the result is -v: a zero inner
        # product comes back as -0.0, as from every other scan path (merge_reference.pack_keys)
        return -((-out) + np.float32(0.0))
    return out + np.float32(0.0)


def rank(s, k, metric):
    """best k of every row of the score matrix s: by score (inner product: larger first), equal scores by ascending row id;
    slots beyond the rows are id -1 with -FLT_MAX (inner product) / +FLT_MAX (squared L2)"""
    nq, nb = s.shape
    key = -s.astype(np.float64) if metric == IP else s.astype(np.float64)
    order = np.argsort(key, axis=1, kind="stable")[:, :k]  # (stable: the lower id first among equal scores)
    D = np.full((nq, k), -FLT_MAX if metric == IP else FLT_MAX, np.float32)
    I = np.full((nq, k), -1, np.int64)
    m = min(k, nb)
    I[:, :m] = order[:, :m]
    D[:, :m] = np.take_along_axis(s, order[:, :m], axis=1)
    return D, I


def expected(xb, xq, k, metric, scale=1.0, rounding=bf16_rne, norms="fp32"):
    """(D float32 [nq][k], I int64 [nq][k]) the approximate index must return, bit for bit"""
    return rank(scores(xb, xq, metric, scale, rounding, norms), k, metric)


def float_reference(xb, xq, metric, dp, norms32_b=None, norms32_q=None):
    """Ordinary floats: (ref float64 [nq][nb], bound float64 [nq][nb]) with |kernel score - ref| <= bound for EVERY order of
    the fp32 accumulation.

    ref is the float64 dot product of the RNE-rounded operands; for squared L2 max(0, nx + ny - 2 dot) with the float64
    norms of the unrounded values.  The bound: the products are exact (two 8-bit significands), a sum of n = dp fp32 terms in
    any order and any tree is off by at most gamma_(n-1) * sum|p_i| <= n * 2^-24 * sum|p_i| (u = 2^-24, n (n - 1) u <= 1).
    Squared L2 adds: the error of the kernel's fp32 norms (norms32_b / norms32_q, the oracle's bits, against the float64
    ones), one rounding of nx + ny (2^-24 of it), twice the dot product's error, and the rounding of the fma (2^-24 of its
    exact argument, itself at most nx + ny + 2 (sum|p_i| + the dot product's error)); the clamp at 0 moves nothing apart."""
    u = 2.0 ** -24
    rb, rq = bf16_rne(xb).astype(np.float64), bf16_rne(xq).astype(np.float64)
    dot = rq @ rb.T
    bdot = dp * u * (np.abs(rq) @ np.abs(rb).T)
    if metric == IP:
        return dot, bdot
    nb64, nq64 = (np.asarray(xb, np.float64) ** 2).sum(1), (np.asarray(xq, np.float64) ** 2).sum(1)
    nb32, nq32 = np.asarray(norms32_b, np.float64), np.asarray(norms32_q, np.float64)
    ref = np.maximum(0.0, nq64[:, None] + nb64[None, :] - 2.0 * dot)
    nsum = nq32[:, None] + nb32[None, :]
    bound = (np.abs(nq32 - nq64)[:, None] + np.abs(nb32 - nb64)[None, :] + u * nsum + 2.0 * bdot
             + u * (nsum * (1 + u) + 2.0 * (np.abs(rq) @ np.abs(rb).T) + 2.0 * bdot))
    return ref, bound


# ---- non-finite and overflowing inputs ------------------------------------------------------------------------------------------
FORMS16 = ("ip", "l2n")
# outcome of (ordinary query, poisoned row) on the bf16 scan; a dict: by the sign of the query's entry at C_INF (pinf) / 0 (fltmax)
TABLE16 = {
    "nan": {"ip": "never", "l2n": "never"},
    "pinf": {"ip": {1: "best", -1: "never"}, "l2n": "never"},
    "pinf0": {"ip": "never", "l2n": "never"},
    "both": {"ip": "never", "l2n": "never"},
    "huge": {"ip": "hit", "l2n": "never"},                     # bf16(3e19) is finite; the fp32 norm overflows
    "twin": {"ip": "hit", "l2n": "hit"},                       # bf16(1.8e19) = 1.8014e19: finite, and so is its square
    "fltmax": {"ip": {1: "best", -1: "never"}, "l2n": "never"},  # bf16(FLT_MAX) = +inf: the one term is q[0] * inf
}
PAIRS16 = {
    ("twin", "twin"): {"ip": "hit", "l2n": "never"},
    ("huge", "huge"): {"ip": "best", "l2n": "never"},
    ("fltmax+", "fltmax"): {"ip": "best", "l2n": "never"},     # (fp32: a hit at exactly +FLT_MAX)
    ("fltmax-", "fltmax"): {"ip": "never", "l2n": "never"},    # (fp32: a hit at exactly -FLT_MAX)
}
ROUNDING_CHANGES = ("fltmax",)


def classify16(xq, xb, form):
    """nonfinite_cases.classify on the bf16 scan's arithmetic: products of the rounded operands, norms of the fp32 values"""
    assert form in FORMS16
    return nc.classify(xq, xb, form, mult=(bf16_rne(xq), bf16_rne(xb)))


def _f32_of_int(m):
    """the float32 nearest to the Python integer m (ties to even), +-inf beyond the range: one exact rounding"""
    if m == 0:
        return np.float32(0.0)
    sign, n = (-1.0 if m < 0 else 1.0), abs(m)
    e = n.bit_length() - 24
    if e > 0:
        q, r = divmod(n, 1 << e)
        half = 1 << (e - 1)
        q += 1 if (r > half or (r == half and (q & 1))) else 0
        n = q << e
    if n >= 1 << 128:
        return np.float32(sign * np.inf)
    return np.float32(sign * float(n))  # (at most 24 significant bits: float() and float32() are exact)


def _unit(v):
    """(unit, coefficients): v's finite entries as integer multiples of one unit -- 1, or the one huge magnitude they all share"""
    v = np.asarray(v, np.float64)
    fin = np.where(np.isfinite(v), v, 0.0)
    big = np.abs(fin) >= 2.0 ** 30
    if not big.any():
        unit = 1.0
    else:
        unit = float(np.abs(fin[big]).max())
        if not (np.abs(fin[big]) == unit).all() or (fin[~big] != 0).any():
            raise PreconditionError("a vector that mixes huge and ordinary finite entries: its sums depend on their order")
    c = fin / unit
    if not np.array_equal(c, np.rint(c)):
        raise PreconditionError("a value is no integer")
    return unit, c


def _sig_bits(unit):
    m, _ = np.frexp(unit)
    n = int(m * (1 << 53))
    return (n // (n & -n)).bit_length() if unit != 1.0 else 0


def expected_nonfinite(xb, xq, k, metric, table=None):
    """(D float32 [nq][k], I int64 [nq][k]) the approximate index must return on the data of nonfinite_cases.poison_ints, bit for
    bit: section 2's rule applied to the scores of the rounded operands.  table (a nonfinite_cases.Table): only the pairs of its
    poisoned rows and queries are classified by the term rules, every other pair is an ordinary finite hit"""
    xb, xq = np.ascontiguousarray(xb, np.float32), np.ascontiguousarray(xq, np.float32)
    nq, nb = xq.shape[0], xb.shape[0]
    form = "ip" if metric == IP else "l2n"
    out = np.ones((nq, nb), np.uint8)
    prow = np.arange(nb) if table is None else np.array(sorted(table.rows), np.int64)
    pq = np.arange(nq) if table is None else np.array(sorted(table.queries), np.int64)
    for q0 in range(0, nq, 16):   # (the rules look at every term: a few queries at a time)
        out[q0:q0 + 16, prow] = classify16(xq[q0:q0 + 16], xb[prow], form)
    for q in pq:
        for b0 in range(0, nb, 1024):
            out[q, b0:b0 + 1024] = classify16(xq[q:q + 1], xb[b0:b0 + 1024], form)[0]
    rq, rb = bf16_rne(xq), bf16_rne(xb)
    uq, ub = [_unit(v) for v in rq], [_unit(v) for v in rb]
    cq, cb = np.stack([c for _, c in uq]), np.stack([c for _, c in ub])
    unq, unb = np.array([u for u, _ in uq]), np.array([u for u, _ in ub])
    hit = out == 1
    # one right answer: bits(unit_q unit_b) + bits(sum |c_q c_b|) <= 24 for every finite pair
    bq, bb = np.array([_sig_bits(u) for u in unq]), np.array([_sig_bits(u) for u in unb])
    room = 24 - (bq[:, None] + bb[None, :])
    if (hit & ((np.abs(cq) @ np.abs(cb).T) >= 2.0 ** room)).any():
        raise PreconditionError("a finite dot product whose partial sums are not exact in fp32")
    with np.errstate(all="ignore"):
        dot = (cq @ cb.T) * (unq[:, None] * unb[None, :])   # (an integer of at most 24 bits times a power of two: exact in float64)
    if not np.array_equal(dot[hit].astype(np.float32).astype(np.float64), dot[hit]):
        raise PreconditionError("a finite dot product that is no fp32 number")
    if metric == IP:
        s = np.where(hit, dot, np.where(out == 2, np.inf, np.nan)).astype(np.float32)
        s = -((-s) + np.float32(0.0))   # (a zero inner product comes back as -0.0: `scores`)
        v = -s.astype(np.float64)
    else:
        def norms(x):   # the fp32 chain over the UNROUNDED values: exact for small integers, one rounding for a single huge entry
            with np.errstate(all="ignore"):
                sq = x * x   # float32
                n = sq.astype(np.float64).sum(1)
                one = (x != 0).sum(1) <= 1
                small = n < LIMIT
                if not (one | small | ~np.isfinite(n) | (n > float(FLT_MAX))).all():
                    raise PreconditionError("a norm whose fp32 chain depends on its order")
                return np.where(one | small, n, np.inf).astype(np.float32)
        with np.errstate(all="ignore"):
            nsum = norms(xq)[:, None] + norms(xb)[None, :]   # float32 + float32: one rounding
        s = np.full((nq, nb), np.nan, np.float32)
        small = hit & (nsum.astype(np.float64) + 2.0 * np.abs(dot) < LIMIT)
        s[small] = (nsum.astype(np.float64) - 2.0 * dot)[small].astype(np.float32)
        for q, b in np.argwhere(hit & ~small):   # (pairs with a `twin` on one side: exact integers, rounded once)
            s[q, b] = _f32_of_int(int(nsum[q, b]) - 2 * int(dot[q, b]))
        assert np.isfinite(s[hit]).all(), "a finite pair whose fma overflows: the rules and the arithmetic disagree"
        s = np.maximum(s, np.float32(0.0)) + np.float32(0.0)
        v = s.astype(np.float64)
    adm = out > 0
    v = np.where(adm, v, np.inf)
    # (an admissible value is below +inf, so the inadmissible pairs sort behind all of them; stable: the lower id first)
    order = np.argsort(v, axis=1, kind="stable")[:, :k]
    D = np.full((nq, k), -FLT_MAX if metric == IP else FLT_MAX, np.float32)
    I = np.full((nq, k), -1, np.int64)
    have = np.minimum(adm.sum(1), k)
    for q in range(nq):
        I[q, :have[q]] = order[q, :have[q]]
        D[q, :have[q]] = s[q, order[q, :have[q]]]
    return D, I
