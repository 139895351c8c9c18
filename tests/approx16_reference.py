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

`float_reference` is the bounded comparison for ordinary floats (exponents that differ across a row)."""
import numpy as np

IP, L2 = 0, 1
FLT_MAX = np.float32(3.4028234663852886e38)
LIMIT = 1 << 24


class PreconditionError(AssertionError):
    """the inputs are not ones on which every summation order gives the same fp32 answer"""


def bf16_rne(x):
    """float32 -> the nearest bf16 (ties to the even significand), returned as float32; finite values only"""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    u = (u + np.uint64(0x7FFF) + ((u >> np.uint64(16)) & np.uint64(1))) & np.uint64(0xFFFF0000)
    return u.astype(np.uint32).view(np.float32)


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
