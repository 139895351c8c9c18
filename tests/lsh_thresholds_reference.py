"""Exact host restatement of IndexLSH's trained thresholds (FAISS 1.7.2 IndexLSH::train with train_thresholds, restated
from the published source: no FAISS binary exists here, so every "bit for bit" of the threshold tests is against this
file, not against FAISS), for tests/test_lsh_thresholds_gpu.py and tests/fuzz_lsh_thresholds_gpu.py.

ref_projections  x . R[j] in float64, cast to float32 (exact for the exact inputs of lsh_reference), -0.0 -> +0.0
ref_thresholds   per bit the median of the training rows' projections: the sorted column's s[n // 2] for odd n,
                 (s[n // 2 - 1] + s[n // 2]) / 2 computed in float32 for even n
                 -- an ordinary sort, so infinities take part like any other value: a middle that is infinite gives a
                 threshold of +-inf, (finite + inf) / 2 and (FLT_MAX + FLT_MAX) / 2 are +inf in float32, and
                 (-inf + inf) / 2 is a NaN
thresholds_of    the same medians of given float32 projections [n, nbits]
ref_train        what train() must do with the rows: ("ok", thresholds), or ("projection" | "median", bit) -- refused,
                 naming the first bit whose column holds a NaN projection or whose median is a NaN
ref_codes_thr    bit j of a row = (x . R[j] - t[j] >= 0): the float32 projection, the float32 subtraction, the sign test,
                 as FAISS computes it (lsh_reference.faiss_bits).  For finite projections and thresholds that is
                 `x . R[j] >= t[j]`; it is not when both are the same infinity (inf - inf is a NaN: bit 0)
median64, threshold_tol
                 the float64 medians and the derived bound of an fp32 projection's error, for general float inputs"""
import numpy as np

from lsh_reference import ref_codes  # noqa: F401  (re-exported: the tests compare ref_codes_thr(x, R, 0) with it)
from lsh_reference import projections32


def ref_projections(x, R):
    """[n, nbits] float32: float64 products cast to float32, + 0.0 so that a zero is +0.0"""
    return projections32(x, R) + np.float32(0.0)


def thresholds_of(p):
    """float32 projections [n, nbits] -> float32 [nbits]: the per-column medians (-0.0 counts as +0.0)"""
    s = np.sort(np.asarray(p, np.float32) + np.float32(0.0), axis=0)
    n = s.shape[0]
    if n < 1:
        raise ValueError("ref_thresholds: no training rows")
    if n % 2:
        return np.ascontiguousarray(s[n // 2])
    with np.errstate(all="ignore"):  # (float32 throughout: FLT_MAX + FLT_MAX overflows to +inf, -inf + inf is a NaN)
        return ((s[n // 2 - 1] + s[n // 2]) / np.float32(2)).astype(np.float32)


def ref_thresholds(x, R):
    """x [n, d] training rows, R [nbits, d] -> float32 [nbits]"""
    return thresholds_of(ref_projections(x, R))


def ref_train(x, R):
    """-> ("ok", float32 [nbits]) or ("projection", bit) / ("median", bit): the first bit, ascending, that train() must
    refuse -- a NaN among its projections, or a NaN median (+inf and -inf around the middle of an even n)"""
    p = ref_projections(x, R)
    t = ref_thresholds(x, R)  # (a column with a NaN sorts it last: its median is not used)
    for b in range(p.shape[1]):
        if np.isnan(p[:, b]).any():
            return "projection", b
        if np.isnan(t[b]):
            return "median", b
    return "ok", t


def ref_codes_thr(x, R, t, chunk=8192):
    """x [n, d], R [nbits, d], t [nbits] (or a scalar) -> uint8 [n, (nbits + 7) // 8]: bit j = (x . R[j] - t[j] >= 0) in float32"""
    return ref_codes(x, R, t, chunk)


def unpack_bits(codes, nbits):
    """uint8 [n, B] -> bool [n, nbits]"""
    return np.unpackbits(np.asarray(codes, np.uint8), axis=1, bitorder="little")[:, :nbits].astype(bool)


def median64(x, R):
    """float64 [nbits]: the same order statistics over float64 projections"""
    s = np.sort(np.asarray(x, np.float64) @ np.asarray(R, np.float64).T, axis=0)
    n = s.shape[0]
    return s[n // 2] if n % 2 else (s[n // 2 - 1] + s[n // 2]) / 2


def threshold_tol(x, R, t):
    """float64 [nbits]: d * 2^-24 * max ||x|| * max ||a_j|| + ulp(t_j) -- the standard bound of an fp32 dot product of
    length d in any summation order (each of the d products and d - 1 sums rounds once: relative d * u of sum |x_i a_i|
    <= ||x|| ||a||, u = 2^-24), which a median inherits because an order statistic is 1-Lipschitz in the sup norm; the
    ulp covers the rounding of the even-n average"""
    x = np.asarray(x, np.float64)
    R = np.asarray(R, np.float64)
    d = x.shape[1]
    bound = d * 2.0 ** -24 * np.sqrt((x * x).sum(1)).max() * np.sqrt((R * R).sum(1)).max()
    return bound + np.spacing(np.abs(np.asarray(t, np.float32))).astype(np.float64)
