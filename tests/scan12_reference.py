"""The prefilter's 12-bit row copies (knn_flat_set_scan16 mode 2), restated in numpy / float64.

Nothing of the library is used here.  What changes against tests/scan16_reference.py is the ROW copy only: an exponent e
with max|x| 2^-e in [2^10, 2^11) (clamped from below at -128), n = round-to-nearest-even(x 2^-e) clamped to [-2047, 2047],
x' = 2^e n.  Integers of 12 bits are fp16 numbers, so the scan still multiplies exact fp16 values: the query copies, the
formula of B_q, the approximate score and the window are tests/scan16_reference.py's, fed with the statistics R, X', X of
these copies and with k' = min(2048, max(3k, k + 128)).

The adversarial data.  At d = 64 the aligned cases of the fp16 suite sit on this grid as they are: their scaled rows are
integers of [2^13, 2^14) in steps of 8 -- one fp16 ulp there and one step of the 12-bit grid -- with a copy error of 3.75
per entry, just under half a step.  The d = 1024 case (steps of 64) and the edge cases (entries that round to 0, the
exponent clamp, subnormal rows and queries, subnormal scores, the exponent gate, an overflowing norm) are taken over as
data and judged by the 12-bit model; `clamped_max` (a row whose largest entry rounds up to 2048) and the two `rounds_to_zero`
cases (sized by this format's k') are new."""
import math

import numpy as np

import scan16_reference as sr
from scan16_reference import Case, IP, pad  # noqa: F401

NMAX = 2047


def kprime(k):
    return min(sr.KP_MAX, max(3 * k, k + 128))


def copies(x, emin=-128):
    """x [n, d] float32 -> (n [n, d] float64 of integers in [-2047, 2047], e [n] int64)"""
    x = np.asarray(x, np.float32)
    a = np.abs(x.astype(np.float64))
    a = np.where(np.isnan(a), 0.0, a)
    mx = a.max(axis=1) if x.shape[1] else np.zeros(len(x))
    ok = (mx > 0) & np.isfinite(mx)
    e = np.zeros(len(x), np.int64)
    e[ok] = np.frexp(mx[ok])[1] - 1 - 10
    if emin is not None:
        e = np.maximum(e, emin)
    with np.errstate(over="ignore", invalid="ignore"):
        n = np.rint(np.ldexp(x.astype(np.float64), (-e)[:, None].astype(np.int32)))  # (rint: ties to even)
    n = np.clip(np.where(np.isnan(n), 0.0, n), -NMAX, NMAX)
    return n, e


def restored(n, e):
    return np.ldexp(n, np.asarray(e)[:, None].astype(np.int32))


def stats(xb):
    """(R, X', X, EMAX) of the 12-bit copies, as scan16_reference.stats gives them for the fp16 copies"""
    xb = np.asarray(xb, np.float32)
    if len(xb) == 0:
        return 0.0, 0.0, 0.0, -(2 ** 31)
    n, e = copies(xb)
    x = xb.astype(np.float64)
    xp = restored(n, e)
    with np.errstate(over="ignore", invalid="ignore"):
        return (float(np.sqrt(((x - xp) ** 2).sum(1)).max()), float(np.sqrt((xp ** 2).sum(1)).max()),
                float(np.sqrt((x ** 2).sum(1)).max()), int(e.max()))


def bound(q, st, dp, dp16, tail=None):
    """B_q: the unchanged formula (its fourth term: exact products of fp16 values, accumulated in fp32)"""
    return sr.bound(q, st, dp, dp16, tail)


def approx_scores(xb, xq):
    """[nq, nb] float32: ldexp(<q~, n> in float64, e_q + e_x), rounded once to fp32"""
    n, eb = copies(xb)
    hq, eq = sr.copies(xq)
    dot = hq.astype(np.float64) @ n.T
    with np.errstate(over="ignore"):
        return np.ldexp(dot, (eq[:, None] + eb[None, :]).astype(np.int32)).astype(np.float32)


def predict(xb, xq, k, st=None, bscale=1.0):
    """scan16_reference.predict for the 12-bit copies: same keys, same window rule, this format's statistics and k'"""
    xb = np.asarray(xb, np.float32)
    xq = np.asarray(xq, np.float32)
    d = xb.shape[1]
    st = stats(xb) if st is None else st
    B = bound(xq, st, pad(d, 32), pad(d, 64)) * bscale
    _, eq = sr.copies(xq)
    pre = ~np.isfinite(xq).all(1) | ~np.isfinite(B.astype(np.float32)) | (eq + st[3] > 80)
    ap = approx_scores(xb, xq)
    kp = kprime(k)
    out = []
    for q in range(len(xq)):
        t, inside, fits = sr.window(ap[q], k, kp, B[q])
        out.append(dict(B=float(B[q]), flagged=bool(pre[q]), t=float(t), inside=inside, fits=fits, falls_back=bool(pre[q] or not fits)))
    good = [len(o["inside"]) for o in out if not o["falls_back"]]
    return dict(queries=out, approx=ap, fallback=any(o["falls_back"] for o in out), candidates_max=max(good) if good else 0)


assert_robust = sr.assert_robust


# ---------------------------------------------------------------------------------------------------------------------
# cases of this format's own
# ---------------------------------------------------------------------------------------------------------------------
def clamped_max(d=64, seed=21, k=10, nbg=400, nclamp=40):
    """Rows whose largest entry is 2047.5 .. 2047.97 on the row's own grid: it rounds to 2048 and is clamped to 2047 -- a copy
    error of up to 0.97 steps in that entry, twice what rounding alone leaves, and all of it inside R.  The queries weigh
    column 0, where those entries sit."""
    rng = np.random.default_rng(seed)
    rows = np.rint(rng.uniform(-900.0, 900.0, (nclamp, d)))
    rows[:, 0] = 2047.5 + (np.arange(nclamp) % 16) / 32.0  # 2047.5 .. 2047.96875
    scale = 2.0 ** rng.integers(-6, 7, (nclamp, 1)).astype(np.float64)
    bg = rng.standard_normal((nbg, d)) * 3.0
    xb = np.vstack([bg, rows * scale * 2.0 ** -11]).astype(np.float32)
    xq = rng.standard_normal((4, d))
    xq[:, 0] = np.abs(xq[:, 0]) + 2.0
    return Case(f"clamped_max_d{d}", xb, xq.astype(np.float32), k, dict(fallback=None, candidates_max=None, clamped=list(range(nbg, nbg + nclamp))))


def rounds_to_zero(overflow, d=64, seed=3, k=10, nbg=500):
    """scan16_reference.flushed with this format's k': rows of which the copy keeps column 0 only (the other entries are 2^30
    times smaller: they round to 0), queries that are 0 there -- approximate scores exactly 0, one tie over all such rows."""
    rng = np.random.default_rng(seed)
    kp = kprime(k)
    nf = kp + 30 if overflow else kp - k - 10
    xq = np.rint(rng.standard_normal((4, d)) * 8.0).astype(np.float32)
    xq[:, 0] = 0.0
    xq[xq.sum(1) == 0, 1] += 1.0
    f = rng.standard_normal((nf, d)) * 2.0 ** -30
    f[:, 0] = rng.uniform(1.0, 1.9, nf)
    qbar = xq.sum(0)
    bg = -np.abs(rng.uniform(1.0, 2.0, (nbg, 1))) * qbar[None, :] + rng.standard_normal((nbg, d)) * 0.01
    bg[:, 0] = rng.uniform(-1.0, 1.0, nbg)
    xb = np.vstack([bg, f]).astype(np.float32)
    return Case("rounds_to_zero_overflow" if overflow else "rounds_to_zero_fits", xb, xq, k,
                dict(fallback=overflow, candidates_max=None if overflow else nf, flushed=list(range(nbg, nbg + nf))))


def all_cases():
    """name -> Case.  `expect` of the cases taken over is the fp16 construction's; only the aligned cases' and this file's
    own are claims about the 12-bit copies (tests/test_scan12_reference.py says which it checks)."""
    cs = [sr.aligned_rows(64), sr.aligned_rows(1024), sr.aligned_query(64), rounds_to_zero(False), rounds_to_zero(True), clamped_max(),
          sr.tiny(64), sr.tiny(64, subq=True), sr.subnormal_query_case(64), sr.subnormal_scores(64), sr.subnormal_scores(64, p=-125),
          sr.subnormal_scores(1024), sr.subnormal_scores(1280), sr.gate(False), sr.gate(True), sr.overflowing_norm()]
    return {c.name: c for c in cs}


# the cases whose predicted windows no rounding of the library's can change (assert_robust; tests/test_scan12_reference.py
# proves it): only these are compared count for count on the GPU.  Not among them: tiny_d64 (on this grid a key lies within
# 2^-10 of a window's edge) and the cases whose scores all tie at 0 (the windows sit ON their edge; they fall back either way).
ROBUST = ("aligned_rows_d64", "aligned_rows_d1024", "aligned_query_d64", "rounds_to_zero_fits", "rounds_to_zero_overflow", "clamped_max_d64",
          "subnormal_query_d64", "gate_pass", "gate_over", "overflowing_norm")


# ---------------------------------------------------------------------------------------------------------------------
# the window estimate of DESIGN 4.9's table
# ---------------------------------------------------------------------------------------------------------------------
def quantize_fp16_bits(x, bits):
    """fp16 copies (scan16_reference.copies) cut to `bits` significant bits, round to nearest even: (x', as float64)"""
    h, e = sr.copies(x, -128)
    v = h.astype(np.float64)
    m, ex = np.frexp(v)
    v = np.ldexp(np.rint(np.ldexp(m, bits)), ex - bits)
    return sr.restored(v, e)


def fixed_point(x, bits):
    """`bits`-bit fixed point with a power-of-two row scale: max|x| 2^-e in [2^(bits-2), 2^(bits-1)), clamped to +-(2^(bits-1) - 1)"""
    x = np.asarray(x, np.float32).astype(np.float64)
    e = np.frexp(np.abs(x).max(1))[1] - 1 - (bits - 2)
    lim = 2.0 ** (bits - 1) - 1
    n = np.clip(np.rint(np.ldexp(x, (-e)[:, None].astype(np.int32))), -lim, lim)
    return np.ldexp(n, e[:, None].astype(np.int32))


def window_estimate(xp, xb, xq, nb=10_000_000, k=100):
    """(R, mean B_q, expected rows of a window beyond the k-th) for row copies xp of normalised gaussian rows xb, extrapolated
    to nb rows: scores of a normalised query are N(0, 1/d), the k-th best of nb sits at the k / nb quantile, and the window
    reaches 2 B_q below it."""
    x = xb.astype(np.float64)
    d = xb.shape[1]
    st = (float(np.sqrt(((x - xp) ** 2).sum(1)).max()), float(np.sqrt((xp ** 2).sum(1)).max()), float(np.sqrt((x ** 2).sum(1)).max()), 0)
    B = float(sr.bound(xq, st, pad(d, 32), pad(d, 64)).mean())
    sigma = 1.0 / math.sqrt(d)
    tail = lambda t: 0.5 * math.erfc(t / sigma / math.sqrt(2.0))  # noqa: E731
    lo, hi = 0.0, 1.0
    for _ in range(200):  # the k / nb quantile by bisection
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if tail(mid) > k / nb else (lo, mid)
    t = 0.5 * (lo + hi)
    return st[0], B, nb * (tail(t - 2.0 * B) - tail(t))
