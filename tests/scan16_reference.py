"""The exact 16-bit prefilter's error bound, restated in numpy / float64, and adversarial data for it.

Nothing of the library is used here.  The model: fp16 copies with a power-of-two scale per vector (`copies`), the index-wide
statistics R, X', X (`stats`), the per-query bound B (`bound`), the approximate scores the MFMA pass stands for
(`approx_scores`) and the window of rows the tail re-scores (`window`, `predict`).  The case generators build rows and
queries whose true error |s - s~| comes close to B, or that sit at the edges of the copy format: each returns a `Case`
with the data, k, and what the construction itself says must happen (`expect`), so that the model's prediction can be
checked against the construction before the library is checked against the model.

Shared by tests/test_scan16_reference.py (CPU: the bound is sound, the cases are not vacuous, the predictions are robust)
and tests/test_scan16_bound_gpu.py (the library against the predictions).

How the aligned cases stay exact.  The scaled copies x~ are integers in one binade [2^13, 2^14), multiples of `step`
(8 = one fp16 ulp there at d = 64, 64 at d = 1024), and the scaled query is 2^13 (aligned rows) or 9 * 2^10 (aligned
query): a product has at most 11 + 4 = 15 significant bits and a sum of 1280 of them at most 26 - 3 = 23 (the low three
bits of every x~ are zero), so the fp32 accumulation of the MFMA is exact in any order and the model's s~ is the
hardware's.  A binade-wide choice of 4-bit mantissas, as one might first try, cannot work: the approximate scores would
then be multiples of 2^10 |q_i| while the whole window 2B is about 2 d c |q_i| = 480 |q_i| at d = 64."""
from dataclasses import dataclass, field

import numpy as np

IP = 0
U = 2.0 ** -24
KP_MAX = 2048
FLT_MAX = float(np.finfo(np.float32).max)
# the library rounds R, X', X and B up: a relative 2^-20 and one float step each (s16_up).  B_lib <= B_ref (1 + LIB_REL) + LIB_ABS:
# three such roundings of the statistics and one of B stay below 2^-17 relative; the float step of B itself is at most 2^-149
# when B is below the normal range.
LIB_REL = 2.0 ** -17
LIB_ABS = 2.0 ** -148


def kprime(k):
    return min(KP_MAX, max(2 * k, k + 64))


def pad(d, m):
    return (d + m - 1) // m * m


def tail_term(dp):
    """roundings below the normal range: dp steps of the fp32 chain and the ldexp of the approximate score"""
    return (dp + 1) * 2.0 ** -149


PARENT_TAIL = 2.0 ** -140  # the term before this suite: sound only for dp <= 1024


def copies(x, emin=None):
    """x [n, d] float32 -> (x~ [n, d] float16, e [n] int64): x~ = fp16(x 2^-e), e = ilogb(max|x|) - 13 clamped from below at
    emin (None: no clamp); a zero row or one whose maximum is not finite takes max(0, emin); scaled magnitudes below 2^-14
    are stored as 0."""
    x = np.asarray(x, np.float32)
    a = np.abs(x.astype(np.float64))
    a = np.where(np.isnan(a), 0.0, a)
    mx = a.max(axis=1) if x.shape[1] else np.zeros(len(x))
    ok = (mx > 0) & np.isfinite(mx)
    e = np.zeros(len(x), np.int64)
    e[ok] = np.frexp(mx[ok])[1] - 1 - 13
    if emin is not None:
        e = np.maximum(e, emin)
    with np.errstate(over="ignore", invalid="ignore"):
        h = np.ldexp(x.astype(np.float64), (-e)[:, None].astype(np.int32)).astype(np.float16)
    h = np.where(np.abs(h.astype(np.float64)) >= 2.0 ** -14, h, np.float16(0)).astype(np.float16)
    return h, e


def restored(h, e):
    """x' = 2^e x~ in float64"""
    return np.ldexp(h.astype(np.float64), np.asarray(e)[:, None].astype(np.int32))


def stats(xb):
    """(R, X', X, EMAX) over the rows: float64 maxima of ||x - x'||, ||x'||, ||x||, no round-up margin, and the largest row
    exponent.  Zeros for an empty index."""
    xb = np.asarray(xb, np.float32)
    if len(xb) == 0:
        return 0.0, 0.0, 0.0, -(2 ** 31)
    h, e = copies(xb, -128)
    x = xb.astype(np.float64)
    xp = restored(h, e)
    return (float(np.sqrt(((x - xp) ** 2).sum(1)).max()), float(np.sqrt((xp ** 2).sum(1)).max()),
            float(np.sqrt((x ** 2).sum(1)).max()), int(e.max()))


def g(n, v):
    return n * v / (1.0 - n * v)


def bound(q, st, dp, dp16, tail=None):
    """B_ref(q) = |q| R + |q - q'| X' + g(dp, u) |q| X + g(dp16, 4u) |q'| X' + tail, in float64, for every query of q [nq, d]"""
    R, Xp, X = (v if v <= FLT_MAX else np.inf for v in st[:3])  # (the index keeps them as floats)
    q = np.asarray(q, np.float32)
    h, e = copies(q)
    x = q.astype(np.float64)
    xp = restored(h, e)
    nq, nd, nqp = (np.sqrt((v ** 2).sum(1)) for v in (x, x - xp, xp))
    t = tail_term(dp) if tail is None else tail
    with np.errstate(invalid="ignore", over="ignore"):
        return nq * R + nd * Xp + g(dp, U) * nq * X + g(dp16, 4 * U) * nqp * Xp + t


def approx_scores(xb, xq):
    """[nq, nb] float32: ldexp(<q~, x~> in float64, e_q + e_x), rounded once to fp32"""
    hb, eb = copies(xb, -128)
    hq, eq = copies(xq)
    dot = hq.astype(np.float64) @ hb.astype(np.float64).T
    with np.errstate(over="ignore"):
        return np.ldexp(dot, (eq[:, None] + eb[None, :]).astype(np.int32)).astype(np.float32)


def window(approx, k, kp, B):
    """One query: (t~, ids of the rows whose approximate key is <= t~ + 2B, fits).  Keys are -score, ties to the lower id."""
    key = -approx.astype(np.float64) + 0.0
    order = np.argsort(key, kind="stable")
    nb = len(key)
    if nb < k:
        return np.inf, order, True
    t = key[order[k - 1]]
    lim = t + 2.0 * B
    inside = order[key[order] <= lim]
    fits = nb < kp or key[order[kp - 1]] > lim
    return t, inside, bool(fits)


def predict(xb, xq, k, st=None, bscale=1.0):
    """What a prefiltered search of xq must report: per query its bound, its flag before the scan (a value or the bound not
    finite, e_q + EMAX > 80), the rows inside its window and whether the window fits k'; for the search `fallback` (some
    query flagged or not fitting) and `candidates_max` (the largest window over the queries that do not fall back).
    st: the statistics the index holds (default: those of xb).  bscale: scales B (0.9: a library with too small a bound)."""
    xb = np.asarray(xb, np.float32)
    xq = np.asarray(xq, np.float32)
    d = xb.shape[1]
    st = stats(xb) if st is None else st
    B = bound(xq, st, pad(d, 32), pad(d, 64)) * bscale
    _, eq = copies(xq)
    pre = ~np.isfinite(xq).all(1) | ~np.isfinite(B.astype(np.float32)) | (eq + st[3] > 80)
    ap = approx_scores(xb, xq)
    kp = kprime(k)
    out = []
    for q in range(len(xq)):
        t, inside, fits = window(ap[q], k, kp, B[q])
        out.append(dict(B=float(B[q]), flagged=bool(pre[q]), t=float(t), inside=inside, fits=fits, falls_back=bool(pre[q] or not fits)))
    good = [len(o["inside"]) for o in out if not o["falls_back"]]
    return dict(queries=out, approx=ap, fallback=any(o["falls_back"] for o in out), candidates_max=max(good) if good else 0)


def assert_robust(pred, what=""):
    """No approximate key lies within a relative 2^-10 of a window edge t~ + 2 B_ref, nor between the edge and the furthest
    place the library's may lie (B_ref <= B_lib <= B_ref (1 + 2^-17) + 2^-148: its statistics and B are only ever rounded up):
    the predicted windows are then the library's, whatever its roundings."""
    for o, ap in zip(pred["queries"], pred["approx"]):
        if o["flagged"] or not np.isfinite(o["t"]):
            continue
        edge = o["t"] + 2.0 * o["B"]
        off = -ap.astype(np.float64) + 0.0 - edge
        assert np.abs(off).min() > 2.0 ** -10 * abs(edge), (what, np.abs(off).min(), edge)
        above = off[off > 0]
        assert len(above) == 0 or above.min() > 2.0 ** -10 * abs(edge) + 2.0 * (LIB_REL * o["B"] + LIB_ABS), (what, above.min(), edge)


# ---------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------
@dataclass
class Case:
    name: str
    xb: np.ndarray
    xq: np.ndarray
    k: int
    expect: dict = field(default_factory=dict)   # fallback, candidates_max (None: only the model says), victim / decoy rows, query
    parts: dict = field(default_factory=dict)    # named row ranges (for the add orders)


C_HALF_ULP = 3.75  # just under half an fp16 ulp (8) of the binade [2^13, 2^14)


def _pair_row(sig, orient, H, step, lo):
    """A scaled row of integers in [2^13, 2^14): entry i = sig_i t_i orient (lo + h_i), t = +1, -1, +1, ...; the h_i (multiples
    of step) sit on the entries with t_i orient = +1 and sum to H, so <sig, row> = H for either orientation while the
    row points along (orient = +1) or against (-1) the pattern sig t."""
    d = len(sig)
    t = np.where(np.arange(d) % 2 == 0, 1.0, -1.0)
    units, P = int(H // step), d // 2
    assert units * step == H and H >= 0
    h = np.full(P, units // P, np.float64) + (np.arange(P) < units % P)
    mag = np.full(d, float(lo))
    mag[(t * orient) > 0] += h * step
    assert mag.max() < 2 ** 14 - 8 and mag.min() >= lo
    return sig * t * orient * mag


def _background(rng, n, d, integer=False, amp=30.0):
    """rows far below everything else: a lower binade (norms, copy errors and scores all small)"""
    b = rng.standard_normal((n, d)) * amp
    return np.rint(b) if integer else b


def aligned_rows(d=64, seed=1, nbg=600, k=10, ndecoy=2):
    """First term tight: the victim's copy error is c in every entry, against the query's signs; the decoys' with them."""
    rng = np.random.default_rng(seed)
    step = 8 if d <= 64 else 64
    lo = 2 ** 13 + step
    c = C_HALF_ULP
    sig = rng.choice([-1.0, 1.0], d)
    P = d // 2
    Hd = step * P * 16                       # the best decoy's approximate score (per unit of |q_i|)
    gap = int((2 * d * c - 1) // step) * step  # < 2 d c: the victim's exact score stays above the decoys'
    if gap == 2 * d * c:
        gap -= step
    Hv = Hd - gap
    rows, names = [], {}
    bg = _background(rng, nbg, d)
    solids = [_pair_row(sig, 1, Hd + step * P * (4 + j), step, lo) for j in range(k - 1)]
    victim = _pair_row(sig, 1, Hv, step, lo) + sig * c           # exact = Hv + d c
    decoys = [_pair_row(sig, 1, Hd - step * j, step, lo) - sig * c for j in range(ndecoy)]  # exact = Hd - step j - d c
    scale = 2.0 ** -13
    core = np.array(solids + [victim] + decoys) * scale
    xq = np.array([sig, sig * 2.0 ** -3, sig * 2.0 ** 5], np.float32)
    st = stats(np.vstack([bg * scale, core]).astype(np.float32))
    B = float(bound(xq[:1], st, pad(d, 32), pad(d, 64))[0]) / scale   # in the rows' scaled units
    nfar = 4
    far = [_pair_row(sig, 1, Hd - int(np.ceil(2 * B * (1.0 + 0.1 * (j + 1)) / step)) * step, step, lo) for j in range(nfar)]  # beyond the window
    order = dict(bg=bg * scale, solid=np.array(solids) * scale, far=np.array(far) * scale, special=np.array([victim] + decoys) * scale)
    xb = np.vstack([order[n] for n in ("bg", "solid", "far", "special")]).astype(np.float32)
    pos, parts = 0, {}
    for n in ("bg", "solid", "far", "special"):
        parts[n] = (pos, pos + len(order[n]))
        pos += len(order[n])
    v = parts["special"][0]
    return Case(f"aligned_rows_d{d}", xb, xq, k,
                dict(fallback=False, candidates_max=k - 1 + 1 + ndecoy, victim=v, decoys=list(range(v + 1, v + 1 + ndecoy)), query=0),
                parts)


def aligned_query(d=64, seed=2, nbg=600, k=10, ndecoy=2):
    """Second term tight: every row is its own copy (R = 0); query 0 = q' + eps with eps = c sign(victim's entries): along the
    victim, against the decoys (rows of the opposite orientation)."""
    rng = np.random.default_rng(seed)
    step, lo, c, qm = 8, 2 ** 13 + 8, C_HALF_ULP, 9.0 * 2 ** 10
    sig = rng.choice([-1.0, 1.0], d)
    t = np.where(np.arange(d) % 2 == 0, 1.0, -1.0)
    P = d // 2
    Hd = step * P * 4
    # exact - approx = eps . x' = +- c sum|x'|, approx = qm H: the victim stays ahead while qm (Hd - Hv) < c (sum|v| + sum|decoy|)
    tot = 2 * d * lo + 2 * Hd
    gap = int((c * tot / qm - 1) // step) * step
    Hv = Hd - gap
    assert qm * gap < c * (tot - gap)
    solids = [_pair_row(sig, 1, Hd + step * (8 + 4 * j), step, lo) for j in range(k - 1)]
    victim = _pair_row(sig, 1, Hv, step, lo)
    decoys = [_pair_row(sig, -1, Hd - step * j, step, lo) for j in range(ndecoy)]
    bg = _background(rng, nbg, d, integer=True, amp=8.0)  # (scores within +-300 of 0: the window ends above 500)
    scale = 2.0 ** -13
    qexact = sig * qm * 2.0 ** -13
    q0 = (sig * qm + c * sig * t) * 2.0 ** -13
    xq = np.array([q0, qexact, qexact * 2.0 ** 4], np.float32)
    core = np.array(solids + [victim] + decoys)
    st = stats((np.vstack([bg, core]) * scale).astype(np.float32))
    B = float(bound(xq[:1], st, pad(d, 32), pad(d, 64))[0]) / scale / (qm * 2.0 ** -13)  # in units of H
    far = [_pair_row(sig, 1, Hd - int(np.ceil(2 * B * (1.0 + 0.1 * (j + 1)) / step)) * step, step, lo) for j in range(4)]  # beyond the window
    xb = (np.vstack([bg, np.array(solids), np.array(far), np.array([victim] + decoys)]) * scale).astype(np.float32)
    v = nbg + len(solids) + len(far)
    return Case(f"aligned_query_d{d}", xb, xq, k,
                dict(fallback=False, candidates_max=k - 1 + 1 + ndecoy, victim=v, decoys=list(range(v + 1, v + 1 + ndecoy)), query=0))


def flushed(overflow, d=64, seed=3, k=10, nbg=500):
    """Rows whose column 0 is large and whose other entries are more than 2^27 times smaller: the copy keeps column 0 only.
    The queries are 0 in column 0: the exact score comes from flushed entries alone, the approximate score is exactly 0.
    The background scores far below 0, so the nf flushed rows tie at the top of the approximate order."""
    rng = np.random.default_rng(seed)
    kp = kprime(k)
    nf = kp + 30 if overflow else kp - k - 10
    xq = np.rint(rng.standard_normal((4, d)) * 8.0).astype(np.float32)
    xq[:, 0] = 0.0
    xq[xq.sum(1) == 0, 1] += 1.0
    f = rng.standard_normal((nf, d)) * 2.0 ** -30
    f[:, 0] = rng.uniform(1.0, 1.9, nf)      # scaled by 2^13: [2^13, 2^14); the rest below 2^-14 there
    qbar = xq.sum(0)
    bg = -np.abs(rng.uniform(1.0, 2.0, (nbg, 1))) * qbar[None, :] + rng.standard_normal((nbg, d)) * 0.01
    bg[:, 0] = rng.uniform(-1.0, 1.0, nbg)
    xb = np.vstack([bg, f]).astype(np.float32)
    return Case("flushed_overflow" if overflow else "flushed_fits", xb, xq, k,
                dict(fallback=overflow, candidates_max=None if overflow else nf, flushed=list(range(nbg, nbg + nf))))


TINY_GROUPS = ((-114, 3), (-115, 3), (-116, 40), (-118, 40), (-120, 40), (-127, 40), (-135, 40), (-143, 40), (-149, 40))


def subnormal_query(rng, d, top=7):
    """whole multiples of 2^-149 up to top 2^-149 in magnitude: its own copy (no clamp for queries: e_q down to -162)"""
    q = rng.integers(-top, top + 1, d).astype(np.float64)
    q[0] = top
    return (q * 2.0 ** -149).astype(np.float32)


def tiny(d=64, seed=4, k=10, subq=False):
    """Rows at and below the exponent clamp: three rows with the largest entry at 2^-114 (e = -127), three at 2^-115 (e = -128),
    forty each at 2^-116, 2^-118, 2^-120 (clamped: the copy loses 1, 3, 5 bits and flushes the small entries) and in the
    fp32 subnormals (2^-127, 2^-135; from 2^-143 down every copy entry is 0), and zero rows.  Queries around 2^-20: every
    score is below the normal range, and with only six rows above the clamp each top-10 needs clamped rows.
    subq: the one query is of subnormals instead -- every score and every approximate score is 0, no window fits."""
    rng = np.random.default_rng(seed)
    groups = []
    for p, n in TINY_GROUPS:
        r = rng.standard_normal((n, d))
        groups.append(r / np.abs(r).max(1, keepdims=True) * 2.0 ** p * 1.5)
    groups.append(np.zeros((20, d)))
    xb = np.vstack(groups).astype(np.float32)
    xb = xb[rng.permutation(len(xb))]
    xq = (rng.standard_normal((5, d)) * 2.0 ** -20).astype(np.float32)
    if subq:
        return Case(f"tiny_subnormal_query_d{d}", xb, subnormal_query(rng, d)[None, :], k, dict(fallback=True, candidates_max=0))
    return Case(f"tiny_d{d}", xb, xq, k, dict(fallback=False, candidates_max=None))


def subnormal_query_case(d=64, seed=8, k=10, nb=500):
    """Queries of fp32 subnormals (multiples of 2^-149 up to 1000 of them) against rows around 2^9: the best scores lie
    just below the normal range; the windows fit."""
    rng = np.random.default_rng(seed)
    xb = (rng.standard_normal((nb, d)) * 2.0 ** 9).astype(np.float32)
    xq = np.array([subnormal_query(rng, d, 1000) for _ in range(3)])
    return Case(f"subnormal_query_d{d}", xb, xq, k, dict(fallback=False, candidates_max=None))


def subnormal_scores(d, seed=5, k=4, nb=300, p=-130):
    """Rows +-{1, 2, 3} 2^p and queries +-2^-20, all their own copies (R = 0, q = q'): every product is a multiple of
    2^(p - 20) and every score is subnormal.  Row 0 against query 0 is the worst case of the fp32 chain at p = -130: all d
    products are +2^-150, each step ties and rounds to even, so s = 0 while s~ = d 2^-150.  There the last term of B is
    most of every score and no window fits; at p = -125 and d = 64 the scores are multiples of 16 x 2^-149 against a B of
    little more than 65 x 2^-149, and the windows fit: the search delivers the prefilter's own output."""
    rng = np.random.default_rng(seed)
    sig = rng.choice([-1.0, 1.0], d)
    xb = rng.choice([-3.0, -2.0, -1.0, 1.0, 2.0, 3.0], (nb, d)) * 2.0 ** p
    xb[0] = sig * 2.0 ** p
    xq = rng.choice([-1.0, 1.0], (4, d)) * 2.0 ** -20
    xq[0] = sig * 2.0 ** -20
    fits = p != -130
    return Case(f"subnormal_scores_d{d}" + (f"_p{-p}" if fits else ""), xb.astype(np.float32), xq.astype(np.float32), k,
                dict(fallback=not fits, candidates_max=None if fits else 0, victim=0, query=0))


def gate(over, d=64, seed=6, k=5, nbg=400):
    """A few rows around 2^63 (EMAX = 50); queries around 2^43 (e_q = 30: the sum 80 passes) -- and, with over, two around
    2^44 (81: flagged).  Scores about 2^106 d."""
    rng = np.random.default_rng(seed)
    bg = rng.standard_normal((nbg, d))
    big = rng.uniform(0.5, 1.0, (12, d)) * rng.choice([-1.0, 1.0], (12, d)) * 2.0 ** 64
    big[:, 0] = 2.0 ** 63 * 1.5
    xb = np.vstack([bg, big]).astype(np.float32)
    xq = rng.uniform(0.5, 1.0, (5, d)) * rng.choice([-1.0, 1.0], (5, d)) * 2.0 ** 44
    xq[:, 1] = 2.0 ** 43 * 1.25
    if over:
        xq[1, 1] = 2.0 ** 44
        xq[3, 2] = -2.0 ** 44 * 1.5
    return Case("gate_over" if over else "gate_pass", xb, xq.astype(np.float32), k, dict(fallback=over, candidates_max=None))


def overflowing_norm(d=64, seed=7, k=5):
    """Finite rows whose norm is not: every entry +-3e38.  X = +inf, B is not finite, every query is flagged.  Queries around
    2^-40 keep e_q + EMAX at 61 and the scores finite."""
    rng = np.random.default_rng(seed)
    xb = (rng.choice([-1.0, 1.0], (300, d)) * 3e38).astype(np.float32)
    xq = (rng.standard_normal((3, d)) * 2.0 ** -40).astype(np.float32)
    return Case("overflowing_norm", xb, xq, k, dict(fallback=True, candidates_max=0))


def all_cases():
    """name -> Case: everything the CPU test checks for soundness"""
    cs = [aligned_rows(64), aligned_rows(1024), aligned_query(64), flushed(False), flushed(True), tiny(64), tiny(64, subq=True),
          subnormal_query_case(64), subnormal_scores(64), subnormal_scores(64, p=-125), subnormal_scores(1024), subnormal_scores(1280), gate(False), gate(True), overflowing_norm()]
    return {c.name: c for c in cs}
