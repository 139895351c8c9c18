"""Non-finite and overflowing inputs for the fp32 flat scan: the generator and the hand-derived outcome of every poisoned
(query, row) pair.  Shared by tests/test_nonfinite_reference.py (CPU: pins the oracle) and tests/test_flat_nonfinite_gpu.py
(GPU: compares the library with the oracle).  Plain numpy, nothing of the library under test.

The rule: a pair whose "smaller is better" value v (inner product: v = -score; squared L2: v = the
distance) is +inf or a NaN never becomes a hit; everything else does.  So under inner product a score of +inf is the BEST
hit, a score of -inf or NaN is none; a score of exactly +-FLT_MAX is an ordinary hit and keeps its row id.  A query with
fewer than k admissible rows is padded with id -1 and -FLT_MAX (inner product) / +FLT_MAX (L2).

Kinds of poisoned rows (columns are fixed, d >= 8; ordinary data is standard normal and never exactly 0):

  nan     NaN at column C_NAN                       every form: never (every chain through it is a NaN)
  pinf    +inf at column C_INF                      IP: other[C_INF] > 0 -> +inf, the best hit (ties: lower id);
                                                        other[C_INF] < 0 -> -inf, never.
                                                    L2 norm formula: nrm = +inf, fma(-2, +-inf, +inf) = NaN or +inf: never.
                                                    L2 differences: (q - inf)^2 = +inf: never.
  pinf0   +inf at column C_ZERO, where EVERY query  0 * inf = NaN in the dot product; the norm is +inf, the difference
          is exactly 0                              +inf: never, every form
  both    +inf at C_B1, -inf at C_B2, where EVERY   (+inf) + (-inf) = NaN in the dot product; norm +inf; difference
          query is positive                         +inf: never, every form
  huge    every entry 3e19                          IP: |dot| <= 3e19 * sum |q| < 1e23: an ordinary hit.
                                                    L2: nrm = +inf (9e38 > FLT_MAX), fma(-2, finite, +inf) = +inf: never;
                                                    against a copy of itself dot = +inf too: NaN, never (norm formula),
                                                    every difference 0: distance exactly 0 (difference form).
  twin    [1.8e19, 0, 0, ...]                       nrm = 3.24e38, finite: an ordinary (far) hit for an ordinary query in
                                                    every form.  Against the twin QUERY (the same vector): IP 3.24e38, an
                                                    ordinary hit; norm formula 3.24e38 + 3.24e38 = +inf: never; difference
                                                    form: exactly 0.  This kind separates the two L2 formulas.
  fltmax  [FLT_MAX, 0, 0, ...]                      against the probe queries [+-1, 0, ...] the dot product has ONE
                                                    non-zero term, exactly +-FLT_MAX: an ordinary hit that must come back
                                                    with its row id (the pad value is the same number with id -1).
                                                    L2: nrm = +inf: never.

Kinds of poisoned queries: nan, pinf (the same vectors as the rows: zero hits under L2; the nan query has zero hits under
inner product too, every slot (-1, -FLT_MAX)), huge (a copy of the huge row: search_self's case), twin, fltmax+ / fltmax-
(the probes [+1, 0, ...] and [-1, 0, ...]; ordinary vectors, they are listed because their outcome against `fltmax` is
exact), and near (an ordinary query whose copy, with one entry poisoned, sits in the database).

`Table.classify` derives the outcome of ANY pair of the generated vectors from its terms alone, by rules that hold for
every summation order (one fp32 fma chain, one rounding per step):
  * a NaN term (NaN entry, 0 * inf, inf - inf), or terms of +inf and -inf together, make the chain a NaN;
  * otherwise an infinite term makes the chain that infinity, provided the finite terms cannot overflow the other way
    (their absolute sum is far below FLT_MAX, or they all have the infinity's sign);
  * finite terms whose absolute values sum to less than FLT_MAX (1 - 1e-3) give a finite chain (every partial sum is
    bounded by that sum);
  * a single non-zero term is the chain's value, rounded once (exactly +-FLT_MAX for the fltmax probes);
  * terms of one sign whose sum exceeds FLT_MAX (1 + 1e-3) overflow to that infinity (the partial sums are monotone);
  * anything else would depend on the order: the generator makes no such pair, and classify raises if it meets one.
`ISSUE_TABLE` states the cells for an ordinary other side literally; test_nonfinite_reference.py checks classify against
it and the oracle against both.
"""
import numpy as np

IP, L2 = 0, 1
FLT_MAX = np.float32(np.finfo(np.float32).max)
C_INF, C_NAN, C_ZERO, C_B1, C_B2 = 1, 2, 3, 4, 5
ROW_KINDS = ("nan", "pinf", "pinf0", "both", "huge", "twin", "fltmax")
QUERY_KINDS = ("nan", "pinf", "huge", "twin", "fltmax+", "fltmax-")
FORMS = ("ip", "l2n", "l2d")  # inner product; squared L2 by the norm formula (>= 20 queries); by differences (< 20)

# outcome of (ordinary query, poisoned row): "never", "hit" (finite score), "best" (inner product +inf);
# pinf under inner product depends on the sign of the query's entry at C_INF
ISSUE_TABLE = {
    "nan": {"ip": "never", "l2n": "never", "l2d": "never"},
    "pinf": {"ip": {1: "best", -1: "never"}, "l2n": "never", "l2d": "never"},
    "pinf0": {"ip": "never", "l2n": "never", "l2d": "never"},
    "both": {"ip": "never", "l2n": "never", "l2d": "never"},
    "huge": {"ip": "hit", "l2n": "never", "l2d": "never"},
    "twin": {"ip": "hit", "l2n": "hit", "l2d": "hit"},      # (an ordinary query; the twin QUERY: hit / never / zero)
    # (an ordinary query q: the one term q[0] * FLT_MAX is finite for |q[0]| < 1 and +-inf beyond -- hit, best or never)
    "fltmax": {"ip": {1: ("hit", "best"), -1: ("hit", "never")}, "l2n": "never", "l2d": "never"},
}
# (twin query, twin row), (huge query, huge row), (fltmax probes, fltmax row); "zero": a hit at distance exactly 0
ISSUE_PAIRS = {
    ("twin", "twin"): {"ip": "hit", "l2n": "never", "l2d": "zero"},
    ("huge", "huge"): {"ip": "best", "l2n": "never", "l2d": "zero"},
    ("fltmax+", "fltmax"): {"ip": "hit", "l2n": "never", "l2d": "never"},
    ("fltmax-", "fltmax"): {"ip": "hit", "l2n": "never", "l2d": "never"},
}


def form_of(metric, nq, norm_l2=False):
    """the arithmetic a batch of nq queries is scored with (FAISS's rule: fewer than 20 queries -> differences)"""
    if metric == IP:
        return "ip"
    return "l2n" if (nq >= 20 or norm_l2) else "l2d"


def make_row(kind, d, base=None):
    """the vector of a poisoned kind; kinds that poison ONE entry start from `base` (a near-duplicate keeps the rest)"""
    if kind in ("huge",):
        return np.full(d, 3e19, np.float32)
    if kind in ("twin", "fltmax", "fltmax+", "fltmax-"):
        v = np.zeros(d, np.float32)
        v[0] = {"twin": np.float32(1.8e19), "fltmax": FLT_MAX, "fltmax+": np.float32(1), "fltmax-": np.float32(-1)}[kind]
        return v
    v = np.array(base, np.float32, copy=True)
    if kind == "nan":
        v[C_NAN] = np.nan
    elif kind == "pinf":
        v[C_INF] = np.inf
    elif kind == "pinf0":
        v[C_ZERO] = np.inf
    elif kind == "both":
        v[C_B1], v[C_B2] = np.inf, -np.inf
    else:
        raise ValueError(kind)
    return v


def _chain_class(T):
    """T float64 [..., d]: the terms of one fma chain per leading index.  Returns (cls int8, val float64): cls 0 finite
    (val: the sum, exact when one term is non-zero), 1 +inf, 2 -inf, 3 NaN; raises on a chain whose class depends on the order"""
    with np.errstate(all="ignore"):
        nan = np.isnan(T).any(-1)
        pinf = (T == np.inf).any(-1)
        ninf = (T == -np.inf).any(-1)
        fin = np.where(np.isfinite(T), T, 0.0)
        sabs = np.abs(fin).sum(-1)
        ssum = fin.sum(-1)
        nnz = (fin != 0).sum(-1)
        one_sign = (fin >= 0).all(-1) | (fin <= 0).all(-1)
    fmax = float(FLT_MAX)
    small = (sabs < fmax * (1 - 1e-3)) | ((nnz <= 1) & (sabs <= fmax))
    over = one_sign & (sabs > fmax * (1 + 1e-3))
    cls = np.full(T.shape[:-1], -1, np.int8)
    cls[small] = 0
    cls[over & (ssum > 0) & ~small] = 1
    cls[over & (ssum < 0) & ~small] = 2
    # (an infinity of one sign beside finite terms of that sign stays that infinity; a NaN stays a NaN whatever else happens)
    with np.errstate(all="ignore"):
        same = (pinf & ~ninf & (fin >= 0).all(-1)) | (ninf & ~pinf & (fin <= 0).all(-1))
    infinite = (pinf ^ ninf) & ~nan
    if (infinite & ~small & ~same).any():
        raise AssertionError("an infinite term beside finite terms that could overflow: the outcome depends on the order")
    cls[pinf] = 1
    cls[ninf] = 2
    cls[nan | (pinf & ninf)] = 3
    if (cls < 0).any():
        raise AssertionError("a chain whose overflow depends on the summation order: the generator is wrong")
    return cls, ssum


def classify(xq, xb, form, mult=None):
    """outcome of every (query, row) pair of float32 xq [nq][d], xb [nb][d]: uint8 [nq][nb] of
    0 never, 1 hit (finite), 2 best (inner product +inf), 3 zero (squared L2 exactly 0).
    mult = (xq', xb'): the dot product's terms are those of these vectors instead (the bf16 scan multiplies rounded copies,
    tests/approx16_reference.py); the norms of form "l2n" stay those of xq and xb"""
    q = np.asarray(xq, np.float32).astype(np.float64)
    b = np.asarray(xb, np.float32).astype(np.float64)
    mq, mb = (q, b) if mult is None else (np.asarray(m, np.float32).astype(np.float64) for m in mult)
    out = np.zeros((q.shape[0], b.shape[0]), np.uint8)
    fmax = float(FLT_MAX)
    with np.errstate(all="ignore"):
        if form == "l2d":
            assert mult is None
            t = q[:, None, :] - b[None, :, :]
            cls, val = _chain_class(t * t)
            out[cls == 0] = 1
            out[(cls == 0) & (val == 0)] = 3
            return out
        cls, ip = _chain_class(mq[:, None, :] * mb[None, :, :])
        if form == "ip":
            out[cls == 0] = 1
            out[cls == 1] = 2
            return out
        qc, qn = _chain_class(q * q)
        bc, bn = _chain_class(b * b)
        assert not (qc == 2).any() and not (bc == 2).any()
        # t = nrm(q) + nrm(b): NaN if either is; +inf if either is or the sum overflows; v = fma(-2, ip, t)
        tn = (qc[:, None] == 3) | (bc[None, :] == 3)
        ts = np.where(qc == 0, qn, 0.0)[:, None] + np.where(bc == 0, bn, 0.0)[None, :]
        tinf = ((qc[:, None] == 1) | (bc[None, :] == 1) | (ts > fmax * (1 + 1e-3))) & ~tn
        tfin = ~tn & ~tinf
        if (tfin & (ts >= fmax * (1 - 1e-3))).any():
            raise AssertionError("a norm sum at the edge of overflow: the generator is wrong")
        # finite t: ip is finite too (|ip|^2 <= nrm nrm), and |t - 2 ip| <= 2 t stays far from FLT_MAX or is judged below
        v = ts - 2.0 * ip
        hit = tfin & (cls == 0)
        if (hit & (np.abs(v) >= fmax * (1 - 1e-3)) & (np.abs(v) <= fmax * (1 + 1e-3))).any() or (tfin & (cls != 0) & (cls != 3)).any():
            raise AssertionError("a distance at the edge of overflow: the generator is wrong")
        out[hit & (v < fmax)] = 1
        return out


class Table:
    """what `poison` did and what must come of it.  rows / queries: {index: kind}; near: {query: its poisoned copy's row};
    outcome(form): classify() over the whole (small) problem; expected_ids(form): per query the admissible row ids."""

    def __init__(self, xb, xq, rows, queries, near):
        self.xb, self.xq, self.rows, self.queries, self.near = xb, xq, dict(rows), dict(queries), dict(near)

    def outcome(self, form):
        return classify(self.xq, self.xb, form)

    def rows_of(self, kind):
        return sorted(r for r, k in self.rows.items() if k.split(":")[-1] == kind)

    def queries_of(self, kind):
        return sorted(q for q, k in self.queries.items() if k == kind)

    def ordinary_queries(self):
        return [q for q in range(self.xq.shape[0]) if self.queries.get(q, "near") == "near"]


def special_rows(nb, tile=256, nchunks=1):
    """row positions that a scan kernel treats specially (clipped to the database, distinct, ascending): rows 0 and nb - 1,
    the rows either side of a tile boundary, the last ragged tile, a row with row % 128 == 0 and one with row % 64 == 0
    (samples of the statistical seed), and the first tile of every chunk (the parked tile whose minimum is published)"""
    ntiles = (nb + tile - 1) // tile
    pos = {0, nb - 1, tile - 1, tile, (ntiles - 1) * tile, (ntiles - 1) * tile + 1, 128, 384, 64, 192}
    for c in range(nchunks):
        first = (c * ntiles // nchunks) * tile
        pos |= {first, first + 3, first + 37}
    return sorted(p for p in pos if 0 <= p < nb)


def poison(rng, nb, nq, d, where, query_kinds=QUERY_KINDS, near=2):
    """(xb float32 [nb][d], xq float32 [nq][d], table).  Standard normal data; row where[i] becomes kind
    ROW_KINDS[i % 7] (`where`: row positions, e.g. special_rows(...); or (row, kind) pairs); the LAST len(query_kinds)
    queries become the poisoned query kinds, in order; the first `near` queries are each copied into the database with one
    entry poisoned (kinds pinf, nan, ... in turn) at rows taken from the middle of `where`'s gaps: such a copy would lead its
    query's list if it were admitted where it must not be.  Every query is exactly 0 at C_ZERO and positive at C_B1, C_B2."""
    assert d >= 8 and nq >= near + len(query_kinds)
    xb = rng.standard_normal((nb, d), dtype=np.float32)
    xq = rng.standard_normal((nq, d), dtype=np.float32)
    xb[xb == 0] = 1
    xq[xq == 0] = 1
    xq[:, C_ZERO] = 0
    xq[:, C_B1:C_B2 + 1] = np.abs(xq[:, C_B1:C_B2 + 1])
    pairs = [(w if isinstance(w, tuple) else (int(w), ROW_KINDS[i % len(ROW_KINDS)])) for i, w in enumerate(where)]
    rows, queries, nears = {}, {}, {}
    for r, kind in pairs:
        assert 0 <= r < nb and r not in rows
        xb[r] = make_row(kind, d, xb[r])
        rows[r] = kind
    # near-duplicates: query i's copy with one poisoned entry.  Kind pinf (the query is NEGATIVE at C_INF: score -inf) and
    # nan: never admissible in any form, yet the row that would lead the list by the rest of its entries
    free = [r for r in range(nb // 2, nb) if r not in rows] + [r for r in range(nb // 2) if r not in rows]
    for i in range(near):
        kind = ("pinf", "nan")[i % 2]
        xq[i, C_INF] = -abs(xq[i, C_INF])  # (no pinf row is a +inf hit of this query, its own copy least of all)
        # (inner product: the huge / twin / fltmax rows score 3e19 * sum(q) and q[0] * 1.8e19 or FLT_MAX -- negative for this
        # query, so that its own copy leads the list and not they)
        xq[i, 0] = -abs(xq[i, 0])
        if xq[i].sum(dtype=np.float64) > -1:
            xq[i, 7] -= np.float32(xq[i].sum(dtype=np.float64) + 1)
        r = free[i * 7 % len(free)]
        while r in rows:
            r = free[(free.index(r) + 1) % len(free)]
        xb[r] = make_row(kind, d, xq[i])
        rows[r] = "near:" + kind
        nears[i] = r
    for j, kind in enumerate(query_kinds):
        qi = nq - len(query_kinds) + j
        xq[qi] = make_row(kind, d, xq[qi])
        queries[qi] = kind
    return xb, xq, Table(xb, xq, rows, queries, nears)


def poison_ints(rng, nb, nq, d, where, query_kinds=QUERY_KINDS, near=2, lim=6):
    """`poison` with every ordinary entry mapped to a non-zero integer of its sign, at most `lim` in magnitude (zeros, the
    poisoned entries and the huge values stay): for the paths whose arithmetic has one right answer only on such data (LSH
    codes against a +-1 rotation, the bf16 scan).  The map is entry by entry, so a near-duplicate stays a copy of its query
    and every sign that `poison` arranged holds; a near-duplicate's query is then made to sum to at most -1 again."""
    xb, xq, t = poison(rng, nb, nq, d, where, query_kinds, near)

    def ints(x):
        with np.errstate(invalid="ignore", over="ignore"):
            small = np.isfinite(x) & (np.abs(x) < 1e6) & (x != 0)
            return np.where(small, np.sign(x) * np.clip(np.ceil(np.abs(x) * 2), 1, lim), x).astype(np.float32)
    xb, xq = ints(xb), ints(xq)
    for q, r in t.near.items():
        s = xq[q].sum(dtype=np.float64)
        if s > -1:
            xq[q, 7] -= np.float32(s + 1)
            xb[r, 7] = xq[q, 7]
    return xb, xq, Table(xb, xq, t.rows, t.queries, t.near)
