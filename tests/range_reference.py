"""Host model of range_search_impl (csrc/range.inc) and exact small-integer problems for it: plain Python and numpy, nothing
of the library under test.  Used by tests/test_range_reference.py (CPU) and tests/test_range_redo_exact_gpu.py.

The model restates plan_range and range_segcap (csrc/plan.h) and the host loop of range_search_impl:

  blocks    queries in blocks of QB = 16384; every block is planned on its own size, the L2 formula on the whole batch
  segcap    entries of a (query, chunk) staging segment: the block's share of 192 MB / 12 bytes, at most a chunk's rows
  runs      copy-out in runs of whole queries of at most out_cap = max(192 MB / 12, ntotal) entries (one query at least);
            a run without results launches nothing
  overflow  a query whose count in some chunk is ABOVE segcap; the overflowing queries of a run are rescanned once, as a
            compact batch: ceil(no / query tile) query tiles over the block's chunks

From the per-(query, chunk) counts it predicts what last_range() and last_scan() report.  The counts come from the kept
(query, row) pairs in the form a range search returns them, (lims, I), or from `keep_all`.

The problems are "family-sorted": d = 8, every entry an integer in [-8, 8].  A row carries a family code in its first six
entries (three of them +-8: 160 codes, squared norm 192) and two entries of noise in [-2, 2]; a query carries a code and
two weights in [-1, 1].  A query and a row of the same family score 192 +- 4 by inner product and at most 18 by squared
L2; different families score at most 128 + 4 and at least 128; the radii (IP 160, L2 32) keep exactly the own family.
Every product, norm and sum is a small integer, exact in fp32 whatever the order of summation and whichever L2 formula:
the expected (lims, D, I) is integer arithmetic (`expected`), vectorised over slabs of queries."""
from collections import namedtuple
from itertools import combinations, product

import numpy as np

IP, L2 = 0, 1
QB = 16384
STAGE_ENTRIES = (192 << 20) // 12
OUT_ENTRIES = (192 << 20) // 12
RADIUS = {IP: np.float32(160.0), L2: np.float32(32.0)}

Plan = namedtuple("Plan", "kernel qt dt nqtiles nchunks tiles_base tiles_rem grid diff lds segcap")


def _cdiv(a, b):
    return (a + b - 1) // b


def plan_range(ntotal, metric, nq, num_cus=256, batch=0):
    """One block of nq queries (plan_range + range_segcap).  batch: the caller's whole batch (0: this block is the batch)."""
    batch_nq = max(nq, batch) if batch > 0 else nq
    diff = metric == L2 and batch_nq < 20
    wide = not diff and nq > 64
    qt, dt = (128, 128) if wide else (32, 256)
    nqtiles = _cdiv(nq, qt)
    tiles = _cdiv(ntotal, dt)
    nchunks = max(1, min(tiles, _cdiv(2 * num_cus, nqtiles)))
    tiles_base, tiles_rem = tiles // nchunks, tiles % nchunks
    lds = max((dt + qt) * 128 * 2, qt * (dt + 1) * 4) + dt * 4 + qt * 4
    kernel = "range_scan_q32_d256_diff" if diff else ("range_scan_q128_d128" if wide else "range_scan_q32_d256")
    chunk_rows = (tiles_base + (1 if tiles_rem else 0)) * dt
    segcap = max(1, min(chunk_rows, STAGE_ENTRIES // (nq * nchunks)))
    return Plan(kernel, qt, dt, nqtiles, nchunks, tiles_base, tiles_rem, nqtiles * nchunks, int(diff), lds, segcap)


def chunk_bounds(pl, ntotal):
    """(c_lo, c_hi) int64 [nchunks]: the rows of every chunk as range_scan_kernel computes them"""
    c = np.arange(pl.nchunks, dtype=np.int64)
    c_lo = (c * pl.tiles_base + np.minimum(c, pl.tiles_rem)) * pl.dt
    c_hi = np.minimum(ntotal, c_lo + (pl.tiles_base + (c < pl.tiles_rem)) * pl.dt)
    return c_lo, c_hi


def counts_from_result(lims, I):
    """counts(plan, ntotal, b0, m) -> int64 [m][nchunks] of the kept pairs (lims, I)"""
    lims = np.asarray(lims).astype(np.int64)
    I = np.asarray(I, np.int64)

    def counts(pl, ntotal, b0, m):
        lo, hi = lims[b0], lims[b0 + m]
        ids = I[lo:hi]
        q = np.repeat(np.arange(m, dtype=np.int64), np.diff(lims[b0:b0 + m + 1]))
        _, c_hi = chunk_bounds(pl, ntotal)
        ch = np.searchsorted(c_hi, ids, side="right")
        return np.bincount(q * pl.nchunks + ch, minlength=m * pl.nchunks).reshape(m, pl.nchunks)

    return counts


def keep_all(pl, ntotal, b0, m):
    """counts of a search that keeps every row"""
    c_lo, c_hi = chunk_bounds(pl, ntotal)
    return np.broadcast_to(c_hi - c_lo, (m, pl.nchunks)).copy()


def predict(ntotal, metric, nq, num_cus, counts, batch=0):
    """What range_search_impl does with these counts.  Returns a dict:
    blocks: [{b0, m, plan, cnt [m][nchunks], runs: [{qa, qb, n, over: block-relative queries rescanned}]}],
    lims [nq + 1], last_range: {query_blocks, redos, redo_queries}, last_scan: {kernel, query_tile, db_tile, nchunks, grid}
    of the last launch (None: nothing was launched)."""
    out = {"blocks": [], "lims": np.zeros(nq + 1, np.int64), "last_range": {"query_blocks": 0, "redos": 0, "redo_queries": 0},
           "last_scan": None}
    if nq == 0 or ntotal == 0:
        return out
    out_cap = max(OUT_ENTRIES, ntotal)
    whole = max(nq, batch) if batch > 0 else nq
    info = out["last_range"]
    for b0 in range(0, nq, QB):
        m = min(QB, nq - b0)
        pl = plan_range(ntotal, metric, m, num_cus, whole)
        info["query_blocks"] += 1
        launch = {"kernel": pl.kernel, "query_tile": pl.qt, "db_tile": pl.dt, "nchunks": pl.nchunks, "grid": pl.grid}
        out["last_scan"] = dict(launch)
        cnt = np.asarray(counts(pl, ntotal, b0, m), np.int64)
        assert cnt.shape == (m, pl.nchunks)
        bl = np.concatenate([[0], np.cumsum(cnt.sum(1))])  # the block's lims, relative to its first result
        out["lims"][b0 + 1:b0 + m + 1] = out["lims"][b0] + bl[1:]
        overq = (cnt > pl.segcap).any(1)
        runs, qa = [], 0
        while qa < m:
            # the longest run of whole queries from qa with at most out_cap entries, one query at least
            qb = min(m, max(qa + 1, int(np.searchsorted(bl, bl[qa] + out_cap, side="right")) - 1))
            n = int(bl[qb] - bl[qa])
            over = (qa + np.flatnonzero(overq[qa:qb])) if n else np.zeros(0, np.int64)
            runs.append({"qa": qa, "qb": qb, "n": n, "over": over})
            if len(over):
                info["redos"] += 1
                info["redo_queries"] += len(over)
                out["last_scan"] = dict(launch, grid=_cdiv(len(over), pl.qt) * pl.nchunks)
            qa = qb
        out["blocks"].append({"b0": b0, "m": m, "plan": pl, "cnt": cnt, "runs": runs})
    return out


# ---- small-integer family data -----------------------------------------------------------------------------------------
def _codes():
    out = []
    for dims in combinations(range(6), 3):
        for signs in product((8, -8), repeat=3):
            v = np.zeros(6, np.int8)
            v[list(dims)] = signs
            out.append(v)
    return np.array(out, np.int8)  # [160][6]


CODES = _codes()
NFAM = len(CODES)


def rows_of(fam, rng):
    """int8 [n][8]: the rows of families fam [n] (-1: a background row, no family: the zero code)"""
    fam = np.asarray(fam, np.int64)
    x = np.zeros((len(fam), 8), np.int8)
    x[fam >= 0, :6] = CODES[fam[fam >= 0]]
    x[:, 6:] = rng.integers(-2, 3, (len(fam), 2))
    return x


def queries_of(fam, rng):
    """int8 [n][8]: queries of families fam [n] (every one a real family)"""
    fam = np.asarray(fam, np.int64)
    assert (fam >= 0).all()
    x = np.zeros((len(fam), 8), np.int8)
    x[:, :6] = CODES[fam]
    x[:, 6:] = rng.integers(-1, 2, (len(fam), 2))
    return x


def f32(x):
    return np.ascontiguousarray(x, np.float32)


def scores_int(xb_i, xq_i, metric):
    """float32 [nq][nb]: the exact scores.  Every operand and every partial sum is an integer far below 2^24, so the float32
    matrix product IS the integer arithmetic, in whatever order BLAS sums (cross_check redoes a sample in int32)."""
    b, q = xb_i.astype(np.float32), xq_i.astype(np.float32)
    ip = q @ b.T
    if metric == IP:
        return ip
    ip *= -2.0
    ip += (q * q).sum(1)[:, None]
    ip += (b * b).sum(1)[None, :]
    return ip


def expected(xb_i, xq_i, radius, metric, slab_pairs=1 << 23):
    """(lims uint64, D float32, I int64) of a range search over integer rows and queries, by integer arithmetic"""
    nb, nq = xb_i.shape[0], xq_i.shape[0]
    r = float(np.float32(radius))
    step = max(1, slab_pairs // max(nb, 1))
    counts = np.zeros(nq, np.int64)
    Ds, Is = [], []
    for q0 in range(0, nq, step):
        s = scores_int(xb_i, xq_i[q0:q0 + step], metric)
        keep = s > r if metric == IP else s < r
        qi, ri = np.nonzero(keep)  # (row-major: query by query, ascending rows)
        counts[q0:q0 + step] = keep.sum(1)
        Ds.append(s[qi, ri])
        Is.append(ri.astype(np.int64))
    lims = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
    cat = lambda parts, dt: np.concatenate(parts).astype(dt, copy=False) if parts else np.zeros(0, dt)
    return lims, cat(Ds, np.float32), cat(Is, np.int64)


def cross_check(oracle, xb_i, xq_i, want, metric, rng, n=4096):
    """On a sample of kept pairs (and of arbitrary pairs) the oracle's chain gives the bits of the integer arithmetic,
    with either L2 formula."""
    lims, D, I = want
    xb, xq = f32(xb_i), f32(xq_i)
    nq, nb = xq.shape[0], xb.shape[0]
    if len(I):
        pick = np.unique(rng.integers(0, len(I), min(n, len(I))))
        qidx = np.searchsorted(lims.astype(np.int64), pick, side="right") - 1
        qi, bi = xq_i[qidx].astype(np.int32), xb_i[I[pick]].astype(np.int32)
        s = (qi * bi).sum(1) if metric == IP else ((qi - bi) ** 2).sum(1)
        assert np.array_equal(s.astype(np.float32).view(np.uint32), D[pick].view(np.uint32))
        for mode in ((0, 2) if metric == L2 else (0,)):
            got = oracle.pair_distances(xb, xq, qidx, I[pick], metric, l2_mode=mode)
            assert np.array_equal(got.view(np.uint32), D[pick].view(np.uint32)), (metric, mode)
    qidx, ridx = rng.integers(0, nq, n), rng.integers(0, nb, n)
    s = (xq_i[qidx].astype(np.int32) * xb_i[ridx].astype(np.int32)).sum(1)
    if metric == L2:
        d = xq_i[qidx].astype(np.int32) - xb_i[ridx].astype(np.int32)
        s = (d * d).sum(1)
    for mode in ((0, 2) if metric == L2 else (0,)):
        got = oracle.pair_distances(xb, xq, qidx, ridx, metric, l2_mode=mode)
        assert np.array_equal(got, s.astype(np.float32)), (metric, mode)


# ---- problems ------------------------------------------------------------------------------------------------------------
class Problem:
    """rows and queries (int8), metric, radius, the roles the generator meant the queries to play and the model's plan of
    the first block; `want` (the integer expectation) and `pred` (the model's prediction) are worked out on first use."""

    def __init__(self, name, xb_i, xq_i, metric, num_cus, roles):
        self.name, self.xb_i, self.xq_i, self.metric, self.num_cus, self.roles = name, xb_i, xq_i, metric, num_cus, roles
        self.radius = RADIUS[metric]
        self.nb, self.nq = xb_i.shape[0], xq_i.shape[0]
        self._want = self._pred = None

    @property
    def want(self):
        if self._want is None:
            self._want = expected(self.xb_i, self.xq_i, self.radius, self.metric)
        return self._want

    @property
    def pred(self):
        if self._pred is None:
            lims, _, I = self.want
            self._pred = predict(self.nb, self.metric, self.nq, self.num_cus, counts_from_result(lims, I))
            assert np.array_equal(self._pred["lims"], lims.astype(np.int64))
        return self._pred


# families of the banded problems; the rest of the 160 are for cold queries and for queries without results
F_BIG, F_EXACT, F_PLUS1, F_TAIL, F_STRADDLE, F_BOTH = 0, 1, 2, 3, 4, 5
COLD_FAMS = np.arange(8, 40)      # a handful of isolated rows each
EMPTY_FAMS = np.arange(40, NFAM)  # no row carries them


def _tile_edge_queries(nq, qt):
    """first and last query of every tile, hence both neighbours of every tile boundary, and the very last query (one
    tile: two more, at a quarter and at three quarters)"""
    qs = {nq // 4, 3 * nq // 4} if nq <= qt else set()
    for t in range(_cdiv(nq, qt)):
        qs.add(t * qt)
        qs.add(min(nq, (t + 1) * qt) - 1)
    return sorted(qs)


def _layout(pl, nb):
    """Bands of consecutive rows by family, placed on the plan's chunks (S = segcap), and the chunks they are meant for.

    Sixteen chunks or more (a single block's plan):
      F_BIG       from the middle of chunk 1 to the middle of chunk 3: chunk 2 whole                       -> overflow in 2
      F_EXACT     exactly S rows at the start of chunk 5                                                   -> none
      F_PLUS1     exactly S + 1 rows inside chunk 7                                                        -> overflow in 7
      F_TAIL      from the start of the last but one chunk to row nb - 1: the ragged last chunk whole      -> overflow
      F_STRADDLE  min(S, 100) rows on either side of the boundary of chunks 9 | 10                         -> none
      F_BOTH      exactly S rows at the start of chunk 12 and S + 40 rows in chunk 13                      -> overflow in 13 only
    Four to fifteen chunks (the first of several blocks: 128 query tiles leave four chunks at 256 CUs), chunks of at least
    S + 160 rows:
      F_PLUS1 S + 1 rows in chunk 0, F_BIG S + 50 rows in chunk 1, F_EXACT S rows at the start of chunk 2, F_STRADDLE 50 rows
      on either side of 2 | 3, F_TAIL from 60 rows into the last chunk to row nb - 1."""
    S = pl.segcap
    c_lo, c_hi = (a.tolist() for a in chunk_bounds(pl, nb))
    last = pl.nchunks - 1
    if pl.nchunks >= 16:
        w = min(S, 100)
        bands = {F_BIG: [((c_lo[1] + c_hi[1]) // 2, (c_lo[3] + c_hi[3]) // 2)], F_EXACT: [(c_lo[5], c_lo[5] + S)],
                 F_PLUS1: [(c_lo[7] + 3, c_lo[7] + 3 + S + 1)], F_TAIL: [(c_lo[last - 1], nb)],
                 F_STRADDLE: [(c_lo[10] - w, c_lo[10] + w)], F_BOTH: [(c_lo[12], c_lo[12] + S), (c_lo[13] + 1, c_lo[13] + 1 + S + 40)]}
        where = {"big": 2, "big_whole": True, "exact": 5, "plus1": 7, "straddle": 10, "both": (12, 13)}
    else:
        assert pl.nchunks >= 4, "the banded problem wants four chunks"
        bands = {F_PLUS1: [(c_lo[0] + 3, c_lo[0] + 3 + S + 1)], F_BIG: [(c_lo[1] + 10, c_lo[1] + 10 + S + 50)],
                 F_EXACT: [(c_lo[2], c_lo[2] + S)], F_STRADDLE: [(c_lo[3] - 50, c_lo[3] + 50)], F_TAIL: [(c_lo[last] + 60 if last == 3 else c_lo[last], nb)]}
        where = {"big": 1, "big_whole": False, "exact": 2, "plus1": 0, "straddle": 3, "both": None}
    spans = sorted(s for v in bands.values() for s in v)
    assert spans[0][0] >= 0 and spans[-1][1] <= nb and all(a[1] <= b[0] for a, b in zip(spans, spans[1:])), "bands overlap"
    return bands, where


def banded(name, nb, nq, metric, num_cus, seed=0, later_hot=()):
    """The partial-overflow problem on the plan of the first block (min(nq, QB) queries): the bands of `_layout`, and
    cold families with 3 to 6 isolated rows each outside the bands.  The first and last query of every query tile and the
    very last query of the block are hot (the overflowing families in turn); queries 1 and qt - 2 are F_EXACT's, 2 and qt - 3
    F_STRADDLE's; six consecutive queries in the middle of the first tile have no results; the others are cold (3 in 10) or
    empty at random.  later_hot: queries of later blocks that get the hot families too (their block has its own plan)."""
    rng = np.random.default_rng(seed)
    m = min(nq, QB)
    pl = plan_range(nb, metric, m, num_cus, nq)
    bands, where = _layout(pl, nb)
    fam = np.full(nb, -1, np.int64)
    for f in COLD_FAMS:
        fam[rng.integers(0, nb, int(rng.integers(3, 7)))] = f
    for f, spans in bands.items():
        for lo, hi in spans:
            fam[lo:hi] = f
    xb_i = rows_of(fam, rng)

    qfam = np.where(rng.random(nq) < 0.3, rng.choice(COLD_FAMS, nq), rng.choice(EMPTY_FAMS, nq))
    hot_fams = [f for f in (F_BIG, F_PLUS1, F_TAIL, F_BOTH) if f in bands]
    roles = {"hot": {}, "exact": [], "straddle": [], "empty_block": None, "later_hot": {}}
    for i, q in enumerate(_tile_edge_queries(m, pl.qt)):
        roles["hot"][q] = qfam[q] = hot_fams[i % len(hot_fams)]
    for role, f, qs in (("exact", F_EXACT, (1, pl.qt - 2)), ("straddle", F_STRADDLE, (2, pl.qt - 3))):
        for q in qs:
            if q < m and q not in roles["hot"] and q not in roles["exact"]:
                qfam[q] = f
                roles[role].append(q)
    e0 = min(m, pl.qt) // 2 - 3
    if e0 > 3:
        qfam[e0:e0 + 6] = EMPTY_FAMS[:6]
        roles["empty_block"] = (e0, e0 + 6)
    for i, q in enumerate(later_hot):
        roles["later_hot"][q] = qfam[q] = hot_fams[i % len(hot_fams)]
    p = Problem(name, xb_i, queries_of(qfam, rng), metric, num_cus, roles)
    p.bands, p.where, p.qfam, p.plan = bands, where, qfam, pl
    return p


def check_banded(p):
    """The conditions that make a banded case mean something: asserted on the CPU at 256 CUs, and by the GPU tests at the
    device's CU count before they search.  Returns the model's prediction."""
    pl, S, w = p.plan, p.plan.segcap, p.where
    pred = p.pred
    blk = pred["blocks"][0]
    cnt, m = blk["cnt"], blk["m"]
    assert blk["plan"] == pl
    c_lo, c_hi = chunk_bounds(pl, p.nb)
    rows = c_hi - c_lo
    last = pl.nchunks - 1
    over = set(int(q) for r in blk["runs"] for q in r["over"])
    hot = p.roles["hot"]
    assert len(hot) >= 3 and min(hot) == 0 and max(hot) == m - 1
    assert set(hot.values()) == {f for f in (F_BIG, F_PLUS1, F_TAIL, F_BOTH) if f in p.bands}
    # the hot queries overflow in the intended chunks and nowhere else
    lims, _, I = p.want
    for q, f in hot.items():
        ov = np.flatnonzero(cnt[q] > S).tolist()
        if f == F_BIG:
            assert ov == [w["big"]], (p.name, q, ov)
            if w["big_whole"]:  # a whole chunk and parts of both neighbours
                assert cnt[q, 2] == rows[2] and 0 < cnt[q, 1] <= S and 0 < cnt[q, 3] <= S
        elif f == F_PLUS1:
            assert ov == [w["plus1"]] and cnt[q, w["plus1"]] == S + 1 == cnt[q].sum(), (p.name, q, ov)
        elif f == F_BOTH:  # a run of exactly segcap in a query that is rescanned for another
            assert ov == [w["both"][1]] and cnt[q, w["both"][0]] == S and cnt[q, w["both"][1]] == S + 40, (p.name, q, ov)
        else:  # the ragged last chunk, up to the last row
            assert last in ov and I[int(lims[q + 1]) - 1] == p.nb - 1 and cnt[q, last] > S, (p.name, q, ov)
    assert (p.nb - c_lo[last]) % pl.dt != 0, "the last chunk is ragged"
    assert over == set(hot), (p.name, sorted(over), sorted(hot))
    # the boundary queries: exactly segcap in one chunk, or two parts below it across a chunk boundary: never rescanned
    assert p.roles["exact"] and p.roles["straddle"]
    for q in p.roles["exact"]:
        assert cnt[q, w["exact"]] == S == cnt[q].sum() and q not in over
    for q in p.roles["straddle"]:
        a, b = cnt[q, w["straddle"] - 1], cnt[q, w["straddle"]]
        assert 0 < a < S and 0 < b < S and cnt[q].sum() == a + b and q not in over
    # the cold ones overflow nowhere; some queries have nothing, consecutive ones among them
    tot = cnt.sum(1)
    cold = np.setdiff1d(np.arange(m), list(hot) + p.roles["exact"] + p.roles["straddle"])
    assert (tot[cold] <= 6).all() and (tot[cold] > 0).any() and (tot[cold] == 0).any()
    if p.roles["empty_block"]:
        e0, e1 = p.roles["empty_block"]
        assert (tot[e0:e1] == 0).all()
    else:
        assert m < 32
    # a partial overflow: a strict, scattered subset is rescanned, in fewer query tiles than the first pass where that has several
    info = pred["last_range"]
    assert 0 < info["redo_queries"] == len(hot) < p.nq and info["redos"] == 1 and len(blk["runs"]) == 1
    assert np.any(np.diff(sorted(hot)) > 1)
    tiles2 = _cdiv(len(hot), pl.qt)
    assert tiles2 < pl.nqtiles or pl.nqtiles == 1
    return pred


def two_runs(name, nb, nq, metric, num_cus, seed=0):
    """The copy-out problem: more than out_cap results in one block of wide tiles, in two runs.

    Family F_EXACT owns the first segcap rows of EVERY chunk, family F_BIG the rows behind them, but for a few isolated rows
    of cold families.  F_EXACT's queries come first -- exactly segcap entries in every chunk: full segments, no overflow, as
    many as out_cap holds (about all the block's: segments and copy-out have the same 192 MB) -- with an empty query among
    them and an empty one (z1) behind them.  Then the first F_BIG query, which no longer fits: the second run starts there,
    with an empty query (z2) right behind it, two more F_BIG queries, and cold and empty queries to the end."""
    rng = np.random.default_rng(seed)
    pl = plan_range(nb, metric, nq, num_cus, nq)
    S = pl.segcap
    c_lo, c_hi = chunk_bounds(pl, nb)
    assert (c_hi - c_lo).min() > S, "every chunk holds more than segcap rows"
    fam = np.full(nb, F_BIG, np.int64)
    for f in COLD_FAMS:
        fam[rng.integers(0, nb, int(rng.integers(3, 7)))] = f
    for lo in c_lo:
        fam[lo:lo + S] = F_EXACT
    per_exact, per_big = S * pl.nchunks, int((fam == F_BIG).sum())
    out_cap = max(OUT_ENTRIES, nb)
    n_exact = (out_cap - per_big) // per_exact + 1  # with this many the first F_BIG query no longer fits
    assert n_exact * per_exact <= out_cap < n_exact * per_exact + per_big
    order = [F_EXACT] * 5 + [int(EMPTY_FAMS[0])] + [F_EXACT] * (n_exact - 5) + [int(EMPTY_FAMS[1]), F_BIG, int(EMPTY_FAMS[2]), F_BIG, F_BIG]
    assert len(order) + 4 <= nq, (len(order), nq)
    qfam = np.where(rng.random(nq) < 0.5, rng.choice(COLD_FAMS, nq), rng.choice(EMPTY_FAMS, nq))
    qfam[:len(order)] = order
    z1 = n_exact + 1
    p = Problem(name, rows_of(fam, rng), queries_of(qfam, rng), metric, num_cus, {"z1": z1, "z2": z1 + 2, "over": [z1 + 1, z1 + 3, z1 + 4]})
    p.qfam, p.plan = qfam, pl
    return p


def check_two_runs(p):
    pl, S = p.plan, p.plan.segcap
    pred = p.pred
    assert len(pred["blocks"]) == 1 and pl.qt == 128
    blk = pred["blocks"][0]
    runs, cnt = blk["runs"], blk["cnt"]
    tot = cnt.sum(1)
    out_cap = max(OUT_ENTRIES, p.nb)
    assert tot.sum() > out_cap and len(runs) == 2
    r1, r2 = runs
    assert 0 < r1["n"] <= out_cap and 0 < r2["n"] <= out_cap and r1["qb"] == r2["qa"] and r2["qb"] == p.nq
    # the first run holds no overflowing query (its segments are full to the last entry), the second does
    assert len(r1["over"]) == 0 and r2["over"].tolist() == p.roles["over"]
    full = tot[:r1["qb"]] > 6
    assert full.sum() > 100 and (cnt[:r1["qb"]][full] == S).all()
    # a query without results on each side of the boundary: the first run's last, and the one behind the second run's first
    # (a run starts with the query that did not fit, never with an empty one)
    assert r1["qb"] - 1 == p.roles["z1"] and r2["qa"] + 1 == p.roles["z2"]
    assert tot[p.roles["z1"]] == 0 and tot[p.roles["z2"]] == 0 and tot[r2["qa"]] > 0
    # block-relative, run-relative and compact positions of the rescanned queries all differ
    assert r2["qa"] > 0 and (r2["over"] - r2["qa"]).tolist() != list(range(len(r2["over"])))
    assert (tot[r2["qa"]:] <= 6).sum() > 2 and (tot[r2["qa"]:] > S).sum() == 3
    assert pred["last_range"] == {"query_blocks": 1, "redos": 1, "redo_queries": 3}
    assert pred["last_scan"]["grid"] == pl.nchunks and pl.nqtiles > 1
    return pred


def two_blocks(name, nb, metric, num_cus, seed=0):
    """QB + 5 uploaded queries: the banded problem on the first block's plan, with the hot families in the 5-query last
    block as well (whose own plan has the narrow tile, other chunks and room for every band)."""
    return banded(name, nb, QB + 5, metric, num_cus, seed, later_hot=(QB, QB + 2, QB + 4))


def check_two_blocks(p):
    pred = check_banded(p)
    assert len(pred["blocks"]) == 2
    b1, b2 = pred["blocks"]
    assert b2["b0"] == QB and b2["m"] == 5
    assert b2["plan"].qt == 32 and b1["plan"].qt == 128 and b2["plan"].nchunks != b1["plan"].nchunks and not b2["plan"].diff
    assert b1["plan"].segcap < b1["plan"].tiles_base * b1["plan"].dt  # segcap below a chunk's rows in the first block
    assert not any(len(r["over"]) for r in b2["runs"]) and (b2["cnt"] <= b2["plan"].segcap).all()
    assert b2["cnt"].sum(1)[[0, 2, 4]].min() > b1["plan"].segcap and b1["cnt"].sum() > 0  # both blocks return results
    assert pred["last_range"]["query_blocks"] == 2 and pred["last_range"]["redos"] == 1
    assert pred["last_scan"] == {"kernel": b2["plan"].kernel, "query_tile": 32, "db_tile": 256, "nchunks": b2["plan"].nchunks, "grid": b2["plan"].grid}
    return pred


def self_rows(n, seed=0):
    """int8 [n][8]: rows of the 160 families in random order, about n / 160 of each: a self-search with the family radii
    returns about n * n / 160 results, spread over every chunk"""
    rng = np.random.default_rng(seed)
    return rows_of(rng.integers(0, NFAM, n), rng)


# The shapes of the GPU cases.  The budgets are fixed (192 MB of segments per block, 192 MB per copy-out run, 16384 queries
# per block), so these are about the smallest that reach each path at 256 CUs (test_range_reference.py pins the plans):
#   wide    300 queries: 3 query tiles x 171 chunks of 640 / 512 rows, segcap 327
#   narrow  64 queries: 2 query tiles x 256 chunks of 1536 / 1280 rows, segcap 1024 (a chunk beats it from 5 tiles of 256 rows on)
#   diff    19 queries: 512 chunks of 2048 / 1792 rows, segcap 1724 (a chunk beats it from 7 tiles on)
#   runs    1100 queries x 240 000 rows: 9 query tiles x 57 chunks, segcap 267, 1088 queries fill out_cap with full segments
#   blocks  16384 + 5 queries x 2041 rows: 128 query tiles x 4 chunks of 512 rows, segcap 256; then 1 tile x 8 chunks of 256
CASES_A = [
    # (name, nb, nq, metric)
    ("wide-ip", 100_000, 300, IP),
    ("wide-l2", 100_000, 300, L2),
    ("narrow-ip", 330_100, 64, IP),
    ("narrow-l2", 330_100, 64, L2),
    ("diff-l2", 918_750, 19, L2),
]
CASE_B = ("runs-ip", 240_000, 1100, IP)
CASES_C = [("blocks-ip", 2041, IP), ("blocks-l2", 2041, L2)]
SELF_ROWS = QB + 37
