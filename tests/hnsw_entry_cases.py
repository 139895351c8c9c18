"""The cases of tests/test_hnsw_entry_exact_gpu.py, shared with tests/test_hnsw_reference.py: the CPU test asserts for every
one of them that its expected result tells the right entry rule from each wrong one, and (real-valued rows) that no
comparison a rule makes is within rounding of a tie.  NumPy and tests/hnsw_reference.py only.

A case is a graph whose level 0 is disjoint islands (rings of `size` nodes at scattered ids, no link leaving one) and whose
ports -- the first `ports_per` nodes of every island -- carry levels above 0 that link ports across islands.  Searched with
efSearch = k = n, the result is the exact top k of the union of the islands of the entry nodes: it names the entries.

Integer rows and queries in [-8, 8], d <= 128: every product, every partial sum and every bf16 copy is exact, so the fp32
chains, the bf16 coarse scan and float64 agree, and equal scores are real ties.  Gaussian rows (d = 100, 1028): the coarse
case plants, per query, five ports at well separated scores (the cut after the fourth), the descents take the rows as drawn;
margins are asserted on the CPU."""
from collections import namedtuple
from functools import lru_cache

import numpy as np

import hnsw_reference as ref

M = 4
METRICS = (0, 1)

# entry: what the test passes to set_entry (None: the default, 4).  tie: "cut" -- two ports with identical rows in different
# islands straddle the coarse cut of query 0; "path" -- an equal-score pair among the proposals of a step of query 0's descent.
# empty1: every third port's level-1 list is empty; empty_top2: the entry point's level-2 list is empty (max_level 3);
# holes: every fourth upper list has a -1 in its third slot, real ids behind it
Spec = namedtuple("Spec", "islands size ports_per max_level d family seed nq entry tie empty1 empty_top2 holes")


def _spec(islands, max_level, seed, entry=None, size=8, ports_per=1, d=32, family="int", nq=6, tie=None, empty1=False,
          empty_top2=False, holes=False):
    return Spec(islands, size, ports_per, max_level, d, family, seed, nq, entry, tie, empty1, empty_top2, holes)


SPECS = {
    # the 64-port boundary, at the default set_entry
    "ports63": _spec(63, 2, 1),
    "ports64": _spec(64, 2, 2),
    # the coarse rule
    "coarse-c1": _spec(96, 2, 3, entry=1),
    "coarse-c4": _spec(96, 2, 3, entry=4),
    "coarse-c64": _spec(96, 2, 3, entry=64),
    "coarse-shared": _spec(32, 2, 4, entry=4, size=24, ports_per=3),
    "coarse-tie": _spec(96, 2, 5, entry=4, tie="cut"),
    "toggle-descent": _spec(96, 2, 3, entry=0),  # (the graph and rows of coarse-c1 / -c4 / -c64 under set_entry(0))
    # the descent rule
    "descent-l1": _spec(96, 1, 32, entry=0, empty1=True, holes=True),
    "descent-l2": _spec(96, 2, 36, entry=0, empty1=True, holes=True),
    "descent-l3": _spec(96, 3, 40, entry=0, empty1=True, holes=True, empty_top2=True),
    "descent-tie": _spec(96, 2, 11, entry=0, tie="path"),
    "descent-counts": _spec(96, 2, 10, entry=0, nq=600, holes=True),
    # real-valued rows
    "gauss-coarse": _spec(96, 2, 14, entry=4, d=100, family="gauss"),
    "gauss-descent": _spec(96, 2, 20, entry=0, d=100, family="gauss", holes=True),
    "gauss-wide": _spec(96, 2, 18, entry=0, size=4, d=1028, family="gauss"),
}
INT_CASES = tuple(k for k, s in SPECS.items() if s.family == "int")
GAUSS_CASES = tuple(k for k, s in SPECS.items() if s.family == "gauss")
PLANT_L2 = (0.3, 0.5, 0.7, 0.9, 1.1)   # planted port = q + s * g: squared L2 about 100 s^2 = 9, 25, 49, 81, 121 (the others: 200)
PLANT_IP = (1.5, 1.3, 1.1, 0.9, 0.7)   # planted port = a * q + 0.3 g: inner product about 100 a (the others: within +-40)

Case = namedtuple("Case", "name spec metric x q levels lists offsets nbrs entry_point max_level ports n")


class _Scorer:
    def __init__(self, x, qrow, metric):
        self.x, self.qrow, self.metric = x, qrow, metric

    def __call__(self, ids):
        return ref.scores(self.x, self.qrow, ids, self.metric)


@lru_cache(maxsize=None)
def case(name, metric):
    sp = SPECS[name]
    rng = np.random.default_rng(1000 + sp.seed)
    n = sp.islands * sp.size
    assert n <= 1000
    members = rng.permutation(n).reshape(sp.islands, sp.size)  # scattered ids: a port's row in the coarse index != its id order
    lists = [None] * n
    for isl in members:
        for j, i in enumerate(isl):
            lists[int(i)] = [[int(isl[(j + 1) % sp.size]), int(isl[(j + 3) % sp.size])]]
    ports = np.sort(members[:, :sp.ports_per].reshape(-1))
    # levels: every port at level >= 1, a third of them at >= 2, a third of those at 3 (as far as max_level goes)
    levels = np.zeros(n, np.int32)
    shuffled = rng.permutation(ports)
    levels[shuffled] = 1
    cnt = shuffled.size
    for l in range(2, sp.max_level + 1):
        cnt = max(cnt // 3, 4)
        levels[shuffled[:cnt]] = l
    entry_point = int(shuffled[int(rng.integers(0, cnt))])
    assert levels[entry_point] == sp.max_level == levels.max()
    for l in range(1, sp.max_level + 1):
        at = np.flatnonzero(levels >= l)
        for pos, p in enumerate(at.tolist()):
            others = at[at != p]
            ids = rng.choice(others, size=min(M, others.size), replace=False).tolist()
            if sp.holes and pos % 4 == 1 and p != entry_point:
                ids = ids[:2] + [-1] + ids[2:3]  # (what lies behind the hole is not part of the list)
            if sp.empty1 and l == 1 and pos % 3 == 0 and p != entry_point:
                ids = []
            if sp.empty_top2 and l == 2 and p == entry_point:
                ids = []
            lists[p].append(ids)
    levels, offsets, nbrs = ref.tables(levels, lists, M)
    if sp.family == "int":
        x = rng.integers(-8, 9, (n, sp.d)).astype(np.float32)
        q = rng.integers(-8, 9, (sp.nq, sp.d)).astype(np.float32)
    else:
        x = rng.standard_normal((n, sp.d), dtype=np.float32)
        q = rng.standard_normal((sp.nq, sp.d), dtype=np.float32)
        if sp.entry:  # the coarse case: per query five planted ports of five islands, the cut after the fourth
            chosen = rng.permutation(ports)[:sp.nq * 5].reshape(sp.nq, 5)
            for j in range(sp.nq):
                g = rng.standard_normal((5, sp.d), dtype=np.float32)
                if metric == ref.METRIC_L2:
                    x[chosen[j]] = q[j][None, :] + np.array(PLANT_L2, np.float32)[:, None] * g
                else:
                    x[chosen[j]] = np.array(PLANT_IP, np.float32)[:, None] * q[j][None, :] + np.float32(0.3) * g
    if sp.tie == "cut":
        s = ref.scores(x, q[0], ports, metric).tolist()
        order = sorted(range(ports.size), key=lambda r: (s[r], int(ports[r])))
        a, b = int(ports[order[sp.entry - 1]]), int(ports[order[sp.entry + 7]])
        x[b] = x[a]  # (two ports, two islands, one row, at ranks c and c + 1 of query 0; the copy may have either id)
    if sp.ports_per > 1:  # query 0's best port and a port of the same island, one coordinate apart: entries that share an island
        s = ref.scores(x, q[0], ports, metric)
        best = int(ports[np.argmin(s)])
        isl = members[np.flatnonzero((members == best).any(axis=1))[0]]
        sibling = int([p for p in isl[:sp.ports_per] if p != best][0])
        x[sibling] = x[best]
        x[sibling, 0] += -1 if x[best, 0] > -8 else 1
    if sp.tie == "path":
        # the first query whose descent moves: a second proposal of that step holds the winner's row (equal scores among the
        # proposals); the next query: a proposal holds the row of the node its descent ends at (an equal score of lower id
        # replaces the current node, one of greater id does not)
        for j in range(sp.nq):
            trace = []
            ref.descend(levels, offsets, nbrs, M, entry_point, sp.max_level, _Scorer(x, q[j], metric), trace=trace)
            moves = [t for t in trace if t[0] != t[1] and len(t[2]) >= 2]
            if moves:
                cur, w, others = moves[0]
                x[[o for o in others if o != cur][0]] = x[w]
                break
        for j in range(j + 1, sp.nq):
            end = ref.descend(levels, offsets, nbrs, M, entry_point, sp.max_level, _Scorer(x, q[j], metric))
            lower = [int(o) for o in ref._list(offsets, nbrs, M, end, 1) if o < end]
            if lower:
                x[lower[0]] = x[end]
                break
    return Case(name, sp, metric, np.ascontiguousarray(x), np.ascontiguousarray(q), levels, lists, offsets, nbrs, entry_point,
                sp.max_level, ports, n)


def rule_of(c):
    """"coarse" or "descent": the rule the library must apply to this case"""
    entry = 4 if c.spec.entry is None else c.spec.entry
    return "coarse" if entry > 0 and c.ports.size >= ref.COARSE_MIN else "descent"


def _descent_entries(c, j, **kw):
    return [ref.descend(c.levels, c.offsets, c.nbrs, M, c.entry_point, c.max_level, _Scorer(c.x, c.q[j], c.metric), **kw)]


def _coarse_entries(c, j, count, **kw):
    if c.ports.size < ref.COARSE_MIN:  # (the 63-port case asks what the coarse rule WOULD pick: a wrong rule there)
        s = ref.scores(c.x, c.q[j], c.ports, c.metric).tolist()
        return c.ports[sorted(range(c.ports.size), key=lambda r: (s[r], int(c.ports[r])))[:count]]
    return ref.coarse_entries(c.levels, c.x, c.q[j], count, c.metric, **kw)


def entries(c, j):
    """the level-0 entry nodes of query j under the rule that applies"""
    if rule_of(c) == "descent":
        return _descent_entries(c, j)
    return ref.coarse_entries(c.levels, c.x, c.q[j], 4 if c.spec.entry is None else c.spec.entry, c.metric)


def reach(c, ents):
    return ref.entry_reach(c.offsets, c.nbrs, M, ents)


def reaches(c, queries=None):
    """per query, the sorted reachable set under the right rule"""
    return [reach(c, entries(c, j)) for j in (range(c.q.shape[0]) if queries is None else queries)]


def wrong_entries(c, j):
    """{wrong rule: its entry nodes for query j}: what a subtly wrong library would enter at"""
    count = 4 if not c.spec.entry else c.spec.entry
    higher = lambda s, i: (s, -i)  # noqa: E731  (the greater id on ties)
    out = {}
    if rule_of(c) == "coarse":
        out["the descent instead"] = _descent_entries(c, j)
        if count > 1:
            out["c - 1 entries"] = _coarse_entries(c, j, count - 1)
        out["c + 1 entries"] = _coarse_entries(c, j, count + 1)
        out["port table shifted by one"] = _coarse_entries(c, j, count, shift=1)
        if c.spec.tie:
            out["the greater id on ties"] = _coarse_entries(c, j, count, key=higher)
    else:
        out["the coarse rule instead"] = _coarse_entries(c, j, count)
        out["entry_point, no descent"] = [c.entry_point]
        out["descent stopped at level 1"] = _descent_entries(c, j, walk=range(c.max_level, 1, -1))
        out["descent skipping the top level"] = _descent_entries(c, j, walk=range(c.max_level - 1, 0, -1))
        if c.spec.tie:
            out["the greater id on ties"] = _descent_entries(c, j, key=higher)
            out["no move on an equal score"] = _descent_entries(c, j, key=lambda s, i: (s, 0))
    return out


def grouped_expected(c, queries, oracle):
    """(D, I) of `queries` (rows of c.q) at k = n: one oracle search per distinct entry set, not per query"""
    D = np.empty((len(queries), c.n), np.float32)
    I = np.empty((len(queries), c.n), np.int64)
    groups = {}
    for pos, j in enumerate(queries):
        groups.setdefault(tuple(int(e) for e in np.sort(entries(c, j))), []).append(pos)
    for ents, rows in groups.items():
        qs = np.ascontiguousarray(c.q[[queries[p] for p in rows]])
        D[rows], I[rows] = ref.expected(c.x, qs, reach(c, list(ents)), c.n, c.metric, oracle)
    return D, I
