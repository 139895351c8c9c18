"""Plain host replay of the HNSW construction, for tests/test_hnsw_build_exact_gpu.py and tests/test_hnsw_build_reference.py.
NumPy and the CPU oracle only: nothing here loads the library under test.  Written from DESIGN.md section 4.5.

Construction can be pinned exactly by the argument tests/hnsw_reference.py uses for the search: with efConstruction >= the
number of linked nodes the beam never fills, every reachable node is a candidate and is re-scored by the contract's chain.
From there on a batch is deterministic bookkeeping over scores whose bits the oracle produces, so a sequential program
that replays an `add` call batch by batch must arrive at the library's graph: every list, every level, every slot.

MT19937              the standard's 32-bit generator (numpy seeds its own differently)
call_order           the order an add call links its rows in: Fisher-Yates on MT19937, seeded by the call's first row
batch_size           rows of the next batch
level_table          slots below each level (FAISS's set_default_probas: levels until the probability falls below 1e-9)
Scores               the two pair matrices: Vd (the walk's key: orders candidate lists, decides the 127 cut) and Vn (what
                     the selection computes); smaller is better, ties always go to the lower id
select               the pruning heuristic over one group
walk_candidates      the host walkers' candidates restated (greedy descent, then what the level reaches): for cases that run
                     on the host walkers, where no level needs to be connected
Graph / replay_add   the graph and one add call replayed onto it; returns one report per batch
tables               the graph as knn_hnsw_graph_export lays it out
check_invariants     shape properties every replayed graph has

The conditions under which "all linked nodes of level >= l" IS the candidate set are asserted at the start of every batch:
  (a) efConstruction >= linked nodes, and efConstruction <= 1024 (above that the device beam is off);
  (b) on every level l the nodes of level >= l are strongly connected through their level-l lists, so a walk from any
      entry reaches all of them (the device enters level 0 where an approximate bf16 scan says: not restated);
  (c) unless the case is declared `host_upper`: at most 127 linked nodes above level 0 -- the device's upper-level
      candidates come from the bf16 coarse scan, so only their SET is pinned, and the set is complete only while it fits
      one selection group.
"""
import numpy as np

METRIC_INNER_PRODUCT, METRIC_L2 = 0, 1
GROUP = 128  # members of a selection group at the most: the centre and 127 others


class MT19937:
    """std::mt19937"""

    def __init__(self, seed=5489):
        self.mt = [0] * 624
        self.mt[0] = seed & 0xFFFFFFFF
        for i in range(1, 624):
            self.mt[i] = (1812433253 * (self.mt[i - 1] ^ (self.mt[i - 1] >> 30)) + i) & 0xFFFFFFFF
        self.pos = 624

    def __call__(self):
        if self.pos == 624:
            mt = self.mt
            for i in range(624):
                y = (mt[i] & 0x80000000) | (mt[(i + 1) % 624] & 0x7FFFFFFF)
                mt[i] = mt[(i + 397) % 624] ^ (y >> 1) ^ (0x9908B0DF if y & 1 else 0)
            self.pos = 0
        y = self.mt[self.pos]
        self.pos += 1
        y ^= y >> 11
        y ^= (y << 7) & 0x9D2C5680
        y ^= (y << 15) & 0xEFC60000
        return y ^ (y >> 18)


def call_order(n0, n):
    order = list(range(n0, n0 + n))
    rng = MT19937((789 + n0 * 2654435761) & 0xFFFFFFFF)
    for i in range(n - 1, 0, -1):
        j = rng() % (i + 1)
        order[i], order[j] = order[j], order[i]
    return order


def batch_size(done, n, pos, max_batch):
    """done: nodes linked so far; n: rows of the add call; pos: rows of the call already linked"""
    b = max(1, min(max_batch, done // 4))
    return min(b, max(32, n // 32), n - pos)


def level_table(M):
    """cum[l] = slots of the levels below l; level 0 has 2M slots, every other level M"""
    mult = np.float32(1.0 / np.log(float(M)))
    cum, level = [0], 0
    while True:
        proba = np.float32(np.exp(np.float64(np.float32(-level) / mult)) * (1.0 - np.exp(np.float64(np.float32(-1.0) / mult))))
        if proba < 1e-9:
            return np.array(cum, np.int32)
        cum.append(cum[-1] + (2 * M if level == 0 else M))
        level += 1


class Scores:
    def __init__(self, x, metric, oracle):
        x = np.ascontiguousarray(x, np.float32)
        n = x.shape[0]
        a = np.repeat(np.arange(n, dtype=np.int64), n)
        b = np.tile(np.arange(n, dtype=np.int64), n)
        zero = np.float32(0.0)
        if metric == METRIC_INNER_PRODUCT:
            self.Vd = (-oracle.pair_distances(x, x, a, b, metric)).reshape(n, n) + zero
            self.Vn = self.Vd
        else:
            self.Vd = oracle.pair_distances(x, x, a, b, metric, l2_mode=2).reshape(n, n) + zero  # sum of squared differences
            self.Vn = oracle.pair_distances(x, x, a, b, metric).reshape(n, n) + zero  # max(0, fma(-2, dot, nrm_i + nrm_j))
        assert self.Vd.dtype == np.float32 and self.Vn.dtype == np.float32
        assert np.array_equal(self.Vd, self.Vd.T) and np.array_equal(self.Vn, self.Vn.T)


def closer(a, b):
    """the heuristic's comparison: strictly smaller"""
    return a < b


def request_key(r):
    """the order of the reverse requests (node, level, v, from)"""
    return r


def select(Vn, centre, members, cap):
    """members in any order -> (kept ids, their Vn to the centre), at most cap: in order of (Vn(c, centre), id), c is kept
    unless some kept s has Vn(c, s) < Vn(c, centre), or c was kept already, or c is the centre"""
    kept = []
    for c in sorted(members, key=lambda c: (Vn[c, centre], c)):
        if len(kept) == cap:
            break
        if c == centre or c in kept:
            continue
        if any(closer(Vn[c, s], Vn[c, centre]) for s in kept):
            continue
        kept.append(c)
    return kept, [Vn[c, centre] for c in kept]


class Graph:
    def __init__(self, M):
        self.M = M
        self.cum = level_table(M)
        self.levels = []   # top level of every row the index holds
        self.lists = []    # [node][level] -> ids, in list order
        self.linked = []   # [node] linked into the graph
        self.entry, self.max_level = -1, -1

    def cap(self, level):
        return 2 * self.M if level == 0 else self.M

    def nlinked(self):
        return sum(self.linked)

    def nodes_of_level(self, l):
        return [i for i in range(len(self.levels)) if self.linked[i] and self.levels[i] >= l]


def _reaches_all(adj, nodes):
    seen, stack = {nodes[0]}, [nodes[0]]
    while stack:
        for j in adj[stack.pop()]:
            if j not in seen:
                seen.add(j)
                stack.append(j)
    return len(seen) == len(nodes)


def level_strongly_connected(g, l):
    nodes = g.nodes_of_level(l)
    if len(nodes) <= 1:
        return True
    fwd = {i: g.lists[i][l] for i in nodes}
    rev = {i: [] for i in nodes}
    for i in nodes:
        for j in fwd[i]:
            rev[j].append(i)
    return _reaches_all(fwd, nodes) and _reaches_all(rev, nodes)


def reachable_on_level(g, l, start):
    """the nodes a walk on level l reaches from `start` (itself included)"""
    seen, stack = {start}, [start]
    while stack:
        for j in g.lists[stack.pop()][l]:
            if j not in seen:
                seen.add(j)
                stack.append(j)
    return sorted(seen)


def walk_candidates(g, sc, p, lowest):
    """What the HOST walkers find for row p on the levels min(level[p], max_level) .. lowest, with a beam that never fills:
    FAISS's descent, restated.  From the entry point, on every level above the row's own, move to the best of the current
    node and its links (key (Vd, id)) until nothing improves, then step down; on the row's levels the candidates are all
    nodes the level's lists reach from where the walk stands, sorted, and the next level down starts at the best of them.
    Exact scores and a fixed order: nothing here needs the level to be connected."""
    key = lambda c: (sc.Vd[p, c], c)
    top, cur = min(g.levels[p], g.max_level), g.entry
    for l in range(g.max_level, top, -1):
        while True:
            best = min(g.lists[cur][l] + [cur], key=key)
            if best == cur:
                break
            cur = best
    found = {}
    for l in range(top, lowest - 1, -1):
        found[l] = sorted(reachable_on_level(g, l, cur), key=key)
        cur = found[l][0]
    return found


def assert_conditions(g, efc, host_upper, walk=""):
    """walk: "" -- every level's candidates are "all linked nodes of the level": (a), (b) on every level, (c) unless
    host_upper; "upper" -- the levels above 0 come from walk_candidates (KNN355_HNSW_HOST_UPPER=1): (a), (b) on level 0;
    "all" -- so does level 0 (KNN355_HNSW_HOST_BEAM=1): (a) alone"""
    linked = g.nlinked()
    assert linked <= efc <= 1024, f"(a) efConstruction {efc}, {linked} linked nodes"
    for l in range(g.max_level + 1) if not walk else ([0] if walk == "upper" else []):
        assert level_strongly_connected(g, l), f"(b) level {l} is not strongly connected at {linked} linked nodes"
    upper = len(g.nodes_of_level(1))
    assert host_upper or walk or upper <= GROUP - 1, f"(c) {upper} linked nodes above level 0"
    return upper


def link_batch(g, sc, batch, efc, walk=""):
    """links the rows `batch` (ascending) against the frozen graph -> (pruning groups of 65..96 members, of 97..128)"""
    top0 = g.max_level
    requests = []  # (node, level, v, from)
    for p in batch:
        walked = walk_candidates(g, sc, p, 0 if walk == "all" else 1) if walk else {}
        for l in range(min(g.levels[p], top0) + 1):
            if l in walked:
                cands = walked[l][:min(efc, GROUP - 1)]
            else:
                nodes = np.array(g.nodes_of_level(l), np.int64)  # (batch members are not linked yet: never candidates)
                cands = nodes[np.lexsort((nodes, sc.Vd[p, nodes]))][:min(efc, GROUP - 1)].tolist()
            kept, v = select(sc.Vn, p, cands, g.cap(l))
            g.lists[p][l] = kept
            requests += [(c, l, vc, p) for c, vc in zip(kept, v)]
    requests.sort(key=request_key)
    mid = big = 0
    r0 = 0
    while r0 < len(requests):
        node, l = requests[r0][:2]
        r1 = r0
        while r1 < len(requests) and requests[r1][:2] == (node, l):
            r1 += 1
        new = [r[3] for r in requests[r0:r1]]
        cur = g.lists[node][l]
        if len(cur) + len(new) <= g.cap(l):
            g.lists[node][l] = cur + new
        else:
            group = cur + new[:GROUP - 1 - len(cur)]
            mid += 65 <= 1 + len(group) <= 96
            big += 97 <= 1 + len(group) <= 128
            g.lists[node][l] = select(sc.Vn, node, group, g.cap(l))[0]
        r0 = r1
    # the first row of the batch that holds the batch's highest level takes the entry point, if that level is new
    for p in batch:
        if g.levels[p] > g.max_level:
            g.max_level, g.entry = g.levels[p], p
    for p in batch:
        g.linked[p] = True
    return mid, big


def call_batches(done, n0, n, max_batch):
    """the batches (ids ascending inside each) of an add call of rows n0 .. n0 + n onto `done` linked nodes; the very
    first row of an empty graph is a batch of its own (it becomes the entry point and takes no links)"""
    order = call_order(n0, n)
    batches, pos = [], 0
    while pos < n:
        b = 1 if done == 0 else batch_size(done, n, pos, max_batch)
        batches.append(sorted(order[pos:pos + b]))
        pos, done = pos + b, done + b
    return batches


def replay_add(g, sc, n0, levels, efc, max_batch, host_upper=False, walk=""):
    """one add call of rows n0 .. n0 + len(levels) with the given levels -> one report per batch:
    {"rows", "linked", "upper" (linked nodes above level 0 at the batch's start), "groups_65_96", "groups_97_128"}"""
    assert n0 == len(g.levels)
    for lv in levels:
        assert 0 <= lv < len(g.cum) - 1
        g.levels.append(int(lv))
        g.lists.append([[] for _ in range(int(lv) + 1)])
        g.linked.append(False)
    reports = []
    for batch in call_batches(g.nlinked(), n0, len(levels), max_batch):
        if g.entry < 0:
            p, = batch
            g.entry, g.max_level, g.linked[p] = p, g.levels[p], True
            continue
        done = g.nlinked()
        upper = assert_conditions(g, efc, host_upper, walk)
        mid, big = link_batch(g, sc, batch, efc, walk)
        reports.append({"rows": len(batch), "linked": done, "upper": upper, "groups_65_96": mid, "groups_97_128": big})
    return reports


def tables(g):
    """(levels int32 [n], offsets int64 [n + 1], nbrs int32 padded with -1, cum int32)"""
    levels = np.array(g.levels, np.int32)
    offsets = np.zeros(len(levels) + 1, np.int64)
    offsets[1:] = np.cumsum(g.cum[levels + 1])
    nbrs = np.full(int(offsets[-1]), -1, np.int32)
    for i, per_level in enumerate(g.lists):
        for l, ids in enumerate(per_level):
            assert len(ids) <= g.cap(l)
            o = int(offsets[i]) + int(g.cum[l])
            nbrs[o:o + len(ids)] = ids
    return levels, offsets, nbrs, g.cum.copy()


def check_invariants(g):
    """what tests/test_hnsw_gpu.py::test_graph_invariants_and_determinism asks of a built graph, on every list"""
    levels, offsets, nbrs, cum = tables(g)
    n = len(levels)
    assert offsets[-1] == nbrs.size and cum[1] == 2 * g.M and cum[2] - cum[1] == g.M
    assert levels.max() == g.max_level and levels[g.entry] == g.max_level
    assert nbrs.max() < n and nbrs.min() >= -1
    for i in range(n):
        for l in range(levels[i] + 1):
            lst = nbrs[offsets[i] + cum[l]:offsets[i] + cum[l + 1]]
            used = lst[lst >= 0]
            assert (lst[len(used):] == -1).all(), "neighbour lists are packed to the front"
            assert i not in used and len(set(used.tolist())) == len(used)
            assert (levels[used] >= l).all(), "links stay inside their level"


def first_difference(ours, theirs):
    """(node, level, ours, theirs) of the first list that differs between two (levels, offsets, nbrs, cum) graphs, or None"""
    levels, offsets, nbrs, cum = ours
    for i in range(len(levels)):
        for l in range(levels[i] + 1):
            a, b = int(offsets[i]) + int(cum[l]), int(offsets[i]) + int(cum[l + 1])
            if not np.array_equal(nbrs[a:b], theirs[2][a:b]):
                return i, l, nbrs[a:b].tolist(), theirs[2][a:b].tolist()
    return None
