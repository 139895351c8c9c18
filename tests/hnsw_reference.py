"""Plain host reference for the HNSW search, for tests/test_hnsw_exact_gpu.py, tests/test_hnsw_entry_exact_gpu.py,
tests/test_hnsw_gpu.py and tests/test_hnsw_reference.py.  NumPy and the CPU oracle only: nothing here touches the library under test.

A beam search can be checked exactly without restating its expansion order: with ef >= the number of nodes reachable at level
0 from the entry nodes the beam never fills, nothing is pruned, every reachable node is scored, and (keep == ef) every one of
them is re-scored by the contract's chain.  The result is then the exact top k of the REACHABLE SET under the contract's key:
score, then lower id.

level0_tables            the tables knn_hnsw_graph_import takes, for a graph whose nodes all sit at level 0
reachable                level-0 closure of a set of entry nodes; a list is read up to its first -1 only (the fill, as
                         knn_hnsw_graph_import defines it and as FAISS's walk reads a list)
strongly_connected       is every node reachable from every node at level 0?
expected                 the oracle's flat search over the rows x[reach], reach sorted ascending so that "ties go to the lower
                         id" survives the remap; squared L2 in the difference form (l2_mode=2: the HNSW index scores that way
                         at every batch size); short rows padded with id -1 and -FLT_MAX (inner product) / +FLT_MAX (L2)
assert_output_contract   what ANY HNSW result must satisfy, approximate ones included: ids in [0, n) or -1, padding only at
                         the end and with the pad score, no id twice, (score, id) keys strictly ordered, and every returned
                         score carries exactly the contract's bits for its (query, id)

Which level-0 nodes a search ENTERS at (tests/test_hnsw_entry_exact_gpu.py: graphs whose level 0 is disjoint islands, so
that the reachable set names the entries):

tables                   the tables knn_hnsw_graph_import takes, for a graph with levels above 0
scores                   float64 scores of one query against rows, smaller is better (-dot / the sum of squared differences)
descend                  the greedy descent through the levels above 0, as the host walk runs it
coarse_entries           the c best of the nodes above level 0 under (score, lower id); None where the descent applies
entry_reach              the entries -> the sorted union of their level-0 islands
margins                  real-valued rows: every comparison a rule makes, in float64, against the worst-case rounding bound
                         of the arithmetic that makes it
"""
import numpy as np

FLT_MAX = np.float32(np.finfo(np.float32).max)
METRIC_INNER_PRODUCT, METRIC_L2 = 0, 1


def level0_tables(lists, m0):
    """lists: per node, the level-0 neighbour ids as given (-1 = empty slot, holes allowed), at most m0 each
    -> (levels int32 [n] all 0, offsets int64 [n + 1], nbrs int32 [n * m0] padded with -1, cum int32 [0, m0])"""
    n = len(lists)
    nbrs = np.full((n, m0), -1, np.int32)
    for i, l in enumerate(lists):
        assert len(l) <= m0, (i, len(l), m0)
        nbrs[i, :len(l)] = l
    return (np.zeros(n, np.int32), np.arange(n + 1, dtype=np.int64) * m0, nbrs.reshape(-1), np.array([0, m0], np.int32))


def _list0(offsets, nbrs, cum, i):
    l = nbrs[int(offsets[i]):int(offsets[i]) + int(cum[1])]
    holes = np.flatnonzero(l < 0)
    return l[:holes[0]] if holes.size else l


def reachable(levels, offsets, nbrs, cum, entries):
    """sorted int64 array of the nodes a level-0 walk can reach from `entries` (the entries included)"""
    n = len(levels)
    seen = np.zeros(n, bool)
    stack = []
    for e in np.atleast_1d(np.asarray(entries, np.int64)).tolist():
        assert 0 <= e < n
        if not seen[e]:
            seen[e] = True
            stack.append(e)
    while stack:
        i = stack.pop()
        for j in _list0(offsets, nbrs, cum, i).tolist():
            assert 0 <= j < n, (i, j)
            if not seen[j]:
                seen[j] = True
                stack.append(j)
    return np.flatnonzero(seen).astype(np.int64)


def strongly_connected(levels, offsets, nbrs, cum, *_):
    """every node reaches every node at level 0: node 0 reaches all, and all reach node 0 (closure of the reversed graph)"""
    n = len(levels)
    if n <= 1:
        return True
    if reachable(levels, offsets, nbrs, cum, [0]).size != n:
        return False
    rev = [[] for _ in range(n)]
    for i in range(n):
        for j in _list0(offsets, nbrs, cum, i).tolist():
            rev[j].append(i)
    seen = np.zeros(n, bool)
    seen[0] = True
    stack = [0]
    while stack:
        i = stack.pop()
        for j in rev[i]:
            if not seen[j]:
                seen[j] = True
                stack.append(j)
    return bool(seen.all())


def _pad(metric):
    return -FLT_MAX if metric == METRIC_INNER_PRODUCT else FLT_MAX


def expected(x, q, reach, k, metric, oracle):
    """-> (D float32 [nq, k], I int64 [nq, k]): the exact top k of the rows `reach` under (score, lower id)"""
    x = np.ascontiguousarray(x, np.float32)
    q = np.ascontiguousarray(q, np.float32)
    reach = np.sort(np.asarray(reach, np.int64))
    assert reach.size == 0 or (np.diff(reach) > 0).all(), "reach holds an id twice"
    D = np.full((q.shape[0], k), _pad(metric), np.float32)
    I = np.full((q.shape[0], k), -1, np.int64)
    kk = min(k, reach.size)
    if kk:
        Dl, Il = oracle.flat_search(np.ascontiguousarray(x[reach]), q, kk, metric, l2_mode=2)
        assert (Il >= 0).all(), "hnsw_reference: the oracle left a slot unfilled (a score that is not finite?)"
        D[:, :kk] = Dl
        I[:, :kk] = reach[Il]
    return D, I


def contract_scores(x, q, qidx, ids, metric, oracle):
    """the contract's score bits of the pairs (q[qidx[p]], x[ids[p]]), as a search returns them: the flat chain for the inner
    product, the sum of squared differences for squared L2.  (An inner product of exactly zero comes back as -0.0: the key
    is v = -<q, y> + 0.0 and the score -v.)"""
    want = oracle.pair_distances(x, q, qidx, ids, metric, l2_mode=2)
    if metric == METRIC_INNER_PRODUCT:
        want = -((-want) + np.float32(0.0))
    return want


def assert_output_contract(D, I, x, q, metric, n, oracle):
    D = np.asarray(D)
    I = np.asarray(I)
    nq, k = I.shape
    assert D.shape == (nq, k) and D.dtype == np.float32 and I.dtype == np.int64 and q.shape[0] == nq
    valid = I >= 0
    assert ((I == -1) | (valid & (I < n))).all(), "an id outside [0, n) that is not -1"
    # padding: only at the end of a row, with the pad score
    assert (valid[:, 1:] <= valid[:, :-1]).all(), "a -1 in the middle of a row"
    assert (D[~valid].view(np.uint32) == np.array([_pad(metric)], np.float32).view(np.uint32)[0]).all(), "a -1 slot without the pad score"
    # no id twice (the -1 slots are made distinct among themselves)
    s = np.sort(np.where(valid, I, -1 - np.arange(k, dtype=np.int64)[None, :]), axis=1)
    dup = np.flatnonzero((s[:, 1:] == s[:, :-1]).any(axis=1))
    assert dup.size == 0, f"an id twice in the rows of queries {dup[:8].tolist()}"
    # strictly ordered keys: better score first, equal scores by lower id
    assert np.isfinite(D[valid]).all()
    a, b = D[:, :-1], D[:, 1:]
    better = a > b if metric == METRIC_INNER_PRODUCT else a < b
    ordered = better | ((a == b) & (I[:, :-1] < I[:, 1:]))
    both = valid[:, :-1] & valid[:, 1:]
    bad = np.argwhere(both & ~ordered)
    assert bad.size == 0, f"(score, id) keys out of order at (query, slot) {bad[:8].tolist()}"
    # the contract's bits
    qidx = np.broadcast_to(np.arange(nq, dtype=np.int64)[:, None], (nq, k))[valid]
    want = contract_scores(x, q, qidx, I[valid], metric, oracle)
    wrong = np.flatnonzero(D[valid].view(np.uint32) != want.view(np.uint32))
    assert wrong.size == 0, (f"{wrong.size} of {want.size} returned scores do not carry the contract's bits, first (query, id, got, want): "
                             f"{[(int(qidx[p]), int(I[valid][p]), float(D[valid][p]), float(want[p])) for p in wrong[:4]]}")


# ---- the entry rules ------------------------------------------------------------------------------------------------
COARSE_MIN = 64  # nodes above level 0 from which the coarse rule applies


def tables(levels, lists, M):
    """lists[i][l]: the neighbour ids of node i at level l as given (-1 = empty slot, holes allowed), l = 0 .. levels[i]
    -> (levels int32 [n], offsets int64 [n + 1], nbrs int32 [offsets[n]]).  A node of top level L owns cum[L + 1] slots,
    cum = [0, 2M, 3M, 4M, ...]: level 0 at [off, off + 2M), level l >= 1 at [off + cum[l], off + cum[l + 1])."""
    levels = np.asarray(levels, np.int32)
    n = len(levels)
    assert len(lists) == n and (levels >= 0).all()
    cum = [0] + [(l + 2) * M for l in range(int(levels.max(initial=0)) + 1)]
    offsets = np.zeros(n + 1, np.int64)
    offsets[1:] = np.cumsum([cum[int(L) + 1] for L in levels])
    nbrs = np.full(int(offsets[n]), -1, np.int32)
    for i in range(n):
        assert len(lists[i]) == levels[i] + 1, (i, len(lists[i]), int(levels[i]))
        for l, ids in enumerate(lists[i]):
            assert len(ids) <= cum[l + 1] - cum[l], (i, l, len(ids))
            lo = int(offsets[i]) + cum[l]
            nbrs[lo:lo + len(ids)] = ids
    return levels, offsets, nbrs


def _list(offsets, nbrs, M, i, l):
    """node i's level-l list up to its first -1"""
    lo = int(offsets[i]) + (0 if l == 0 else (l + 1) * M)
    ids = nbrs[lo:lo + (2 * M if l == 0 else M)]
    holes = np.flatnonzero(ids < 0)
    return ids[:holes[0]] if holes.size else ids


def scores(x, qrow, ids, metric):
    """float64 [len(ids)]: smaller is better"""
    y = np.asarray(x, np.float64)[np.asarray(ids, np.int64)]
    qrow = np.asarray(qrow, np.float64)
    return -(y @ qrow) if metric == METRIC_INNER_PRODUCT else ((y - qrow[None, :]) ** 2).sum(axis=1)


def descend(levels, offsets, nbrs, M, entry_point, max_level, score, walk=None, key=None, trace=None):
    """The host walk's greedy descent: score the entry; at each level from max_level down to 1 propose the whole list of the
    current node (up to its first -1), move to the best (score, id) among the proposals if it beats the current (score, id)
    -- among equal scores the lower id wins, and an equal-score neighbour of lower id REPLACES the current node -- and
    repeat at the same level; otherwise (an empty list included) go one level down.  -> the node held when level 0 is
    reached; entry_point itself when max_level == 0.  score(ids) -> float64, smaller is better.

    walk / key are for the tests' wrong rules only: the levels walked instead of max_level .. 1, and the order on
    (score, id) instead of the tuple order.  trace: a list that receives (current, winner, [the others compared, the
    current node among them unless it won]) per step."""
    key = key or (lambda s, i: (s, i))
    cur = int(entry_point)
    cur_s = float(score([cur])[0])
    for level in (range(int(max_level), 0, -1) if walk is None else walk):
        while True:
            assert levels[cur] >= level, f"node {cur} (top level {int(levels[cur])}) is walked at level {level}"
            ids = [int(j) for j in _list(offsets, nbrs, M, cur, level)]
            best, best_s = cur, cur_s
            for j, s in zip(ids, score(ids).tolist() if ids else []):
                if key(s, j) < key(best_s, best):
                    best, best_s = j, s
            if trace is not None:
                trace.append((cur, best, sorted(j for j in set(ids + [cur]) if j != best)))
            if best == cur:
                break
            cur, cur_s = best, best_s
    return cur


def ports_of(levels):
    """the nodes above level 0, ascending: the rows of the coarse index, in its order"""
    return np.flatnonzero(np.asarray(levels) >= 1).astype(np.int64)


def coarse_entries(levels, x, qrow, c, metric, key=None, shift=0):
    """-> int64 [min(c, #ports)]: the best of the nodes with levels >= 1 under (score, lower id), scores in float64; None
    with fewer than 64 of them (the descent applies then).  key / shift are for the tests' wrong rules only: the order
    on (score, id), and ports[i + shift] named where ports[i] was chosen."""
    key = key or (lambda s, i: (s, i))
    ports = ports_of(levels)
    if ports.size < COARSE_MIN:
        return None
    s = scores(x, qrow, ports, metric).tolist()
    order = sorted(range(ports.size), key=lambda r: key(s[r], int(ports[r])))[:max(0, min(c, ports.size))]
    return ports[(np.asarray(order, np.int64) + shift) % ports.size]


def entry_reach(offsets, nbrs, M, entries):
    """sorted int64 array: the union of the level-0 islands of the entries"""
    n = len(offsets) - 1
    return reachable(np.zeros(n, np.int32), offsets, nbrs, np.array([0, 2 * M], np.int32), entries)


def rounding_bound(x, qrow, ids, metric, coarse=False, bf16=False):
    """float64 [len(ids)]: the worst-case error of the computed score of (qrow, x[ids]).  One fp32 chain of d terms is off by
    at most d * 2^-24 * sum |t_i|, t_i = q_i y_i (inner product) or (q_i - y_i)^2 (squared L2: the descent's pair scores).
    The coarse scan may score squared L2 as |q|^2 + |y|^2 - 2 <q, y> instead: its terms sum to at most
    sum (|q_i| + |y_i|)^2, which bounds the difference form too, so a coarse score is given that sum.  bf16 copies (both
    operands rounded to 8 bits, 2^-9 each) add 2^-8 times the same sum."""
    y = np.asarray(x, np.float64)[np.asarray(ids, np.int64)]
    a = np.asarray(qrow, np.float64)[None, :]
    if metric == METRIC_INNER_PRODUCT:
        terms = np.abs(y * a).sum(axis=1)
    elif coarse:
        terms = ((np.abs(y) + np.abs(a)) ** 2).sum(axis=1)
    else:
        terms = ((y - a) ** 2).sum(axis=1)
    return (y.shape[1] * 2.0 ** -24 + (2.0 ** -8 if bf16 else 0.0)) * terms


def margins(x, qrow, metric, trace=None, cut=None, bf16=False):
    """-> the smallest gap / bound over the comparisons that decide a rule's choice for one query, gaps in float64.
    trace (from descend): at every step the winner against each other node compared there (the current node included).
    cut: (inside, outside), the coarse scan's chosen ports against the others -- only the worst of the chosen and the best
    of the others matter, and every pair is bounded by them.  The bound of a comparison is the sum of its two scores'
    rounding bounds.  A caller asserts the result above 4; inf when nothing is compared."""
    worst = np.inf
    pairs = []
    if trace is not None:
        pairs += [(w, o, False) for _, w, others in trace for o in others]
    if cut is not None and len(cut[0]) and len(cut[1]):
        inside, outside = (np.asarray(c, np.int64) for c in cut)
        si, so = scores(x, qrow, inside, metric), scores(x, qrow, outside, metric)
        pairs.append((int(inside[np.argmax(si)]), int(outside[np.argmin(so)]), True))
    for w, o, coarse in pairs:
        s = scores(x, qrow, [w, o], metric)
        b = rounding_bound(x, qrow, [w, o], metric, coarse, bf16 and coarse)
        assert s[1] >= s[0], (w, o, s.tolist())
        worst = min(worst, float((s[1] - s[0]) / (b[0] + b[1])) if b.sum() > 0 else (np.inf if s[1] > s[0] else 0.0))
    return worst


