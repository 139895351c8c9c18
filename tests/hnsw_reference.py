"""Plain host reference for the HNSW search, for tests/test_hnsw_exact_gpu.py, tests/test_hnsw_gpu.py and
tests/test_hnsw_reference.py.  NumPy and the CPU oracle only: nothing here touches the library under test.

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
