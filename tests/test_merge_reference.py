"""CPU: the host reference of the shard key exchange (tests/merge_reference.py) against a hand-written example and against the
oracle's flat search, the generator of synthetic exchanges, and the comparison the GPU tests use against the ways a merge
kernel goes wrong.  The GPU side is tests/test_merge_keys_exact_gpu.py."""
import numpy as np
import pytest

import merge_reference as mr
from merge_reference import FLT_MAX, IP, KEY_PAD, L2


def _w(v):
    return int(mr.f2ord(np.float32(v)).reshape(-1)[0])


def test_f2ord_orders_floats_and_round_trips():
    v = np.array([-FLT_MAX, -2.5, -1e-45, -0.0, 0.0, 1e-45, 1.0, FLT_MAX], np.float32)
    w = mr.f2ord(v)
    assert w.dtype == np.uint64 and (w < 1 << 32).all()
    assert (w[1:] > w[:-1]).all(), "-0.0 sorts in front of +0.0: the scan packs v + 0 for that reason"
    assert np.array_equal(mr.ord2f(w).view(np.uint32), v.view(np.uint32))
    assert _w(-0.0) == 0x7FFFFFFF and _w(0.0) == 0x80000000 and _w(1.0) == 0xBF800000 and _w(-FLT_MAX) == 0x00800000


def test_pack_keys_by_hand():
    D = np.array([[0.5, 0.0, -0.0, 0.0]], np.float32)
    I = np.array([[3, 0, 7, -1]], np.int64)
    got = mr.pack_keys(D, I, L2, 1000)
    assert got.dtype == np.uint64
    assert got.tolist() == [[(0xBF000000 << 32) | 1003, (0x80000000 << 32) | 1000, (0x80000000 << 32) | 1007, 0xFFFFFFFFFFFFFFFF]]
    # inner product packs -D, and -(+0.0) = -0.0 becomes +0.0 as well
    got = mr.pack_keys(D, I, IP, 0xFFFFFFF8)
    assert got.tolist() == [[(0x40FFFFFF << 32) | 0xFFFFFFFB, (0x80000000 << 32) | 0xFFFFFFF8, (0x80000000 << 32) | 0xFFFFFFFF,
                             0xFFFFFFFFFFFFFFFF]]
    with pytest.raises(AssertionError):
        mr.pack_keys(D, I, IP, 0xFFFFFFF9)  # row 7 would be id 2^32


def test_merge_by_hand():
    """3 lists x 2 queries + an all-padding query, k = 4.  Query 0: a tie on the score word across lists 0 and 2 (the lower id
    first).  Query 1: short -- three real keys in all.  Query 2: nothing."""
    P = int(KEY_PAD)

    def key(v, i):
        return (_w(v) << 32) | i

    keys = np.array([
        [[key(1.0, 10), key(2.0, 11), key(5.0, 12), key(9.0, 13)], [key(-1.0, 14), P, P, P], [P, P, P, P]],
        [[key(0.5, 100), key(3.0, 101), key(3.5, 102), key(4.0, 103)], [P, P, P, P], [P, P, P, P]],
        [[key(2.0, 5), key(2.5, 201), key(6.0, 202), key(7.0, 203)], [key(-3.0, 204), key(0.0, 205), P, P], [P, P, P, P]],
    ], dtype=np.uint64)
    mr.check_well_formed(keys)
    D, I = mr.merge(keys, 4, L2)
    assert D.dtype == np.float32 and I.dtype == np.int64
    assert I.tolist() == [[100, 10, 5, 11], [204, 14, 205, -1], [-1, -1, -1, -1]]
    assert D.tolist() == [[0.5, 1.0, 2.0, 2.0], [-3.0, -1.0, 0.0, FLT_MAX], [FLT_MAX] * 4]
    D, I = mr.merge(keys, 4, IP)  # the same keys read as inner products: the score is the negated word's float
    assert I.tolist() == [[100, 10, 5, 11], [204, 14, 205, -1], [-1, -1, -1, -1]]
    assert D.view(np.uint32).tolist() == np.array([[-0.5, -1.0, -2.0, -2.0], [3.0, 1.0, -0.0, -FLT_MAX], [-FLT_MAX] * 4], np.float32).view(np.uint32).tolist()
    # k smaller than the lists, and k larger than everything there is
    assert mr.merge(keys, 2, L2)[1].tolist() == [[100, 10], [204, 14], [-1, -1]]
    assert mr.merge(keys[:1, :, :2], 4, L2)[1].tolist() == [[10, 11, -1, -1], [14, -1, -1, -1], [-1, -1, -1, -1]]


@pytest.mark.parametrize("metric", [IP, L2])
@pytest.mark.parametrize("nq", [7, 23])  # (both squared-L2 formulas: fewer than 20 queries, and not)
def test_merge_of_packed_shard_results_is_the_flat_search(oracle, metric, nq):
    rng = np.random.default_rng(41)
    nb, d, k = 300, 24, 40
    xb = rng.standard_normal((nb, d), dtype=np.float32)
    xb[275:280] = xb[3:8]      # duplicates across the shards: the lower global id first
    xb[100] = 0.0
    xq = rng.standard_normal((nq, d), dtype=np.float32)
    xq[1] = xb[4]
    xq[2] = 0.0                # every inner product is 0.0: ids alone order the result
    bounds = [(0, 150), (150, 270), (270, 300)]  # the last shard holds fewer than k rows: its lists end in padding
    parts = []
    for lo, hi in bounds:
        D, I = oracle.flat_search(xb[lo:hi], xq, k, metric)
        parts.append(mr.pack_keys(D, I, metric, lo))
    keys = mr.check_well_formed(np.stack(parts))
    assert (keys[2, :, 30:] == KEY_PAD).all() and (keys[2, :, :30] != KEY_PAD).all()
    mr.assert_same(mr.merge(keys, k, metric), oracle.flat_search(xb, xq, k, metric), "merge of three shards")
    assert mr.merge(keys, k, metric)[1][1, :2].tolist() == [4, 276]


SHAPES = [(1, 3, 1), (3, 4, 5), (4, 9, 64), (8, 5, 65), (2, 3, 1000), (17, 2, 100)]


@pytest.mark.parametrize("nlists,nq,k", SHAPES)
@pytest.mark.parametrize("pattern", mr.PATTERNS)
def test_generated_exchanges_are_well_formed(pattern, nlists, nq, k):
    keys = mr.exchange(pattern, nlists, nq, k)
    assert keys.shape == (nlists, nq, k) and keys.dtype == np.uint64
    mr.check_well_formed(keys)
    assert (keys != KEY_PAD).all()
    assert np.array_equal(keys, mr.exchange(pattern, nlists, nq, k)), "the generator is deterministic"
    words, ids = keys >> np.uint64(32), (keys & np.uint64(0xFFFFFFFF)).astype(np.int64)
    assert np.isfinite(mr.ord2f(words)).all() and (words != 0x7FFFFFFF).all(), "words of finite floats after + 0 only"
    span = (1 << 32) // nlists
    for l in range(nlists):  # a list's ids come from its own range
        assert (ids[l] >= l * span).all() and ((ids[l] < (l + 1) * span) | (l == nlists - 1)).all()
    top = mr.merge_keys(keys, k)
    if pattern == "one_word":
        assert (words == words[:1, :, :1]).all()
    if pattern == "two_clusters":
        near = np.minimum(np.abs(words.astype(np.int64) - _w(-1e30)), np.abs(words.astype(np.int64) - _w(1e30)))
        assert (near <= 3).all()
    if pattern == "extremes":
        lo, hi = (_w(-FLT_MAX) << 32) | 0, (_w(FLT_MAX) << 32) | mr.ID_LAST
        has_lo, has_hi = (keys == np.uint64(lo)).any(axis=(0, 2)), (keys == np.uint64(hi)).any(axis=(0, 2))
        assert (has_lo & has_hi).all() if nlists * k > 1 else ((has_lo ^ has_hi).all() and has_lo.any() and has_hi.any())
    if pattern == "one_list_wins":
        assert np.array_equal(top, keys[nlists - 1])
    if pattern == "round_robin":
        every = np.sort(np.transpose(keys, (1, 0, 2)).reshape(nq, nlists * k), axis=1)
        assert np.array_equal(every.reshape(nq, k, nlists), np.transpose(keys, (1, 2, 0))), "rank r sits in list r % nlists"


@pytest.mark.parametrize("nlists,nq,k", SHAPES)
def test_short_exchanges_hold_exactly_the_real_keys_asked_for(nlists, nq, k):
    for real in mr.short_reals(k):
        keys = mr.exchange("short", nlists, nq, k, real=real)
        mr.check_well_formed(keys)
        want = min(real, nlists * k)
        assert ((keys != KEY_PAD).sum(axis=(0, 2)) == want).all()
        per_list = (keys != KEY_PAD).sum(axis=2)  # [nlists][nq]
        if nlists >= 3 and want <= (nlists - nlists // 3) * k:
            assert (per_list == 0).any(axis=0).all(), "some lists are all padding"
        if nlists >= 3 and 3 <= want <= k:
            assert (per_list.max(axis=0) > per_list.min(axis=0) + 1).all(), "uneven"
    # one count per query
    reals = np.arange(nq) % 3
    keys = mr.exchange("short", nlists, nq, k, real=reals)
    assert np.array_equal((keys != KEY_PAD).sum(axis=(0, 2)), np.minimum(reals, nlists * k))


def test_status_rows():
    keys = mr.exchange("gaussian", 4, 6, 8)
    st = mr.with_status_rows(keys, failed=(1, 3))
    assert st.shape == (4, 7, 8)
    assert np.array_equal(st[0, :6], keys[0]) and np.array_equal(st[2, :6], keys[2])
    assert (st[1, :6] == KEY_PAD).all() and (st[3, :6] == KEY_PAD).all()
    assert st[:, 6].tolist() == [[int(KEY_PAD)] * 8, [1] + [int(KEY_PAD)] * 7, [int(KEY_PAD)] * 8, [3] + [int(KEY_PAD)] * 7]
    D, I = mr.merge(st, 8, IP)
    assert I[6].tolist() == [1, 3, -1, -1, -1, -1, -1, -1]
    mr.assert_same((D[:6], I[:6]), mr.merge(keys[[0, 2]], 8, IP))


@pytest.mark.parametrize("metric", [IP, L2])
def test_the_comparison_rejects_what_a_merge_kernel_gets_wrong(metric):
    nlists, nq, k = 3, 5, 8
    keys = mr.exchange("one_word", nlists, nq, k, seed=3)
    want = mr.merge(keys, k, metric)
    mr.assert_same(mr.merge(keys, k, metric), want)

    def rejected(got):
        with pytest.raises(AssertionError):
            mr.assert_same(got, want)

    D, I = (a.copy() for a in want)
    assert D[2, 3].view(np.uint32) == D[2, 4].view(np.uint32), "tied on the score: only the ids tell the order"
    I[2, [3, 4]] = I[2, [4, 3]]
    rejected((D, I))                                                        # two tied ids swapped
    rejected(mr.merge(np.repeat(keys[:1], nlists, axis=0), k, metric))      # every list read at list 0's address (no l * nq)
    rejected(mr.merge(np.roll(keys, -1, axis=1), k, metric))                # query q reads query q + 1's lists
    rejected(mr.merge(keys, k, IP if metric == L2 else L2))                 # D negated for the wrong metric
    one = want[0].copy()
    one[4, 7] = -one[4, 7]
    rejected((one, want[1]))                                                # ... in a single slot
    short = mr.exchange("short", nlists, nq, k, real=k - 1)
    want = mr.merge(short, k, metric)
    assert want[1][0, k - 1] == -1 and want[0][0, k - 1] == (-FLT_MAX if metric == IP else FLT_MAX)
    D, I = (a.copy() for a in want)
    I[0, k - 1] = 0
    rejected((D, I))                                                        # a padding slot with I = 0
    D, I = (a.copy() for a in want)
    D[0, k - 1] = -D[0, k - 1]
    rejected((D, I))                                                        # a padding slot with the other metric's D
    zero = np.zeros((1, 2), np.float32)
    with pytest.raises(AssertionError):
        mr.assert_same((-zero, np.zeros((1, 2), np.int64)), (zero, np.zeros((1, 2), np.int64)))  # -0.0 is not +0.0
