"""Host reference of the shard key exchange (sharded.py, knn_flat_search_keys_dev, knn_merge_keys_dev): plain numpy.

A shard's result travels as k packed keys per query, ``uint64 = f2ord(score) << 32 | global row id``; ascending key order is
best first, ties on the score go to the lower id, and ``KEY_PAD`` (all ones) means "no key".  The merge of ``nlists`` such
lists is a selection over 64-bit integers, so its reference is ``numpy.sort`` on ``uint64`` and every comparison is bit for
bit.  ``exchange`` generates well-formed synthetic exchanges (what an all-gather of healthy ranks can deliver): every list
sorted ascending and padded at the tail, every list's ids from a range of its own -- so all keys of a query are distinct.
"""
import numpy as np

IP, L2 = 0, 1
KEY_PAD = np.uint64(0xFFFFFFFFFFFFFFFF)
FLT_MAX = np.finfo(np.float32).max
ID_LAST = 0xFFFFFFFE  # the largest id the `extremes` pattern uses
PATTERNS = ("gaussian", "one_word", "two_clusters", "extremes", "one_list_wins", "round_robin")  # and "short", which takes `real`

_U32 = np.uint64(32)
_LOW = np.uint64(0xFFFFFFFF)


def f2ord(v):
    """order-preserving 32-bit word of an fp32 value (as uint64): a < b as floats <=> f2ord(a) < f2ord(b)"""
    u = np.ascontiguousarray(v, np.float32).view(np.uint32).astype(np.uint64)
    neg = (u & 0x80000000) != 0
    return np.where(neg, (~u) & 0xFFFFFFFF, u | 0x80000000)


def ord2f(o):
    """inverse of f2ord"""
    o = o.astype(np.uint64)
    u = np.where((o & 0x80000000) != 0, o & 0x7FFFFFFF, (~o) & 0xFFFFFFFF).astype(np.uint32)
    return u.view(np.float32)


def kmax_of(k):
    """the most survivors the selection sorts for k results (select_topk_kernel: kmax = k + max(k >> 2, 32))"""
    return k + max(k >> 2, 32)


def short_reals(k):
    """the real-key counts of the `short` pattern: both sides of k and of the early-out ``real <= khi`` of the bracket search"""
    return (0, 1, k - 1, k, k + 1, kmax_of(k), kmax_of(k) + 1)


def pack_keys(D, I, metric, id_base):
    """(D, I) of a flat search of one shard -> uint64 [nq][k] keys with global ids ``I + id_base``.  The score word is that
    of ``v + 0`` with v = -D for inner product and D for L2 (the addition turns -0.0 into +0.0, as the scan does before it
    packs a key); slots with I < 0 are KEY_PAD."""
    D = np.asarray(D, np.float32)
    I = np.asarray(I, np.int64)
    v = (-D if metric == IP else D) + np.float32(0)
    ids = I + np.int64(id_base)
    real = I >= 0
    assert ((ids >= 0) & (ids < 1 << 32))[real].all(), "id_base + row does not fit 32 bits"
    keys = (f2ord(v) << _U32) | (ids.astype(np.uint64) & _LOW)
    keys[~real] = KEY_PAD
    return keys


def unpack(keys, metric):
    """keys -> (D float32, I int64): KEY_PAD gives I = -1 and D = -FLT_MAX (inner product) / +FLT_MAX (L2)"""
    keys = np.asarray(keys, np.uint64)
    pad = keys == KEY_PAD
    v = ord2f(keys >> _U32)
    D = np.where(pad, -FLT_MAX if metric == IP else FLT_MAX, -v if metric == IP else v).astype(np.float32)
    I = np.where(pad, -1, (keys & _LOW).astype(np.int64))
    return D, I


def merge_keys(keys, k):
    """keys uint64 [nlists][nq][kin] -> the k smallest keys per query, ascending: uint64 [nq][k]"""
    keys = np.asarray(keys, np.uint64)
    nlists, nq, kin = keys.shape
    flat = np.sort(np.transpose(keys, (1, 0, 2)).reshape(nq, nlists * kin), axis=1)
    if flat.shape[1] < k:
        flat = np.concatenate([flat, np.full((nq, k - flat.shape[1]), KEY_PAD, np.uint64)], axis=1)
    return np.ascontiguousarray(flat[:, :k])


def merge(keys, k, metric):
    """the reference of knn_merge_keys_dev: (D [nq][k], I [nq][k])"""
    return unpack(merge_keys(keys, k), metric)


def assert_same(got, want, what=""):
    """the comparison of the GPU tests: ids equal, distances equal as bit patterns (so -0.0 != +0.0 and a NaN equals itself)"""
    Dg, Ig = (np.asarray(a) for a in got)
    Dw, Iw = (np.asarray(a) for a in want)
    assert Ig.dtype == np.int64 and Dg.dtype == np.float32 and Ig.shape == Iw.shape and Dg.shape == Dw.shape, what
    if not np.array_equal(Ig, Iw):
        q, j = np.argwhere(Ig != Iw)[0]
        raise AssertionError(f"{what}: ids differ in {int((Ig != Iw).sum())} slots, first at query {q} rank {j}: got {Ig[q, j]}, expected {Iw[q, j]}")
    bg, bw = np.ascontiguousarray(Dg).view(np.uint32), np.ascontiguousarray(Dw).view(np.uint32)
    if not np.array_equal(bg, bw):
        q, j = np.argwhere(bg != bw)[0]
        raise AssertionError(f"{what}: distance bits differ in {int((bg != bw).sum())} slots, first at query {q} rank {j}: "
                             f"got {Dg[q, j]!r} ({bg[q, j]:#010x}), expected {Dw[q, j]!r} ({bw[q, j]:#010x})")


# ---- synthetic exchanges -------------------------------------------------------------------------------------------------
def _words(v):
    """score words of fp32 values after `+ 0`; finite and not NaN, or the generator is wrong"""
    v = np.asarray(v, np.float32) + np.float32(0)
    assert np.isfinite(v).all()
    return f2ord(v)


def _list_ids(rng, nlists, nq, k):
    """int64 [nlists][nq][k]: distinct ids, list l's from [l * span + 1, (l + 1) * span - 2) with span = 2^32 // nlists.  The
    ranges are disjoint and leave out id 0 and ID_LAST, which the `extremes` pattern places itself."""
    span = (1 << 32) // nlists
    stride = (span - 3) // k
    assert stride >= 1
    off = np.arange(k, dtype=np.int64) * stride + rng.integers(0, stride, (nlists, nq, k))
    off = rng.permuted(off, axis=2)  # (no order between a key's id and its slot)
    return off + (np.arange(nlists, dtype=np.int64) * span + 1)[:, None, None]


def check_well_formed(keys):
    """every list ascending with its padding at the tail; all real keys of a query distinct"""
    keys = np.asarray(keys, np.uint64)
    nlists, nq, k = keys.shape
    assert (keys[:, :, 1:] >= keys[:, :, :-1]).all(), "a list is not sorted (or has padding in front of a key)"
    flat = np.sort(np.transpose(keys, (1, 0, 2)).reshape(nq, nlists * k), axis=1)
    dup = (flat[:, 1:] == flat[:, :-1]) & (flat[:, 1:] != KEY_PAD)
    assert not dup.any(), "duplicate keys in one query"
    return keys


def _short_counts(rng, nlists, k, real):
    """how many of `real` keys each list holds: a third of the lists (in a shuffled order) stays empty as long as the others
    have room, and the others share the keys unevenly"""
    counts = np.zeros(nlists, np.int64)
    n_live = nlists - nlists // 3
    while n_live * k < real:
        n_live += 1
    order = rng.permutation(nlists)[:n_live]
    left = real
    for l in order:
        take = min(k, left, max(1, (2 * left + 2) // 3))  # two thirds of what is left: uneven by construction
        counts[l] = take
        left -= take
    for l in order:  # (more keys than the two-thirds rule placed: fill up in the same order)
        more = min(k - counts[l], left)
        counts[l] += more
        left -= more
    assert left == 0 and counts.sum() == real and counts.max() <= k
    return counts


def exchange(pattern, nlists, nq, k, seed=0, real=None):
    """uint64 [nlists][nq][k]: one well-formed synthetic all-gather buffer.

    gaussian       independent normal scores
    one_word       every key of a query carries the same score word: only the ids separate them
    two_clusters   words from f2ord(-1e30), f2ord(1e30) and their neighbours a few ulps away: a nearly empty 64-bit range
    extremes       gaussian, with the key (f2ord(-FLT_MAX), id 0) and the key (f2ord(FLT_MAX), id ID_LAST) in every query (a
                   query of one single slot holds one of the two, alternating)
    one_list_wins  the best k keys all sit in the last list
    round_robin    the key of rank r sits in list r % nlists
    short          exactly `real` real keys per query (an int, or one per query), clamped to nlists * k, spread unevenly over
                   the lists, some lists all padding
    """
    rng = np.random.default_rng([seed, nlists, nq, k, sum(map(ord, pattern))])
    shape = (nlists, nq, k)
    ids = _list_ids(rng, nlists, nq, k)
    live = np.ones(shape, bool)
    if pattern == "gaussian":
        words = _words(rng.standard_normal(shape, dtype=np.float32))
    elif pattern == "one_word":
        words = np.broadcast_to(_words(rng.standard_normal((1, nq, 1), dtype=np.float32)), shape)
    elif pattern == "two_clusters":
        centre = np.where(rng.integers(0, 2, shape) == 0, np.float32(-1e30), np.float32(1e30)).astype(np.float32)
        words = f2ord(centre) + rng.integers(-3, 4, shape).astype(np.int64).astype(np.uint64)  # (neighbouring words = neighbouring floats)
        words = _words(ord2f(words & _LOW))
    elif pattern == "extremes":
        words = _words(rng.standard_normal(shape, dtype=np.float32)).copy()
        lo_slot, hi_slot = (0, slice(None), 0), (nlists - 1, slice(None), k - 1)
        if nlists * k == 1:
            even = np.arange(nq) % 2 == 0
            words[0, :, 0] = np.where(even, f2ord(np.float32(-FLT_MAX)), f2ord(np.float32(FLT_MAX)))
            ids[0, :, 0] = np.where(even, 0, ID_LAST)
        else:
            words[lo_slot], ids[lo_slot] = f2ord(np.float32(-FLT_MAX)), 0
            words[hi_slot], ids[hi_slot] = f2ord(np.float32(FLT_MAX)), ID_LAST
    elif pattern == "one_list_wins":
        v = np.abs(rng.standard_normal(shape, dtype=np.float32)) + np.float32(1)
        v[nlists - 1] = -v[nlists - 1] if nlists > 1 else v[0]
        words = _words(v)
    elif pattern == "round_robin":
        n = nlists * k
        # strictly increasing words (negative finite floats around -1): rank r goes to list r % nlists, slot r // nlists
        w = f2ord(np.float32(-1.0)).reshape(-1)[0] + np.cumsum(rng.integers(1, 1000, (nq, n)), axis=1).astype(np.uint64)
        w = _words(ord2f(w))
        assert (w[:, 1:] > w[:, :-1]).all()
        words = np.ascontiguousarray(np.transpose(w.reshape(nq, k, nlists), (2, 0, 1)))
    elif pattern == "short":
        assert real is not None
        reals = np.minimum(np.broadcast_to(np.asarray(real, np.int64), (nq,)), nlists * k)
        words = _words(rng.standard_normal(shape, dtype=np.float32))
        live = np.zeros(shape, bool)
        for q in range(nq):
            counts = _short_counts(rng, nlists, k, int(reals[q]))
            live[:, q, :] = np.arange(k)[None, :] < counts[:, None]
    else:
        raise ValueError(pattern)
    keys = (np.asarray(words, np.uint64) << _U32) | ids.astype(np.uint64)
    keys = np.where(live, keys, KEY_PAD)
    keys = check_well_formed(np.sort(keys, axis=2))
    if pattern == "short":
        assert np.array_equal((keys != KEY_PAD).sum(axis=(0, 2)), reals)
    return keys


def with_status_rows(keys, failed):
    """keys [world][nq][k] -> [world][nq + 1][k], the send buffers of ``ShardedFlatIndex._search_on_current_stream`` stacked as the
    all-gather delivers them: row nq is the status row -- all padding on a healthy rank; a rank in `failed` sends "no rows" for
    keys and its rank number as the one key of its status row (score word 0: not the word of any float the scan packs)"""
    keys = np.asarray(keys, np.uint64)
    world, nq, k = keys.shape
    out = np.full((world, nq + 1, k), KEY_PAD, np.uint64)
    out[:, :nq] = keys
    for r in failed:
        out[r, :nq] = KEY_PAD
        out[r, nq, 0] = np.uint64(r)
    return out
