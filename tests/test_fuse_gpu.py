"""GPU: knn_eval_fuse (csrc/fuse.inc) bit for bit against tests/fuse_reference.py.

One workgroup of four waves serves a query row.  The sorted union sorts next_pow2(ka + kb) (order word, position) pairs
in LDS, marks the repeats in rank order and compacts the survivors across its waves; the prefix mode compacts A, keeps its
ids in LDS and compacts the entries of B that are not among them.  The shapes here sit where that can go wrong: widths
around one wave, one pass of the workgroup and the powers of two of the sort, k_out on both sides of the number of
survivors, repeats in other waves and passes than their first occurrence, sub-normal and tiny doubles, rows cut into
slabs.  Integers are compared with array_equal, scores as uint64 patterns; there is no tolerance anywhere."""
from pathlib import Path

import numpy as np
import pytest

import fuse_reference as ref

pytestmark = pytest.mark.gpu

KNOB = "KNN355_EVAL_SLAB_ROWS"
KNN_ERR_INVALID = -1
PREFIX, UNION = ref.PREFIX_FILL, ref.SORTED_UNION
S64, S32, SBITS = -7777, -5555, 0xDEADBEEFDEADBEEF  # what the output arrays hold before a call
DBL_MAX = ref.DBL_MAX
I64_MIN = -2**63
ODD_SCORES = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, DBL_MAX, -DBL_MAX, 1e-60, 1e-80, 5e-324, 1.5, -1.5], np.float64)
GOLDEN = Path(__file__).resolve().parent / "golden" / "reference_fuse.npz"


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _ptr(a):
    return None if a is None else a.ctypes.data


def _last_error():
    from knn_for_homology_amd import _lib
    return _lib.lib().knn_last_error().decode()


def c_fuse(hits_a_, scores_a_, keep_a, hits_b_, scores_b_, mode, ascending, k_out, sources=True, **over):
    """the C entry point -> (return code, hits, score bits, source, filled), the outputs pre-filled with the sentinels;
    `over` replaces arguments by name (ka, kb, nq) or drops a pointer (hits_a=None ...)"""
    from knn_for_homology_amd import _lib
    hits_a = np.ascontiguousarray(hits_a_, np.int64)
    hits_b = np.ascontiguousarray(hits_b_, np.int64)
    scores_a = np.ascontiguousarray(scores_a_, np.float64)
    scores_b = np.ascontiguousarray(scores_b_, np.float64)
    keep_a = None if keep_a is None else np.ascontiguousarray(keep_a, np.uint8)
    nq, ka = hits_a.shape
    shape = (max(nq, 1), max(k_out, 1))
    hits = np.full(shape, S64, np.int64)
    so = np.full(shape, SBITS, np.uint64)
    source = np.full(shape, S32, np.int32) if sources else None
    filled = np.full(shape[0], S32, np.int32)
    a = dict(hits_a=hits_a, scores_a=scores_a, ka=ka, hits_b=hits_b, scores_b=scores_b, kb=hits_b.shape[1], nq=nq, hits=hits, so=so,
             filled=filled)
    a.update(over)
    rc = _lib.lib().knn_eval_fuse(_ptr(a["hits_a"]), _ptr(a["scores_a"]), _ptr(keep_a), a["ka"], _ptr(a["hits_b"]), _ptr(a["scores_b"]),
                                  a["kb"], a["nq"], mode, ascending, k_out, _ptr(a["hits"]), _ptr(a["so"]), _ptr(source), _ptr(a["filled"]))
    return rc, hits[:nq], so[:nq], (source[:nq] if sources else None), filled[:nq]


def _same(got, want):
    rc, hits, so, source, filled = got
    assert rc == 0, _last_error()
    assert np.array_equal(filled, want[3]), "filled_out"
    assert np.array_equal(hits, want[0]), "hits_out"
    assert np.array_equal(so, _bits(want[1])), "scores_out (as bits)"
    if source is not None:
        assert np.array_equal(source, want[2]), "source_out"


def _check(hits_a, scores_a, keep_a, hits_b, scores_b, mode, ascending, k_out):
    want = ref.fuse(hits_a, scores_a, keep_a, hits_b, scores_b, mode, ascending, k_out)
    _same(c_fuse(hits_a, scores_a, keep_a, hits_b, scores_b, mode, ascending, k_out), want)
    return want


def _case(rng, nq, ka, kb, nids=None, values=None, keep=False):
    """rows of random ids from [-2, nids) in no order (repeats are the rule), scores from a small set (ties are the rule)
    or random doubles; keep: a random keep_a"""
    nids = max(3, (ka + kb) // 2) if nids is None else nids
    hits_a = rng.integers(-2, nids, (nq, ka)).astype(np.int64)
    hits_b = rng.integers(-2, nids, (nq, kb)).astype(np.int64)
    if values is None:
        scores_a, scores_b = rng.normal(size=(nq, ka)), rng.normal(size=(nq, kb))
    else:
        scores_a, scores_b = rng.choice(values, (nq, ka)), rng.choice(values, (nq, kb))
    keep_a = (rng.random((nq, ka)) < 0.6).astype(np.uint8) if keep else None
    return hits_a, scores_a.astype(np.float64), keep_a, hits_b, scores_b.astype(np.float64)


# ---- widths around a wave, a pass of the workgroup and the powers of two of the sort -----------------------------------
SHAPES = [(1, 1), (63, 1), (32, 32), (64, 1), (200, 56), (200, 57), (300, 300), (512, 512), (1000, 25), (2048, 2048), (2048, 1), (1, 2048)]


@pytest.mark.parametrize("ka, kb", SHAPES)
@pytest.mark.parametrize("mode", [PREFIX, UNION])
def test_shapes(gpu_faiss, ka, kb, mode):
    """k_out: 1, below and above the number of survivors, ka + kb; both directions; with and without keep_a"""
    rng = np.random.default_rng(1000 * ka + kb)
    n = ka + kb
    for keep in (False, True):
        ha, sa, ka_, hb, sb = _case(rng, 3, ka, kb, values=np.arange(-4, 5) / 2.0 if keep else None, keep=keep)
        survivors = int(ref.fuse(ha, sa, ka_, hb, sb, mode, 1, n)[3].min())
        for k_out in sorted({1, max(1, survivors // 2), max(1, survivors - 1), min(n, survivors + 1), n}):
            for ascending in (0, 1):
                _check(ha, sa, ka_, hb, sb, mode, ascending, k_out)


# ---- repeats --------------------------------------------------------------------------------------------------------------
def test_repeats_more_than_a_wave_and_a_pass_behind_their_first_occurrence(gpu_faiss):
    """600 distinct ascending scores: ranks are positions.  Ranks 0..99 hold ids 0..99, ranks 100..299 hold them again
    twice over (every repeat 100 or 200 ranks behind its first occurrence, in another wave and, from rank 256 on, in
    another pass), ranks 300..599 hold new ids: the survivors come from waves 0, 1 and from the second and third pass
    and must close up."""
    ids = np.concatenate([np.arange(100), np.arange(100), np.arange(100), np.arange(300, 600)]).astype(np.int64)[None, :]
    scores = np.arange(600, dtype=np.float64)[None, :] * 1e-70
    want = _check(ids[:, :300], scores[:, :300], None, ids[:, 300:], scores[:, 300:], UNION, 1, 400)
    assert want[0][0].tolist() == list(range(100)) + list(range(300, 600)) and want[3][0] == 400
    want = _check(ids[:, :300], scores[:, :300], None, ids[:, 300:], scores[:, 300:], UNION, 0, 250)  # the walk starts at the far end
    assert want[0][0].tolist() == list(range(599, 349, -1))
    # the same ids through the prefix mode: A's repeats stay, B's members of A go
    want = _check(ids[:, :150], scores[:, :150], None, ids[:, 150:], scores[:, 150:], PREFIX, 0, 600)
    assert want[0][0, :450].tolist() == list(range(100)) + list(range(50)) + list(range(300, 600)) and want[3][0] == 450


@pytest.mark.parametrize("ka, kb", [(5, 3), (300, 300), (2048, 2048)])
def test_one_id_throughout_and_all_ids_distinct(gpu_faiss, ka, kb):
    rng = np.random.default_rng(ka)
    n = ka + kb
    sa, sb = rng.normal(size=(2, ka)), rng.normal(size=(2, kb))
    one_a, one_b = np.full((2, ka), 7, np.int64), np.full((2, kb), 7, np.int64)
    want = _check(one_a, sa, None, one_b, sb, UNION, 1, n)
    assert (want[3] == 1).all() and (want[0][:, 1:] == -1).all()
    want = _check(one_a, sa, None, one_b, sb, PREFIX, 1, n)
    assert (want[3] == ka).all()  # A's repeats are kept, all of B is a member
    ids = np.stack([rng.permutation(n), rng.permutation(n)]).astype(np.int64)
    for mode in (PREFIX, UNION):
        want = _check(ids[:, :ka], sa, None, ids[:, ka:], sb, mode, 0, n)
        assert (want[3] == n).all()


# ---- scores ---------------------------------------------------------------------------------------------------------------
def test_equal_scores_keep_the_order_of_the_positions(gpu_faiss):
    ka, kb = 300, 200
    ids = np.random.default_rng(3).permutation(ka + kb).astype(np.int64)[None, :]
    for value in (0.25, np.nan, 0.0):
        sa, sb = np.full((1, ka), value), np.full((1, kb), value)
        for ascending in (0, 1):
            want = _check(ids[:, :ka], sa, None, ids[:, ka:], sb, UNION, ascending, ka + kb)
            assert np.array_equal(want[0], ids) and want[2][0].tolist() == list(range(ka + kb))  # A before B
    z = np.random.default_rng(4).choice(np.array([0.0, -0.0]), (1, ka + kb))  # the two zeros and nothing else: positions again
    want = _check(ids[:, :ka], z[:, :ka], None, ids[:, ka:], z[:, ka:], UNION, 0, ka + kb)
    assert np.array_equal(want[0], ids) and np.array_equal(_bits(want[1]), _bits(z))


def test_nan_infinities_zeros_and_tiny_doubles(gpu_faiss):
    rng = np.random.default_rng(5)
    for ka, kb in ((75, 75), (300, 213)):
        ha, sa, _, hb, sb = _case(rng, 4, ka, kb, nids=2 * (ka + kb), values=ODD_SCORES)
        assert np.isnan(sa).sum() > 10 and (_bits(sa) == 1 << 63).sum() > 10 and (sa == 5e-324).sum() > 10
        for k_out in (ka, ka + kb):
            for ascending in (0, 1):
                _check(ha, sa, None, hb, sb, UNION, ascending, k_out)


def test_doubles_below_float32_order(gpu_faiss):
    """1e-60 against 1e-80, and sub-normal doubles against zero and each other: a float32 path, or a double compare that
    flushes sub-normals, ties them and falls back on the positions, which give another order here"""
    ids_a, ids_b = np.array([[1, 2, 3, 4]], np.int64), np.array([[5, 6, 7, 8]], np.int64)
    sa = np.array([[1e-60, 1e-310, 5e-324, 0.0]])
    sb = np.array([[1e-80, 1e-320, -5e-324, 1e-45]])
    want = _check(ids_a, sa, None, ids_b, sb, UNION, 1, 8)
    assert want[0][0].tolist() == [7, 4, 3, 6, 2, 5, 1, 8]
    want = _check(ids_a, sa, None, ids_b, sb, UNION, 0, 8)
    assert want[0][0].tolist() == [8, 1, 5, 2, 6, 3, 4, 7]


def test_ids_are_whole_int64_values(gpu_faiss):
    ha = np.array([[-1, 2, I64_MIN, 2**62, 2**32 + 2, 2]], np.int64)
    hb = np.array([[2**32 + 2, 2**62, -3, 2, 2**62 + 1, I64_MIN + 1]], np.int64)
    sa = np.array([[0.0, 6.0, 1.0, 4.0, 3.0, 2.0]])
    sb = np.array([[9.0, 8.0, 7.0, 6.5, 5.0, 0.5]])
    want = _check(ha, sa, None, hb, sb, UNION, 1, 12)
    assert want[0][0, :4].tolist() == [2, 2**32 + 2, 2**62, 2**62 + 1] and want[3][0] == 4  # (2^32 + 2 is not 2)
    want = _check(ha, sa, None, hb, sb, PREFIX, 1, 12)
    assert want[0][0, :5].tolist() == [2, 2**62, 2**32 + 2, 2, 2**62 + 1] and want[3][0] == 5


# ---- the prefix mode ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ka, kb", [(7, 9), (300, 300), (513, 70)])
def test_prefix_keep_none_all_alternating_null(gpu_faiss, ka, kb):
    rng = np.random.default_rng(ka + kb)
    ha, sa, _, hb, sb = _case(rng, 4, ka, kb)
    keeps = {"none": np.zeros((4, ka), np.uint8), "all": np.ones((4, ka), np.uint8), "odd bytes": np.full((4, ka), 0x80, np.uint8),
             "alternating": (np.arange(4 * ka).reshape(4, ka) % 2).astype(np.uint8), "null": None}
    for name, keep in keeps.items():
        for k_out in (ka, ka + kb):
            want = _check(ha, sa, keep, hb, sb, PREFIX, 0, k_out)
        if name == "none":
            assert (want[2][:, 0] >= ka).all()  # nothing of A: the first output is B's
    assert np.array_equal(ref.fuse(ha, sa, keeps["all"], hb, sb, PREFIX, 0, ka)[0], ref.fuse(ha, sa, None, hb, sb, PREFIX, 0, ka)[0])


def test_prefix_fills_exactly_on_the_last_entry_of_b_and_short_rows(gpu_faiss):
    """row 0 fills on B's last entry (the reference's `for ... else` raises there; this is a full row); row 1 stays one
    short; row 2 holds nothing at all.  B's repeats are kept."""
    ha = np.array([[3, 4, 3, -1, 6], [3, 4, 3, -1, 6], [-1, -1, -1, -1, -1]], np.int64)
    keep = np.array([[1, 0, 1, 1, 1], [1, 0, 1, 1, 1], [1, 1, 1, 1, 1]], np.uint8)
    hb = np.array([[4, 3, 9, 9, 6, -2, 10], [4, 3, 9, 9, 6, -2, 6], [-1, -2, -3, -4, -5, -6, -7]], np.int64)
    sa = np.arange(15, dtype=np.float64).reshape(3, 5)
    sb = -np.arange(21, dtype=np.float64).reshape(3, 7)
    for ascending in (0, 1):
        want = _check(ha, sa, keep, hb, sb, PREFIX, ascending, 7)
        assert want[0].tolist() == [[3, 3, 6, 4, 9, 9, 10], [3, 3, 6, 4, 9, 9, -1], [-1] * 7] and want[3].tolist() == [7, 6, 0]
        pad = DBL_MAX if ascending else -DBL_MAX
        assert want[1][1, 6] == pad and (want[1][2] == pad).all() and want[2][1, 6] == -1
    rng = np.random.default_rng(11)
    ha, sa, keep, hb, sb = _case(rng, 5, 300, 300, nids=200, keep=True)  # 200 ids: no row reaches 500 outputs
    want = _check(ha, sa, keep, hb, sb, PREFIX, 0, 500)
    assert (want[3] < 500).all() and (want[3] > 100).all()


# ---- slabs ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [1, 3, 4])
@pytest.mark.parametrize("mode", [PREFIX, UNION])
def test_slabs(gpu_faiss, monkeypatch, rows, mode):
    """7 rows in slabs of 1, 3 and 4: the results equal the uncut call's.  The knob is read on every call."""
    rng = np.random.default_rng(9)
    ha, sa, keep, hb, sb = _case(rng, 7, 70, 45, keep=True)
    want = ref.fuse(ha, sa, keep, hb, sb, mode, 1, 80)
    monkeypatch.delenv(KNOB, raising=False)
    whole = c_fuse(ha, sa, keep, hb, sb, mode, 1, 80)
    monkeypatch.setenv(KNOB, str(rows))
    cut = c_fuse(ha, sa, keep, hb, sb, mode, 1, 80)
    _same(whole, want)
    _same(cut, want)
    assert all(np.array_equal(a, b) for a, b in zip(whole[1:], cut[1:]))
    _same(c_fuse(ha, sa, keep, hb, sb, mode, 1, 80, sources=False), want)


@pytest.mark.parametrize("k", [3, 65])
@pytest.mark.parametrize("mode", [PREFIX, UNION])
def test_optional_columns_across_slabs(gpu_faiss, monkeypatch, k, mode):
    """5 rows in slabs of 2: keep_a and source_out, each present and absent"""
    rng = np.random.default_rng(90 + k)
    ha, sa, keep, hb, sb = _case(rng, 5, k, k, keep=True)
    monkeypatch.setenv(KNOB, "2")
    for keep_a in (keep, None):
        want = ref.fuse(ha, sa, keep_a, hb, sb, mode, 1, k + 1)
        for sources in (True, False):
            _same(c_fuse(ha, sa, keep_a, hb, sb, mode, 1, k + 1, sources=sources), want)


# ---- a seeded sweep -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(4))
def test_random_sweep(gpu_faiss, seed):
    rng = np.random.default_rng(4242 + seed)
    for _ in range(10):
        nq = int(rng.integers(1, 9))
        ka, kb = (int(rng.choice([1, 2, int(rng.integers(1, 130)), int(rng.integers(1, 700))])) for _ in range(2))
        k_out = int(rng.choice([1, ka, ka + kb, int(rng.integers(1, ka + kb + 1))]))
        ha, sa, keep, hb, sb = _case(rng, nq, ka, kb, nids=int(rng.integers(1, 2 * (ka + kb) + 1)),
                                     values=ODD_SCORES if rng.random() < 0.4 else None, keep=rng.random() < 0.5)
        _check(ha, sa, keep, hb, sb, int(rng.integers(0, 2)), int(rng.integers(0, 2)), k_out)


# ---- the Python facade ----------------------------------------------------------------------------------------------------
def test_facade_on_the_reference_fixture(gpu_faiss):
    from knn_for_homology_amd.evaluation import combine_hits, merge_hits
    g = np.load(GOLDEN)
    hits, scores = combine_hits(g["combined_hits_a"], g["combined_e_values_a"], g["combined_hits_b"], g["combined_scores_b"])
    assert hits.dtype == np.int64 and scores.dtype == np.float64
    assert np.array_equal(hits, g["combined_hits"]) and np.array_equal(_bits(scores), _bits(g["combined_scores"]))
    for name in ("both", "both_uneven"):
        hits, scores = merge_hits(g[f"{name}_hits_a"], g[f"{name}_e_values_a"], g[f"{name}_hits_b"], g[f"{name}_e_values_b"],
                                  pad_hit=0, pad_score=10**6)
        assert np.array_equal(hits, g[f"{name}_hits"]) and np.array_equal(_bits(scores), _bits(g[f"{name}_e_values"]))


def test_facade_short_rows_padding_and_sources(gpu_faiss):
    from knn_for_homology_amd.evaluation import combine_hits, merge_hits
    ha = np.array([[3, 4, 5], [3, 4, 5]], np.int32)          # (any integer type: converted to int64)
    ea = np.array([[1e-50, 1e-3, 0.5], [1e-50, 1e-3, 0.5]])
    hb = np.array([[4, 9, 3, 5], [4, 3, 3, 4]])
    sb = np.array([[0.9, 0.8, 0.7, 0.6], [0.9, 0.8, 0.7, 0.6]], np.float32)
    with pytest.raises(ValueError, match="row 1"):
        combine_hits(ha, ea, hb, sb)
    hits, scores, source = combine_hits(ha, ea, hb, sb, short="pad", want_sources=True)
    assert hits.tolist() == [[3, 4, 9], [3, 4, -1]] and source.tolist() == [[0, 1, 4], [0, 1, -1]]
    assert np.array_equal(_bits(scores[0]), _bits([-np.log(1e-50 + 10**-200), -np.log(1e-3 + 10**-200), np.float64(np.float32(0.8))]))
    assert scores[1, 2] == -DBL_MAX
    assert combine_hits(ha[:1], ea[:1], hb[:1], sb[:1], k_out=5, short="pad")[0].tolist() == [[3, 4, 9, 5, -1]]
    hits, scores = combine_hits(ha, ea, hb, sb, threshold=1.0, k_out=2)
    assert hits.tolist() == [[3, 4], [3, 4]]
    # merge: library padding, replaced padding, sources index the concatenated inputs
    rng = np.random.default_rng(12)
    a_hits, a_scores, _, b_hits, b_scores = _case(rng, 6, 40, 30, nids=25)
    hits, scores, source = merge_hits(a_hits, a_scores, b_hits, b_scores, want_sources=True)
    want = ref.fuse(a_hits, a_scores, None, b_hits, b_scores, UNION, 1, 40)
    assert np.array_equal(hits, want[0]) and np.array_equal(_bits(scores), _bits(want[1])) and np.array_equal(source, want[2])
    assert (want[3] < 40).all() and (hits[:, -1] == -1).all() and (scores[:, -1] == DBL_MAX).all()
    cat_hits, cat_scores = np.concatenate([a_hits, b_hits], axis=1), np.concatenate([a_scores, b_scores], axis=1)
    real = source >= 0
    rows = np.nonzero(real)[0]
    assert np.array_equal(hits[real], cat_hits[rows, source[real]])
    assert np.array_equal(_bits(scores[real]), _bits(cat_scores[rows, source[real]]))
    h2, s2 = merge_hits(a_hits, a_scores, b_hits, b_scores, pad_hit=0, pad_score=10**6)
    assert np.array_equal(h2[real], hits[real]) and (h2[~real] == 0).all() and (s2[~real] == 1e6).all()
    h3, s3 = merge_hits(a_hits, a_scores, b_hits, b_scores, k_out=70, ascending=False)
    want = ref.fuse(a_hits, a_scores, None, b_hits, b_scores, UNION, 0, 70)
    assert np.array_equal(h3, want[0]) and np.array_equal(_bits(s3), _bits(want[1]))
    with pytest.raises(ValueError):
        merge_hits(a_hits, a_scores[:, :-1], b_hits, b_scores)
    with pytest.raises(ValueError):
        merge_hits(a_hits, a_scores, b_hits[:-1], b_scores[:-1])
    with pytest.raises(ValueError):
        merge_hits(a_hits[0], a_scores[0], b_hits[0], b_scores[0])


# ---- errors: refused on the host, nothing allocated or launched, the outputs as they were --------------------------------
def _refused(got, what):
    rc, hits, so, source, filled = got
    assert rc == KNN_ERR_INVALID and what in _last_error(), _last_error()
    assert (hits == S64).all() and (so == SBITS).all() and (source == S32).all() and (filled == S32).all()


def test_refusals(gpu_faiss):
    ha, hb = np.zeros((3, 4), np.int64), np.ones((3, 5), np.int64)
    sa, sb = np.zeros((3, 4)), np.zeros((3, 5))
    for k in (0, -1, 2049):
        _refused(c_fuse(ha, sa, None, hb, sb, UNION, 1, 4, ka=k), "ka outside")
        _refused(c_fuse(ha, sa, None, hb, sb, PREFIX, 1, 4, kb=k), "kb outside")
    for k_out in (0, -2, 10):
        _refused(c_fuse(ha, sa, None, hb, sb, UNION, 1, k_out), "k_out outside")
    for mode in (-1, 2, 7):
        _refused(c_fuse(ha, sa, None, hb, sb, mode, 1, 4), "unknown mode")
    _refused(c_fuse(ha, sa, None, hb, sb, UNION, 1, 4, nq=-1), "negative nq")
    for name in ("hits_a", "scores_a", "hits_b", "scores_b", "hits", "so", "filled"):  # (an array left out keeps its sentinels too)
        _refused(c_fuse(ha, sa, None, hb, sb, UNION, 1, 4, **{name: None}), "null pointer")
    # nq = 0 returns before any pointer is looked at
    rc = c_fuse(ha, sa, None, hb, sb, UNION, 1, 4, nq=0, hits_a=None, scores_a=None, hits_b=None, scores_b=None, hits=None, so=None,
                filled=None)[0]
    assert rc == 0
    got = c_fuse(ha, sa, None, hb, sb, UNION, 1, 4, nq=0)
    assert got[0] == 0 and (got[1] == S64).all() and (got[4] == S32).all()
    # and the same arguments pass once they are right
    got = c_fuse(ha, sa, None, hb, sb, UNION, 1, 4)
    assert got[0] == 0 and got[1].tolist() == [[0, 1, -1, -1]] * 3 and got[4].tolist() == [2] * 3
