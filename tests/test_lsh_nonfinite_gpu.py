"""GPU: IndexLSH on non-finite and overflowing rows -- lsh_encode_kernel with and without thresholds, the medians of
lsh_median_kernel over columns that hold infinities, and the fused IndexRefineFlat(IndexLSH) search -- against the host
restatements, bit for bit: codes, thresholds, ids and distance bits.  The references are pinned by hand on the CPU
(tests/test_lsh_nonfinite_reference.py); the rows come from tests/lsh_nonfinite_cases.py (single poisoned entries over small
integers and a +-1 rotation: every projection has one right answer in every summation order).

The code bit is FAISS's: float32 (projection - threshold) >= 0, so a NaN projection's bit is 0 and so is the bit of a
projection that equals an infinite threshold (inf - inf is a NaN).  Bits at and above nbits do not exist: two rows' Hamming
distance counts the nbits real bits only, whatever the rows hold."""
import numpy as np
import pytest

import lsh_nonfinite_cases as lc
import nonfinite_cases as nc
from lsh_reference import assert_same_codes, assert_same_search, pm1_rotation, ref_codes, ref_search
from lsh_thresholds_reference import ref_codes_thr, ref_projections, ref_train
from refine_reference import FLT_MAX, METRIC_INNER_PRODUCT, METRIC_L2, ref_refine

pytestmark = pytest.mark.gpu

INF = np.float32(np.inf)


def _index(gpu_faiss, R, thresholds=None):
    """IndexLSH over the rotation R; thresholds: None (none), or float32 [nbits] installed through knn_lsh_set_thresholds
    (what read_index does with an index file's)"""
    from knn_for_homology_amd import _lib
    idx = gpu_faiss.IndexLSH(R.shape[1], R.shape[0], True, thresholds is not None, _rotation=R)
    if thresholds is not None:
        t = np.ascontiguousarray(thresholds, np.float32)
        _lib.check(_lib.lib().knn_lsh_set_thresholds(idx._h, t.ctypes.data))
        idx.is_trained = True
    return idx


def _codes_and_search(idx, x, xq, want_b, want_q, k, what):
    idx.add(x)
    assert_same_codes(idx.codes(), want_b, what)
    D, I = idx.search(xq, k)
    De, Ie = ref_search(want_b, want_q, k)
    assert_same_search(D, I, De, Ie, what)


# (nbits, d, n): code widths 128, 256 and 200 (no multiple of 128: 56 padding bits); d no multiple of 32; n = 128 j + 1 and
# 128 j - 1 (the clamped rows of a ragged last tile); poisoned rows at lsh_nonfinite_cases.special_rows
ENCODE_CASES = [(128, 33, 257), (256, 37, 383), (200, 100, 129), (200, 33, 255)]


@pytest.mark.parametrize("nbits,d,n", ENCODE_CASES)
def test_encoding_without_thresholds(gpu_faiss, nbits, d, n):
    rng = np.random.default_rng(nbits + d + n)
    R = pm1_rotation(rng, nbits, d)
    x, kinds = lc.poison_rows(rng, n, d)
    assert set(kinds.values()) == set(lc.KINDS) and {0, 127, 128, n - 2, n - 1} <= set(kinds)
    want = lc.expected_codes(x, R)
    assert np.array_equal(want, ref_codes(x, R))
    # every row is a query too: poisoned queries against poisoned and ordinary rows, in both orders of a ragged batch
    xq = np.ascontiguousarray(x[::-1])
    _codes_and_search(_index(gpu_faiss, R), x, xq, want, np.ascontiguousarray(want[::-1]), 40, f"nbits={nbits} d={d} n={n}")


@pytest.mark.parametrize("nbits,d,n", ENCODE_CASES)
def test_encoding_with_thresholds(gpu_faiss, nbits, d, n):
    """finite thresholds, then +inf and -inf in a few bits -- among them bits onto which the pinf rows project +inf and bits
    onto which they project -inf -- against rows whose projection is +inf, -inf, finite and NaN"""
    rng = np.random.default_rng(nbits * 3 + d + n)
    R = pm1_rotation(rng, nbits, d)
    x, kinds = lc.poison_rows(rng, n, d)
    p = lc.classify(x, R)
    finite = (rng.integers(-6, 7, nbits) / 2).astype(np.float32)   # integers and half-integers: rows sit on some of them
    plus, minus = np.flatnonzero(R[:, lc.C_INF] > 0), np.flatnonzero(R[:, lc.C_INF] < 0)
    infinite = finite.copy()
    infinite[[plus[0], minus[0], plus[-1]]] = INF
    infinite[[plus[1], minus[1], minus[-1]]] = -INF
    for tv in (INF, -INF):   # projections of all four kinds meet thresholds of both infinities
        cols = p[:, infinite == tv]
        assert (cols == INF).any() and (cols == -INF).any() and np.isfinite(cols).any() and np.isnan(cols).any(), tv
    assert (p == finite).any() and (p[:, np.isinf(infinite)] == infinite[np.isinf(infinite)]).any(), "a projection equal to its (infinite) threshold"
    for name, t in (("finite", finite), ("infinite", infinite)):
        want = lc.expected_codes(x, R, t)
        assert np.array_equal(want, ref_codes_thr(x, R, t))
        xq = np.ascontiguousarray(x[::-1])
        _codes_and_search(_index(gpu_faiss, R, t), x, xq, want, np.ascontiguousarray(want[::-1]), 40,
                          f"{name} thresholds nbits={nbits} d={d} n={n}")


# ---- train_thresholds on columns with infinities --------------------------------------------------------------------------------
def _same_bits(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == np.float32 and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
    assert bad.size == 0, f"{what}: {bad.size} of {got.size} thresholds differ; first: bit {bad[0]}: got {got[bad[0]]!r}, expected {want[bad[0]]!r}"


@pytest.mark.parametrize("n,case", [(n, case) for n in (7, 8, 1029, 1030) for case in ("few", "middle", "most_big", "around", "nan")
                                    if case != "around" or n % 2 == 0])
def test_train_thresholds_on_columns_with_infinities(gpu_faiss, n, case):
    """few: fewer than half of the rows infinite (a finite median); middle: the middle itself infinite (odd n: s[n / 2]; even n:
    (finite + inf) / 2) -- thresholds of +-inf, training succeeds; most_big: (2^127 + 2^127) / 2 = +inf in float32 for even n;
    around: +inf and -inf around the middle of an even n -- refused; nan: one NaN projection -- refused.  After each
    successful training the training rows are encoded and compared."""
    from knn_for_homology_amd._lib import Knn355Error
    x, R = lc.train_case(n, case, nbits=70, d=37)
    what, t = ref_train(x, R)
    idx = gpu_faiss.IndexLSH(R.shape[1], R.shape[0], True, True, _rotation=R)
    if what != "ok":
        assert case in ("around", "nan")
        msg = (r"a projection onto bit 0 is NaN" if what == "projection" else r"the median \(\+inf and -inf around the middle\) of bit 0 is NaN")
        with pytest.raises(Knn355Error, match=msg):
            idx.train(x)
        assert not idx.is_trained and idx.thresholds.size == 0
        return
    assert np.isfinite(t).all() if (case == "few" or (case == "most_big" and n % 2)) else np.isinf(t).all()
    idx.train(x)
    _same_bits(idx.thresholds, t, f"{case} n={n}")
    want = lc.expected_codes(x, R, t)
    assert np.array_equal(want, ref_codes_thr(x, R, t))
    if case == "middle":
        on = ref_projections(x, R) == t
        assert (on & np.isinf(t)).any(), "no row's projection equals its infinite threshold"
    idx.add(x)
    assert_same_codes(idx.codes(), want, f"{case} n={n}")


# ---- the fused IndexRefineFlat over IndexLSH ------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", [METRIC_L2, METRIC_INNER_PRODUCT])
@pytest.mark.parametrize("nbits", [128, 200])
def test_fused_refine_over_poisoned_rows(gpu_faiss, oracle, nbits, metric):
    """The base's rows hold every poisoned kind of nonfinite_cases (over small integers: the +-1 rotation's codes have one right
    answer; a `huge` row's projection is 3e19 times a sum of d = 37 signs, odd, so its sign has one too).  Expected: the
    oracle's exact re-ranking of the reference's Hamming candidates -- never-pairs dropped, starved queries padded, an
    inner-product +inf leading."""
    nb, nq, d, k, kf = 300, 33, 37, 10, 8
    rng = np.random.default_rng(nbits + metric)
    xb, xq, table = nc.poison_ints(rng, nb, nq, d, nc.special_rows(nb, 128))
    assert set(v.split(":")[-1] for v in table.rows.values()) == set(nc.ROW_KINDS)
    R = pm1_rotation(rng, nbits, d)
    cb, cq = ref_codes(xb, R), ref_codes(xq, R)
    kb = k * kf
    _, Ih = ref_search(cb, cq, kb)
    De, Ie = ref_refine(oracle, xb, xq, Ih, k, metric, allow_unfilled=True)
    # not vacuous, on the reference's answer
    assert ((Ie >= 0).sum(1) < k).any(), "no query has fewer than k hits"
    assert (De[Ie < 0] == (-FLT_MAX if metric == METRIC_INNER_PRODUCT else FLT_MAX)).all()
    poisoned = np.array(sorted(table.rows))
    assert np.isin(Ih, poisoned).any(), "no query's candidates name a poisoned row"
    if metric == METRIC_INNER_PRODUCT:
        assert np.isposinf(De).any(), "no +inf inner-product hit"
        assert (np.isposinf(De[:, 1:]) <= np.isposinf(De[:, :-1])).all(), "+inf leads"
    for q, r in table.near.items():
        assert r not in Ie[q], "a poisoned copy is no hit"
    idx = gpu_faiss.IndexRefineFlat(gpu_faiss.IndexLSH(d, nbits, _rotation=R), metric=metric)
    idx.add(xb)
    idx.k_factor = kf
    assert_same_codes(idx.base_index.codes(), cb)
    D, I = idx.search(xq, k)
    assert_same_search(D, I, De, Ie, f"nbits={nbits} metric={metric}")
