"""CPU: tests/fuse_reference.py (the restatement of knn_eval_fuse's contract that the GPU tests compare against) gives
exactly what the reference's own loops gave (tests/golden/reference_fuse.npz, written by make_fuse_golden.py from
pfam/proteins.py:216-240 and 340-372), and does what the contract says where the fixture cannot go: ties across the
lists, NaN, negative ids."""
from pathlib import Path

import numpy as np
import pytest

import fuse_reference as ref

GOLDEN = Path(__file__).resolve().parent / "golden" / "reference_fuse.npz"
DBL_MAX = ref.DBL_MAX


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def test_combined_is_the_reference_loop(golden):
    """prefix, then fill: keep = E < 0.1, A's scores -log(E + 1e-200) (numpy.log is elementwise: the bits are the
    reference's), k_out = A's width; every fixture row fills"""
    g = golden
    e = g["combined_e_values_a"]
    scores_a = -np.log(e + 10**-200)
    hits, scores, source, filled = ref.fuse(g["combined_hits_a"], scores_a, e < 0.1, g["combined_hits_b"], g["combined_scores_b"],
                                            ref.PREFIX_FILL, 0, e.shape[1])
    assert (filled == e.shape[1]).all()
    assert np.array_equal(hits, g["combined_hits"])
    assert np.array_equal(_bits(scores), _bits(g["combined_scores"]))
    kept = (e < 0.1).sum(axis=1)
    assert (kept == 0).any() and (kept == e.shape[1]).any()  # empty prefixes and whole rows of A are in the fixture
    assert ((source[:, -1] >= e.shape[1]) | (kept == e.shape[1])).all()


@pytest.mark.parametrize("name", ["both", "both_uneven"])
def test_both_aligned_is_the_reference_loop(golden, name):
    """sorted union, ascending, k_out = A's width, the reference's own padding (id 0, e-value 10**6)"""
    g = golden
    a, b = g[f"{name}_e_values_a"], g[f"{name}_e_values_b"]
    hits, scores, _, filled = ref.fuse(g[f"{name}_hits_a"], a, None, g[f"{name}_hits_b"], b, ref.SORTED_UNION, 1, a.shape[1])
    assert (filled < a.shape[1]).any() and (filled == a.shape[1]).any()
    assert (hits[np.arange(a.shape[1])[None, :] >= filled[:, None]] == -1).all()
    hits, scores = ref.with_padding(hits, scores, filled, 0, 10**6)
    assert np.array_equal(hits, g[f"{name}_hits"])
    assert np.array_equal(_bits(scores), _bits(g[f"{name}_e_values"]))


def test_fixture_holds_what_float32_cannot_order(golden):
    for name in ("both", "both_uneven"):
        a, b = golden[f"{name}_e_values_a"], golden[f"{name}_e_values_b"]
        tiny = lambda x: ((x > 1e-300) & (x < 1e-46)).sum(axis=1)
        assert ((tiny(a) > 1) & (tiny(b) > 1)).sum() >= 5
        assert (a.astype(np.float32)[(a > 0) & (a < 1e-46)] == 0).all()


# ---- hand-typed rows ----------------------------------------------------------------------------------------------------
def _one(hits_a, scores_a, keep_a, hits_b, scores_b, mode, ascending, k_out):
    out = ref.fuse(np.array([hits_a]), np.array([scores_a], np.float64), None if keep_a is None else np.array([keep_a]),
                   np.array([hits_b]), np.array([scores_b], np.float64), mode, ascending, k_out)
    return out[0][0].tolist(), out[1][0].tolist(), out[2][0].tolist(), int(out[3][0])


def test_ties_across_the_lists_go_by_position():
    a, b = ([5, 6, 7], [1.0, 2.0, 1.0]), ([8, 5, 9], [1.0, 0.5, 2.0])
    # ascending: 0.5 (B's 5), then the 1.0s by position: A's 5 (seen), 7, B's 8, then the 2.0s: 6, 9
    h, s, src, n = _one(a[0], a[1], None, b[0], b[1], ref.SORTED_UNION, 1, 6)
    assert (h, src, n) == ([5, 7, 8, 6, 9, -1], [4, 2, 3, 1, 5, -1], 5) and s == [0.5, 1.0, 1.0, 2.0, 2.0, DBL_MAX]
    # descending: the 2.0s by position, the 1.0s by position, 0.5 (5 was seen)
    h, s, src, n = _one(a[0], a[1], None, b[0], b[1], ref.SORTED_UNION, 0, 6)
    assert (h, src, n) == ([6, 9, 5, 7, 8, -1], [1, 5, 0, 2, 3, -1], 5) and s == [2.0, 2.0, 1.0, 1.0, 1.0, -DBL_MAX]
    h, _, src, n = _one(a[0], a[1], None, b[0], b[1], ref.SORTED_UNION, 0, 2)
    assert (h, src, n) == ([6, 9], [1, 5], 2)


def test_nan_goes_last_and_the_zeros_tie():
    nan = float("nan")
    a, b = ([1, 2, 3], [nan, 1.0, -0.0]), ([4, 5], [0.0, nan])
    h, s, src, n = _one(a[0], a[1], None, b[0], b[1], ref.SORTED_UNION, 1, 5)
    assert (h, src, n) == ([3, 4, 2, 1, 5], [2, 3, 1, 0, 4], 5)
    assert _bits(s[:3]).tolist() == _bits([-0.0, 0.0, 1.0]).tolist() and np.isnan(s[3:]).all()  # the input's bits: -0.0 stays -0.0
    h, s, src, n = _one(a[0], a[1], None, b[0], b[1], ref.SORTED_UNION, 0, 5)
    assert (h, src, n) == ([2, 3, 4, 1, 5], [1, 2, 3, 0, 4], 5)


def test_negative_ids_do_not_exist():
    h, s, src, n = _one([-1, 7, -5], [0.1, 0.2, 0.3], None, [7, -1, 8], [0.05, 0.0, 0.4], ref.SORTED_UNION, 1, 3)
    assert (h, src, n) == ([7, 8, -1], [3, 5, -1], 2) and s == [0.05, 0.4, DBL_MAX]
    # id 0 is an ordinary id (the reference pads with it)
    h, _, src, n = _one([0, 0], [5.0, 5.0], None, [0, 3], [5.0, 1.0], ref.SORTED_UNION, 1, 4)
    assert (h, src, n) == ([3, 0, -1, -1], [3, 0, -1, -1], 2)


def test_prefix_then_fill():
    a = ([3, 4, 3, -1, 6], [0.5, 0.4, 0.3, 0.2, 0.1], [1, 0, 1, 1, 1])
    b = ([4, 3, 9, 9, 6, -2, 10], [7.0, 6.0, 5.0, 4.0, 3.0, 2.0, 1.0])
    # A: 3, 3 (a repeat, kept), 6; the 4 is not kept and is no member; -1 does not exist.  B: 4, 9, 9 (kept), 10
    h, s, src, n = _one(a[0], a[1], a[2], b[0], b[1], ref.PREFIX_FILL, 0, 7)  # full on B's last entry
    assert (h, src, n) == ([3, 3, 6, 4, 9, 9, 10], [0, 2, 4, 5, 7, 8, 11], 7) and s == [0.5, 0.3, 0.1, 7.0, 5.0, 4.0, 1.0]
    h, s, src, n = _one(a[0], a[1], a[2], b[0], b[1], ref.PREFIX_FILL, 0, 9)
    assert (h[7:], src[7:], s[7:], n) == ([-1, -1], [-1, -1], [-DBL_MAX] * 2, 7)
    assert _one(a[0], a[1], a[2], b[0], b[1], ref.PREFIX_FILL, 1, 9)[1][7:] == [DBL_MAX] * 2  # ascending chooses the padding only
    assert _one(a[0], a[1], a[2], b[0], b[1], ref.PREFIX_FILL, 0, 2)[0] == [3, 3]
    # no keep array: every non-negative entry of A is kept, and the 4 is a member now
    h, _, src, n = _one(a[0], a[1], None, b[0], b[1], ref.PREFIX_FILL, 0, 12)
    assert (h[:n], src[:n]) == ([3, 4, 3, 6, 9, 9, 10], [0, 1, 2, 4, 7, 8, 11])
