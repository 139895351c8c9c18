"""CPU: tests/assemble_reference.py (the restatement the GPU tests compare knn_eval_assemble with) against outputs typed
in by hand, and the grouping tables the Python facade builds from protein names.  Only the case whose scores are all
distinct is also compared with the reference's bare argsort(-scores) loop: that loop leaves the order of equal scores,
of the two zeros and of NaNs open."""
import numpy as np
import pytest

import assemble_reference as ref

FMAX = float(np.finfo(np.float32).max)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _run(hits, scores, row_group, depth, k_out, ascending=False, offsets=None, self_group=None):
    hits = np.asarray(hits, np.int64)
    scores = np.asarray(scores, np.float32)
    offsets = [0, hits.shape[0]] if offsets is None else offsets
    return ref.assemble(hits, scores, offsets, row_group, self_group, depth, k_out, ascending)


def _expect(got, groups, scores, qrow, hit):
    assert got[0].tolist() == groups
    assert np.array_equal(_bits(got[1]), _bits(np.asarray(scores, np.float32)))
    assert got[2].tolist() == qrow
    assert got[3].tolist() == hit


IDENT = list(range(6))


def test_tie_goes_to_the_smaller_position():
    got = _run([[0, 1, 2], [3, 4, 5]], [[5, 7, 5], [7, 1, 5]], IDENT, 6, 6)
    _expect(got, [[1, 3, 0, 2, 5, 4]], [[7, 7, 5, 5, 5, 1]], [[0, 1, 0, 0, 1, 1]], [[1, 3, 0, 2, 5, 4]])
    got = _run([[0, 1, 2], [3, 4, 5]], [[5, 7, 5], [7, 1, 5]], IDENT, 6, 6, ascending=True)
    _expect(got, [[4, 0, 2, 5, 1, 3]], [[1, 5, 5, 5, 7, 7]], [[1, 0, 0, 1, 0, 1]], [[4, 0, 2, 5, 1, 3]])


def test_the_two_zeros_are_equal():
    """raw orderable bits would put +0.0 in front of -0.0 (descending) whatever their positions"""
    got = _run([[2, 1, 0]], [[-0.0, 0.0, 1.0]], IDENT, 3, 3)
    _expect(got, [[0, 2, 1]], [[1.0, -0.0, 0.0]], [[0, 0, 0]], [[0, 2, 1]])
    got = _run([[2, 1, 0]], [[0.0, -0.0, 1.0]], IDENT, 3, 3)
    _expect(got, [[0, 2, 1]], [[1.0, 0.0, -0.0]], [[0, 0, 0]], [[0, 2, 1]])
    got = _run([[2, 1, 0]], [[0.0, -0.0, -1.0]], IDENT, 3, 3, ascending=True)
    _expect(got, [[0, 2, 1]], [[-1.0, 0.0, -0.0]], [[0, 0, 0]], [[0, 2, 1]])


def test_nan_comes_last_in_both_directions():
    nan = float("nan")
    got = _run([[0, 1, 2, 3]], [[nan, 2.0, nan, 3.0]], IDENT, 4, 4)
    _expect(got, [[3, 1, 0, 2]], [[3.0, 2.0, nan, nan]], [[0] * 4], [[3, 1, 0, 2]])
    got = _run([[0, 1, 2, 3]], [[nan, 2.0, nan, 3.0]], IDENT, 4, 4, ascending=True)
    _expect(got, [[1, 3, 0, 2]], [[2.0, 3.0, nan, nan]], [[0] * 4], [[1, 3, 0, 2]])
    # cut in front of the NaNs: they are never looked at
    got = _run([[0, 1, 2, 3]], [[nan, 2.0, nan, 3.0]], IDENT, 2, 2)
    _expect(got, [[3, 1]], [[3.0, 2.0]], [[0, 0]], [[3, 1]])


def test_a_hit_outside_the_table_keeps_its_place_but_names_no_group():
    """depth 3: -1 and 7 take two of the three places, the hit behind them is not looked at"""
    got = _run([[-1, 0, 7, 1]], [[9, 8, 7, 6]], IDENT, 3, 2)
    _expect(got, [[0, -1]], [[8, -FMAX]], [[0, -1]], [[0, -1]])
    got = _run([[-1, 0, 7, 1]], [[9, 8, 7, 6]], IDENT, 4, 2)
    _expect(got, [[0, 1]], [[8, 6]], [[0, 0]], [[0, 1]])


def test_a_protein_is_emitted_once():
    got = _run([[0, 2, 1], [3, 4, 5]], [[9, 8, 7], [6, 5, 4]], [0, 0, 1, 1, 2, 2], 6, 6)
    _expect(got, [[0, 1, 2, -1, -1, -1]], [[9, 8, 5, -FMAX, -FMAX, -FMAX]], [[0, 0, 1, -1, -1, -1]], [[0, 2, 4, -1, -1, -1]])
    # k_out 2: the walk stops there
    got = _run([[0, 2, 1], [3, 4, 5]], [[9, 8, 7], [6, 5, 4]], [0, 0, 1, 1, 2, 2], 6, 2)
    _expect(got, [[0, 1]], [[9, 8]], [[0, 0]], [[0, 2]])


def test_group_shorter_than_depth_and_empty_groups():
    got = _run([[4, 5, 3], [0, 0, 0]], [[1, 3, 2], [4, 4, 4]], IDENT, 10, 4, offsets=[0, 0, 1, 1, 2, 2])
    _expect(got,
            [[-1] * 4, [5, 3, 4, -1], [-1] * 4, [0, -1, -1, -1], [-1] * 4],
            [[-FMAX] * 4, [3, 2, 1, -FMAX], [-FMAX] * 4, [4, -FMAX, -FMAX, -FMAX], [-FMAX] * 4],
            [[-1] * 4, [0, 0, 0, -1], [-1] * 4, [1, -1, -1, -1], [-1] * 4],
            [[-1] * 4, [5, 3, 4, -1], [-1] * 4, [0, -1, -1, -1], [-1] * 4])
    got = _run([[4, 5, 3]], [[1, 3, 2]], IDENT, 10, 2, ascending=True, offsets=[0, 0, 1])
    _expect(got, [[-1, -1], [4, 3]], [[FMAX, FMAX], [1, 2]], [[-1, -1], [0, 0]], [[-1, -1], [4, 3]])


def test_excluded_self_entries_count_toward_depth():
    got = _run([[0, 1, 2, 3]], [[9, 8, 7, 6]], [0, 0, 1, 2], 3, 2, self_group=[0])
    _expect(got, [[1, -1]], [[7, -FMAX]], [[0, -1]], [[2, -1]])
    got = _run([[0, 1, 2, 3]], [[9, 8, 7, 6]], [0, 0, 1, 2], 3, 2, self_group=[-1])
    _expect(got, [[0, 1]], [[9, 7]], [[0, 0]], [[0, 2]])


def test_distinct_scores_match_the_bare_argsort_loop():
    rng = np.random.default_rng(1)
    ns, k, nb = 17, 9, 40
    hits = rng.integers(0, nb, (ns, k)).astype(np.int64)
    scores = rng.permutation(ns * k).astype(np.float32).reshape(ns, k) - 60.0
    row_group = rng.integers(0, 12, nb).astype(np.int32)
    offsets = [0, 1, 1, 6, 8, 17]
    got = ref.assemble(hits, scores, offsets, row_group, None, k, k, False)
    want = ref.bare_reference(hits, scores, offsets, row_group, k)
    assert (want >= 0).sum() > 20 and (want < 0).any()
    assert np.array_equal(got[0], want)


# ---- the facade's grouping ------------------------------------------------------------------------------------------------
def test_runs_become_query_groups_and_database_ids_go_by_name():
    from knn_for_homology_amd.evaluation import assemble_grouping
    offsets, names, row_group, self_group, id_to_name = assemble_grouping(["a", "a", "b", "a", "c"])
    assert offsets.dtype == np.int64 and offsets.tolist() == [0, 2, 3, 4, 5]
    assert names == ["a", "b", "a", "c"]  # "a" comes back: two query groups ...
    assert row_group.dtype == np.int32 and row_group.tolist() == [0, 0, 1, 0, 2]  # ... with one database id
    assert self_group.dtype == np.int32 and self_group.tolist() == [0, 1, 0, 2]
    assert id_to_name == ["a", "b", "c"]


def test_a_database_of_its_own():
    from knn_for_homology_amd.evaluation import assemble_grouping
    offsets, names, row_group, self_group, id_to_name = assemble_grouping(["a", "b", "b"], ["x", "a", "x", "y"])
    assert offsets.tolist() == [0, 1, 3] and names == ["a", "b"]
    assert row_group.tolist() == [0, 1, 0, 2] and id_to_name == ["x", "a", "y"]
    assert self_group.tolist() == [1, -1]
    offsets, names, row_group, self_group, id_to_name = assemble_grouping([])
    assert offsets.tolist() == [0] and names == [] and row_group.size == 0 and self_group.size == 0 and id_to_name == []


def test_wrapper_refuses_wrong_shapes_before_the_library_is_called():
    from knn_for_homology_amd.evaluation import assemble
    hits = np.zeros((3, 4), np.int64)
    with pytest.raises(ValueError, match="same shape"):
        assemble(hits, np.zeros((3, 3), np.float32), ["a", "a", "b"])
    with pytest.raises(ValueError, match="slice_proteins"):
        assemble(hits, np.zeros((3, 4), np.float32), ["a", "b"])
    with pytest.raises(ValueError, match="2-D"):
        assemble(hits.ravel(), np.zeros(12, np.float32), ["a"] * 12)
