"""CPU: tests/slices_eval_reference.py (the restatement the GPU tests compare knn_eval_slice_annotate and knn_eval_slices
with) against tests/golden/reference_slices_eval.npz, which holds what the reference's own statements
(pfam/slices/slices.py:49-80 and evaluate) produced from the inputs stored next to them
(tests/golden/make_slices_eval_golden.py); and the integer tables slice_tables builds on the host, with the library call
replaced by the restatement.  Integers are compared with array_equal, auc1s as float64 bit patterns."""
from pathlib import Path

import numpy as np
import pytest

import slices_eval_reference as ref

GOLDEN = Path(__file__).resolve().parent / "golden" / "reference_slices_eval.npz"


@pytest.fixture(scope="module")
def golden():
    g = np.load(GOLDEN)
    slices = [(str(p), (int(a), int(b))) for p, a, b in zip(g["slice_protein"], g["slice_start"], g["slice_stop"])]
    protein_to_domain = {str(p): [] for p in g["protein_names"]}
    for p, f, a, b in zip(g["domain_protein"], g["domain_pfam"], g["domain_start"], g["domain_stop"]):
        protein_to_domain[str(p)].append((str(f), (int(a), int(b))))
    return g, slices, protein_to_domain


def _sets(slice_index, family, n):
    out = [set() for _ in range(n)]
    for s, f in zip(slice_index, family):
        out[int(s)].add(str(f))
    return out


def _array(ptr, dtype, n):
    """the n values of a C array argument (None or an address)"""
    if not n:
        return np.zeros(0, dtype)
    ctype = np.ctypeslib.as_ctypes_type(dtype)
    return np.ctypeslib.as_array((ctype * n).from_address(ptr))


class _Stub:
    """stands in for the library: knn_eval_slice_annotate answered by the restatement, through the C arguments"""

    def knn_eval_slice_annotate(self, sp, s0, s1, ns, off, fam, d0, d1, np_, nfam, match_count, annotation, family_sizes):
        offsets = _array(off, np.int64, np_ + 1)
        nd = int(offsets[-1])
        self.tables = tuple(a.copy() for a in (_array(sp, np.int32, ns), _array(s0, np.int32, ns), _array(s1, np.int32, ns), offsets,
                                               _array(fam, np.int32, nd), _array(d0, np.int32, nd), _array(d1, np.int32, nd)))
        self.nfam = nfam
        mc, an, fs = ref.annotate(*self.tables, nfam)
        _array(match_count, np.int32, ns)[:] = mc
        _array(annotation, np.int32, ns)[:] = an
        _array(family_sizes, np.int64, nfam)[:] = fs
        return 0


@pytest.fixture
def stubbed(monkeypatch):
    from knn_for_homology_amd import _lib
    stub = _Stub()
    monkeypatch.setattr(_lib, "lib", lambda: stub)
    return stub


def test_slice_tables_equal_the_references_sets(golden, stubbed):
    from knn_for_homology_amd.evaluation import slice_tables
    g, slices, protein_to_domain = golden
    t = slice_tables(slices, protein_to_domain)
    ns = len(slices)
    # dense codes: every code in [0, nfam) is used, the names are distinct
    assert len(set(t.families)) == len(t.families) == stubbed.nfam
    assert set(t.domain_family.tolist()) == set(range(len(t.families)))
    assert t.domain_family.dtype == np.int32 and t.domain_offsets.dtype == np.int64 and t.slice_protein.dtype == np.int32
    for p in range(len(t.proteins)):
        run = t.domain_family[t.domain_offsets[p]:t.domain_offsets[p + 1]]
        assert (np.diff(run) >= 0).all()
        assert len(run) == len(protein_to_domain[t.proteins[p]])
    assert [t.proteins[p] for p in t.slice_protein] == [s[0] for s in slices]
    # the sets, by name
    matching, intersecting = ref.slice_sets(t.slice_protein, t.slice_start, t.slice_stop, t.domain_offsets, t.domain_family,
                                            t.domain_start, t.domain_stop)
    named = lambda sets: [{t.families[f] for f in s} for s in sets]
    assert named(matching) == _sets(g["matching_slice"], g["matching_family"], ns)
    assert named(intersecting) == _sets(g["intersecting_slice"], g["intersecting_family"], ns)
    assert any(m & i for m, i in zip(matching, intersecting))
    # what slices.py:70-80 made of them
    assert t.has_annotation.dtype == np.bool_ and np.array_equal(t.has_annotation, g["has_annotation"])
    assert [t.families[a] for a in t.annotation[t.has_annotation]] == [str(f) for f in g["annotated"]]
    assert (t.annotation[~t.has_annotation] == -1).all()
    assert np.array_equal(t.match_count, [len(m) for m in matching])
    sizes = dict(zip((str(f) for f in g["family_size_names"]), g["family_size_counts"].tolist()))
    assert {f: int(c) for f, c in zip(t.families, t.family_sizes) if c} == sizes
    assert t.family_sizes.dtype == np.int64


@pytest.mark.parametrize("flag, tag", [(False, "plain"), (True, "ignore_unannotated")])
def test_restatement_equals_the_reference(golden, stubbed, flag, tag):
    from knn_for_homology_amd.evaluation import slice_tables
    g, slices, protein_to_domain = golden
    t = slice_tables(slices, protein_to_domain)
    rows = np.flatnonzero(t.has_annotation)
    is_correct, is_ignore, lead, tp, columns = ref.evaluate(g["hits"], t.annotation[rows], *stubbed.tables, flag)
    assert np.array_equal(is_correct.astype(bool), g[f"is_correct_{tag}"])
    assert np.array_equal(is_ignore.astype(bool), g[f"is_ignore_{tag}"])
    auc1s = lead / t.family_sizes[t.annotation[rows]]
    assert auc1s.dtype == np.float64 and np.array_equal(auc1s.view(np.uint64), g[f"auc1s_{tag}"].view(np.uint64))
    assert np.array_equal(tp, g[f"is_correct_{tag}"].sum(axis=1))
    assert np.array_equal(columns, g[f"is_correct_{tag}"].sum(axis=0))


def test_a_missing_protein_has_no_domains(stubbed):
    from knn_for_homology_amd.evaluation import slice_tables
    slices = [("a", (0, 10)), ("nowhere", (0, 10)), ("b", (0, 10)), ("a", (5, 15))]
    t = slice_tables(slices, {"a": [("Y", (6, 9)), ("X", (1, 3)), ("Y", (0, 2))], "b": [], "unused": [("Z", (0, 1))]})
    assert t.slice_protein.tolist() == [0, -1, 1, 0] and t.proteins == ["a", "b"]
    assert t.families == ["X", "Y"]  # "Z" belongs to no slice's protein: codes stay dense
    assert t.domain_offsets.tolist() == [0, 3, 3]
    assert t.domain_family.tolist() == [0, 1, 1] and t.domain_start.tolist() == [1, 6, 0] and t.domain_stop.tolist() == [3, 9, 2]
    assert t.match_count.tolist() == [2, 0, 0, 1] and t.annotation.tolist() == [-1, -1, -1, 1]
    assert t.has_annotation.tolist() == [False, False, False, True] and t.family_sizes.tolist() == [1, 2]


def test_boundaries_of_the_interval_tests():
    """one slice [10, 20) against domains that touch its ends from either side"""
    def sets(d0, d1):
        m, i = ref.slice_sets([0], [10], [20], [0, 1], [0], [d0], [d1])
        return bool(m[0]), bool(i[0])
    assert sets(10, 20) == (True, False)   # both ends equal: inside
    assert sets(10, 21) == (False, True)
    assert sets(9, 20) == (False, True)
    assert sets(0, 10) == (False, False)   # domain_stop == slice_start: apart
    assert sets(20, 30) == (False, False)  # domain_start == slice_stop: apart
    assert sets(0, 11) == (False, True) and sets(19, 30) == (False, True)


def test_wrapper_refuses_wrong_shapes_before_the_library_is_called(stubbed):
    from knn_for_homology_amd.evaluation import evaluate_slices, slice_tables
    t = slice_tables([("a", (0, 10)), ("a", (5, 15))], {"a": [("X", (1, 3))]})
    with pytest.raises(ValueError, match="2-D"):
        evaluate_slices(np.zeros(4, np.int64), t)
    with pytest.raises(ValueError, match="query_rows"):
        evaluate_slices(np.zeros((2, 4), np.int64), t)  # one annotated slice, two rows
    with pytest.raises(ValueError, match="query_rows"):
        evaluate_slices(np.zeros((1, 4), np.int64), t, query_rows=[2])
