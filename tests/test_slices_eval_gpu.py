"""GPU: knn_eval_slice_annotate and knn_eval_slices (csrc/slices_eval.inc) against tests/slices_eval_reference.py.

slice_eval_kernel gives one wave to a row of hits, four rows to a workgroup, and walks the row 64 hits at a time; per hit
it loads the hit slice's record, searches the protein's sorted domains for the query's family and tests that family's
run of domains; ballots give the leading run, which is carried from chunk to chunk.  slice_annotate_kernel gives one
thread to a slice and counts a family at the first inside domain of its run.  The shapes here sit where that can go
wrong: k around one and two chunks, the first stop hit in the last lane of a chunk, the first lane of the next and
nowhere, row counts around a workgroup, proteins from no domain to 570, the query's family at either end of a protein's
range and absent from it, ids outside every table, rows cut into slabs.  Integers are compared with array_equal, auc1s
as float64 bit patterns; there is no tolerance anywhere."""
from pathlib import Path

import numpy as np
import pytest

import slices_eval_reference as ref

pytestmark = pytest.mark.gpu

KNOB = "KNN355_EVAL_SLAB_ROWS"
KNN_ERR_INVALID = -1
S32, S64, S8 = -7777, -7777, 0xAB  # what the output arrays hold before a call
GOLDEN = Path(__file__).resolve().parent / "golden" / "reference_slices_eval.npz"
TABLE = ("sp", "s0", "s1", "off", "fam", "d0", "d1")


def _ptr(a):
    return None if a is None or a.size == 0 else a.ctypes.data


def _last_error():
    from knn_for_homology_amd import _lib
    return _lib.lib().knn_last_error().decode()


def _table_args(tables):
    a = {name: np.ascontiguousarray(t, np.int64 if name == "off" else np.int32) for name, t in zip(TABLE, tables)}
    a.update(ns=len(a["sp"]), np=len(a["off"]) - 1)
    return a


def c_annotate(tables, nf, **over):
    """the C entry point -> (return code, match_count, annotation, family_sizes), the outputs pre-filled with the
    sentinels; `over` replaces arguments by name (ns, np, nfam) or drops a pointer (sp=None ...)"""
    from knn_for_homology_amd import _lib
    a = _table_args(tables)
    ns = a["ns"]
    a.update(nfam=nf, mc=np.full(max(ns, 1), S32, np.int32), an=np.full(max(ns, 1), S32, np.int32), fs=np.full(max(nf, 1), S64, np.int64))
    out = (a["mc"], a["an"], a["fs"])
    a.update(over)
    rc = _lib.lib().knn_eval_slice_annotate(_ptr(a["sp"]), _ptr(a["s0"]), _ptr(a["s1"]), a["ns"], _ptr(a["off"]), _ptr(a["fam"]), _ptr(a["d0"]),
                                            _ptr(a["d1"]), a["np"], a["nfam"], _ptr(a["mc"]), _ptr(a["an"]), _ptr(a["fs"]))
    return rc, out[0][:ns], out[1][:ns], out[2][:nf]


def c_slices(hits_, query_family, tables, nf, match_count, flag, columns=True, **over):
    """-> (return code, is_correct, is_ignore, lead, tp, column_correct or None)"""
    from knn_for_homology_amd import _lib
    hits = np.ascontiguousarray(hits_, np.int64)
    nq, k = hits.shape
    a = _table_args(tables)
    a.update(hits=hits, nq=nq, k=k, qf=np.ascontiguousarray(query_family, np.int32), nfam=nf,
             mc=None if match_count is None else np.ascontiguousarray(match_count, np.int32),
             ic=np.full((max(nq, 1), k), S8, np.uint8), ig=np.full((max(nq, 1), k), S8, np.uint8),
             lead=np.full(max(nq, 1), S32, np.int32), tp=np.full(max(nq, 1), S32, np.int32),
             cc=np.full(k, S64, np.int64) if columns else None)
    out = (a["ic"], a["ig"], a["lead"], a["tp"], a["cc"])
    a.update(over)
    rc = _lib.lib().knn_eval_slices(_ptr(a["hits"]), a["nq"], a["k"], _ptr(a["qf"]), _ptr(a["sp"]), _ptr(a["s0"]), _ptr(a["s1"]), a["ns"],
                                    _ptr(a["off"]), _ptr(a["fam"]), _ptr(a["d0"]), _ptr(a["d1"]), a["np"], a["nfam"], _ptr(a["mc"]),
                                    1 if flag else 0, _ptr(a["ic"]), _ptr(a["ig"]), _ptr(a["lead"]), _ptr(a["tp"]), _ptr(a["cc"]))
    return rc, out[0][:nq], out[1][:nq], out[2][:nq], out[3][:nq], out[4]


def _same(got, want):
    rc, ic, ig, lead, tp, cc = got
    assert rc == 0, _last_error()
    assert np.array_equal(ic, want[0]), "is_correct"
    assert np.array_equal(ig, want[1]), "is_ignore"
    assert np.array_equal(lead, want[2]), "lead"
    assert np.array_equal(tp, want[3]), "tp"
    if cc is not None:
        assert np.array_equal(cc, want[4]), "column_correct"


def _check(hits, query_family, tables, nfam, flag, want=None):
    """the call against the restatement, with match_count as the restatement's annotate gives it"""
    match_count = ref.annotate(*tables, nfam)[0]
    want = ref.evaluate(hits, query_family, *tables, flag) if want is None else want
    _same(c_slices(hits, query_family, tables, nfam, match_count, flag), want)
    return want


def _tables(rng, counts, nfam, ns, families=None):
    """protein p has counts[p] domains with sorted, repeating family codes; every coordinate is a multiple of 10, so
    that slice and domain ends coincide often; slices name a protein from [-1, np)"""
    counts = np.asarray(counts, np.int64)
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    fam = [np.sort(rng.integers(0, nfam, c)) for c in counts] if families is None else families
    fam = np.concatenate(fam + [np.zeros(0, np.int64)]).astype(np.int32)
    d0 = (10 * rng.integers(0, 30, len(fam))).astype(np.int32)
    d1 = (d0 + 10 * rng.integers(1, 8, len(fam))).astype(np.int32)
    sp = rng.integers(-1, len(counts), ns).astype(np.int32)
    s0 = (10 * rng.integers(0, 30, ns)).astype(np.int32)
    s1 = (s0 + 10 * rng.integers(1, 14, ns)).astype(np.int32)
    return sp, s0, s1, off, fam, d0, d1


def _case(rng, nq, k, counts=(3, 0, 7, 1, 12), nfam=6, ns=150):
    tables = _tables(rng, counts, nfam, ns)
    hits = rng.integers(-2, ns + 2, (nq, k)).astype(np.int64)
    query_family = rng.integers(-1, nfam, nq).astype(np.int32)
    return hits, query_family, tables


# one protein; family 1 lies inside slice 0 and across the left end of slice 1; slice 2 holds family 0 and nothing of
# family 1 (a stop hit with and without the flag); slice 3 has no protein
C, I, X, U = 0, 1, 2, 3
SMALL = (np.array([0, 0, 0, -1], np.int32), np.array([0, 15, 60, 0], np.int32), np.array([30, 30, 70, 30], np.int32),
         np.array([0, 3], np.int64), np.array([0, 1, 1], np.int32), np.array([62, 10, 35], np.int32), np.array([68, 20, 50], np.int32))


# ---- the run across chunks ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 63, 64, 65, 128, 129, 300])
def test_first_stop_around_the_chunk_boundaries(gpu_faiss, k):
    """one row per position of the first stop hit (and one without any); hits 62 .. 66 are ignored ones, straddling the
    first chunk boundary; behind the stop everything is mixed"""
    rng = np.random.default_rng(k)
    stops = [p for p in (0, 1, 62, 63, 64, 65, 66, 67, 127, 128, 129, 191, 192, 255, 256, k - 1) if p < k] + [None]
    hits = np.full((len(stops), k), C, np.int64)
    hits[:, 62:67] = I
    want_lead = []
    for r, p in enumerate(stops):
        if p is not None:
            hits[r, p] = X
            hits[r, p + 1:] = rng.integers(0, 4, k - p - 1)
        want_lead.append(int((hits[r, :k if p is None else p] == C).sum()))
    query_family = np.ones(len(stops), np.int32)
    for flag in (False, True):
        want = _check(hits, query_family, SMALL, 2, flag)
        assert want[2].tolist() == want_lead
    # the unannotated slice ends a run only without the flag
    rows = [r for r, p in enumerate(stops) if p != 0]  # (their hit 0 was a correct one)
    hits[rows, 0] = U
    assert not _check(hits, query_family, SMALL, 2, False)[2][rows].any()
    want = _check(hits, query_family, SMALL, 2, True)
    assert want[2][rows].tolist() == [want_lead[r] - 1 for r in rows]


@pytest.mark.parametrize("nq", [1, 3, 4, 5, 257])
def test_row_counts_around_a_workgroup(gpu_faiss, nq):
    hits, query_family, tables = _case(np.random.default_rng(nq), nq, 70)
    for flag in (False, True):
        want = _check(hits, query_family, tables, 6, flag)
    assert want[0].sum() > 0 or nq < 3


# ---- the search in a protein's domains --------------------------------------------------------------------------------------
def test_proteins_from_no_domain_to_570(gpu_faiss):
    """proteins with 0, 1, 65 and 570 domains; the 65 hold the families 1..4 and 6..10, so 0 lies in front of the range,
    11 behind it, 5 inside it and absent; 1 and 10 are its first and last run; the 570 are one family"""
    rng = np.random.default_rng(570)
    nfam = 12
    f65 = np.sort(rng.choice([1, 2, 3, 4, 6, 7, 8, 9, 10], 65))
    f65[0], f65[-1] = 1, 10
    tables = _tables(rng, [0, 1, 65, 570], nfam, 400, families=[np.zeros(0, np.int64), np.array([7]), f65, np.full(570, 3)])
    ns = 400
    hits = rng.integers(0, ns, (2 * nfam + 2, 130)).astype(np.int64)
    query_family = np.concatenate([np.arange(nfam), np.arange(nfam), [-1, 3]]).astype(np.int32)
    for flag in (False, True):
        want = _check(hits, query_family, tables, nfam, flag)
    assert want[0][[1, 10, 3, 7]].sum(axis=1).min() > 0 and want[0][[0, 5, 11]].sum() == 0
    rc, mc, an, fs = c_annotate(tables, nfam)
    wmc, wan, wfs = ref.annotate(*tables, nfam)
    assert rc == 0 and np.array_equal(mc, wmc) and np.array_equal(an, wan) and np.array_equal(fs, wfs)
    assert mc[tables[0] == 3].max() == 1 and {0, 1, 2} <= set(mc.tolist())
    # one slice over all 570 domains of the one family: it counts once
    sp, s0, s1, off, fam, d0, d1 = tables
    one = (np.array([3], np.int32), np.array([0], np.int32), np.array([1000], np.int32), off, fam, d0, d1)
    rc, mc, an, fs = c_annotate(one, nfam)
    assert rc == 0 and mc.tolist() == [1] and an.tolist() == [3] and fs.tolist() == [0, 0, 0, 1] + [0] * 8


def test_a_family_both_matching_and_intersecting(gpu_faiss):
    """slice [0, 30): family 1 has a domain inside and one across the right end: the hit is correct and ignored"""
    tables = (np.array([0], np.int32), np.array([0], np.int32), np.array([30], np.int32), np.array([0, 3], np.int64),
              np.array([0, 1, 1], np.int32), np.array([25, 10, 25], np.int32), np.array([40, 20, 35], np.int32))
    got = c_slices([[0, 0]], [1], tables, 2, None, False)
    assert got[0] == 0 and got[1].tolist() == [[1, 1]] and got[2].tolist() == [[1, 1]] and got[3].tolist() == [2] and got[4].tolist() == [2]
    got = c_slices([[0, 0]], [0], tables, 2, None, False)  # family 0 only intersects
    assert got[1].tolist() == [[0, 0]] and got[2].tolist() == [[1, 1]] and got[3].tolist() == [0]


# ---- ids outside the tables -------------------------------------------------------------------------------------------------
def test_ids_outside_the_tables(gpu_faiss):
    rng = np.random.default_rng(11)
    hits, query_family, tables = _case(rng, 9, 66)
    ns = len(tables[0])
    hits[:, :6] = [-1, -2, ns, ns + 1, -2**63, 2**32 + 1]  # (2^32 + 1 is not slice 1)
    query_family[4] = -1
    assert (tables[0] == -1).any()
    for flag in (False, True):
        want = _check(hits, query_family, tables, 6, flag)
        assert not want[0][:, :6].any() and not want[1][:, :6].any() and not want[2].any()
        assert not want[0][4].any() and not want[1][4].any() and want[3][4] == 0
    # the flag off: match_count is not looked at and may be missing; column_correct may be missing
    want = ref.evaluate(hits, query_family, *tables, False)
    _same(c_slices(hits, query_family, tables, 6, None, False), want)
    _same(c_slices(hits, query_family, tables, 6, np.full(ns, 0, np.int32), False, columns=False), want)


# ---- slabs ------------------------------------------------------------------------------------------------------------------
def test_slabs(gpu_faiss, monkeypatch):
    """100 rows, 23 per slab: four full slabs and one of 8; column_correct is the sum over the slabs"""
    hits, query_family, tables = _case(np.random.default_rng(23), 100, 67)
    match_count = ref.annotate(*tables, 6)[0]
    want = ref.evaluate(hits, query_family, *tables, True)
    monkeypatch.delenv(KNOB, raising=False)
    whole = c_slices(hits, query_family, tables, 6, match_count, True)
    monkeypatch.setenv(KNOB, "23")
    cut = c_slices(hits, query_family, tables, 6, match_count, True)
    _same(whole, want)
    _same(cut, want)
    assert want[4].sum() == want[3].sum() > 0
    _same(c_slices(hits, query_family, tables, 6, match_count, True, columns=False), want)


@pytest.mark.parametrize("k", [3, 65])
def test_optional_columns_across_slabs(gpu_faiss, monkeypatch, k):
    """5 rows in slabs of 2: match_count (the flag off) and column_correct, each present and absent"""
    hits, query_family, tables = _case(np.random.default_rng(230 + k), 5, k)
    match_count = ref.annotate(*tables, 6)[0]
    want = ref.evaluate(hits, query_family, *tables, False)
    monkeypatch.setenv(KNOB, "2")
    for mc in (match_count, None):
        for columns in (True, False):
            _same(c_slices(hits, query_family, tables, 6, mc, False, columns=columns), want)


# ---- annotate ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ns", [1, 255, 256, 257])
def test_annotate_slice_counts(gpu_faiss, ns):
    tables = _tables(np.random.default_rng(ns), (3, 0, 7, 1, 12), 6, ns)
    rc, mc, an, fs = c_annotate(tables, 6)
    wmc, wan, wfs = ref.annotate(*tables, 6)
    assert rc == 0, _last_error()
    assert np.array_equal(mc, wmc) and np.array_equal(an, wan) and np.array_equal(fs, wfs)


def test_annotate_many_slices_of_one_family(gpu_faiss):
    """20 000 slices hold family 2 (and every third of them family 4 as well): the atomics of whole waves meet on one word"""
    ns = 20001
    sp = np.zeros(ns, np.int32)
    s0 = np.zeros(ns, np.int32)
    s1 = np.where(np.arange(ns) % 3 == 0, 60, 30).astype(np.int32)
    s1[-1] = 5  # the last slice holds nothing
    tables = (sp, s0, s1, np.array([0, 3], np.int64), np.array([2, 2, 4], np.int32), np.array([10, 12, 40], np.int32), np.array([20, 22, 50], np.int32))
    rc, mc, an, fs = c_annotate(tables, 5)
    assert rc == 0, _last_error()
    assert fs.tolist() == [0, 0, 20000, 0, 6667]
    assert np.array_equal(mc[:-1], np.where(np.arange(ns - 1) % 3 == 0, 2, 1)) and mc[-1] == 0
    assert np.array_equal(an[:-1], np.where(np.arange(ns - 1) % 3 == 0, -1, 2)) and an[-1] == -1


# ---- errors: refused on the host, nothing allocated or launched, the outputs as they were -------------------------------
def _refused_annotate(got, what):
    rc, mc, an, fs = got
    assert rc == KNN_ERR_INVALID and what in _last_error(), _last_error()
    assert (mc == S32).all() and (an == S32).all() and (fs == S64).all()


def _refused_slices(got, what):
    rc, ic, ig, lead, tp, cc = got
    assert rc == KNN_ERR_INVALID and what in _last_error(), _last_error()
    assert (ic == S8).all() and (ig == S8).all() and (lead == S32).all() and (tp == S32).all() and (cc == S64).all()


BAD_TABLES = [
    (dict(off=np.array([-1, 1, 3], np.int64)), "negative domain offset"),
    (dict(off=np.array([0, 2, 1], np.int64)), "domain offsets decrease"),
    (dict(off=np.array([1, 0, 3], np.int64)), "domain offsets decrease"),
    (dict(fam=np.array([0, 4, 1], np.int32)), "domain family outside"),
    (dict(fam=np.array([0, -1, 1], np.int32)), "domain family outside"),
    (dict(fam=np.array([0, 2, 1], np.int32)), "not sorted"),
    (dict(sp=np.array([0, 2, -1], np.int32)), "slice protein outside"),
    (dict(sp=np.array([0, -2, -1], np.int32)), "slice protein outside"),
]
# three slices, two proteins of one and two domains, four families
GOOD = (np.array([0, 1, -1], np.int32), np.array([0, 0, 0], np.int32), np.array([50, 50, 50], np.int32),
        np.array([0, 1, 3], np.int64), np.array([3, 1, 2], np.int32), np.array([10, 10, 20], np.int32), np.array([20, 20, 60], np.int32))


def test_annotate_refusals(gpu_faiss):
    for name in ("ns", "np", "nfam"):
        _refused_annotate(c_annotate(GOOD, 4, **{name: -1}), "negative")
    for name in TABLE + ("mc", "an", "fs"):
        _refused_annotate(c_annotate(GOOD, 4, **{name: None}), "null pointer")
    for over, what in BAD_TABLES:
        _refused_annotate(c_annotate(GOOD, 4, **over), what)
    _refused_annotate(c_annotate(GOOD, 4, np=2**31), "np > INT32_MAX")
    rc, mc, an, fs = c_annotate(GOOD, 4)
    assert rc == 0 and mc.tolist() == [1, 1, 0] and an.tolist() == [3, 1, -1] and fs.tolist() == [0, 1, 0, 1]


def test_slices_refusals(gpu_faiss):
    hits = np.zeros((5, 4), np.int64)
    qf = np.array([0, 1, 2, 3, -1], np.int32)
    mc = np.array([1, 1, 0], np.int32)
    for name in ("nq", "ns", "np", "nfam"):
        _refused_slices(c_slices(hits, qf, GOOD, 4, mc, True, **{name: -1}), "negative")
    _refused_slices(c_slices(hits, qf, GOOD, 4, mc, True, k=0), "k >= 1")
    _refused_slices(c_slices(hits, qf, GOOD, 4, mc, True, k=-3), "k >= 1")
    _refused_slices(c_slices(hits, qf, GOOD, 4, mc, True, k=2**31), "k > INT32_MAX")
    for name in TABLE + ("hits", "qf", "mc", "ic", "ig", "lead", "tp"):  # (an output left out keeps its sentinels: it was never passed)
        _refused_slices(c_slices(hits, qf, GOOD, 4, mc, True, **{name: None}), "null pointer")
    _refused_slices(c_slices(hits, [0, 1, 2, 4, -1], GOOD, 4, mc, True), "query family")
    for over, what in BAD_TABLES:
        _refused_slices(c_slices(hits, qf, GOOD, 4, mc, True, **over), what)
    # and the same arguments pass once they are right
    got = c_slices(hits, qf, GOOD, 4, mc, True)
    assert got[0] == 0, _last_error()
    assert got[1].tolist() == [[0] * 4, [0] * 4, [0] * 4, [1] * 4, [0] * 4] and got[3].tolist() == [0, 0, 0, 4, 0]
    assert got[5].tolist() == [1] * 4


def test_empty_calls(gpu_faiss):
    hits = np.zeros((5, 4), np.int64)
    qf = np.zeros(5, np.int32)
    # no rows: returns before any pointer is looked at
    got = c_slices(hits[:0], qf[:0], GOOD, 4, None, False, hits=None, qf=None, ic=None, ig=None, lead=None, tp=None)
    assert got[0] == 0 and (got[5] == S64).all()
    # no slices: no hit names one, every output is zeros
    none = tuple(t[:0] for t in GOOD[:3]) + GOOD[3:]
    got = c_slices(hits, qf, none, 4, None, True)
    assert got[0] == 0, _last_error()
    assert not got[1].any() and not got[2].any() and not got[3].any() and not got[4].any() and not got[5].any()
    rc, mc, an, fs = c_annotate(none, 4)
    assert rc == 0 and fs.tolist() == [0] * 4
    # no proteins, no families: every slice is without domains
    bare = (np.full(3, -1, np.int32), GOOD[1], GOOD[2], np.zeros(1, np.int64)) + tuple(t[:0] for t in GOOD[4:])
    rc, mc, an, fs = c_annotate(bare, 0, off=None)
    assert rc == 0 and mc.tolist() == [0] * 3 and an.tolist() == [-1] * 3
    got = c_slices(hits, np.full(5, -1, np.int32), bare, 0, mc, True)
    assert got[0] == 0 and not got[1].any() and not got[2].any()


# ---- the Python facade on what the reference produced -----------------------------------------------------------------------
def test_facade_on_the_golden_fixture(gpu_faiss):
    from knn_for_homology_amd.evaluation import evaluate_slices, slice_tables
    g = np.load(GOLDEN)
    slices = [(str(p), (int(a), int(b))) for p, a, b in zip(g["slice_protein"], g["slice_start"], g["slice_stop"])]
    protein_to_domain = {str(p): [] for p in g["protein_names"]}
    for p, f, a, b in zip(g["domain_protein"], g["domain_pfam"], g["domain_start"], g["domain_stop"]):
        protein_to_domain[str(p)].append((str(f), (int(a), int(b))))
    t = slice_tables(slices, protein_to_domain)
    assert t.has_annotation.dtype == np.bool_ and np.array_equal(t.has_annotation, g["has_annotation"])
    assert [t.families[a] for a in t.annotation[t.has_annotation]] == [str(f) for f in g["annotated"]]
    sizes = dict(zip((str(f) for f in g["family_size_names"]), g["family_size_counts"].tolist()))
    assert {f: int(c) for f, c in zip(t.families, t.family_sizes) if c} == sizes
    for flag, tag in ((False, "plain"), (True, "ignore_unannotated")):
        is_correct, is_ignore, auc1s, columns = evaluate_slices(g["hits"], t, ignore_unannotated=flag, want_column_counts=True)
        assert is_correct.dtype == np.bool_ and np.array_equal(is_correct, g[f"is_correct_{tag}"])
        assert is_ignore.dtype == np.bool_ and np.array_equal(is_ignore, g[f"is_ignore_{tag}"])
        assert auc1s.dtype == np.float64 and np.array_equal(auc1s.view(np.uint64), g[f"auc1s_{tag}"].view(np.uint64))
        assert np.array_equal(columns, g[f"is_correct_{tag}"].sum(axis=0))
    # rows of slices without an annotation yield 0
    rows = np.flatnonzero(~t.has_annotation)[:3]
    out = evaluate_slices(g["hits"][:3], t, query_rows=rows)
    assert len(out) == 3 and not out[0].any() and not out[1].any() and out[2].tolist() == [0.0] * 3
