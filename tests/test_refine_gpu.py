"""GPU: IndexRefineFlat bit for bit -- ids and score BITS -- against the host restatement of tests/refine_reference.py
(the CPU oracle's flat search over exactly the candidate rows, difference-form L2 at every batch size), with the
candidates taken from the host restatement of the base index (tests/lsh_reference.py::ref_search), not from the library.

Covered: the fused IndexLSH path on the exact inputs of the LSH tests (integer rows, +-1 rotation: heavy Hamming ties and
exact score ties) at every code width, d, metric, (k, k_factor) and nq; kb >= ntotal against IndexFlat.search; float rows
(normalised Gaussian, the committed embeddings); more than one 16384-query batch; the generic path (IndexFlat and
IndexHNSWFlat bases, hand-made labels through knn_flat_refine); the refusals; the "IxRF" file; knn_lsh_search unchanged."""
import struct
from pathlib import Path

import numpy as np
import pytest

from lsh_reference import assert_same_search, int_rows, pm1_rotation, ref_codes, ref_search
from refine_reference import FLT_MAX, METRIC_INNER_PRODUCT, METRIC_L2, ref_refine

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).resolve().parent / "golden"

NBITS = (1, 7, 64, 65, 200, 1024, 2048)
DS = (1, 33, 100, 1024)
K_KFACTOR = ((1, 1), (10, 1), (10, 4.5), (100, 20.48), (1000, 2), (2048, 1))
NQS = (1, 19, 20, 33, 300)
METRICS = (None, METRIC_INNER_PRODUCT)  # the default (the base's METRIC_L2) and the knn355 extra


def _kb(k, k_factor):
    return int(np.float32(k) * np.float32(k_factor))


def _refined_lsh(gpu_faiss, R, metric=None):
    return gpu_faiss.IndexRefineFlat(gpu_faiss.IndexLSH(R.shape[1], R.shape[0], _rotation=R), metric=metric)


def _metric(metric):
    return METRIC_L2 if metric is None else metric


# ---- 1. the fused path on exact inputs ---------------------------------------------------------------------------
@pytest.mark.parametrize("d", DS)
@pytest.mark.parametrize("nbits", NBITS)
def test_fused_exact_inputs(gpu_faiss, oracle, nbits, d):
    """every metric x (k, k_factor) x nq of the lists above for this (nbits, d); 3000 integer rows (kb = 2048 is a real
    selection), a third of the queries are database rows.  nq = 19 / 20 straddle FAISS's flat-search L2 rule: the refined
    L2 bits are the difference form on both sides (the restatement's l2_mode=2)."""
    rng = np.random.default_rng(nbits * 131 + d)
    nb = 3000
    R = pm1_rotation(rng, nbits, d)
    xb = int_rows(rng, nb, d)
    cb = ref_codes(xb, R)
    idx = {m: _refined_lsh(gpu_faiss, R, m) for m in METRICS}
    for m in METRICS:
        idx[m].add(xb)
        assert idx[m].ntotal == nb and idx[m].refine_index.metric_type == _metric(m)
    for nq in NQS:
        xq = int_rows(rng, nq, d)
        xq[: nq // 3] = xb[rng.integers(0, nb, nq // 3)]
        _, Ih = ref_search(cb, ref_codes(xq, R), 2048)  # sorted by (distance, id): its first kb columns are the top kb
        for k, kf in K_KFACTOR:
            kb = _kb(k, kf)
            assert k <= kb <= 2048
            for m in METRICS:
                idx[m].k_factor = kf
                D, I = idx[m].search(xq, k)
                De, Ie = ref_refine(oracle, xb, xq, Ih[:, :kb], k, _metric(m))
                assert_same_search(D, I, De, Ie, f"nbits={nbits} d={d} nq={nq} k={k} k_factor={kf} (kb={kb}) metric={_metric(m)}")


# ---- 2. kb >= ntotal: the flat search itself ---------------------------------------------------------------------
@pytest.mark.parametrize("ntotal", (1, 5, 300, 2048))
@pytest.mark.parametrize("metric", METRICS)
def test_every_row_a_candidate_equals_flat_search(gpu_faiss, metric, ntotal):
    """kb = 2048 >= ntotal: every row is re-scored, so the result is IndexFlat.search's bit for bit -- inner product at any
    nq, L2 below FAISS's 20-query threshold (the flat search's difference form); ntotal < k leaves a -1 / FLT_MAX tail"""
    d = 100
    rng = np.random.default_rng(ntotal + 7 * _metric(metric))
    xb = rng.standard_normal((ntotal, d)).astype(np.float32)
    xb[ntotal // 2] = xb[0]  # an exact tie
    idx = gpu_faiss.IndexRefineFlat(gpu_faiss.IndexLSH(d, 64), metric=metric)
    flat = gpu_faiss.IndexFlat(d, _metric(metric))
    idx.add(xb)
    flat.add(xb)
    for nq in ((1, 19) if _metric(metric) == METRIC_L2 else (1, 19, 20, 300)):
        xq = rng.standard_normal((nq, d)).astype(np.float32)
        xq[0] = xb[0]
        for k, kf in ((2048, 1), (10, 204.8), (1, 2048)):
            assert _kb(k, kf) == 2048
            idx.k_factor = kf
            D, I = idx.search(xq, k)
            De, Ie = flat.search(xq, k)
            assert_same_search(D, I, De, Ie, f"ntotal={ntotal} nq={nq} k={k} metric={_metric(metric)}")
            if ntotal < k:
                assert (I[:, ntotal:] == -1).all() and (I[:, :ntotal] >= 0).all()
                assert (D[:, ntotal:] == (FLT_MAX if _metric(metric) == METRIC_L2 else -FLT_MAX)).all()


# ---- 3. float rows -----------------------------------------------------------------------------------------------
def _library_codes(gpu_faiss, base, x):
    """the codes the library's (separately pinned) encoder gives x under base's rotation and thresholds.  Float
    projections have no exact host restatement (a projection next to zero may round to either sign), so for float rows
    the restatement's Hamming search runs over these codes; the search itself stays on the host."""
    enc = gpu_faiss.IndexLSH(base.d, base.nbits, _rotation=base._rot)
    enc.add(x)
    return enc.codes()


def _float_case(gpu_faiss, oracle, xb, xq, nbits, what):
    d = xb.shape[1]
    for metric in METRICS:
        idx = gpu_faiss.IndexRefineFlat(gpu_faiss.IndexLSH(d, nbits), metric=metric)
        idx.add(xb)
        cb, cq = idx.base_index.codes(), _library_codes(gpu_faiss, idx.base_index, xq)
        for k, kf in ((1, 1), (10, 4.5), (20, 5), (100, 1.5)):
            kb = _kb(k, kf)
            idx.k_factor = kf
            D, I = idx.search(xq, k)
            _, Ih = ref_search(cb, cq, kb)
            De, Ie = ref_refine(oracle, xb, xq, Ih, k, _metric(metric))
            assert_same_search(D, I, De, Ie, f"{what} nbits={nbits} k={k} kb={kb} metric={_metric(metric)}")
            # derived: the result is a subset of the base index's own kb labels, and the restatement's set
            _, Ib = idx.base_index.search(xq, kb)
            for i in range(xq.shape[0]):
                got = I[i][I[i] >= 0]
                assert np.isin(got, Ib[i]).all(), f"{what}: query {i} returned an id outside the base's shortlist"
                assert sorted(got.tolist()) == sorted(Ie[i][Ie[i] >= 0].tolist())


@pytest.mark.parametrize("nbits", (64, 1024))
@pytest.mark.parametrize("d", (33, 1024))
def test_normalised_gaussian_rows(gpu_faiss, oracle, nbits, d):
    rng = np.random.default_rng(nbits + d)
    xb = rng.standard_normal((4000, d)).astype(np.float32)
    xq = rng.standard_normal((37, d)).astype(np.float32)
    gpu_faiss.normalize_L2(xb)
    gpu_faiss.normalize_L2(xq)
    _float_case(gpu_faiss, oracle, xb, xq, nbits, f"gaussian d={d}")


@pytest.mark.parametrize("name", ("pfam-20-10", "pfam-20-10-sum", "pfam-20-dist", "small-random"))
def test_committed_embeddings(gpu_faiss, oracle, name):
    xb = np.ascontiguousarray(np.load(GOLDEN / name / "train.npy"), np.float32)
    xq = np.ascontiguousarray(np.load(GOLDEN / name / "test.npy"), np.float32)
    _float_case(gpu_faiss, oracle, xb, xq, 256, name)


# ---- 4. more than one batch --------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
def test_two_batches_equal_two_calls(gpu_faiss, oracle, metric):
    """16384 + 700 queries take two batches of knn_lsh_search_refine (the piped downloads): the same bits as the two
    pieces searched on their own, and the restatement's on a sample of the queries"""
    d, nbits, nb, k, kf = 32, 64, 5000, 10, 4.5
    rng = np.random.default_rng(4 + _metric(metric))
    R = pm1_rotation(rng, nbits, d)
    xb = int_rows(rng, nb, d)
    xq = int_rows(rng, 16384 + 700, d)
    idx = _refined_lsh(gpu_faiss, R, metric)
    idx.add(xb)
    idx.k_factor = kf
    D, I = idx.search(xq, k)
    Da, Ia = idx.search(np.ascontiguousarray(xq[:16384]), k)
    Db, Ib = idx.search(np.ascontiguousarray(xq[16384:]), k)
    assert_same_search(D, I, np.concatenate([Da, Db]), np.concatenate([Ia, Ib]))
    sample = np.concatenate([np.arange(0, 16384, 257), np.arange(16384 - 3, 16384 + 700, 7)])
    xs = np.ascontiguousarray(xq[sample])
    _, Ih = ref_search(ref_codes(xb, R), ref_codes(xs, R), _kb(k, kf))
    De, Ie = ref_refine(oracle, xb, xs, Ih, k, _metric(metric))
    assert_same_search(np.ascontiguousarray(D[sample]), np.ascontiguousarray(I[sample]), De, Ie)


# ---- 5. the generic path -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("base_kind", ("flat", "hnsw"))
@pytest.mark.parametrize("base_metric", (METRIC_INNER_PRODUCT, METRIC_L2))
def test_generic_base_indexes(gpu_faiss, oracle, base_kind, base_metric):
    """IndexRefineFlat(IndexFlat / IndexHNSWFlat): base.search(x, kb), then knn_flat_refine -- against the restatement fed
    with the base's own labels; the refine index has the base's metric (FAISS), or the other one (metric=)"""
    d, nb = 48, 2500
    rng = np.random.default_rng(base_metric + 10 * (base_kind == "hnsw"))
    xb = rng.standard_normal((nb, d)).astype(np.float32)
    for metric in (None, 1 - base_metric):
        base = gpu_faiss.IndexFlat(d, base_metric) if base_kind == "flat" else gpu_faiss.IndexHNSWFlat(d, 16, base_metric)
        idx = gpu_faiss.IndexRefineFlat(base, metric=metric)
        assert idx.metric_type == base_metric and idx.refine_index.metric_type == (base_metric if metric is None else metric)
        idx.add(xb)
        assert idx.ntotal == nb == idx.refine_index.ntotal
        for nq in (1, 19, 20, 130):
            xq = rng.standard_normal((nq, d)).astype(np.float32)
            for k, kf in ((1, 1), (10, 4.5), (100, 20.48)):
                idx.k_factor = kf
                _, labels = base.search(xq, _kb(k, kf))
                D, I = idx.search(xq, k)
                De, Ie = ref_refine(oracle, xb, xq, labels, k, idx.refine_index.metric_type)
                assert_same_search(D, I, De, Ie, f"{base_kind} base metric {base_metric} refine metric {idx.refine_index.metric_type} nq={nq} k={k}")


def _flat_refine(flat, xq, labels, k, D=None, I=None):
    from knn_for_homology_amd import _lib
    nq, kb = labels.shape
    D = np.empty((nq, k), np.float32) if D is None else D
    I = np.empty((nq, k), np.int64) if I is None else I
    rc = _lib.lib().knn_flat_refine(flat._h, xq.ctypes.data, nq, labels.ctypes.data, kb, k, D.ctypes.data, I.ctypes.data)
    return rc, D, I


@pytest.mark.parametrize("metric", (METRIC_INNER_PRODUCT, METRIC_L2))
@pytest.mark.parametrize("d", (1, 33, 1024))
def test_flat_refine_hand_made_labels(gpu_faiss, oracle, metric, d):
    """knn_flat_refine directly: -1 entries, a label given twice (scored twice, returned twice), rows of -1 only, kb from 1
    to 2048 (1 to 8 slices of 256 candidates, the last one partial), labels in any order"""
    rng = np.random.default_rng(d + metric)
    nb, nq = 700, 23
    xb = int_rows(rng, nb, d)
    xq = int_rows(rng, nq, d)
    flat = gpu_faiss.IndexFlat(d, metric)
    flat.add(xb)
    for kb, k in ((1, 1), (6, 3), (255, 100), (256, 256), (257, 1), (600, 600), (1000, 31), (2048, 2048)):
        labels = rng.integers(0, nb, (nq, kb)).astype(np.int64)
        if kb <= nb:
            for i in range(nq):  # distinct labels ...
                labels[i] = rng.permutation(nb)[:kb]
        labels[rng.random((nq, kb)) < 0.2] = -1
        if kb >= 2:
            labels[3, 1] = labels[3, 0] = 5  # ... but for one given twice
        labels[7] = -1
        rc, D, I = _flat_refine(flat, xq, labels, k)
        assert rc == 0
        De, Ie = ref_refine(oracle, xb, xq, labels, k, metric)
        assert_same_search(D, I, De, Ie, f"d={d} metric={metric} kb={kb} k={k}")
        assert (I[7] == -1).all()


def test_flat_refine_refuses_labels_outside_the_index(gpu_faiss):
    from knn_for_homology_amd import _lib
    d, nb, nq, kb, k = 16, 50, 4, 8, 3
    rng = np.random.default_rng(0)
    flat = gpu_faiss.IndexFlat(d, METRIC_L2)
    flat.add(rng.standard_normal((nb, d)).astype(np.float32))
    xq = rng.standard_normal((nq, d)).astype(np.float32)
    for bad in (nb, -2, 1 << 40):
        labels = rng.integers(0, nb, (nq, kb)).astype(np.int64)
        labels[2, 5] = bad
        D = np.full((nq, k), 123.0, np.float32)
        I = np.full((nq, k), 456, np.int64)
        rc, D, I = _flat_refine(flat, xq, labels, k, D, I)
        assert rc == -1, f"label {bad}: KNN_ERR_INVALID expected, got {rc}"  # KNN_ERR_INVALID
        assert (D == 123.0).all() and (I == 456).all(), "a refused call wrote into D / I"
        assert b"label" in _lib.lib().knn_last_error()
    labels = rng.integers(0, nb, (nq, kb)).astype(np.int64)
    assert _flat_refine(flat, xq, labels, 0)[0] == -1            # k < 1
    assert _flat_refine(flat, xq, labels, kb + 1)[0] == -1       # k > kb
    big = np.zeros((nq, 2049), np.int64)
    assert _flat_refine(flat, xq, big, 3)[0] == -4               # kb > KNN_MAX_K: KNN_ERR_UNSUPPORTED
    assert _lib.lib().knn_flat_refine(flat._h, xq.ctypes.data, 0, labels.ctypes.data, kb, k, None, None) == 0  # nq = 0
    empty = gpu_faiss.IndexFlat(d, METRIC_INNER_PRODUCT)
    rc, D, I = _flat_refine(empty, xq, np.full((nq, kb), -1, np.int64), k)
    assert rc == 0 and (I == -1).all() and (D == -FLT_MAX).all()
    assert _flat_refine(empty, xq, np.zeros((nq, kb), np.int64), k)[0] == -1  # label 0 of an index without rows


# ---- 6. refusals -------------------------------------------------------------------------------------------------
def test_refusals(gpu_faiss):
    from knn_for_homology_amd import _lib
    d = 32
    rng = np.random.default_rng(1)
    xb = rng.standard_normal((500, d)).astype(np.float32)
    xq = rng.standard_normal((5, d)).astype(np.float32)
    idx = gpu_faiss.IndexRefineFlat(gpu_faiss.IndexLSH(d, 64))
    assert idx.k_factor == 1.0 and isinstance(idx.k_factor, float) and idx.is_trained and idx.d == d
    for bad in (0.99, 0, -3, float("nan")):
        with pytest.raises(ValueError):
            idx.k_factor = bad
    assert idx.k_factor == 1.0
    D, I = idx.search(xq, 4)  # no rows yet: every slot unfilled
    assert (I == -1).all() and (D == FLT_MAX).all()
    idx.add(xb)
    with pytest.raises(AssertionError):
        idx.search(xq, 0)
    with pytest.raises(_lib.Knn355Error):
        idx.search(xq, 2049)
    idx.k_factor = 2.5
    with pytest.raises(_lib.Knn355Error):
        idx.search(xq, 1000)  # k * k_factor = 2500 > 2048
    idx.search(xq, 800)
    with pytest.raises(AssertionError):
        idx.search(xq[:, :16].copy(), 4)
    with pytest.raises(TypeError):
        idx.search(xq.astype(np.float64), 4)
    # rows added to one of the two behind the wrapper's back
    idx.base_index.add(xb[:3])
    with pytest.raises(RuntimeError):
        idx.search(xq, 4)
    rc = _lib.lib().knn_lsh_search_refine(idx.base_index._h, idx.refine_index._h, xq.ctypes.data, 5, 4, 4,
                                          np.empty((5, 4), np.float32).ctypes.data, np.empty((5, 4), np.int64).ctypes.data)
    assert rc == -1 and b"same rows" in _lib.lib().knn_last_error()
    idx.reset()
    assert idx.ntotal == 0 == idx.refine_index.ntotal == idx.base_index.ntotal
    idx.add(xb)
    idx.k_factor = 1
    idx.search(xq, 4)
    # different d
    other = gpu_faiss.IndexFlat(d + 1, METRIC_L2)
    other.add(rng.standard_normal((500, d + 1)).astype(np.float32))
    rc = _lib.lib().knn_lsh_search_refine(idx.base_index._h, other._h, xq.ctypes.data, 5, 4, 4,
                                          np.empty((5, 4), np.float32).ctypes.data, np.empty((5, 4), np.int64).ctypes.data)
    assert rc == -1
    idx.refine_index = other
    with pytest.raises(RuntimeError):
        idx.search(xq, 4)
    # FAISS: the base index must be empty when it is wrapped
    filled = gpu_faiss.IndexFlat(d, METRIC_L2)
    filled.add(xb)
    with pytest.raises(RuntimeError):
        gpu_faiss.IndexRefineFlat(filled)


# ---- 7. files ----------------------------------------------------------------------------------------------------
def test_index_file(gpu_faiss, tmp_path):
    d, nbits, nb = 24, 70, 900
    rng = np.random.default_rng(2)
    xb = rng.standard_normal((nb, d)).astype(np.float32)
    xq = rng.standard_normal((21, d)).astype(np.float32)
    for metric, inner in ((None, b"IxF2"), (METRIC_INNER_PRODUCT, b"IxFI")):
        idx = gpu_faiss.IndexRefineFlat(gpu_faiss.IndexLSH(d, nbits), metric=metric)
        idx.add(xb)
        idx.k_factor = 4.5
        path = tmp_path / f"refine_{inner.decode()}.index"
        gpu_faiss.write_index(idx, str(path))
        raw = path.read_bytes()
        hdr = "<iqqq?i"
        hsz = struct.calcsize(hdr)
        assert raw[:4] == b"IxRF"
        assert struct.unpack(hdr, raw[4:4 + hsz]) == (d, nb, 1 << 20, 1 << 20, True, METRIC_L2)  # the wrapper's metric = the base's
        assert raw[4 + hsz:8 + hsz] == b"IxHe"
        assert struct.unpack(hdr, raw[8 + hsz:8 + 2 * hsz]) == (d, nb, 1 << 20, 1 << 20, True, METRIC_L2)
        # the refine index's block ends the file but for the factor: fourcc, header, count, nb * d floats
        flat_size = 4 + hsz + 8 + nb * d * 4
        off = len(raw) - 4 - flat_size
        assert raw[off:off + 4] == inner
        assert struct.unpack(hdr, raw[off + 4:off + 4 + hsz]) == (d, nb, 1 << 20, 1 << 20, True, _metric(metric))
        assert struct.unpack("<Q", raw[off + 4 + hsz:off + 12 + hsz]) == (nb * d,)
        assert raw[off + 12 + hsz:len(raw) - 4] == xb.tobytes()
        assert struct.unpack("<f", raw[-4:]) == (4.5,)
        # the base index's block is what write_index gives the base on its own
        gpu_faiss.write_index(idx.base_index, str(tmp_path / "base.index"))
        assert raw[4 + hsz:off] == (tmp_path / "base.index").read_bytes()
        back = gpu_faiss.read_index(str(path))
        assert isinstance(back, gpu_faiss.IndexRefineFlat) and back.k_factor == 4.5 and back.ntotal == nb and back.d == d
        assert back.refine_index.metric_type == _metric(metric) and back.metric_type == METRIC_L2
        for k in (1, 10, 300):
            D, I = idx.search(xq, k)
            Db, Ib = back.search(xq, k)
            assert_same_search(Db, Ib, D, I, f"read_index(write_index(x)) k={k}")
        for cut in (3, 4 + hsz, off + 2, len(raw) - 5, len(raw) - 1):
            (tmp_path / "cut.index").write_bytes(raw[:cut])
            with pytest.raises(RuntimeError):
                gpu_faiss.read_index(str(tmp_path / "cut.index"))
        # inner indexes that disagree: the refine block of an index with one row fewer / another d
        for rows, dd in ((nb - 1, d), (nb, d + 1)):
            o = gpu_faiss.IndexFlat(dd, _metric(metric))
            o.add(rng.standard_normal((rows, dd)).astype(np.float32))
            gpu_faiss.write_index(o, str(tmp_path / "o.index"))
            (tmp_path / "mismatch.index").write_bytes(raw[:off] + (tmp_path / "o.index").read_bytes() + raw[-4:])
            with pytest.raises(RuntimeError, match="disagree"):
                gpu_faiss.read_index(str(tmp_path / "mismatch.index"))


def test_index_file_generic_base(gpu_faiss, tmp_path):
    d, nb = 16, 400
    rng = np.random.default_rng(5)
    xb = rng.standard_normal((nb, d)).astype(np.float32)
    xq = rng.standard_normal((9, d)).astype(np.float32)
    idx = gpu_faiss.IndexRefineFlat(gpu_faiss.IndexFlat(d, METRIC_INNER_PRODUCT))
    idx.add(xb)
    idx.k_factor = 3
    gpu_faiss.write_index(idx, str(tmp_path / "f.index"))
    raw = (tmp_path / "f.index").read_bytes()
    assert raw[:4] == b"IxRF" and raw[37:41] == b"IxFI" and struct.unpack("<f", raw[-4:]) == (3.0,)
    back = gpu_faiss.read_index(str(tmp_path / "f.index"))
    D, I = idx.search(xq, 7)
    Db, Ib = back.search(xq, 7)
    assert_same_search(Db, Ib, D, I)


# ---- 8. knn_lsh_search unchanged ---------------------------------------------------------------------------------
@pytest.mark.parametrize("nbits,d,nq,kb", [(64, 32, 33, 45), (1024, 100, 300, 2048), (200, 1024, 19, 1000)])
def test_plain_lsh_search_is_untouched_by_a_refined_one(gpu_faiss, nbits, d, nq, kb):
    """IndexLSH.search(x, kb) on the wrapped base index, before and after refined searches on the same handles: identical
    arrays, and the restatement's"""
    rng = np.random.default_rng(nbits + d)
    R = pm1_rotation(rng, nbits, d)
    xb = int_rows(rng, 5000, d)
    xq = int_rows(rng, nq, d)
    idx = _refined_lsh(gpu_faiss, R)
    idx.add(xb)
    D0, I0 = idx.base_index.search(xq, kb)
    De, Ie = ref_search(ref_codes(xb, R), ref_codes(xq, R), kb)
    assert_same_search(D0, I0, De, Ie)
    idx.k_factor = kb / 10 if kb >= 10 else 1
    idx.search(xq, 10 if kb >= 10 else 1)
    idx.k_factor = 1
    idx.search(xq, kb)
    D1, I1 = idx.base_index.search(xq, kb)
    assert np.array_equal(I0, I1) and np.array_equal(D0.view(np.uint32), D1.view(np.uint32))
    t = idx.last_refine()
    assert t["rescore_ms"] > 0 and t["select_ms"] > 0
