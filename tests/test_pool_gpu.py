"""GPU: knn_pool_ranges / knn_pool_ranges_dev and pooling.py, bit for bit against tests/pool_reference.py (the CPU
restatement of the contract above knn_pool_ranges in include/knn355.h).  Every comparison is on raw bits; where NaNs are
expected, NaN-ness by position and bits elsewhere.

Shapes are the smallest at which each part can go wrong: d = 2 (one partial lane), 8, 20 (a tail lane behind whole
ones), 1024 (four column blocks, one workgroup), 1028 (a fifth block of one lane: two workgroups per range in the plain
build, eight waves in the normalizing one), 3072 (twelve blocks: three workgroups, or sixteen waves of which four only
compute norms); at most 1500 rows; range lengths 1, 2, 8, 9 (the load group of eight), 63, 64, 65, 129 (the 64-row
norm batch) and 1000, overlapping, unordered, with a duplicate and one range over all rows."""
import ctypes

import numpy as np
import pytest

import pool_reference as ref

pytestmark = pytest.mark.gpu

ROWS = 1500
DS = (2, 8, 20, 1024, 1028, 3072)
KNOB = "KNN355_POOL_CHUNK_ROWS"


@pytest.fixture(scope="module")
def pooling(gpu_faiss):
    from knn_for_homology_amd import pooling
    return pooling


@pytest.fixture(scope="module")
def torch_mod(gpu_faiss):
    import torch
    return torch


@pytest.fixture(scope="module")
def cases():
    """d -> (x, starts, stops, the restated plain result): computed once, never modified"""
    out = {}
    for d in DS:
        x = ref.residues(ROWS, d, 100 + d)
        starts, stops = ref.ranges(ROWS, 200 + d)
        x.setflags(write=False)
        out[d] = (x, starts, stops, ref.pool_sequential(x, starts, stops))
    return out


def assert_same(got, want, what=""):
    assert got.dtype == np.float32 and got.shape == want.shape, (got.dtype, got.shape, want.shape)
    bad = ref.bits_differ(got, want)
    assert len(bad) == 0, f"{what}: {len(bad)} entries differ, first {bad[:4].tolist()}"


@pytest.mark.parametrize("d", DS)
def test_plain_bit_for_bit(pooling, cases, d):
    x, starts, stops, want = cases[d]
    assert_same(pooling.pool_ranges(x, starts, stops), want, f"d={d}")


def test_adds_are_in_row_order(pooling):
    x = ref.order_sensitive()
    starts, stops = np.asarray([0, 3, 0], np.int64), np.asarray([len(x), 900, 64], np.int64)
    seq, tree = ref.pool_sequential(x, starts, stops), ref.pool_pairwise(x, starts, stops)
    assert len(ref.bits_differ(seq[:2], tree[:2])) > 0 and seq[0, 0] != tree[0, 0], "the case must tell a reordered sum apart"
    assert_same(pooling.pool_ranges(x, starts, stops), seq)
    assert_same(pooling.pool_ranges(x, starts, stops, normalize=False), seq)


def test_special_values(pooling):
    x, starts, stops = ref.special_values()
    got = pooling.pool_ranges(x, starts, stops)
    assert_same(got, ref.pool_sequential(x, starts, stops))
    assert (got[0].view(np.uint32) == 0x80000000).all(), "a first row of -0.0 must survive"
    assert ((np.abs(got[4]) > 0) & (np.abs(got[4]) < np.finfo(np.float32).tiny)).all(), "subnormal means were flushed"
    assert np.isnan(got[9, 8]) and np.isnan(got[8, 7]) and got[8, 5] == np.inf and got[8, 6] == -np.inf


@pytest.mark.parametrize("d", (2, 20, 1024, 1028, 3072))
def test_normalize_is_normalize_l2_then_pooling(pooling, gpu_faiss, oracle, cases, d):
    x, starts, stops, _ = cases[d]
    keep = x.copy()
    got = pooling.pool_ranges(x, starts, stops, normalize=True)
    assert np.array_equal(x.view(np.uint32), keep.view(np.uint32)), "the input was modified"
    assert_same(got, ref.pool_normalized(x, starts, stops, oracle), f"d={d} against the oracle")
    y = x.copy()
    gpu_faiss.normalize_L2(y)
    assert_same(got, pooling.pool_ranges(y, starts, stops), f"d={d} against knn_normalize_l2 + plain")


def test_normalize_edge_rows(pooling, oracle):
    x, starts, stops = ref.normalize_edge_rows()
    keep = x.copy()
    got = pooling.pool_ranges(x, starts, stops, normalize=True)
    assert_same(got, ref.pool_normalized(x, starts, stops, oracle))
    assert np.array_equal(x.view(np.uint32), keep.view(np.uint32))
    assert (got[1] == 0).all() and (got[3] == 0).all() and np.isnan(got[5, 2]) and np.isnan(got[6, 1])


@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("d", (2, 20, 1024, 1028))
def test_float16_is_astype_float32_then_float32(pooling, cases, d, normalize):
    _, starts, stops, _ = cases[d]
    h = ref.residues(ROWS, d, 300 + d, np.float16)
    h[7, 0] = np.float16(6e-8)  # a float16 subnormal
    keep = h.copy()
    got = pooling.pool_ranges(h, starts, stops, normalize=normalize)
    assert np.array_equal(h.view(np.uint16), keep.view(np.uint16))
    assert_same(got, pooling.pool_ranges(h.astype(np.float32), starts, stops, normalize=normalize))
    if not normalize:
        assert_same(got, ref.pool_sequential(h, starts, stops))


# ---- the device entry --------------------------------------------------------------------------
@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("d", DS)
def test_device_entry_matches_the_host_entry(pooling, torch_mod, cases, d, normalize):
    torch = torch_mod
    x, starts, stops, want = cases[d]
    host = pooling.pool_ranges(x, starts, stops, normalize=normalize)
    if not normalize:
        assert_same(host, want)
    t = torch.from_numpy(x.copy()).cuda()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        assert torch.cuda.current_stream().cuda_stream != 0
        out = pooling.pool_ranges(t, starts, stops, normalize=normalize)
        out2 = pooling.pool_ranges(t, torch.from_numpy(starts).cuda(), torch.from_numpy(stops).cuda(), normalize=normalize)
    assert out.is_cuda and out.dtype == torch.float32 and out.device == t.device
    assert_same(out.cpu().numpy(), host, f"d={d}")
    assert_same(out2.cpu().numpy(), host, f"d={d}, ranges on the device")
    assert np.array_equal(t.cpu().numpy().view(np.uint32), x.view(np.uint32)), "the input was modified"


@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("dtype", [np.float32, np.float16])
def test_device_views(pooling, torch_mod, dtype, normalize):
    """a row-strided view of a wider tensor, t[1:] at d = 20, and a base that is no multiple of four elements"""
    torch = torch_mod
    rows = 300
    starts, stops = ref.ranges(rows, 77)
    for d, wide in ((20, 24), (20, 23), (1026, 1028), (8, 9)):
        w = ref.residues(rows, wide, 400 + wide, dtype)
        host = pooling.pool_ranges(np.ascontiguousarray(w[:, :d]), starts, stops, normalize=normalize)
        assert_same(pooling.pool_ranges(w[:, :d], starts, stops, normalize=normalize), host, "a numpy view is copied")
        view = torch.from_numpy(w).cuda()[:, :d]
        assert view.stride(0) == wide and not view.is_contiguous()
        assert_same(pooling.pool_ranges(view, starts, stops, normalize=normalize).cpu().numpy(), host, f"t[:, :{d}] of {wide} columns")
    x = ref.residues(rows + 1, 20, 500, dtype)
    host = pooling.pool_ranges(x[1:], starts, stops, normalize=normalize)
    t = torch.from_numpy(x).cuda()
    assert_same(pooling.pool_ranges(t[1:], starts, stops, normalize=normalize).cpu().numpy(), host, "t[1:]")
    for d in (20, 8, 2):
        flat = torch.from_numpy(np.concatenate([np.zeros(1, dtype), ref.residues(rows, d, 600 + d, dtype).ravel()])).cuda()
        off = flat[1:].view(rows, d)
        assert off.data_ptr() % (4 * off.element_size()) != 0
        host = pooling.pool_ranges(off.cpu().numpy(), starts, stops, normalize=normalize)
        assert_same(pooling.pool_ranges(off, starts, stops, normalize=normalize).cpu().numpy(), host, f"a base one element off, d={d}")


def test_pooled_rows_feed_the_index_on_the_device(pooling, torch_mod, gpu_faiss):
    """pool_ranges -> normalize_L2 -> add_dev -> search without leaving the device: the hits of the host path"""
    torch = torch_mod
    from knn_for_homology_amd import _lib
    L = _lib.lib()
    d, n = 64, 200
    lengths = np.random.default_rng(8).integers(1, 40, n)
    x = ref.residues(int(lengths.sum()), d, 9)
    host = pooling.reduce_per_protein(x, lengths=lengths)
    gpu_faiss.normalize_L2(host)
    index = gpu_faiss.IndexFlat(d, gpu_faiss.METRIC_INNER_PRODUCT)
    index.add(host)
    D, I = index.search(host[:50], 10)
    dev = pooling.reduce_per_protein(torch.from_numpy(x).cuda(), lengths=lengths)
    _lib.check(L.knn_normalize_l2_dev(dev.data_ptr(), n, d, None))
    index2 = gpu_faiss.IndexFlat(d, gpu_faiss.METRIC_INNER_PRODUCT)
    _lib.check(L.knn_flat_add_dev(index2._h, dev.data_ptr(), n, None))
    assert_same(index2.reconstruct_n(0, n), host)
    D2, I2 = index2.search(dev[:50].cpu().numpy(), 10)
    assert np.array_equal(I, I2) and np.array_equal(D.view(np.uint32), D2.view(np.uint32))


# ---- the host entry's chunks -------------------------------------------------------------------
@pytest.mark.parametrize("chunk_rows", [1, 100, 129, 700])
@pytest.mark.parametrize("normalize", [False, True])
def test_host_entry_in_small_chunks(pooling, oracle, cases, monkeypatch, chunk_rows, normalize):
    """ranges that straddle chunk ends, the range over all rows longer than every chunk; d = 20 and the fp16 rows"""
    x, starts, stops, want = cases[20]
    if normalize:
        want = ref.pool_normalized(x, starts, stops, oracle)
    monkeypatch.setenv(KNOB, str(chunk_rows))
    assert_same(pooling.pool_ranges(x, starts, stops, normalize=normalize), want, f"{chunk_rows} rows per chunk")
    h = x.astype(np.float16)
    got16 = pooling.pool_ranges(h, starts, stops, normalize=normalize)
    monkeypatch.delenv(KNOB)
    assert_same(got16, pooling.pool_ranges(h, starts, stops, normalize=normalize), "fp16 rows in chunks")


# ---- the drop-ins --------------------------------------------------------------------------------
def test_reduce_per_protein_on_ragged_lengths(pooling, torch_mod, oracle):
    rng = np.random.default_rng(21)
    lengths = np.concatenate(([1, 2, 64, 65, 513], rng.integers(1, 90, 40)))
    emb = [ref.residues(int(L), 1024, 700 + i) for i, L in enumerate(lengths)]
    with np.errstate(all="ignore"):
        numpy_loop = np.stack([e.mean(axis=0) for e in emb])
    got = pooling.reduce_per_protein(emb)
    assert_same(got, numpy_loop, "against numpy's own mean")
    packed = np.concatenate(emb)
    assert_same(pooling.reduce_per_protein(packed, lengths=lengths), got)
    assert_same(pooling.reduce_per_protein([torch_mod.from_numpy(e).cuda() for e in emb]).cpu().numpy(), got)
    stops = np.cumsum(lengths)
    assert_same(pooling.reduce_per_protein(emb, normalize=True), ref.pool_normalized(packed, stops - lengths, stops, oracle))
    # cath/embed.py:92: i.mean(1) on [3, L, 1024] is three row ranges of the [3 L, 1024] matrix
    three = ref.residues(3 * 37, 1024, 31).reshape(3, 37, 1024)
    assert_same(pooling.reduce_per_protein(three.reshape(-1, 1024), lengths=[37, 37, 37]), three.mean(1))


def test_extract_domain_representations_from_gpu_embeddings(pooling, torch_mod):
    """the drop-in fed by an embedder that yields GPU tensors, several calls: the reference function's dicts"""
    import test_pool_reference as tpr
    with np.load(tpr.GOLDEN) as z:
        g = {k: z[k] for k in z.files}
    emb, test, train = tpr.golden_dicts(g)
    gen = ((sid, torch_mod.from_numpy(e.copy()).cuda()) for sid, e in emb)
    data_test, data_train = pooling.extract_domain_representations(gen, test, train, batch_bytes=60000)
    for name, data in (("train", data_train), ("test", data_test)):
        assert list(data) == [str(k) for k in g[f"{name}_keys"]]
        assert_same(np.stack(list(data.values())), g[f"{name}_values"], name)
    with pytest.raises(ValueError, match="not inside"):
        pooling.extract_domain_representations(iter(emb[:1]), {emb[0][0]: [(1, 2, "a")]}, {emb[0][0]: []})


# ---- refusals --------------------------------------------------------------------------------------
def test_refusals_leave_the_library_working(pooling, gpu_faiss, cases):
    from knn_for_homology_amd import _lib
    L = _lib.lib()
    x, starts, stops, want = cases[8]
    one = np.zeros(1, np.int64)

    def host(xa, dtype, rows, d, s, e, n, flags, out):
        return L.knn_pool_ranges(xa, dtype, rows, d, s, e, n, flags, out)

    out = np.full((2, 8), 7.0, np.float32)
    px, po = x.ctypes.data, out.ctypes.data
    for (s, e), text in (((-1, 3), "0 <= start"), ((5, 5), "start < stop"), ((6, 5), "start < stop"), ((0, ROWS + 1), "stop <= rows"),
                         ((ROWS, ROWS + 1), "stop <= rows")):
        a, b = np.asarray([0, s], np.int64), np.asarray([4, e], np.int64)
        with pytest.raises(_lib.Knn355Error, match="range 1") as err:
            pooling.pool_ranges(x, a, b)
        assert text in str(err.value)
    # stop - start >= 2^24: refused on the ranges alone, before a row is uploaded (the row count is only claimed)
    a, b = np.asarray([0], np.int64), np.asarray([1 << 24], np.int64)
    assert host(px, 0, 1 << 25, 8, a.ctypes.data, b.ctypes.data, 1, 0, po) == -1 and b"2^24" in L.knn_last_error()
    s, e = starts.ctypes.data, stops.ctypes.data
    for args, text in (((px, 2, ROWS, 8, s, e, 2, 0, po), b"dtype"), ((px, 0, ROWS, 8, s, e, 2, 2, po), b"flags"),
                       ((px, 0, ROWS, 1, s, e, 2, 0, po), b"d <="), ((px, 0, ROWS, (1 << 20) + 1, s, e, 2, 0, po), b"d <="),
                       ((None, 0, ROWS, 8, s, e, 2, 0, po), b"null"), ((px, 0, ROWS, 8, None, e, 2, 0, po), b"null"),
                       ((px, 0, ROWS, 8, s, None, 2, 0, po), b"null"), ((px, 0, ROWS, 8, s, e, 2, 0, None), b"null"),
                       ((px, 0, -1, 8, s, e, 2, 0, po), b"negative"), ((px, 0, ROWS, 8, s, e, -1, 0, po), b"negative")):
        assert host(*args) == -1 and text in L.knn_last_error(), (args, L.knn_last_error())
    assert L.knn_pool_ranges_dev(px, 0, ROWS, 8, 7, s, e, 2, 0, po, None) == -1 and b"row_stride" in L.knn_last_error()
    assert (out == 7.0).all(), "a refused call wrote its output"
    assert host(None, 0, 0, 8, None, None, 0, 0, None) == 0, "n = 0 is a success that touches nothing"
    assert pooling.pool_ranges(x, one[:0], one[:0]).shape == (0, 8)
    # the Python boundary checks shapes before a pointer is handed over
    for bad in (lambda: pooling.pool_ranges(x[:, :1], one, one + 1), lambda: pooling.pool_ranges(x.astype(np.float64), one, one + 1),
                lambda: pooling.pool_ranges(x[:, ::2], one, one + 1), lambda: pooling.pool_ranges(x[0], one, one + 1),
                lambda: pooling.pool_ranges(x, one, np.ones(2, np.int64)), lambda: pooling.pool_ranges(x, one.astype(np.float32), one + 1),
                lambda: pooling.pool_ranges([[1.0, 2.0]], one, one + 1), lambda: pooling.reduce_per_protein(x, lengths=[ROWS - 1]),
                lambda: pooling.reduce_per_protein(x, lengths=[ROWS, 0]), lambda: pooling.reduce_per_protein([])):
        with pytest.raises(ValueError):
            bad()
    # and everything works afterwards
    assert_same(pooling.pool_ranges(x, starts, stops), want)
    index = gpu_faiss.IndexFlat(8, gpu_faiss.METRIC_L2)
    index.add(want)
    D, I = index.search(want[:5], 3)
    assert index.ntotal == len(want) and I.shape == (5, 3) and (I >= 0).all() and (I < len(want)).all()


def test_device_entry_reports_a_bad_range_through_the_status_word(pooling, torch_mod, cases):
    """every bad range is rejected by the check before any row is read for it; the good ranges' rows are still written"""
    torch = torch_mod
    from knn_for_homology_amd import _lib
    L = _lib.lib()
    x, starts, stops, want = cases[20]
    t = torch.from_numpy(x.copy()).cuda()
    a, b = starts.copy(), stops.copy()
    bad = {3: (-5, 2), 5: (9, 9), 11: (ROWS - 1, ROWS + 1), 12: (40, 30)}
    for o, (s, e) in bad.items():
        a[o], b[o] = s, e
    ta, tb = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    for normalize in (0, 1):
        out = torch.full((len(a), 20), 7.0, dtype=torch.float32, device="cuda")
        rc = L.knn_pool_ranges_dev(t.data_ptr(), 0, ROWS, 20, 20, ta.data_ptr(), tb.data_ptr(), len(a), normalize, out.data_ptr(),
                                   ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == -1 and b"range 3 " in L.knn_last_error(), L.knn_last_error()
        got = out.cpu().numpy()
        good = np.asarray([o not in bad for o in range(len(a))])
        assert (got[~good] == 7.0).all(), "the row of a bad range was written"
        if not normalize:
            assert_same(got[good], want[good])
    with pytest.raises(_lib.Knn355Error, match="range 3 "):
        pooling.pool_ranges(t, a, b)
    assert_same(pooling.pool_ranges(t, starts, stops).cpu().numpy(), want)
