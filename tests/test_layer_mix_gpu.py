"""GPU: LayerMix (knn_for_homology_amd/layers.py, csrc/mix.inc) bit for bit against the numpy restatement in
layer_mix_reference.py -- the rows of a mix, strided and device-resident layers, non-finite inputs, search and sweep against
cath.search.search + compute_is_correct per mix, and every refusal with its outputs untouched."""
import ctypes

import numpy as np
import pytest

import layer_mix_reference as ref

pytestmark = pytest.mark.gpu

N = 193  # odd: the last workgroup's tail


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_bits(got, want):
    """uint32 equality; NaNs compare as NaN-ness, not payload"""
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and np.array_equal(bits(got)[~nan], bits(want)[~nan])


@pytest.fixture(scope="module")
def layers_mod(gpu_faiss):
    from knn_for_homology_amd import layers
    return layers


@pytest.fixture(scope="module", params=[1024, 1000, 1001])
def mixer(request, layers_mod):
    """d = 1024: 16-byte loads; d = 1000: 16-byte loads, padding columns 1000 .. 1023; d = 1001: an odd row stride, float by float"""
    x = ref.inputs(N, request.param)
    return x, layers_mod.LayerMix(x)


def normalized(gpu_faiss, x):
    x = np.ascontiguousarray(x).copy()
    gpu_faiss.normalize_L2(x)
    return x


def test_mix_bits_on_the_grid(gpu_faiss, layers_mod, mixer):
    x, lm = mixer
    ratios = layers_mod.simplex_ratios(5)
    assert len(ratios) == 15
    for w in list(ratios) + list(ref.EXTRA_WEIGHTS):
        got = lm.index(w).reconstruct_n()
        assert got.shape == x[0].shape
        assert np.array_equal(bits(got), bits(normalized(gpu_faiss, ref.mix(x, w)))), w


def test_fewer_and_more_layers(gpu_faiss, layers_mod):
    x = ref.inputs(N, 200, nlayers=4, seed=3)
    for nl, w in ((1, (0.7,)), (2, (0.3, -1.7)), (4, (0.3, 0.1, 0.7, -0.9))):
        lm = layers_mod.LayerMix(x[:nl], metric=gpu_faiss.METRIC_L2)  # (L2: the rows stay as mixed)
        assert np.array_equal(bits(lm.index(w).reconstruct_n()), bits(ref.mix(x[:nl], w))), nl


def test_strided_layers_equal_separate_arrays(gpu_faiss, layers_mod):
    import torch
    x = ref.inputs(N, 1024, seed=1)
    wide = np.ascontiguousarray(np.concatenate(x, axis=1))
    w = (0.25, 0.75, 0.3)
    want = layers_mod.LayerMix(x).index(w).reconstruct_n()
    assert np.array_equal(bits(want), bits(normalized(gpu_faiss, ref.mix(x, w))))
    # the host matrix: each column block goes up as a layer
    assert np.array_equal(bits(layers_mod.LayerMix(wide, d=1024).index(w).reconstruct_n()), bits(want))
    # the matrix on the device: its column blocks are read where they lie, at the row stride 3072
    dev = torch.from_numpy(wide).cuda()
    assert np.array_equal(bits(layers_mod.LayerMix(dev, d=1024).index(w).reconstruct_n()), bits(want))
    # ... and blocks that start one float off a 16-byte boundary (float by float), out of a [N, 3073] matrix
    odd = torch.from_numpy(np.ascontiguousarray(np.concatenate([np.zeros((N, 1), np.float32), wide], axis=1))).cuda()
    blocks = [odd[:, 1 + 1024 * i:1 + 1024 * (i + 1)] for i in range(3)]
    assert np.array_equal(bits(layers_mod.LayerMix(blocks).index(w).reconstruct_n()), bits(want))


@pytest.mark.parametrize("d", [1024, 1001])
def test_non_finite_values_in_a_zero_weighted_layer(gpu_faiss, layers_mod, d):
    x = ref.inputs(N, d, seed=2)
    x[0][3, 5] = np.nan
    x[0][4, 6] = np.inf
    x[0][5, 7] = -0.0
    x[1][5, 7] = -0.0  # (-0.0 + -0.0) + 0 * c: the sign of the zero follows IEEE
    x[0][6, d - 1] = -np.inf
    lm = layers_mod.LayerMix(x, metric=gpu_faiss.METRIC_L2)  # (L2: the rows stay as mixed)
    for w in ((0.0, 1.0, 0.0), (0.0, 0.75, 0.25), (0.0, -1.0, 0.0)):
        want = ref.mix(x, w)
        assert np.isnan(want[3, 5]) and np.isnan(want[4, 6]) and np.isnan(want[6, d - 1]) and np.isnan(want).sum() == 3
        got = lm.index(w).reconstruct_n()
        assert same_bits(got, want), w
    # and through the normalisation of the inner-product index: the restatement, then knn_normalize_l2
    got = layers_mod.LayerMix(x).index((0.0, 0.75, 0.25)).reconstruct_n()
    assert same_bits(got, normalized(gpu_faiss, ref.mix(x, (0.0, 0.75, 0.25))))


@pytest.mark.parametrize("n,hits,weights", [(600, 10, ((0.25, 0.75, 0.0), (0.5, 0.25, 0.25))), (129, 10, ((0.25, 0.0, 0.75),))])
def test_search_equals_cath_search_of_the_restated_mix(gpu_faiss, layers_mod, n, hits, weights):
    from knn_for_homology_amd.cath.search import search
    x, _ = ref.clustered_layers(n, 256, 40, seed=n)
    lm = layers_mod.LayerMix(x)
    for w in weights:
        got_hits, got_scores = lm.search(w, hits=hits)  # (k = hits + 1 = 11)
        want_hits, want_scores = search(ref.mix(x, w), hits=hits)
        assert got_hits.shape == (n, hits) and np.array_equal(got_hits, want_hits), w
        assert np.array_equal(bits(got_scores), bits(want_scores)), w


@pytest.fixture(scope="module")
def sweep_case(gpu_faiss, layers_mod):
    """N = 600, the 15 ratios of granularity 5, four levels with 40 classes at the finest: the per-mix results of
    cath.search.search on the restated mixes, computed once"""
    from knn_for_homology_amd.cath.search import search
    from knn_for_homology_amd.evaluation import compute_is_correct
    x, mapping = ref.clustered_layers(600, 256, 40, seed=5)
    ratios = layers_mod.simplex_ratios(5)
    searched = [search(ref.mix(x, w), hits=3) for w in ratios]
    counts = np.asarray([compute_is_correct(h, mapping)[:, :, 0].sum(axis=0) for h, _ in searched], np.int64)
    return x, mapping, ratios, searched, counts


def test_sweep_counts_are_compute_is_corrects(layers_mod, sweep_case):
    x, mapping, ratios, searched, counts = sweep_case
    assert len(np.unique(mapping[:, 0])) >= 35 and 0 < counts.min() and counts.max() < 600 and len(np.unique(counts[:, 0])) > 5
    lm = layers_mod.LayerMix(x)
    got = lm.sweep(ratios, mapping)
    assert got.counts.dtype == np.int64 and got.counts.shape == (15, 4) and got.hits is None and got.scores is None
    assert np.array_equal(got.counts, counts)
    assert got.means.dtype == np.float64 and np.array_equal(got.means, counts / 600)
    # one level alone
    one = lm.sweep(ratios, mapping, level=3)
    assert np.array_equal(one.counts, counts[:, 3]) and np.array_equal(one.means, counts[:, 3] / 600)
    # the handle is reused from mix to mix: the same sweep again in reverse order leaves nothing behind
    back = lm.sweep(ratios[::-1], mapping)
    assert np.array_equal(back.counts, counts[::-1])
    ms = lm.last_ms()
    assert ms["mix"] > 0 and ms["search"] > 0 and ms["score"] > 0


def test_sweep_returns_the_hits_of_search(layers_mod, sweep_case):
    x, mapping, ratios, searched, counts = sweep_case
    lm = layers_mod.LayerMix(x)
    got = lm.sweep(ratios, mapping, hits=3, want_hits=True)
    assert np.array_equal(got.counts, counts)
    assert got.hits.shape == (15, 600, 3) and got.scores.shape == (15, 600, 3)
    for g, w in enumerate(ratios):
        assert np.array_equal(got.hits[g], searched[g][0]) and np.array_equal(bits(got.scores[g]), bits(searched[g][1])), w
    h, s = lm.search(ratios[7], hits=3)
    assert np.array_equal(got.hits[7], h) and np.array_equal(bits(got.scores[7]), bits(s))


def test_mixed_index_is_an_added_and_normalized_index(gpu_faiss, layers_mod):
    """what knn_flat_add + knn_flat_normalize_rows leave: rows, search results, and an index that takes further adds; with the
    row copies of the 16-bit prefilter kept as well"""
    x = ref.inputs(300, 96, seed=4)
    w = (0.3, 0.3, 0.4)
    mixed = ref.mix(x, w)
    plain = gpu_faiss.IndexFlat(96, gpu_faiss.METRIC_INNER_PRODUCT)
    plain.add(mixed)
    plain.normalize_rows()
    for scan16 in (0, 1):
        lm = layers_mod.LayerMix(x)
        if scan16:
            lm._flat.set_scan16(1)
        view = lm.index((1.0, 0.0, 0.0)).view()
        index = lm.index(w)
        with pytest.raises(Exception, match="stale"):  # the old rows are gone: their view is stale, as behind a reset
            view.search_self(2)
        assert index.ntotal == 300 and np.array_equal(bits(index.reconstruct_n()), bits(plain.reconstruct_n()))
        for a, b in zip(index.search_self(5), plain.search_self(5)):
            assert np.array_equal(bits(a) if a.dtype == np.float32 else a, bits(b) if b.dtype == np.float32 else b)
        q = normalized(gpu_faiss, ref.inputs(7, 96, seed=9)[0])
        for a, b in zip(index.search(q, 4), plain.search(q, 4)):
            assert np.array_equal(bits(a) if a.dtype == np.float32 else a, bits(b) if b.dtype == np.float32 else b)
        index.add(q)
        assert index.ntotal == 307 and np.array_equal(bits(index.reconstruct_n(300, 7)), bits(q))


# ---- refusals: KNN_ERR_INVALID through the facade's error, outputs untouched, the index as it was ----
SENTINEL = -7777


class Raw:
    """a knn_mix handle and the arguments of knn_mix_sweep, made by hand so that each can be wrong on its own"""

    def __init__(self, gpu_faiss, d=64, nlayers=3, set_layers=(0, 1, 2), n=50):
        from knn_for_homology_amd import _lib
        self.lib, self.L = _lib, _lib.lib()
        self.h = ctypes.c_void_p()
        _lib.check(self.L.knn_mix_create(d, nlayers, ctypes.byref(self.h)))
        self.x = ref.inputs(n, d, nlayers=max(nlayers, 1), seed=6)
        for i in set_layers:
            _lib.check(self.L.knn_mix_set_layer(self.h, i, self.x[i].ctypes.data, n, d))
        self.n, self.d = n, d
        self.weights = np.full((2, nlayers), 0.5, np.float32)
        self.mapping = np.zeros((n, 8), np.int32)
        self.counts = np.full((2, 8), SENTINEL, np.int64)
        self.D = np.full((2, n, 4), -5.0, np.float32)
        self.I = np.full((2, n, 4), SENTINEL, np.int64)

    def sweep(self, flat, k=4, nlevels=4, column=1, out=True):
        return self.L.knn_mix_sweep(self.h, self.weights.ctypes.data, 2, flat._h, k, self.mapping.ctypes.data, nlevels, column, self.counts.ctypes.data,
                                    self.D.ctypes.data if out else None, self.I.ctypes.data if out else None)

    def into(self, flat):
        return self.L.knn_mix_into(self.h, self.weights.ctypes.data, flat._h, 1)

    def untouched(self):
        return (self.counts == SENTINEL).all() and (self.I == SENTINEL).all() and (self.D == -5.0).all()

    def __del__(self):
        self.L.knn_mix_free(self.h)


def filled_index(gpu_faiss, d):
    rows = ref.inputs(9, d, seed=8)[0]
    flat = gpu_faiss.IndexFlat(d, gpu_faiss.METRIC_INNER_PRODUCT)
    flat.add(rows)
    return flat, rows


def refused(raw, rc, flat, rows, match):
    assert rc == -1  # KNN_ERR_INVALID
    with pytest.raises(raw.lib.Knn355Error, match=match):
        raw.lib.check(rc)
    assert raw.untouched()
    # nothing was launched on the index: it still holds the rows it had
    assert flat.ntotal == len(rows) and np.array_equal(bits(flat.reconstruct_n()), bits(rows))


def test_refusals_leave_outputs_and_index_alone(gpu_faiss):
    flat, rows = filled_index(gpu_faiss, 64)
    ok = Raw(gpu_faiss)
    missing = Raw(gpu_faiss, set_layers=(0, 2))
    refused(missing, missing.sweep(flat), flat, rows, "layer has no rows")
    refused(missing, missing.into(flat), flat, rows, "layer has no rows")
    other, other_rows = filled_index(gpu_faiss, 32)
    refused(ok, ok.sweep(other), other, other_rows, "dimension")
    refused(ok, ok.into(other), other, other_rows, "dimension")
    view = flat.view()
    refused(ok, ok.sweep(view), flat, rows, "view is read-only")
    refused(ok, ok.into(view), flat, rows, "view is read-only")
    assert view.ntotal == 9 and np.array_equal(bits(view.reconstruct_n()), bits(rows))  # (the view is still alive)
    refused(ok, ok.sweep(flat, k=4, column=4), flat, rows, "column")
    refused(ok, ok.sweep(flat, k=4, column=-1), flat, rows, "column")
    refused(ok, ok.sweep(flat, k=1, column=1), flat, rows, "column")
    for nlevels in (0, 9, -1):
        refused(ok, ok.sweep(flat, nlevels=nlevels), flat, rows, "nlevels")
    for k in (0, 2049):
        refused(ok, ok.sweep(flat, k=k, column=0), flat, rows, "k must be")
    # nlayers outside 1 .. 4: no handle is made
    for nlayers in (0, 5, -1):
        h = ctypes.c_void_p(12345)
        rc = ok.L.knn_mix_create(64, nlayers, ctypes.byref(h))
        assert rc == -1 and h.value == 12345
        with pytest.raises(ok.lib.Knn355Error, match="nlayers"):
            ok.lib.check(rc)
    # a layer with another row count, a stride below d
    with pytest.raises(ok.lib.Knn355Error, match="same n"):
        ok.lib.check(ok.L.knn_mix_set_layer(ok.h, 1, ok.x[1].ctypes.data, ok.n - 1, ok.d))
    with pytest.raises(ok.lib.Knn355Error, match="row_stride"):
        ok.lib.check(ok.L.knn_mix_set_layer(ok.h, 1, ok.x[1].ctypes.data, ok.n, ok.d - 1))
    # and the same arguments, right, run: the handle was never the problem
    # (counts_out is [G][nlevels] = the first eight entries of the array; every hit shares the one label of the mapping)
    assert ok.sweep(flat) == 0 and (ok.counts.ravel()[:8] == ok.n).all() and (ok.counts.ravel()[8:] == SENTINEL).all()
    assert (ok.I >= 0).all() and (ok.I < ok.n).all() and (ok.I[:, :, 0] == np.arange(ok.n)).all()
    assert flat.ntotal == ok.n


def test_facade_refuses_what_it_can_see(gpu_faiss, layers_mod):
    x = ref.inputs(20, 16)
    with pytest.raises(ValueError):
        layers_mod.LayerMix(x + x[:2])  # five layers
    with pytest.raises(ValueError):
        layers_mod.LayerMix([x[0], x[1][:10]])
    with pytest.raises(TypeError):
        layers_mod.LayerMix([x[0].astype(np.float64)])
    lm = layers_mod.LayerMix(x)
    with pytest.raises(ValueError):
        lm.index((1.0, 0.0))
    with pytest.raises(ValueError):
        lm.sweep(np.ones((2, 3)), np.zeros((19, 4), np.int32))
    with pytest.raises(Exception, match="nlevels"):
        lm.sweep(np.ones((2, 3)), np.zeros((20, 9), np.int32))
