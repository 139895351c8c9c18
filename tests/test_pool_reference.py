"""The pooling contract's restatement (tests/pool_reference.py) against numpy itself and against what the reference's own
extract_domain_representations_from_embedder returned (tests/golden/reference_pool.npz, written by
tests/golden/make_pool_golden.py).

The contract says that numpy's mean(axis=0) of a C-contiguous float32 [L, d] array adds row after row: the first test
checks that on the whole grid, bit for bit, instead of trusting it; d = 1 is shown to be outside it (numpy sums a
single column pairwise), which is why the library refuses d < 2.  The golden comparison with the restatement runs on the
CPU; the same file through the library is the one GPU test here, so that this module fails without the feature."""
from pathlib import Path

import numpy as np
import pytest

import pool_reference as ref

GOLDEN = Path(__file__).resolve().parent / "golden" / "reference_pool.npz"


def same_bits(a, b):
    return a.dtype == b.dtype == np.float32 and a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("d", ref.GRID_D)
def test_numpy_mean_is_the_sequential_contract(d):
    rng = np.random.default_rng(d)
    big = rng.standard_normal((1300, d), dtype=np.float32) * np.float32(3) + np.float32(0.5)
    for L in ref.GRID_L:
        own = np.ascontiguousarray(big[:L])                        # an array of its own
        s = int(rng.integers(1, 1300 - L))
        for a, want in ((own, own.mean(axis=0)), (big, big[s:s + L].mean(axis=0))):
            assert want.dtype == np.float32
            lo = 0 if a is own else s
            got = ref.pool_sequential(a, [lo], [lo + L])[0]
            assert same_bits(got, want), f"L={L} d={d}: numpy's mean departs from the row-by-row order in {(got != want).sum()} columns"


def test_a_single_column_is_outside_the_contract():
    """d = 1: numpy reduces along the only axis left and sums pairwise -- the reason for d >= 2"""
    x = ref.order_sensitive(1024, 8)[:, :1].copy()
    seq = ref.pool_sequential(x, [0], [1024])
    assert not same_bits(seq[0], x.mean(axis=0))
    assert same_bits(ref.pool_sequential(np.repeat(x, 2, axis=1), [0], [1024])[0], np.repeat(x, 2, axis=1).mean(axis=0))


def test_float16_rows_convert_exactly():
    x = ref.residues(300, 20, 3, np.float16)
    starts, stops = ref.ranges(300, 4)
    assert same_bits(ref.pool_sequential(x, starts, stops), ref.pool_sequential(x.astype(np.float32), starts, stops))


def test_the_order_sensitive_case_tells_orders_apart():
    x = ref.order_sensitive()
    seq, tree = ref.pool_sequential(x, [0], [len(x)]), ref.pool_pairwise(x, [0], [len(x)])
    assert len(ref.bits_differ(seq, tree)) > 0 and seq[0, 0] != tree[0, 0]
    assert same_bits(seq[0], x.mean(axis=0))


def test_special_values_follow_numpy():
    x, starts, stops = ref.special_values()
    got = ref.pool_sequential(x, starts, stops)
    with np.errstate(all="ignore"):
        want = np.stack([x[a:b].mean(axis=0) for a, b in zip(starts, stops)])
    # the one departure: a column whose rows are ALL -0.0.  The contract starts from the first row and keeps -0.0; numpy's
    # sum starts from the identity +0.0, and +0.0 + -0.0 = +0.0.  Adding +0.0 first changes no other value.
    all_negative_zero = np.stack([((x[a:b] == 0) & np.signbit(x[a:b])).all(axis=0) for a, b in zip(starts, stops)])
    assert all_negative_zero[0].all() and all_negative_zero[1:3, 0].all() and all_negative_zero.sum() == x.shape[1] + 2
    assert (got[all_negative_zero].view(np.uint32) == 0x80000000).all() and (want[all_negative_zero].view(np.uint32) == 0).all()
    want[all_negative_zero] = np.float32(-0.0)
    assert len(ref.bits_differ(got, want)) == 0
    assert np.signbit(got[0]).all() and (got[0] == 0).all(), "a first row of -0.0 must survive"
    sub = np.abs(got[4])
    assert ((sub > 0) & (sub < np.finfo(np.float32).tiny)).all(), "subnormal means must stay subnormal"
    assert np.isnan(got[9, 8]) and np.isnan(got[8, 7]) and got[8, 5] == np.inf and got[8, 6] == -np.inf


def test_normalized_restatement_scales_rows_first(oracle):
    x, starts, stops = ref.normalize_edge_rows()
    got = ref.pool_normalized(x, starts, stops, oracle)
    assert (got[1] == 0).all()                    # the zero row stays
    assert (got[3] == 0).all()                    # the overflowing norm: factor 0
    assert np.isnan(got[5, 2])                    # inf * 0
    assert np.isnan(got[6, 1]) and same_bits(got[6, 2:], x[40, 2:])  # the NaN row is used as it is
    assert same_bits(got[8], x[60:61].mean(axis=0))                  # norm underflows to 0: unscaled
    y = x[0:10].copy()
    oracle.normalize_l2(y)
    assert same_bits(got[0], y.mean(axis=0))


# ---- the reference's function ----------------------------------------------------------------
@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def golden_ranges(g, name):
    """(starts, stops, annotations) of every domain in the reference's loop order inside one dict, on the packed matrix"""
    first = np.concatenate(([0], np.cumsum(g["lengths"])))[:-1]
    r = g[f"{name}_ranges"]
    return first[r[:, 0]] + r[:, 1] - 1, first[r[:, 0]] + r[:, 2], [str(a) for a in g[f"{name}_annotations"]]


def golden_dicts(g):
    """the embedder and the two range dicts the fixture was made from"""
    ids = [str(i) for i in g["ids"]]
    stops = np.cumsum(g["lengths"])
    emb = [(sid, g["packed"][b - n:b]) for sid, b, n in zip(ids, stops, g["lengths"])]
    dicts = []
    for name in ("test", "train"):
        dd = {sid: [] for sid in ids}
        for (i, a, b), ann in zip(g[f"{name}_ranges"], g[f"{name}_annotations"]):
            dd[ids[i]].append((int(a), int(b), str(ann)))
        dicts.append(dd)
    return emb, dicts[0], dicts[1]


def test_golden_file_is_what_the_script_describes(golden):
    g = golden
    assert g["packed"].dtype == np.float32 and g["packed"].shape == (int(g["lengths"].sum()), 16)
    assert g["lengths"].min() == 1 and g["lengths"].max() == 600 and len(g["lengths"]) >= 24
    assert GOLDEN.stat().st_size < 1 << 20
    for name in ("train", "test"):
        assert len(g[f"{name}_keys"]) < len(g[f"{name}_annotations"]), "an annotation repeats"
        assert g[f"{name}_values"].shape == (len(g[f"{name}_keys"]), 16)


@pytest.mark.parametrize("name", ["train", "test"])
def test_restatement_matches_the_reference_function(golden, name):
    starts, stops, annotations = golden_ranges(golden, name)
    pooled = ref.pool_sequential(golden["packed"], starts, stops)
    data = {}
    for ann, row in zip(annotations, pooled):
        data[ann] = row
    assert list(data) == [str(k) for k in golden[f"{name}_keys"]]
    assert same_bits(np.stack(list(data.values())), golden[f"{name}_values"])


@pytest.mark.gpu
@pytest.mark.parametrize("batch_bytes", [1 << 40, 40000, 1])
def test_extract_domain_representations_matches_the_reference_function(gpu_faiss, golden, batch_bytes):
    """the drop-in, one call and several: the reference's two dicts, keys in its order, values bit for bit"""
    from knn_for_homology_amd import pooling
    emb, test, train = golden_dicts(golden)
    data_test, data_train = pooling.extract_domain_representations(iter(emb), test, train, batch_bytes=batch_bytes)
    for name, data in (("train", data_train), ("test", data_test)):
        assert list(data) == [str(k) for k in golden[f"{name}_keys"]]
        assert same_bits(np.stack(list(data.values())), golden[f"{name}_values"])
