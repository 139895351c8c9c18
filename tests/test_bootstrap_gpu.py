"""GPU: knn_eval_bootstrap (csrc/bootstrap.inc) bit for bit against tests/bootstrap_reference.py, and the facade on top
of it (evaluation.bootstrap_replicates, bootstrap_scores, class_accuracies) against what the reference's own
bootstrap_scores produced (tests/golden/reference_bootstrap.npz).

bootstrap_kernel gives a workgroup of 256 threads to one (replicate, method): the threads stride over the n samples and
add into two LDS histograms of nfam words, then one wave per block of 256 family codes forms the terms 64 codes at a
time and adds them in code order, and thread 0 adds the block sums.  The shapes here sit where that can go wrong: sample
counts around a wave and the workgroup, family counts around a wave, a block and two blocks and at the cap, families
that no sample carries, one LDS word that takes every atomic, slabs.  Doubles are compared as uint64 patterns, integers
with array_equal; there is no tolerance anywhere except against the reference's own pairwise sums (the bound of
tests/test_bootstrap_reference.py)."""
from pathlib import Path

import numpy as np
import pytest

import bootstrap_reference as ref

pytestmark = pytest.mark.gpu

KNOB = "KNN355_EVAL_SLAB_ROWS"
KNN_ERR_INVALID = -1
S64, S32, SD = -7777, -7777, -7777.25  # what the output arrays hold before a call
GOLDEN = Path(__file__).resolve().parent / "golden" / "reference_bootstrap.npz"
CASES = ["n37_f5", "n150_f40", "n400_f300", "n400_f1", "possible"]


def _ptr(a):
    return None if a is None else a.ctypes.data


def _last_error():
    from knn_for_homology_amd import _lib
    return _lib.lib().knn_last_error().decode()


def c_bootstrap(is_correct_, family_, nfam, sample_ids_, **over):
    """the C entry point -> (return code, normalized, raw, correct, present), the outputs pre-filled with the sentinels;
    `over` replaces arguments by name (nm, n, nb, nfam) or drops a pointer (family=None ...)"""
    from knn_for_homology_amd import _lib
    is_correct = np.ascontiguousarray(np.atleast_2d(is_correct_), np.uint8)
    family = np.ascontiguousarray(family_, np.int32)
    sample_ids = np.ascontiguousarray(sample_ids_, np.int32)
    nm, n = is_correct.shape
    nb = sample_ids.shape[0]
    shape = (max(nm, 1), max(nb, 1))
    a = dict(is_correct=is_correct, nm=nm, n=n, family=family, nfam=nfam, sample_ids=sample_ids, nb=nb, correct=np.full(shape, S64, np.int64),
             present=np.full(shape[1], S32, np.int32), normalized=np.full(shape, SD), raw=np.full(shape, SD))
    outs = [a[name] for name in ("normalized", "raw", "correct", "present")]
    a.update(over)
    rc = _lib.lib().knn_eval_bootstrap(_ptr(a["is_correct"]), a["nm"], a["n"], _ptr(a["family"]), a["nfam"], _ptr(a["sample_ids"]), a["nb"],
                                       _ptr(a["correct"]), _ptr(a["present"]), _ptr(a["normalized"]), _ptr(a["raw"]))
    return (rc, *outs)


def _same(got, want):
    rc, normalized, raw, correct, present = got
    assert rc == 0, _last_error()
    assert np.array_equal(correct, want[2]), "correct_out"
    assert np.array_equal(present, want[3]), "present_out"
    assert np.array_equal(raw.view(np.uint64), want[1].view(np.uint64)), "raw_out (as bits)"
    assert np.array_equal(normalized.view(np.uint64), want[0].view(np.uint64)), "normalized_out (as bits)"


def _check(is_correct, family, nfam, sample_ids):
    want = ref.bootstrap(is_correct, family, nfam, sample_ids)
    _same(c_bootstrap(is_correct, family, nfam, sample_ids), want)
    return want


def _case(rng, nm, n, nfam, nb, used=None):
    """family codes drawn from `used` of the nfam codes (default: all of them), the first and the last code always
    among them; methods that are right with probabilities from 0 to 1, stored as the bytes 1, 2 and 255; resamples with
    replacement"""
    codes = np.arange(nfam) if used is None else np.sort(rng.choice(nfam, used, replace=False))
    codes[0], codes[-1] = 0, nfam - 1
    family = rng.choice(codes, n).astype(np.int32)
    family[rng.integers(0, n)] = nfam - 1
    p = np.linspace(0, 1, nm + 2)[1:-1, None]
    is_correct = (rng.random((nm, n)) < p).astype(np.uint8) * rng.choice(np.array([1, 2, 255], np.uint8), (nm, n))
    sample_ids = rng.integers(0, n, (nb, n)).astype(np.int32)
    return is_correct, family, nfam, sample_ids


# ---- samples around a wave and the workgroup, families around a wave, a block, two blocks and at the cap ---------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1000])
def test_sample_counts(gpu_faiss, n):
    rng = np.random.default_rng(n)
    _check(*_case(rng, 2, n, 7, 3))
    want = _check(*_case(rng, 1, n, 300, 3))  # two blocks of codes, most of them absent when n is small
    assert n > 257 or (want[3] < 300).all()


@pytest.mark.parametrize("nfam", [1, 2, 255, 256, 257, 513, 16384])
def test_family_counts(gpu_faiss, nfam):
    """1000 samples: at nfam = 1 every atomic of a workgroup lands on one LDS word; at 16384 the arrays are at the cap
    (128 KiB of LDS) and sparse: most families are absent, and no 0 / 0 may show"""
    rng = np.random.default_rng(nfam)
    want = _check(*_case(rng, 2, 1000, nfam, 3))
    assert np.isfinite(want[0]).all() and (want[3] == 1).all() == (nfam == 1) and (nfam < 1000 or (want[3] < nfam).all())
    assert nfam > 2 or (want[3] == nfam).any()


def test_more_families_than_samples_and_codes_nobody_carries(gpu_faiss):
    rng = np.random.default_rng(21)
    for n, nfam, used in ((40, 513, 30), (300, 16384, 200), (65, 257, 2), (1000, 700, 350)):
        is_correct, family, _, sample_ids = _case(rng, 2, n, nfam, 4, used=used)
        assert len(np.unique(family)) <= used + 1 < nfam
        want = _check(is_correct, family, nfam, sample_ids)
        assert (want[3] <= used + 1).all() and np.isfinite(want[0]).all()


@pytest.mark.parametrize("nm", [1, 2, 5])
@pytest.mark.parametrize("nb", [1, 3, 500])
def test_methods_and_replicates(gpu_faiss, nm, nb):
    rng = np.random.default_rng(10 * nm + nb)
    want = _check(*_case(rng, nm, 130, 20, nb))
    assert want[0].shape == (nm, nb) and want[3].shape == (nb,)


def test_one_id_repeated_n_times(gpu_faiss):
    """replicate 0 draws query 5 every time, replicate 1 query 6, replicate 2 is ordinary: one family present, all of its
    samples correct or none of them"""
    rng = np.random.default_rng(22)
    is_correct, family, nfam, sample_ids = _case(rng, 1, 300, 260, 3)
    is_correct[0, 5], is_correct[0, 6] = 1, 0
    sample_ids[0], sample_ids[1] = 5, 6
    want = _check(is_correct, family, nfam, sample_ids)
    assert want[3][:2].tolist() == [1, 1] and want[2][0, :2].tolist() == [300, 0]
    assert want[0][0, :2].tolist() == [1.0, 0.0] and want[1][0, :2].tolist() == [1.0, 0.0]


def test_always_right_is_one_and_never_right_is_plus_zero(gpu_faiss):
    rng = np.random.default_rng(23)
    _, family, nfam, sample_ids = _case(rng, 1, 1000, 600, 6)
    both = np.stack([np.full(1000, 255, np.uint8), np.zeros(1000, np.uint8)])
    rc, normalized, raw, correct, present = c_bootstrap(both, family, nfam, sample_ids)
    assert rc == 0 and (normalized[0] == 1.0).all() and (raw[0] == 1.0).all() and (correct[0] == 1000).all()
    assert (normalized[1].view(np.uint64) == 0).all() and (raw[1].view(np.uint64) == 0).all() and (correct[1] == 0).all()
    assert (present > 256).all()


def test_block_sums_are_added_in_block_order(gpu_faiss):
    """the case of tests/test_bootstrap_reference.py in which one running sum over the codes gives other doubles"""
    is_correct, family, nfam, sample_ids = ref.block_order_case()
    want = _check(is_correct, family, nfam, sample_ids)
    running = ref.bootstrap(is_correct, family, nfam, sample_ids, total=ref.running_sum)
    assert (want[0] != running[0]).any()


# ---- slabs ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def slab_case():
    rng = np.random.default_rng(24)
    case = _case(rng, 3, 200, 300, 20)
    return case, ref.bootstrap(*case)


@pytest.mark.parametrize("rows", [None, "1", "7"])
def test_slabs(gpu_faiss, slab_case, monkeypatch, rows):
    """20 replicates in one slab, in 20 and in three (7, 7, 6): the same bits"""
    case, want = slab_case
    if rows is None:
        monkeypatch.delenv(KNOB, raising=False)
    else:
        monkeypatch.setenv(KNOB, rows)
    _same(c_bootstrap(*case), want)


# ---- the Python facade against the reference's numbers ---------------------------------------------------------------
@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as f:
        return {name: f[name] for name in f.files}


@pytest.mark.parametrize("name", CASES)
def test_facade_on_the_reference_cases(gpu_faiss, golden, name):
    from knn_for_homology_amd.evaluation import bootstrap_replicates, bootstrap_samples, bootstrap_scores
    g = {key[len(name) + 1:]: golden[key] for key in golden if key.startswith(name + "_")}
    possible = g["is_possible"]
    labels = g["mapping_array"][possible, 0]  # (the fixture's labels are not dense codes)
    is_correct = g["is_correct"][:, possible]
    nm, n = is_correct.shape
    sample_ids = bootstrap_samples(n)
    assert np.array_equal(sample_ids, golden[f"samples_{n}"])
    normalized, raw, correct, present = bootstrap_replicates(is_correct, labels, sample_ids)
    assert normalized.shape == raw.shape == correct.shape == (nm, 500) and present.shape == (500,)
    assert np.array_equal(raw.view(np.uint64), g["boot_raw"].view(np.uint64)), "raw against the reference's list (as bits)"
    assert np.array_equal(correct, np.rint(g["boot_raw"] * n).astype(np.int64))
    assert np.array_equal(present, [len(set(labels[row].tolist())) for row in sample_ids])
    bound = 2 * (n + 2) * 2.0 ** -53
    d = np.abs(normalized - g["boot_normalized"]).max()
    print(f"{name}: |normalized - reference| <= {d:.3e}, bound {bound:.3e}")
    assert d <= bound
    _, family = np.unique(labels, return_inverse=True)
    _same((0, normalized, raw, correct, present), ref.bootstrap(is_correct, family, int(family.max()) + 1, sample_ids))
    for m in range(nm):
        got = bootstrap_scores(is_correct[m], float(g["normalized"][m]), labels)
        assert isinstance(got[0], float) and isinstance(got[1], float)
        dn, dr = abs(got[0] - g["plus_minus"][m][0]), abs(got[1] - g["plus_minus"][m][1])
        print(f"{name}[{m}]: |tuple - reference| = {dn:.3e}, {dr:.3e}, bound {bound + 2.0 ** -52:.3e}")
        assert dn <= bound + 2.0 ** -52 and dr <= bound + 2.0 ** -52
        one = bootstrap_replicates(is_correct[m], labels, sample_ids)
        assert one[0].shape == (500,) and np.array_equal(one[0].view(np.uint64), normalized[m].view(np.uint64)) and np.array_equal(one[2], correct[m])


def test_class_accuracies_batches_the_methods(gpu_faiss, golden):
    """the is_possible case: one batched call for the three methods equals one bootstrap_scores call per method"""
    from knn_for_homology_amd.evaluation import bootstrap_scores, class_accuracies
    mapping_array, possible, is_correct = golden["possible_mapping_array"], golden["possible_is_possible"], golden["possible_is_correct"]
    methods = {f"method {m}": is_correct[m][:, None, None] & np.ones((1, 3, 2), bool) for m in range(3)}
    got = class_accuracies(methods, mapping_array, bootstrap=True)
    plain = class_accuracies(methods, mapping_array)
    assert list(got) == list(plain) == ["method 2", "method 1", "method 0"]
    bound = 2 * (int(possible.sum()) + 2) * 2.0 ** -53 + 2.0 ** -52
    for m in range(3):
        row = got[f"method {m}"]
        assert len(row) == 4 and row[:2] == plain[f"method {m}"]
        assert row[0] == golden["possible_normalized"][m] and row[1] == is_correct[m][possible].mean()
        want = bootstrap_scores(is_correct[m][possible], row[0], mapping_array[possible, 0])
        assert (row[2], row[3]) == want
        assert abs(row[2] - golden["possible_plus_minus"][m][0]) <= bound and abs(row[3] - golden["possible_plus_minus"][m][1]) <= bound
    # resamples handed in: fewer replicates, the same for every method
    from knn_for_homology_amd.evaluation import bootstrap_samples
    ids = bootstrap_samples(int(possible.sum()), 40, seed=7)
    few = class_accuracies(methods, mapping_array, bootstrap=True, sample_ids=ids)
    assert few["method 1"][2:] == bootstrap_scores(is_correct[1][possible], few["method 1"][0], mapping_array[possible, 0], sample_ids=ids)
    assert few["method 1"][2:] == class_accuracies(methods, mapping_array, bootstrap=True, replicates=40, seed=7)["method 1"][2:]


def test_facade_refuses_before_the_library_is_called(gpu_faiss):
    from knn_for_homology_amd.evaluation import bootstrap_replicates, bootstrap_scores
    is_correct = np.ones((2, 6), bool)
    families = np.arange(6) // 2
    ids = np.zeros((3, 6), np.int64)
    for bad in (np.ones((2, 2, 6), bool), np.bool_(True)):
        with pytest.raises(ValueError, match="is_correct"):
            bootstrap_replicates(bad, families, ids)
    for bad in (families[:5], families.reshape(2, 3)):
        with pytest.raises(ValueError, match="families"):
            bootstrap_replicates(is_correct, bad, ids)
    for bad in (ids[:, :5], ids.ravel(), ids[0]):
        with pytest.raises(ValueError, match="sample_ids"):
            bootstrap_replicates(is_correct, families, bad)
    for value in (-1, 6, 2**32):  # (2**32 would wrap to 0 in int32)
        bad = ids.copy()
        bad[1, 2] = value
        with pytest.raises(ValueError, match="lie in"):
            bootstrap_replicates(is_correct, families, bad)
    with pytest.raises(ValueError, match="one query"):
        bootstrap_replicates(np.ones((2, 0), bool), families[:0], ids[:, :0])
    with pytest.raises(ValueError, match="distinct labels"):
        bootstrap_replicates(np.ones(16385, bool), np.arange(16385), np.zeros((1, 16385), np.int32))
    with pytest.raises(ValueError, match="one value per method"):
        bootstrap_scores(is_correct, [0.5], families, sample_ids=ids)
    with pytest.raises(ValueError, match="one replicate"):
        bootstrap_scores(is_correct[0], 0.5, families, sample_ids=ids[:0])
    normalized, raw, correct, present = bootstrap_replicates(is_correct, families, ids)  # every sample is query 0
    assert normalized.tolist() == [[1.0] * 3] * 2 and raw.tolist() == [[1.0] * 3] * 2 and correct.tolist() == [[6] * 3] * 2 and present.tolist() == [1] * 3
    assert bootstrap_replicates(is_correct, families, ids[:0])[0].shape == (2, 0)


# ---- errors: refused on the host, nothing allocated or launched, the outputs as they were ------------------------------
def _refused(got, what):
    rc, normalized, raw, correct, present = got
    assert rc == KNN_ERR_INVALID and what in _last_error(), _last_error()
    assert (normalized == SD).all() and (raw == SD).all() and (correct == S64).all() and (present == S32).all()


def _untouched(got):
    rc, normalized, raw, correct, present = got
    assert rc == 0, _last_error()
    assert (normalized == SD).all() and (raw == SD).all() and (correct == S64).all() and (present == S32).all()


def test_bootstrap_refusals(gpu_faiss):
    is_correct = np.ones((2, 5), np.uint8)
    family = np.array([0, 1, 2, 2, 1], np.int32)
    ids = np.array([[0, 1, 2, 3, 4], [4, 4, 0, 0, 1], [1, 1, 1, 1, 1]], np.int32)  # (families present: 3, 2, 1)
    _refused(c_bootstrap(is_correct, family, 3, ids, nm=-1), "nm")
    _refused(c_bootstrap(is_correct, family, 3, ids, nb=-1), "nb")
    _refused(c_bootstrap(is_correct, family, 3, ids, n=-1), "n < 0")
    _refused(c_bootstrap(is_correct, family, 3, ids, n=0), "n >= 1")
    _refused(c_bootstrap(is_correct, family, 3, ids, n=2**31), "n > INT32_MAX")
    for nfam in (0, -1, 16385):
        _refused(c_bootstrap(is_correct, family, nfam, ids), "nfam")
    for name in ("is_correct", "family", "sample_ids", "correct", "present", "normalized", "raw"):
        _refused(c_bootstrap(is_correct, family, 3, ids, **{name: None}), "null pointer")
    for bad in ([0, 1, 3, 2, 1], [0, 1, 2, 2, -1], [2**31 - 1, 0, 0, 0, 0]):
        _refused(c_bootstrap(is_correct, bad, 3, ids), "family")
    _refused(c_bootstrap(is_correct, family, 2, ids), "family")  # (the same codes under a smaller nfam)
    for r, c, value in ((0, 0, -1), (2, 4, 5), (1, 2, 2**31 - 1), (2, 0, -2**31)):
        bad = ids.copy()
        bad[r, c] = value
        _refused(c_bootstrap(is_correct, family, 3, bad), "sample_ids")
    # nothing to do: 0 before any pointer or any other argument is looked at
    _untouched(c_bootstrap(is_correct, family, 3, ids, nm=0))
    _untouched(c_bootstrap(is_correct, family, 3, ids, nb=0))
    _untouched(c_bootstrap(is_correct, family, 3, ids, nm=0, is_correct=None, family=None, sample_ids=None, correct=None, raw=None))
    _untouched(c_bootstrap(is_correct, family, 3, ids, nb=0, n=0, present=None, normalized=None))
    # and the same arguments pass once they are right
    rc, normalized, raw, correct, present = c_bootstrap(is_correct, family, 3, ids)
    assert rc == 0 and present.tolist() == [3, 2, 1] and correct.tolist() == [[5, 5, 5]] * 2
    assert normalized.tolist() == [[1.0, 1.0, 1.0]] * 2 and raw.tolist() == [[1.0, 1.0, 1.0]] * 2
