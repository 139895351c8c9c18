"""CPU: tests/bootstrap_reference.py (the restatement the GPU tests compare knn_eval_bootstrap with) against
tests/golden/reference_bootstrap.npz, what the reference's own bootstrap_scores (cath/cath.py:404-438) produced
(tests/golden/make_bootstrap_golden.py), and the host-side parts of the facade (the resample stream, class_accuracies
without the bootstrap).

The raw replicates are exact integers over n on both sides and are compared exactly, as are the integer tables against a
direct count.  The reference sums n products c_i * (1 / n_f(i)) with numpy's pairwise sum, the contract sums one quotient
per present family in blocks of 256 codes: two summation orders of at most n non-negative terms whose sum is at most
`present`, one extra rounding per term, and the final division by `present` differ by at most 2 * (n + 2) * 2**-53 --
derived, nothing measured.  The final tuple is a difference of two such numbers and the point estimate: that bound plus
2**-52.  The block order itself is checked on a case in which the orders differ."""
from pathlib import Path

import numpy as np
import pytest

import bootstrap_reference as ref

GOLDEN = Path(__file__).resolve().parent / "golden" / "reference_bootstrap.npz"
CASES = ["n37_f5", "n150_f40", "n400_f300", "n400_f1", "possible"]


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as f:
        return {name: f[name] for name in f.files}


def case_inputs(golden, name):
    """-> (is_correct bool [nm, n], family codes int32 [n], nfam, sample_ids int32 [500, n], the case's arrays)"""
    g = {key[len(name) + 1:]: golden[key] for key in golden if key.startswith(name + "_")}
    possible = g["is_possible"]
    labels, family = np.unique(g["mapping_array"][possible, 0], return_inverse=True)
    is_correct = g["is_correct"][:, possible]
    return is_correct, family.astype(np.int32), len(labels), golden[f"samples_{is_correct.shape[1]}"].astype(np.int32), g


@pytest.fixture(scope="module")
def restated(golden):
    """name -> (inputs, the restatement's four outputs), computed once"""
    return {name: (case_inputs(golden, name), ref.bootstrap(*case_inputs(golden, name)[:4])) for name in CASES}


def replicate_bound(n):
    return 2 * (n + 2) * 2.0 ** -53


def test_fixture_holds_the_cases_of_the_issue(golden):
    assert sorted(golden["cases"].tolist()) == sorted(CASES)
    for name, n, nfam in (("n37_f5", 37, 5), ("n150_f40", 150, 40), ("n400_f300", 400, 300), ("n400_f1", 400, 1)):
        is_correct, family, got_nfam, sample_ids, g = case_inputs(golden, name)
        assert is_correct.shape == (1, n) and got_nfam == nfam and g["is_possible"].all() and sample_ids.shape == (500, n)
    is_correct, family, nfam, sample_ids, g = case_inputs(golden, "possible")
    assert 0 < g["is_possible"].sum() < len(g["is_possible"]) and is_correct.shape == (3, g["is_possible"].sum()) and nfam > 10
    assert g["mapping_array"].shape[1] == 3
    for name in CASES:
        assert golden[f"{name}_boot_normalized"].shape == golden[f"{name}_boot_raw"].shape == (golden[f"{name}_is_correct"].shape[0], 500)
        assert golden[f"{name}_plus_minus"].shape == (golden[f"{name}_is_correct"].shape[0], 2)
    assert all(golden[key].dtype == np.uint16 for key in golden if key.startswith("samples_"))


@pytest.mark.parametrize("name", CASES)
def test_integers_and_raw_are_exact(restated, name):
    (is_correct, family, nfam, sample_ids, g), (_, raw, correct, present) = restated[name]
    n = is_correct.shape[1]
    assert np.array_equal(raw.view(np.uint64), g["boot_raw"].view(np.uint64)), "raw against the reference's list (as bits)"
    assert np.array_equal(correct, np.rint(g["boot_raw"] * n).astype(np.int64))
    assert np.array_equal(correct, is_correct[:, sample_ids].sum(axis=2))
    assert np.array_equal(present, [len(set(family[row].tolist())) for row in sample_ids])
    assert present.max() <= nfam and (name != "n400_f300" or present.max() < nfam)  # (families absent from a resample)


@pytest.mark.parametrize("name", CASES)
def test_normalized_within_the_bound_of_two_summation_orders(restated, name):
    (is_correct, family, nfam, sample_ids, g), (normalized, raw, _, _) = restated[name]
    bound = replicate_bound(is_correct.shape[1])
    d = np.abs(normalized - g["boot_normalized"]).max()
    print(f"{name}: |normalized - reference| <= {d:.3e}, bound {bound:.3e}")
    assert d <= bound
    for m in range(is_correct.shape[0]):
        got = ref.scores(is_correct[m], g["normalized"][m], normalized[m], raw[m])
        dn, dr = abs(got[0] - g["plus_minus"][m][0]), abs(got[1] - g["plus_minus"][m][1])
        print(f"{name}[{m}]: |tuple - reference| = {dn:.3e}, {dr:.3e}, bound {bound + 2.0 ** -52:.3e}")
        assert dn <= bound + 2.0 ** -52 and dr == 0.0


def test_one_family_gives_the_raw_mean(restated):
    """nfam = 1: the only term is correct / n, divided by one present family"""
    _, (normalized, raw, _, present) = restated["n400_f1"]
    assert (present == 1).all() and np.array_equal(normalized.view(np.uint64), raw.view(np.uint64))


def test_resample_stream_is_the_reference_s(golden):
    """numpy's default_rng(42).choice(n, n) stream: a numpy whose stream has drifted from the fixture's fails here"""
    from knn_for_homology_amd.evaluation import bootstrap_samples
    for key in sorted(k for k in golden if k.startswith("samples_")):
        n = int(key[len("samples_"):])
        got = bootstrap_samples(n)
        assert got.dtype == np.int32 and got.shape == (500, n)
        assert np.array_equal(got, golden[key]), f"bootstrap_samples({n}) under numpy {np.__version__}, fixture from {golden['numpy_version']}"
    assert np.array_equal(bootstrap_samples(37, 3), golden["samples_37"][:3])
    assert not np.array_equal(bootstrap_samples(37, 3, seed=43), golden["samples_37"][:3])
    assert bootstrap_samples(5, 0).shape == (0, 5)
    with pytest.raises(ValueError):
        bootstrap_samples(0)


def test_block_order_case_tells_the_orders_apart():
    is_correct, family, nfam, sample_ids = ref.block_order_case()
    blocks, _, _, present = ref.bootstrap(is_correct, family, nfam, sample_ids)
    running, _, _, _ = ref.bootstrap(is_correct, family, nfam, sample_ids, total=ref.running_sum)
    assert nfam == 513 and present.min() > 256
    assert (blocks != running).any(), "the case no longer tells the block order from a running sum"
    assert np.abs(blocks - running).max() <= replicate_bound(len(family))


@pytest.mark.parametrize("count", [255, 256, 257, 513])
def test_block_order_sum(count):
    """1.0 and then 2**-53 again and again: a running sum stays at 1.0 (every addition is a tie that rounds to even).  Up
    to 257 terms the block order is that running sum (the second block holds one term); at 513 the second block sums to
    256 * 2**-53 = 2**-45 first, which then counts."""
    tiny = 2.0 ** -53
    terms = [1.0] + [tiny] * (count - 1)
    assert ref.running_sum(terms) == 1.0
    want = 1.0 if count <= 257 else (1.0 + 2.0 ** -45) + tiny
    assert ref.block_order_sum(terms) == want and (count <= 257 or want == 1.0 + 2.0 ** -45 != 1.0)
    # absent families take a code and add nothing
    holes = [None] * count
    holes[0], holes[count - 1] = 1.0, 2.0 ** -52
    assert ref.block_order_sum(holes) == 1.0 + 2.0 ** -52
    assert ref.block_order_sum([None] * count) == 0.0 and np.signbit(ref.block_order_sum([None] * count)) == False  # noqa: E712
    # the blocks are blocks of codes, not of present families: codes 256 and 257 meet each other before they meet code 0
    if count == 513:
        split = [1.0] + [None] * 255 + [tiny, tiny] + [None] * 255
        assert len(split) == count and ref.block_order_sum(split) == 1.0 + 2.0 ** -52 and ref.running_sum(split) == 1.0


def test_always_right_is_one_and_never_right_is_plus_zero(golden):
    is_correct, family, nfam, sample_ids, _ = case_inputs(golden, "n400_f300")
    both = np.stack([np.ones(400, bool), np.zeros(400, bool)])
    normalized, raw, correct, present = ref.bootstrap(both, family, nfam, sample_ids[:40])
    assert (normalized[0] == 1.0).all() and (raw[0] == 1.0).all() and (correct[0] == 400).all()
    assert (normalized[1].view(np.uint64) == 0).all() and (raw[1].view(np.uint64) == 0).all() and (correct[1] == 0).all()


def test_class_accuracies_without_bootstrap():
    """a three-level mapping with singleton families, which is_possible drops: cath.py:446-447 evaluated directly"""
    from knn_for_homology_amd.evaluation import class_accuracies
    level0 = np.array([5, 5, 5, 9, 9, 2, 7, 7, 7, 7, 3, 11])  # families of 3, 2, 4 members and three singletons
    mapping_array = np.stack([level0, np.arange(12) % 3, np.arange(12) % 2], axis=1)
    rng = np.random.default_rng(4)
    methods = {name: rng.random((12, 3, 4)) < p for name, p in (("low", 0.2), ("high", 0.9), ("mid", 0.5))}
    methods["flat"] = methods["mid"][:, 0, 0].copy()  # the [n] column itself
    is_possible = np.array([True] * 5 + [False] + [True] * 4 + [False] * 2)
    normalization = np.array([1 / 3] * 3 + [1 / 2] * 2 + [0] + [1 / 4] * 4 + [0] * 2)
    families_count = 3
    got = class_accuracies(methods, mapping_array)
    want = {name: ((ic[:, 0, 0] * normalization).sum() / families_count, ic[is_possible, 0, 0].mean())
            for name, ic in methods.items() if ic.ndim == 3}
    want["flat"] = want["mid"]
    assert set(got) == set(want) and all(got[name] == want[name] for name in want)
    values = [v[0] for v in got.values()]
    assert values == sorted(values, reverse=True) and list(got).index("mid") < list(got).index("flat")  # (equal values: input order)
    # a verdict about a singleton does not count
    flipped = {"low": methods["low"].copy()}
    flipped["low"][[5, 10, 11]] ^= True
    assert class_accuracies(flipped, mapping_array)["low"] == got["low"]
    with pytest.raises(ValueError, match="mapping_array"):
        class_accuracies(methods, level0)
    with pytest.raises(ValueError, match="one row per row"):
        class_accuracies({"short": np.ones(11, bool)}, mapping_array)
    with pytest.raises(ValueError, match="more than one member"):
        class_accuracies({"x": np.ones(3, bool)}, np.array([[1], [2], [3]]))
