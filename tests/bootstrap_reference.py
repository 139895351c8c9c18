"""The contract of knn_eval_bootstrap (include/knn355.h), restated in numpy and plain Python.

Written from the header: numpy.bincount gives the integer tables, every division is one of two Python floats (a Python
float is an IEEE double, `/` the correctly rounded division, `+` the correctly rounded sum), and the sum over the
families runs in the contract's order.  Nothing is shared with the library.  Used by tests/test_bootstrap_reference.py
(CPU, against what the reference's own bootstrap_scores produced) and tests/test_bootstrap_gpu.py (bit for bit)."""
import numpy as np

BLOCK = 256  # family codes per block of the summation order
MAX_FAMILIES = 16384


def block_order_sum(terms):
    """the contract's sum over family codes: terms[f] is family f's term, None when the family is absent.  Blocks of 256
    consecutive codes, each block from +0.0 over its present families in code order, then the block sums from +0.0 in
    block order"""
    s = 0.0
    for f0 in range(0, len(terms), BLOCK):
        bs = 0.0
        for x in terms[f0:f0 + BLOCK]:
            if x is not None:
                bs = bs + x
        s = s + bs
    return s


def running_sum(terms):
    """one running sum over the present families in code order: NOT the contract (the block-order case tells them apart)"""
    s = 0.0
    for x in terms:
        if x is not None:
            s = s + x
    return s


def family_terms(count, corr):
    """the per-code terms of one (replicate, method): corr / count where the family is present, else None"""
    return [float(int(r)) / float(int(c)) if c else None for c, r in zip(count, corr)]


def bootstrap(is_correct, family, nfam, sample_ids, total=block_order_sum):
    """-> (normalized float64 [nm, nb], raw float64 [nm, nb], correct int64 [nm, nb], present int32 [nb])"""
    is_correct = np.atleast_2d(np.asarray(is_correct)) != 0
    family = np.asarray(family, np.int64)
    sample_ids = np.asarray(sample_ids, np.int64)
    nm, n = is_correct.shape
    nb = sample_ids.shape[0]
    assert n >= 1 and family.shape == (n,) and sample_ids.shape == (nb, n) and 1 <= nfam <= MAX_FAMILIES
    assert family.min() >= 0 and family.max() < nfam and (nb == 0 or (sample_ids.min() >= 0 and sample_ids.max() < n))
    normalized = np.empty((nm, nb), np.float64)
    raw = np.empty((nm, nb), np.float64)
    correct = np.empty((nm, nb), np.int64)
    present = np.empty(nb, np.int32)
    for b in range(nb):
        fam = family[sample_ids[b]]
        count = np.bincount(fam, minlength=nfam)
        present[b] = int(np.count_nonzero(count))
        for m in range(nm):
            corr = np.bincount(fam[is_correct[m][sample_ids[b]]], minlength=nfam)
            correct[m, b] = int(corr.sum())
            raw[m, b] = float(int(correct[m, b])) / float(n)
            normalized[m, b] = total(family_terms(count, corr)) / float(int(present[b]))
    return normalized, raw, correct, present


def scores(is_correct, normalized, boot_normalized, boot_raw):
    """cath.py:420-438 over one method's replicates -> (plus_minus_normalized, plus_minus_raw)"""
    boot_normalized, boot_raw = np.sort(boot_normalized), np.sort(boot_raw)
    nb = len(boot_raw)
    lower, upper = int(nb * 0.025), int(nb * 0.975)
    mean = np.asarray(is_correct, bool).mean()
    return (max(normalized - boot_normalized[lower], boot_normalized[upper] - normalized),
            max(mean - boot_raw[lower], boot_raw[upper] - mean))


def block_order_case():
    """A case that tells the contract's order from one running sum: 700 queries over 513 families, so that far more than
    256 families are present in every replicate (two blocks and the first code of a third), one method that is right
    about half of the time, four replicates.  Found by a seeded search over the seeds 0 .. 19: the two orders give
    different doubles in at least one replicate for 19 of them, and in all four replicates for seed 2, which is taken
    (tests/test_bootstrap_reference.py asserts the inequality).
    -> (is_correct bool [1, 700], family int32 [700], nfam, sample_ids int32 [4, 700])"""
    rng = np.random.default_rng(BLOCK_ORDER_SEED)
    n, nfam = 700, 513
    family = rng.integers(0, nfam, n).astype(np.int32)
    family[:nfam] = rng.permutation(nfam)  # every code occurs
    is_correct = rng.random((1, n)) < 0.5
    sample_ids = rng.integers(0, n, (4, n)).astype(np.int32)
    return is_correct, family, nfam, sample_ids


BLOCK_ORDER_SEED = 2
