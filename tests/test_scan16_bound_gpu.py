"""GPU: the exact 16-bit prefilter at the edge of its error bound, on the adversarial cases of
tests/scan16_reference.py: rows and queries whose copy error is aligned with the other side (|s - s~| at 0.94 of B_q),
rows whose signal the copy flushes to zero, rows at and below the exponent clamp, fp32 subnormals, either side of the
exponent gate, a norm that overflows a float, statistics that grow over several adds and must shrink at a reset.

Every search is compared bit for bit with the CPU oracle and with the same index under KNN_TUNE_NO_SCAN16, and
`knn_last_scan16_info` with the reference's prediction: the fallback counter grows by one exactly when the model flags a
query or finds a window that does not fit, and `candidates_max` is the model's largest window -- derived from the formula,
never recorded from the library (tests/test_scan16_reference.py proves the predictions robust against the library's
round-up margins).

Where a search falls back, its D and I are the gated fp32 search's, so the comparison with the oracle says nothing about
the prefilter there; only the counter and `candidates_max` do.  The searches that deliver the prefilter's own output
(fallbacks +0) are: the aligned cases, `flushed_fits`, `tiny_d64` (every top-10 needs rows whose exponent is clamped, all
scores subnormal), `subnormal_query_d64`, `subnormal_scores_d64_p125`, `gate_pass`, the unflagged gate queries one by
one, and everything after a reset.  The `subnormal_scores_d{64,1024,1280}` searches and `tiny_subnormal_query_d64`
always fall back: with scores that small B exceeds every gap.  So no GPU test can tell the bound's last term
(dp + 1) 2^-149 from the 2^-140 it replaced at d = 1280; that fix rests on the CPU model alone
(test_scan16_reference.py::test_parent_tail_is_violated_at_1280).  At d = 64 the two do differ on the GPU:
`subnormal_scores_d64_p125` predicts its windows (14 rows) from a B of 65 x 2^-149, and 512 x 2^-149 would widen them.

Mutated libraries were not run on a GPU (B_q scaled by 0.9; the flush left out of `s16_convert`), so nobody has measured
which of these tests such a build fails.  What stands in for it is on the CPU: with 0.9 B_ref the model's window loses
the victim of `aligned_rows_d64` and `aligned_query_d64` (test_scan16_reference.py::test_aligned_cases_reach_the_edge),
so a library with that bound must return the decoy in `test_case[aligned_rows_d64]`, `test_case[aligned_query_d64]`, the
view, shard-key and add-order tests; at d = 1024 the g terms are 67 % of B and hide a 10 % loss.  A build without the flush
would not be seen through `candidates_max`: where an entry is flushed the g terms exceed |q| R by 2^5 / sqrt(d) and more,
so the window barely moves (see the reference test's docstring); the flushed cases pin the tie of exactly-zero approximate
scores and the count instead."""
import numpy as np
import pytest

import scan16_reference as sr
from knn_for_homology_amd._lib import KNN_TUNE_NO_SCAN16, KNN_TUNE_SCAN16_ANY_NB

pytestmark = pytest.mark.gpu

IP = 0
CASES = sr.all_cases()


def _same(a, b):
    return np.array_equal(a[1], b[1]) and np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32))


def _new(faiss, d):
    idx = faiss.IndexFlat(d, IP)
    idx.set_scan16(1)
    return idx


def _check(idx, xb, xq, k, oracle, pred):
    """one prefiltered search of idx (which holds xb) against the oracle, the fp32 path and the model's prediction"""
    before = idx.last_scan16()["fallbacks"]
    idx.set_tuning(0, 0, KNN_TUNE_SCAN16_ANY_NB)
    got = idx.search(xq, k)
    info = idx.last_scan16()
    assert info["used"], info
    assert idx.last_scan()["kernel"] == "flat_scan_q32_d256_f16x", idx.last_scan()  # (a gated fallback leaves the report to the 16-bit pass)
    idx.set_tuning(0, 0, KNN_TUNE_NO_SCAN16)
    ref = idx.search(xq, k)
    assert not idx.last_scan16()["used"]
    idx.set_tuning(0, 0, 0)
    assert _same(got, oracle.flat_search(xb, xq, k, IP)), "16-bit prefilter differs from the oracle"
    assert _same(got, ref), "16-bit prefilter differs from the fp32 scan"
    print(f"fallbacks +{info['fallbacks'] - before} (predicted {int(pred['fallback'])}), candidates_max {info['candidates_max']} "
          f"(predicted {pred['candidates_max']})")
    assert info["fallbacks"] - before == (1 if pred["fallback"] else 0), info
    assert info["candidates_max"] == pred["candidates_max"], (info, pred["candidates_max"])
    return info


@pytest.mark.parametrize("name", [n for n in CASES if n != "overflowing_norm"])
def test_case(gpu_faiss, oracle, name):
    c = CASES[name]
    pred = sr.predict(c.xb, c.xq, c.k)
    assert pred["fallback"] == c.expect["fallback"]  # (which searches deliver the prefilter's own output is the construction's)
    idx = _new(gpu_faiss, c.xb.shape[1])
    idx.add(c.xb)
    _check(idx, c.xb, c.xq, c.k, oracle, pred)


def test_tiny_queries_one_by_one(gpu_faiss, oracle):
    """the clamped rows' index, each query alone (no fallback), then the subnormal query (all scores 0: falls back), then
    the first again"""
    c, sub = CASES["tiny_d64"], CASES["tiny_subnormal_query_d64"]
    idx = _new(gpu_faiss, c.xb.shape[1])
    idx.add(c.xb)
    for xq, fb in [(c.xq[q:q + 1], False) for q in range(len(c.xq))] + [(sub.xq, True), (c.xq[:1], False)]:
        pred = sr.predict(c.xb, xq, c.k)
        assert pred["fallback"] == fb and (fb or pred["candidates_max"] >= c.k)
        _check(idx, c.xb, xq, c.k, oracle, pred)


def test_gate_queries_one_by_one(gpu_faiss, oracle):
    """either side of e_q + EMAX > 80 on one index: each query alone, the flagged ones fall back"""
    c = CASES["gate_over"]
    idx = _new(gpu_faiss, c.xb.shape[1])
    idx.add(c.xb)
    for q in range(len(c.xq)):
        pred = sr.predict(c.xb, c.xq[q:q + 1], c.k)
        assert pred["fallback"] == (q in (1, 3))
        _check(idx, c.xb, c.xq[q:q + 1], c.k, oracle, pred)


def test_overflowing_norm_until_reset(gpu_faiss, oracle):
    """finite rows whose norm is not: X = +inf, every search falls back until the reset; benign rows afterwards take the path"""
    c = CASES["overflowing_norm"]
    idx = _new(gpu_faiss, c.xb.shape[1])
    idx.add(c.xb)
    pred = sr.predict(c.xb, c.xq, c.k)
    assert pred["fallback"] and pred["candidates_max"] == 0
    _check(idx, c.xb, c.xq, c.k, oracle, pred)
    _check(idx, c.xb, c.xq[:1], c.k, oracle, sr.predict(c.xb, c.xq[:1], c.k))
    idx.reset()
    b = CASES["aligned_rows_d64"]
    idx.add(b.xb)
    pred = sr.predict(b.xb, b.xq, b.k)
    assert not pred["fallback"]
    _check(idx, b.xb, b.xq, b.k, oracle, pred)


def test_aligned_rows_through_a_view(gpu_faiss, oracle):
    c = CASES["aligned_rows_d64"]
    idx = _new(gpu_faiss, c.xb.shape[1])
    idx.add(c.xb)
    _check(idx.view(), c.xb, c.xq, c.k, oracle, sr.predict(c.xb, c.xq, c.k))


def test_aligned_rows_as_shard_keys(gpu_faiss, oracle):
    """HipShardBackend.search_keys with an id base: the packed keys of the prefiltered search, no fallback"""
    import torch
    from knn_for_homology_amd.sharded import HipShardBackend
    c = CASES["aligned_rows_d64"]
    base = 70001
    pred = sr.predict(c.xb, c.xq, c.k)
    b = HipShardBackend(c.xb.shape[1], IP)
    b.add(c.xb)
    q = torch.from_numpy(c.xq).cuda()
    before = b.index.last_scan16()["fallbacks"]
    b.index.set_tuning(0, 0, KNN_TUNE_SCAN16_ANY_NB)
    keys = b.search_keys(q, c.k, base).cpu().numpy()
    info = b.index.last_scan16()
    assert info["used"] and info["fallbacks"] == before and info["candidates_max"] == pred["candidates_max"], info
    b.index.set_tuning(0, 0, KNN_TUNE_NO_SCAN16)
    ref = b.search_keys(q, c.k, base).cpu().numpy()
    b.index.set_tuning(0, 0, 0)
    assert not b.index.last_scan16()["used"]
    assert np.array_equal(keys, ref)
    _, I = oracle.flat_search(c.xb, c.xq, c.k, IP)
    assert np.array_equal((keys & 0xFFFFFFFF).astype(np.int64) - base, I)
    assert c.expect["victim"] in I[0] and c.expect["decoys"][0] not in I[0]


def test_statistics_grow_over_three_adds(gpu_faiss, oracle):
    """background, then the solid rows, then the victim and the decoys: R must be the last add's"""
    c = CASES["aligned_rows_d64"]
    idx = _new(gpu_faiss, c.xb.shape[1])
    a, b = c.parts["bg"][1], c.parts["far"][1]
    for part in (c.xb[:a], c.xb[a:b], c.xb[b:]):
        idx.add(part)
    pred = sr.predict(c.xb, c.xq, c.k)
    assert pred["candidates_max"] == c.expect["candidates_max"]
    _check(idx, c.xb, c.xq, c.k, oracle, pred)


def test_statistics_shrink_at_a_reset(gpu_faiss, oracle):
    """the victim first, a reset, benign rows only: the window is the benign rows' (10), not the stale statistics' (13)"""
    c = CASES["aligned_rows_d64"]
    a = c.parts["special"][0]
    idx = _new(gpu_faiss, c.xb.shape[1])
    idx.add(c.xb[a:])
    idx.reset()
    idx.add(c.xb[:a])
    pred = sr.predict(c.xb[:a], c.xq, c.k)
    stale = sr.predict(c.xb[:a], c.xq, c.k, st=sr.stats(c.xb))
    assert pred["candidates_max"] == c.k < stale["candidates_max"] and not pred["fallback"]
    _check(idx, c.xb[:a], c.xq, c.k, oracle, pred)
