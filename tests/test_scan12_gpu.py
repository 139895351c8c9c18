"""GPU: the prefilter on 12-bit row copies (knn_flat_set_scan16 mode 2) returns the fp32 scan's bits.

Every search is compared bit for bit (D as words, I) with the same index under KNN_TUNE_NO_SCAN16 and with the CPU oracle,
and must have taken the path (`last_scan16()["format"] == 12`, kernel `flat_scan_q32_d256_x12`).  On the cases of
tests/scan12_reference.py whose windows no rounding can move (`ROBUST`) the fallback counter and `candidates_max` are
compared with the model's prediction.  Shapes are the smallest at which each branch exists; KNN_TUNE_SCAN16_ANY_NB reaches
the path below 2^18 rows."""
import numpy as np
import pytest

import scan12_reference as s12
from knn_for_homology_amd._lib import (KNN_TUNE_ALWAYS_RESET, KNN_TUNE_EXACT_SEED, KNN_TUNE_NO_PAIRS, KNN_TUNE_NO_SCAN16, KNN_TUNE_NO_SEED,
                                         KNN_TUNE_NO_TILE_MIN_SEED, KNN_TUNE_SCAN16_ANY_NB)

pytestmark = pytest.mark.gpu

IP = 0
CASES = s12.all_cases()


def _same(a, b):
    return np.array_equal(a[1], b[1]) and np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32))


def _new(faiss, d, mode=2):
    idx = faiss.IndexFlat(d, IP)
    idx.set_scan16(mode)
    return idx


def _data(nb, d, nq, seed, normed=True):
    rng = np.random.default_rng(seed)
    xb = rng.standard_normal((nb, d), dtype=np.float32)
    xq = rng.standard_normal((nq, d), dtype=np.float32)
    if normed:
        xb /= np.linalg.norm(xb, axis=1, keepdims=True)
        xq /= np.linalg.norm(xq, axis=1, keepdims=True)
    return xb, xq


def _check(idx, xb, xq, k, oracle, pred=None, flags=0, fmt=12, nchunks=0):
    before = idx.last_scan16()["fallbacks"]
    idx.set_tuning(0, nchunks, KNN_TUNE_SCAN16_ANY_NB | flags)
    got = idx.search(xq, k)
    info = idx.last_scan16()
    assert info["used"] and info["format"] == fmt, info
    assert idx.last_scan()["kernel"] == ("flat_scan_q32_d256_x12" if fmt == 12 else "flat_scan_q32_d256_f16x"), idx.last_scan()
    idx.set_tuning(0, nchunks, KNN_TUNE_NO_SCAN16 | flags)
    ref = idx.search(xq, k)
    assert not idx.last_scan16()["used"] and idx.last_scan16()["format"] == 0
    idx.set_tuning(0, 0, 0)
    assert _same(got, oracle.flat_search(xb, xq, k, IP)), "the 12-bit prefilter differs from the oracle"
    assert _same(got, ref), "the 12-bit prefilter differs from the fp32 scan"
    print(f"fallbacks +{info['fallbacks'] - before}, candidates_max {info['candidates_max']}" + (f" (predicted {int(pred['fallback'])}, {pred['candidates_max']})" if pred else ""))
    if pred:
        assert info["fallbacks"] - before == (1 if pred["fallback"] else 0), info
        assert info["candidates_max"] == pred["candidates_max"], (info, pred["candidates_max"])
    return got, info


@pytest.mark.parametrize("name", [n for n in s12.ROBUST])
def test_case_against_the_model(gpu_faiss, oracle, name):
    c = CASES[name]
    idx = _new(gpu_faiss, c.xb.shape[1])
    idx.add(c.xb)
    _check(idx, c.xb, c.xq, c.k, oracle, s12.predict(c.xb, c.xq, c.k))


@pytest.mark.parametrize("name", [n for n in CASES if n not in s12.ROBUST])
def test_case_bits_only(gpu_faiss, oracle, name):
    c = CASES[name]
    idx = _new(gpu_faiss, c.xb.shape[1])
    idx.add(c.xb)
    _check(idx, c.xb, c.xq, c.k, oracle)


# k' = min(2048, max(3k, k + 128)): 129 at k = 1, 300 at k = 100, 2048 at k = 683 (3k = 2049, capped) and at k = 1920 (k + 128)
SHAPES = [(128, 64, 1, 1), (129, 1000, 31, 1), (130, 1024, 32, 1),
          (299, 1280, 32, 100), (300, 64, 31, 100), (301, 1000, 1, 100), (257, 1024, 32, 100), (513, 1280, 31, 100),
          (2047, 64, 32, 683), (2048, 64, 1, 683), (2049, 1000, 31, 683), (2047, 64, 31, 1920), (2049, 64, 32, 1920)]


@pytest.mark.parametrize("nb,d,nq,k", SHAPES)
def test_shapes(gpu_faiss, oracle, nb, d, nq, k):
    xb, xq = _data(nb, d, nq, seed=nb + d + nq + k)
    idx = _new(gpu_faiss, d)
    idx.add(xb)
    _check(idx, xb, xq, k, oracle)


def test_kprime_equal_k_is_refused(gpu_faiss, oracle):
    xb, xq = _data(2500, 64, 4, seed=1)
    idx = _new(gpu_faiss, 64)
    idx.add(xb)
    idx.set_tuning(0, 0, KNN_TUNE_SCAN16_ANY_NB)
    got = idx.search(xq, 2048)
    assert not idx.last_scan16()["used"]
    assert _same(got, oracle.flat_search(xb, xq, 2048, IP))


def test_nonfinite_row_turns_the_path_off(gpu_faiss, oracle):
    xb, xq = _data(700, 64, 5, seed=2)
    xb[123, 7] = np.inf
    idx = _new(gpu_faiss, 64)
    idx.add(xb)
    idx.set_tuning(0, 0, KNN_TUNE_SCAN16_ANY_NB)
    got = idx.search(xq, 10)
    assert not idx.last_scan16()["used"]
    assert _same(got, oracle.flat_search(xb, xq, 10, IP))
    idx.reset()
    xb2, _ = _data(700, 64, 5, seed=3)
    idx.add(xb2)
    _check(idx, xb2, xq, 10, oracle)


def test_nonfinite_query_falls_back(gpu_faiss, oracle):
    xb, xq = _data(900, 64, 6, seed=4)
    xq[3, 11] = np.nan
    idx = _new(gpu_faiss, 64)
    idx.add(xb)
    _, info = _check(idx, xb, xq, 10, oracle)
    assert info["fallbacks"] == 1


def test_pieces_reserve_regrow_reset_views(gpu_faiss, oracle):
    """rows added in pieces that end inside a 256-row tile, a reservation, growth past it, views before and after, a reset"""
    from knn_for_homology_amd import _lib
    xb, xq = _data(3000, 1000, 9, seed=5)
    idx = _new(gpu_faiss, 1000)
    idx.add(xb[:100])
    idx.add(xb[100:357])
    _check(idx, xb[:357], xq, 20, oracle)
    old = idx.view()
    _check(old, xb[:357], xq, 20, oracle)
    _lib.check(_lib.lib().knn_flat_reserve(idx._h, 1500))
    with pytest.raises(Exception):
        old.search(xq, 20)  # the rows and their copies moved
    v = idx.view()
    idx.add(xb[357:1400])  # fits the reservation
    _check(v, xb[:357], xq, 20, oracle)  # (the view ends inside a tile whose other rows exist now)
    _check(idx, xb[:1400], xq, 20, oracle)
    idx.add(xb[1400:])  # grows: every row copied again
    with pytest.raises(Exception):
        v.search(xq, 20)
    _check(idx, xb, xq, 20, oracle, flags=KNN_TUNE_ALWAYS_RESET)
    _check(idx.view(), xb, xq, 20, oracle)
    idx.reset()
    idx.add(xb[2000:2600])
    _check(idx, xb[2000:2600], xq, 20, oracle)


def test_both_formats_same_bits(gpu_faiss, oracle):
    xb, xq = _data(5000, 1024, 32, seed=6)
    a, b = _new(gpu_faiss, 1024, 1), _new(gpu_faiss, 1024, 2)
    a.add(xb)
    b.add(xb)
    ga, _ = _check(a, xb, xq, 100, oracle, fmt=16)
    gb, _ = _check(b, xb, xq, 100, oracle, fmt=12)
    assert _same(ga, gb)


@pytest.mark.parametrize("flags", [0, KNN_TUNE_ALWAYS_RESET], ids=["default", "always_reset"])
def test_shard_keys_on_both_lanes(gpu_faiss, oracle, flags):
    import torch
    from knn_for_homology_amd.sharded import HipShardBackend
    xb, xq = _data(20000, 100, 32, seed=7)
    k, base = 100, 70000
    b = HipShardBackend(100, IP)
    b.index.set_scan16(2)
    b.add(xb)
    want = oracle.flat_search(xb, xq, k, IP)
    q = torch.from_numpy(xq).cuda()
    torch.cuda.synchronize()
    seen = set()
    for _ in range(4):
        index, stream = b.next_lane()
        index.set_tuning(0, 0, KNN_TUNE_SCAN16_ANY_NB | flags)
        with torch.cuda.stream(stream):
            keys = b.search_keys(q, k, base, index=index)
        torch.cuda.synchronize()
        info = index.last_scan16()
        assert info["used"] and info["format"] == 12, info
        assert np.array_equal((keys.cpu().numpy() & 0xFFFFFFFF).astype(np.int64) - base, want[1])
        index.set_tuning(0, 0, KNN_TUNE_NO_SCAN16 | flags)
        with torch.cuda.stream(stream):
            ref = b.search_keys(q, k, base, index=index)
        torch.cuda.synchronize()
        assert np.array_equal(keys.cpu().numpy(), ref.cpu().numpy())
        seen.add(id(index))
    assert len(seen) == 2


# Where the fp32 search would seed its scan with a sample pass over a strided view (no tile-minimum seed: switched off, or a
# forced chunk count): the 12-bit copies lie in tiles of consecutive rows and cannot serve such a view, so their pass runs
# unseeded.  The neighbours planted in the rows a sample would have taken (the first rows of every block) must come out.
@pytest.mark.parametrize("flags,nchunks,k", [(KNN_TUNE_EXACT_SEED, 0, 10), (KNN_TUNE_NO_TILE_MIN_SEED, 0, 10), (KNN_TUNE_NO_TILE_MIN_SEED, 0, 683),
                                             (0, 7, 683), (KNN_TUNE_NO_PAIRS, 0, 100), (KNN_TUNE_NO_SEED, 0, 100),
                                             (KNN_TUNE_NO_TILE_MIN_SEED | KNN_TUNE_NO_PAIRS, 3, 100)],
                         ids=["exact_seed", "no_tile_min", "no_tile_min_k683", "chunks7_k683", "no_pairs", "no_seed", "no_tile_min_no_pairs_chunks3"])
def test_no_strided_sample_pass(gpu_faiss, oracle, flags, nchunks, k):
    xb, xq = _data(20000, 64, 32, seed=31)
    xb[::8] += xq[np.arange(len(xb[::8])) % 32] * np.float32(0.5)  # the best rows of every query sit where samples are taken
    idx = _new(gpu_faiss, 64)
    idx.add(xb)
    _check(idx, xb, xq, k, oracle, flags=flags, nchunks=nchunks)


ENV_SCRIPT = """
import sys
import numpy as np
sys.path.insert(0, {root!r})
from knn_for_homology_amd import faiss
from knn_for_homology_amd._lib import KNN_TUNE_SCAN16_ANY_NB
rng = np.random.default_rng(0)
xb = rng.standard_normal((2000, 64), dtype=np.float32)
idx = faiss.IndexFlat(64, 0)
idx.set_scan16({mode})
idx.add(xb)
idx.set_tuning(0, 0, KNN_TUNE_SCAN16_ANY_NB)
idx.search(xb[:5], 10)
print("FORMAT", idx.last_scan16()["format"], idx.last_scan()["kernel"])
"""


@pytest.mark.parametrize("env,mode,want", [({"KNN355_SCAN_FORMAT": "16"}, 2, "FORMAT 16 flat_scan_q32_d256_f16x"), ({"KNN355_SCAN_FORMAT": "16"}, 1, "FORMAT 16 flat_scan_q32_d256_f16x"),
                                           ({"KNN355_SCAN16": "0"}, 2, "FORMAT 0 flat_scan_q32_d256"), ({"KNN355_SCAN16": "0"}, 1, "FORMAT 0 flat_scan_q32_d256"),
                                           ({}, 2, "FORMAT 12 flat_scan_q32_d256_x12")],
                         ids=["format16_mode2", "format16_mode1", "scan16_off_mode2", "scan16_off_mode1", "plain_mode2"])
def test_environment_overrides(gpu_faiss, env, mode, want):
    """the library reads KNN355_SCAN_FORMAT and KNN355_SCAN16 when the mode is set: a fresh process per setting"""
    import os
    import subprocess
    import sys
    from pathlib import Path
    root = str(Path(__file__).resolve().parent.parent)
    e = {k: v for k, v in os.environ.items() if k not in ("KNN355_SCAN_FORMAT", "KNN355_SCAN16")}
    e.update(env)
    r = subprocess.run([sys.executable, "-c", ENV_SCRIPT.format(root=root, mode=mode)], env=e, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert want in r.stdout.splitlines(), r.stdout


def test_backend_default_and_explicit_choices(gpu_faiss, oracle):
    """HipShardBackend selects the 12-bit copies; a caller's set_scan16(1) or (0) before the first add is what holds"""
    import torch
    from knn_for_homology_amd.sharded import HipShardBackend
    xb, xq = _data(3000, 64, 8, seed=9)
    q = torch.from_numpy(xq).cuda()
    for mode, fmt in ((None, 12), (1, 16), (0, 0)):
        b = HipShardBackend(64, IP)
        if mode is not None:
            b.index.set_scan16(mode)
        b.reserve(3000)
        b.add(xb)
        b.index.set_tuning(0, 0, KNN_TUNE_SCAN16_ANY_NB)
        keys = b.search_keys(q, 10, 0, index=b.index).cpu().numpy()
        info = b.index.last_scan16()
        assert info["format"] == fmt and info["used"] == (fmt != 0), (mode, info)
        assert np.array_equal((keys & 0xFFFFFFFF).astype(np.int64), oracle.flat_search(xb, xq, 10, IP)[1])
