"""GPU: IndexLSH bit for bit against the exact host restatement of tests/lsh_reference.py -- the codes, and the ids and
distances of every search, with no tolerance anywhere.

The inputs are exact: a rotation in {-1, +1}^(nbits x d) (passed through IndexLSH's _rotation hook) and rows of small
integers, so every fp32 MFMA projection is an exact integer and each code bit has one right answer, zero projections
included.  The cases cover every code width (W = 2 ... 32 words: hamming_scan_kernel<2 ... 32>), the reference's k = 1000
and k up to 2048 (the 4096-key lists and wave_select_mem beyond k = 1400), tie groups that straddle the cut and the chunks,
the final selection of few queries over long compact arrays, searches of several 16384-query batches, two handles
searched at once, indexes filled through add, add_codes and read_index, and the refusals."""
import threading

import numpy as np
import pytest

from lsh_reference import (FLT_MAX, assert_same_codes, assert_same_search, int_rows, pm1_rotation, rand_codes, ref_codes,
                           ref_search, zero_projection_rows)

pytestmark = pytest.mark.gpu

QB = 16384  # queries per batch of knn_lsh_search
ENC_NBITS = (1, 7, 63, 64, 65, 128, 129, 200, 256, 257, 512, 777, 1024, 1025, 2048)
KS = (1, 31, 100, 256, 1000, 1400, 1401, 1536, 1537, 2048)
NQS = (1, 31, 32, 33, 600)


def _plan(nb, nq, k):
    """(chunk_rows, nchunks, kslot) of one batch of knn_lsh_search (restated from lsh.inc: 256-row tiles, 32-query tiles)"""
    nqtiles, ntiles = -(-nq // 32), -(-nb // 256)
    cap = 64
    while cap < 2 * k + 256:
        cap *= 2
    cap = min(max(512, cap), 2048 if k <= 1400 else 4096)
    want = max(1, -(-1024 // nqtiles))
    want = max(1, min(want, max(1, ntiles // max(2, -(-4 * k // 256)))))
    want = max(1, min(want, (2 << 30) // (32 * cap * 8) // nqtiles))
    chunk_rows = -(-ntiles // want) * 256
    return chunk_rows, -(-nb // chunk_rows), k + k // 4


def _index(gpu_faiss, R):
    return gpu_faiss.IndexLSH(R.shape[1], R.shape[0], _rotation=R)


def _add_codes(idx, codes):
    """knn_lsh_add_codes, the entry read_index loads a file's codes through"""
    from knn_for_homology_amd import _lib
    c = np.ascontiguousarray(codes, np.uint8)
    _lib.check(_lib.lib().knn_lsh_add_codes(idx._h, c.ctypes.data, c.shape[0], c.shape[1]))


def _rows_with_zero_projections(rng, R, n):
    """int_rows with, where the tile allows, an all-zero row (every projection 0: every bit 1) and, for even d, rows with
    one exact zero projection each"""
    x = int_rows(rng, n, R.shape[1])
    x[n // 2] = 0
    if R.shape[1] % 2 == 0 and n >= 4:
        z, _ = zero_projection_rows(rng, R, n // 4)
        x[: n // 4] = z
    return x


# ---- encoder ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", (1, 31, 32, 33, 100, 1024))
@pytest.mark.parametrize("nbits", ENC_NBITS)
def test_encoder_codes(gpu_faiss, nbits, d):
    """codes() = ref_codes for 1, 127, 128, 129 and 1000 rows added one call each (partial and whole 128-row tiles),
    d not a multiple of 32 (pad_rows_kernel), nbits > d, sub-byte tails (the bits at and above nbits read back as 0)"""
    rng = np.random.default_rng(nbits * 7919 + d)
    R = pm1_rotation(rng, nbits, d)
    idx = _index(gpu_faiss, R)
    parts = []
    for n in (1, 127, 128, 129, 1000):
        x = _rows_with_zero_projections(rng, R, n)
        idx.add(x)
        parts.append(x)
    x = np.concatenate(parts)
    assert idx.ntotal == x.shape[0]
    assert_same_codes(idx.codes(), ref_codes(x, R), f"nbits={nbits} d={d}")


def test_encoder_crosses_the_slab(gpu_faiss):
    """lsh_encode_host_rows encodes max(128, 256 MiB / (dp * 4)) rows per launch: 65 536 at d = 1024, so 65 536 + 129 rows
    take two slabs, the second of them a partial 128-row tile; zero projections on both sides of the boundary"""
    d, nbits, n = 1024, 256, 65536 + 129
    rng = np.random.default_rng(11)
    R = pm1_rotation(rng, nbits, d)
    x = int_rows(rng, n, d)
    z, _ = zero_projection_rows(rng, R, 8)
    x[65532:65540] = z
    x[0] = x[-1] = 0
    idx = _index(gpu_faiss, R)
    idx.add(x)
    assert_same_codes(idx.codes(), ref_codes(x, R))


@pytest.mark.parametrize("d,nbits", [(1, 1), (32, 32), (33, 7), (100, 65), (1024, 1024), (300, 257)])
def test_encoder_identity_rows(gpu_faiss, d, nbits):
    """rotate_data=False: the rotation is the first nbits rows of the identity, bit j = (x_j >= 0), zeros included"""
    rng = np.random.default_rng(d + nbits)
    idx = gpu_faiss.IndexLSH(d, nbits, rotate_data=False)
    x = int_rows(rng, 300, d, values=(-2, -1, 0, 1, 2))
    idx.add(x)
    assert_same_codes(idx.codes(), ref_codes(x, np.eye(d, dtype=np.float32)[:nbits]))


def test_codes_clear_the_bits_above_nbits(gpu_faiss):
    """FAISS's codes carry zeros above nbits; the device codes carry ones there (0 >= 0 on the zero rotation rows)"""
    for nbits in (7, 13, 129, 2047):
        idx = gpu_faiss.IndexLSH(16, nbits, _rotation=np.random.default_rng(0).standard_normal((nbits, 16)))
        idx.add(np.random.default_rng(nbits).standard_normal((500, 16)).astype(np.float32))
        c = idx.codes()
        assert c.shape == (500, (nbits + 7) // 8)
        assert (c[:, -1] >> (nbits & 7) == 0).all(), nbits
    idx = gpu_faiss.IndexLSH(16, 7)
    idx.add(np.zeros((3, 16), np.float32))  # every projection 0: bits 0..6 set, bit 7 clear
    assert idx.codes().reshape(-1).tolist() == [0x7F] * 3


# ---- search -------------------------------------------------------------------------------------------------------
def _search_case(gpu_faiss, seed, nbits, d, nb, nq, k, via):
    rng = np.random.default_rng(seed)
    R = pm1_rotation(rng, nbits, d)
    idx = _index(gpu_faiss, R)
    if via == "add":
        xb = int_rows(rng, nb, d)
        idx.add(xb)
        cb = ref_codes(xb, R)
    else:
        cb = rand_codes(rng, nb, nbits)
        _add_codes(idx, cb)
    xq = int_rows(rng, nq, d)
    if via == "add" and nb and rng.integers(0, 2):
        xq[: min(nq, nb) // 2] = xb[: min(nq, nb) // 2]  # queries that are database rows
    D, I = idx.search(xq, k)
    De, Ie = ref_search(cb, ref_codes(xq, R), k)
    assert_same_search(D, I, De, Ie, f"seed={seed} nbits={nbits} d={d} nb={nb} nq={nq} k={k} via={via}")


# (nbits, d, nb, nq, k, database through): every code width, every k of KS, nb < k, nq around the 32-query tile and 600
CURATED = [
    (64, 32, 1, 1, 1, "add"),
    (7, 33, 5, 31, 31, "add"),
    (1, 1, 3000, 33, 100, "add"),
    (128, 100, 3000, 32, 1000, "add"),
    (63, 32, 200_000, 1, 256, "codes"),
    (65, 31, 1500, 600, 1000, "add"),
    (200, 64, 20_000, 33, 256, "add"),
    (256, 31, 50_000, 31, 1400, "codes"),
    (129, 32, 20_000, 600, 1401, "codes"),
    (512, 32, 50_000, 31, 1000, "add"),
    (257, 33, 1000, 600, 2048, "add"),
    (300, 64, 30_000, 32, 1536, "codes"),
    (1024, 64, 12_000, 600, 1000, "add"),
    (777, 100, 60_000, 33, 1537, "codes"),
    (1025, 32, 2000, 1, 2048, "add"),
    (2048, 32, 100_000, 1, 2048, "codes"),
    (2048, 1024, 3000, 32, 1000, "add"),
    (1500, 33, 20_000, 33, 31, "add"),
]


@pytest.mark.parametrize("case", range(len(CURATED)))
def test_search_curated(gpu_faiss, case):
    nbits, d, nb, nq, k, via = CURATED[case]
    _search_case(gpu_faiss, 500 + case, nbits, d, nb, nq, k, via)


@pytest.mark.parametrize("seed", range(40))
def test_search_random_cases(gpu_faiss, seed):
    rng = np.random.default_rng(2000 + seed)
    nbits = int(rng.choice(ENC_NBITS))
    d = int(rng.choice([1, 31, 32, 33, 64, 100]))
    nq = int(rng.choice(NQS))
    k = int(rng.choice(KS))
    nb = int(np.exp(rng.uniform(0, np.log(300_000))))
    W = 2  # 64-bit words of a code on the device
    while W * 64 < nbits:
        W *= 2
    nb = max(1, min(nb, int(2e7 / (nq * W))))  # (the host restatement's cost)
    via = "add" if nb * d * nbits <= 1e9 and rng.integers(0, 3) else "codes"
    _search_case(gpu_faiss, 3000 + seed, nbits, d, nb, nq, k, via)


# ---- ties ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nbits,k", [(64, 1000), (1024, 2048), (129, 1537), (2048, 1400)])
def test_ties_a_few_distinct_rows(gpu_faiss, nbits, k):
    """5 distinct rows repeated in random order over 240 000 rows: every distance is a tie group of ~48 000 rows spread over
    every chunk, and the cut falls inside one -- the answer is the group's lowest ids, ascending.  The queries are the 5
    rows themselves (distance 0 to a fifth of the database) and 28 others."""
    d, nb = 32, 240_000
    rng = np.random.default_rng(nbits + k)
    R = pm1_rotation(rng, nbits, d)
    base = int_rows(rng, 5, d)
    assign = rng.integers(0, 5, nb)
    idx = _index(gpu_faiss, R)
    idx.add(np.ascontiguousarray(base[assign]))
    xq = np.concatenate([base, int_rows(rng, 28, d)])
    D, I = idx.search(xq, k)
    De, Ie = ref_search(ref_codes(base, R)[assign], ref_codes(xq, R), k)
    assert_same_search(D, I, De, Ie)
    assert (D[:5] == 0).all() and all(np.array_equal(I[j], np.flatnonzero(assign == j)[:k]) for j in range(5))


@pytest.mark.parametrize("k", [1, 1000, 1400, 1401, 2048])
def test_ties_all_rows_identical(gpu_faiss, k):
    """50 000 copies of one row: every query's answer is ids 0 .. k-1 at one distance"""
    d, nbits, nb = 33, 256, 50_000
    rng = np.random.default_rng(k)
    R = pm1_rotation(rng, nbits, d)
    row = int_rows(rng, 1, d)
    idx = _index(gpu_faiss, R)
    idx.add(np.repeat(row, nb, axis=0))
    xq = np.concatenate([row, int_rows(rng, 32, d)])
    D, I = idx.search(xq, k)
    De, _ = ref_search(ref_codes(row, R), ref_codes(xq, R), 1)
    assert (I == np.arange(k)).all()
    assert np.array_equal(D, np.repeat(De, k, axis=1)) and (D[0] == 0).all()


@pytest.mark.parametrize("k", [256, 1000, 2048])
def test_ties_that_arrive_late_in_their_chunk(gpu_faiss, k):
    """The tied rows with the lowest ids come late in their chunk: the first three quarters of that chunk (and everything
    before it) are rows at distance 5, every row after them is at distance 1.  The chunks behind it hold only rows at
    distance 1, cut their lists within their first tiles and publish 1 as the query's shared running threshold while
    this chunk is still scanning its far rows.  Its rows at distance 1 tie with that threshold and must still be admitted:
    the answer is ids F .. F + k - 1."""
    nbits = d = 64
    nb = 200_000
    chunk_rows, nchunks, _ = _plan(nb, 1, k)
    c = nchunks // 2
    F = c * chunk_rows + 3 * chunk_rows // 4 + 17
    assert F + k <= nb and F - c * chunk_rows > 2 * k + 256  # (its far rows outlast the other chunks' first cut)
    codes = np.full((nb, 8), 0, np.uint8)
    codes[:F, 0] = 0x1F
    codes[F:, 0] = 0x01
    idx = gpu_faiss.IndexLSH(d, nbits, rotate_data=False)
    _add_codes(idx, codes)
    xq = np.full((1, d), -1.0, np.float32)  # code 0
    D, I = idx.search(xq, k)
    De, Ie = ref_search(codes, ref_codes(xq, np.eye(d, dtype=np.float32)), k)
    assert Ie[0, 0] == F and (De == 1).all()
    assert_same_search(D, I, De, Ie, f"F={F} chunk_rows={chunk_rows}")


# ---- the final selection over long compact arrays -------------------------------------------------------------------
@pytest.fixture(scope="module")
def long_db(gpu_faiss):
    """1 000 000 random 1024-bit codes loaded through add_codes, 32 encoded queries; expected results for k = 2048 (the
    k = 1000 answer is their prefix).  Random 1024-bit codes put ~10^4 rows on every distance near the cut: ties too."""
    nbits, d, nb, nq = 1024, 64, 1_000_000, 32
    rng = np.random.default_rng(77)
    R = pm1_rotation(rng, nbits, d)
    cb = rand_codes(rng, nb, nbits)
    idx = _index(gpu_faiss, R)
    _add_codes(idx, cb)
    xq = int_rows(rng, nq, d)
    De, Ie = ref_search(cb, ref_codes(xq, R), 2048)
    return idx, xq, De, Ie


@pytest.mark.parametrize("k", [1000, 2048])
def test_few_queries_long_compact_arrays(long_db, k):
    """32 queries (one query tile) against 1 M rows: knn_lsh_search plans 230 chunks of 4352 rows at k = 1000 and 119
    chunks of 8448 rows at k = 2048, so each query's compact array holds up to 230 x 1250 = 287 500 or 119 x 2560 =
    304 640 keys -- far beyond the 32 768 that select_topk_kernel<32, 1024, false> keeps in registers: launch_select is
    called without a scratch buffer, takes the one-launch selection and re-reads the array from L2 on every probe."""
    idx, xq, De, Ie = long_db
    chunk_rows, nchunks, kslot = _plan(idx.ntotal, xq.shape[0], k)
    assert nchunks * kslot > 32768 and chunk_rows % 256 == 0
    D, I = idx.search(xq, k)
    assert_same_search(D, I, De[:, :k], Ie[:, :k], f"k={k}")


# ---- several batches, two handles --------------------------------------------------------------------------------
@pytest.mark.parametrize("nbits", [1024, 2048])
def test_reference_shape_several_batches(gpu_faiss, nbits):
    """pfam/search.py's shape: k = 1000 over 2 x 16384 + 1 queries (three batches, the last of one query).  The first and
    last rows of every batch and 200 seeded rows against the restatement; the whole call against one call per batch."""
    d, nb, nq, k = 32, 20_000, 2 * QB + 1, 1000
    rng = np.random.default_rng(nbits)
    R = pm1_rotation(rng, nbits, d)
    xb, xq = int_rows(rng, nb, d), int_rows(rng, nq, d)
    xq[QB - 1] = xb[7]
    idx = _index(gpu_faiss, R)
    idx.add(xb)
    D, I = idx.search(xq, k)
    edges = [0, QB - 1, QB, 2 * QB - 1, 2 * QB]
    rows = np.unique(np.concatenate([edges, rng.choice(nq, 200, replace=False)]))
    De, Ie = ref_search(ref_codes(xb, R), ref_codes(xq[rows], R), k)
    assert_same_search(D[rows], I[rows], De, Ie)
    for a in range(0, nq, QB):
        Dp, Ip = idx.search(xq[a:a + QB], k)
        assert_same_search(Dp, Ip, D[a:a + QB], I[a:a + QB], f"batch at {a}")


def test_two_handles_searched_at_once(gpu_faiss):
    """Two indexes, each searched with 16384 + 3000 queries from its own thread at the same time: one of them holds the
    device's copy pipes, the other runs unpiped.  Both equal their sequential results (which equal the restatement on a
    sample of rows)."""
    rng = np.random.default_rng(8)
    d, nb, nq, k = 32, 8000, QB + 3000, 100
    jobs = []
    for nbits in (128, 1024):
        R = pm1_rotation(rng, nbits, d)
        xb, xq = int_rows(rng, nb, d), int_rows(rng, nq, d)
        idx = _index(gpu_faiss, R)
        idx.add(xb)
        jobs.append((idx, xq, ref_codes(xb, R), R))
    seq = [idx.search(xq, k) for idx, xq, _, _ in jobs]
    for (idx, xq, cb, R), (D, I) in zip(jobs, seq):
        rows = np.array([0, QB - 1, QB, nq - 1])
        De, Ie = ref_search(cb, ref_codes(xq[rows], R), k)
        assert_same_search(D[rows], I[rows], De, Ie)
    out, errs = [None, None], []
    start = threading.Barrier(2)

    def run(j):
        try:
            start.wait()
            out[j] = jobs[j][0].search(jobs[j][1], k)
        except Exception as e:  # pragma: no cover
            errs.append(e)

    threads = [threading.Thread(target=run, args=(j,)) for j in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errs, errs
    for j in range(2):
        assert_same_search(*out[j], *seq[j], f"handle {j}")


# ---- an index filled from several sources -----------------------------------------------------------------------------
@pytest.mark.parametrize("nbits", [7, 129, 2048])
def test_mixed_sources(gpu_faiss, tmp_path, nbits):
    """write_index -> read_index (the codes come back through add_codes) -> add more rows; and add / add_codes / add /
    add_codes on one index (add_codes regrows the code array to the exact size, the next add regrows it again): both
    hold the same codes as an index that got every row through add, and search the same"""
    d, k = 33, 1000
    rng = np.random.default_rng(nbits)
    R = pm1_rotation(rng, nbits, d)
    xs = [int_rows(rng, n, d) for n in (3000, 2000, 1500, 700)]
    xq = np.concatenate([xs[1][:5], int_rows(rng, 35, d)])
    full = _index(gpu_faiss, R)
    for x in xs:
        full.add(x)
    a = _index(gpu_faiss, R)
    a.add(xs[0])
    f = tmp_path / "lsh.index"
    gpu_faiss.write_index(a, str(f))
    b = gpu_faiss.read_index(str(f))
    for x in xs[1:]:
        b.add(x)
    c = _index(gpu_faiss, R)
    c.add(xs[0])
    _add_codes(c, ref_codes(xs[1], R))
    c.add(xs[2])
    _add_codes(c, ref_codes(xs[3], R))
    want = ref_codes(np.concatenate(xs), R)
    De, Ie = ref_search(want, ref_codes(xq, R), k)
    for name, idx in (("add", full), ("read_index + add", b), ("add + add_codes", c)):
        assert idx.ntotal == want.shape[0]
        assert_same_codes(idx.codes(), want, name)
        assert_same_search(*idx.search(xq, k), De, Ie, name)


# ---- edges --------------------------------------------------------------------------------------------------------
def test_edges(gpu_faiss):
    from knn_for_homology_amd._lib import Knn355Error
    rng = np.random.default_rng(5)
    d = 16
    R = pm1_rotation(rng, 65, d)
    idx = _index(gpu_faiss, R)
    q = int_rows(rng, 3, d)
    D, I = idx.search(q, 5)  # empty index
    assert D.shape == I.shape == (3, 5) and (D == FLT_MAX).all() and (I == -1).all()
    idx.add(int_rows(rng, 10, d))
    for k in (1, 7, 2048):
        D, I = idx.search(np.zeros((0, d), np.float32), k)
        assert D.shape == I.shape == (0, k) and D.dtype == np.float32 and I.dtype == np.int64
    D, I = idx.search(q, 12)  # nb < k
    assert (I[:, 10:] == -1).all() and (D[:, 10:] == FLT_MAX).all() and sorted(I[0, :10].tolist()) == list(range(10))
    for k in (0, 2049):
        with pytest.raises(Knn355Error):
            idx.search(q, k)
    with pytest.raises(Knn355Error):
        gpu_faiss.IndexLSH(d, 0)
    with pytest.raises(Knn355Error):
        gpu_faiss.IndexLSH(d, 2049, _rotation=np.ones((2049, d), np.float32))
    with pytest.raises(RuntimeError):
        gpu_faiss.IndexLSH(d, d + 1, rotate_data=False)
    with pytest.raises(TypeError):
        idx.search(q.astype(np.float64), 5)
    with pytest.raises(ValueError):
        idx.search(q[0], 5)
    with pytest.raises(ValueError):
        idx.search(np.asfortranarray(int_rows(rng, 4, d)), 5)
    with pytest.raises(AssertionError):
        idx.search(int_rows(rng, 3, d + 1), 5)
    with pytest.raises(TypeError):
        idx.add(q.astype(np.float64))
    assert idx.ntotal == 10
