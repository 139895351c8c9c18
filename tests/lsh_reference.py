"""Exact host restatement of IndexLSH (sign-bit codes + Hamming top-k), for the LSH tests and tests/fuzz_lsh_gpu.py.

projections32
             x . R[j] with the products in float64, rounded to float32 (the exact inputs below have one right answer;
             a NaN, an infinity or one entry of +-2^127 among small integers have one too: lsh_nonfinite_cases)
faiss_bits   the code bit as FAISS 1.7.2 computes it (IndexLSH::sa_encode -> fvecs2bitvecs, restated from the published
             source): the float32 projection, the float32 subtraction of the threshold (0 without thresholds), the sign
             test `>= 0`.  For finite operands this is `p >= t` (denormals kept); it is NOT when p and t are the same
             infinity (inf - inf is a NaN: bit 0) and a NaN projection's bit is 0
ref_codes    bit j of a row = faiss_bits(projections32, 0); FAISS byte order (byte j >> 3, bit j & 7); the bits of the
             last byte at and above nbits are zero
ref_search   Hamming distances over uint64 words, the k smallest per query ordered by (distance, id); rows shorter
             than k are padded with FLT_MAX / -1
assert_same_search, assert_same_codes
             exact comparisons that name the first differing query / position (row / bit) in their message

The exact inputs: a rotation in {-1, +1}^(nbits x d) and rows of small integers (int_rows, pm1_rotation).  Every
product and partial sum is then an integer below 2^24, exact in fp32 in any summation order, so the GPU's MFMA
projection has exactly one right answer -- zero projections included (zero_projection_rows builds them on purpose)."""
import numpy as np

FLT_MAX = np.float32(np.finfo(np.float32).max)


def pm1_rotation(rng, nbits, d):
    """[nbits, d] float32 of random -1 / +1 (not orthonormal: the kernel does not care)"""
    return np.where(rng.integers(0, 2, (nbits, d)) == 1, 1.0, -1.0).astype(np.float32)


def int_rows(rng, n, d, values=(-3, -1, 1, 3)):
    """[n, d] float32 drawn from `values` (odd by default: no projection onto a +-1 row of odd length is zero)"""
    v = np.asarray(values, np.float32)
    return v[rng.integers(0, len(v), (n, d), dtype=np.uint8)]


def rand_codes(rng, n, nbits):
    """[n, (nbits + 7) // 8] uint8 random codes with zero padding bits (a database loaded through add_codes)"""
    c = rng.integers(0, 256, (n, (nbits + 7) // 8), dtype=np.uint8)
    if nbits & 7:
        c[:, -1] &= (1 << (nbits & 7)) - 1
    return c


def zero_projection_rows(rng, R, n):
    """[n, d] float32 rows with x . R[j] == 0 exactly for a random j per row (d must be even): x = R[j] * s with s a
    balanced +-1 sign vector.  -> (rows, j per row)"""
    nbits, d = R.shape
    if d % 2:
        raise ValueError("zero_projection_rows: d must be even")
    js = rng.integers(0, nbits, n)
    s = np.tile(np.repeat(np.array([1.0, -1.0], np.float32), d // 2), (n, 1))
    s = rng.permuted(s, axis=1)
    return np.ascontiguousarray(R[js] * s, np.float32), js


def projections32(x, R):
    """[n, nbits] float32: the float64 products x . R[j], rounded to float32 once"""
    with np.errstate(all="ignore"):
        return (np.asarray(x, np.float64) @ np.asarray(R, np.float64).T).astype(np.float32)


def faiss_bits(p, t=0.0):
    """bool [n, nbits]: (p - t >= 0) with the subtraction in float32 -- p float32 projections, t float32 [nbits] or a scalar"""
    with np.errstate(all="ignore"):
        return (np.asarray(p, np.float32) - np.asarray(t, np.float32)) >= 0


def pack_bits(bits):
    """bool [n, nbits] -> uint8 [n, (nbits + 7) // 8], FAISS byte order, zero padding"""
    return np.packbits(np.asarray(bits, bool), axis=1, bitorder="little")


def ref_codes(x, R, t=0.0, chunk=8192):
    """x [n, d], R [nbits, d] -> uint8 [n, (nbits + 7) // 8]: bit j = faiss_bits(x . R[j], t[j]), FAISS byte order, zero padding"""
    x = np.asarray(x)
    nbits = np.asarray(R).shape[0]
    t = np.broadcast_to(np.asarray(t, np.float32), (nbits,))
    out = np.empty((x.shape[0], (nbits + 7) // 8), np.uint8)
    for i in range(0, x.shape[0], chunk):
        out[i:i + chunk] = pack_bits(faiss_bits(projections32(x[i:i + chunk], R), t))
    return out


def _words(codes):
    """uint8 [n, B] -> uint64 [n, ceil(B / 8)] (rows zero-padded to whole words)"""
    codes = np.asarray(codes, np.uint8)
    n, b = codes.shape
    nw = max(1, (b + 7) // 8)
    buf = np.zeros((n, nw * 8), np.uint8)
    buf[:, :b] = codes
    return buf.view(np.uint64)


def hamming(codes_db, codes_q):
    """uint16 [nq, nb] Hamming distances (small cases and checks only)"""
    db, q = _words(codes_db), _words(codes_q)
    dist = np.zeros((q.shape[0], db.shape[0]), np.uint16)
    for w in range(db.shape[1]):
        dist += np.bitwise_count(q[:, None, w] ^ db[None, :, w])
    return dist


def ref_search(codes_db, codes_q, k, max_elems=1 << 23):
    """-> (D float32 [nq, k], I int64 [nq, k]): the k smallest Hamming distances per query, ties by lower id, padded with
    FLT_MAX / -1 where the database holds fewer than k rows.  Queries go max_elems // nb at a time."""
    db, q = _words(codes_db), _words(codes_q)
    nb, nq = db.shape[0], q.shape[0]
    D = np.full((nq, k), FLT_MAX, np.float32)
    I = np.full((nq, k), -1, np.int64)
    kk = min(k, nb)
    if nb == 0 or nq == 0 or kk == 0:
        return D, I
    ids = np.arange(nb, dtype=np.int64)
    step = max(1, max_elems // nb)
    for a in range(0, nq, step):
        qc = q[a:a + step]
        dist = np.zeros((qc.shape[0], nb), np.uint16)
        for w in range(db.shape[1]):
            dist += np.bitwise_count(qc[:, w:w + 1] ^ db[None, :, w])
        key = (dist.astype(np.int64) << 32) | ids  # unique keys: (distance, id) order is plain integer order
        if kk < nb:
            key = np.partition(key, kk - 1, axis=1)[:, :kk]
        key = np.sort(key, axis=1)
        D[a:a + qc.shape[0], :kk] = (key >> 32).astype(np.float32)
        I[a:a + qc.shape[0], :kk] = key & 0xFFFFFFFF
    return D, I


def search_diff(D, I, De, Ie):
    """None if (D, I) equals the expected (De, Ie) exactly (ids, and distances bit for bit), else a message naming the
    first differing query and position with both sides' id and distance"""
    D, I, De, Ie = (np.asarray(a) for a in (D, I, De, Ie))
    if D.shape != De.shape or I.shape != Ie.shape:
        return f"shapes differ: got D{D.shape} I{I.shape}, expected D{De.shape} I{Ie.shape}"
    if D.dtype != np.float32 or I.dtype != np.int64:
        return f"dtypes: got {D.dtype} / {I.dtype}, expected float32 / int64"
    bad = (I != Ie) | (D.view(np.uint32) != np.asarray(De, np.float32).view(np.uint32))
    if not bad.any():
        return None
    q, j = (int(v) for v in np.argwhere(bad)[0])
    return (f"{int(bad.sum())} of {bad.size} entries differ, {int(bad.any(axis=1).sum())} queries; first: query {q} position {j}: "
            f"got id {int(I[q, j])} distance {float(D[q, j])!r}, expected id {int(Ie[q, j])} distance {float(De[q, j])!r}")


def assert_same_search(D, I, De, Ie, what=""):
    msg = search_diff(D, I, De, Ie)
    assert msg is None, f"{what}: {msg}" if what else msg


def codes_diff(got, want):
    """None if the uint8 code arrays are equal, else a message naming the first differing row, byte and bit"""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return f"codes: got {got.dtype}{got.shape}, expected {want.dtype}{want.shape}"
    bad = got != want
    if not bad.any():
        return None
    r, b = (int(v) for v in np.argwhere(bad)[0])
    x = int(got[r, b]) ^ int(want[r, b])
    bit = (x & -x).bit_length() - 1
    return (f"{int(bad.sum())} bytes in {int(bad.any(axis=1).sum())} rows differ; first: row {r} byte {b} "
            f"(code bit {8 * b + bit}): got {int(got[r, b]):#04x}, expected {int(want[r, b]):#04x}")


def assert_same_codes(got, want, what=""):
    msg = codes_diff(got, want)
    assert msg is None, f"{what}: {msg}" if what else msg
