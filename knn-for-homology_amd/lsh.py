"""faiss.IndexLSH(d, nbits) on the GPU (sign bits of a random orthonormal projection,
Hamming top-k).  Reference call sites: seqvec_search/create_index.py:41-47 (build + write),
pfam/search.py:27-37 (1024 bits, k = 1000), pfam/proteins_search.py:25-26 (2048 bits).

FAISS seeds its RandomRotationMatrix from its own generator, so its exact bits cannot be
reproduced without FAISS; here the matrix is the Q factor of a ``numpy.random.default_rng(5)``
Gaussian matrix (FAISS also uses seed 5).  Parity for this index is therefore stated as
recall against the exact flat search, not code equality.  The file format written by
``write_index`` is FAISS's "IxHe" layout, so FAISS can load the index.

``train_thresholds=True`` (FAISS 1.7.2 IndexLSH::train, restated from the published source): ``train(x)`` learns one
threshold per code bit -- the median of that bit's projection over the training rows -- on the GPU, and bit j of every
code is ``(x . a_j - t_j >= 0)`` from then on, for ``add`` and ``search`` alike.  An index that holds rows cannot be
trained again (FAISS allows it and leaves the stale codes behind).
"""
import ctypes
import struct

import numpy as np

from . import _lib
from .faiss import Index, METRIC_L2, _check_matrix, _r_header, _r_vec, _w_header, _w_vec


def random_rotation(d, nbits, seed=5):
    """[nbits, d] float32 with orthonormal rows (nbits <= d) or orthonormal columns (nbits > d)."""
    n = max(d, nbits)
    g = np.random.default_rng(seed).standard_normal((n, n))
    q, r = np.linalg.qr(g)
    q = q * np.sign(np.diag(r))  # unique factorisation
    return np.ascontiguousarray(q[:nbits, :d], dtype=np.float32)


class IndexLSH(Index):
    def __init__(self, d, nbits, rotate_data=True, train_thresholds=False, _rotation=None):
        self._d, self.nbits = int(d), int(nbits)
        self.rotate_data = bool(rotate_data)
        self.train_thresholds = bool(train_thresholds)
        if _rotation is not None:
            self._rot = np.ascontiguousarray(_rotation, np.float32)
        elif rotate_data:
            self._rot = random_rotation(self._d, self.nbits)
        else:
            if nbits > d:
                raise RuntimeError("IndexLSH: nbits > d requires rotate_data")
            self._rot = np.ascontiguousarray(np.eye(self._d, dtype=np.float32)[: self.nbits])
        self._h = ctypes.c_void_p()
        _lib.check(_lib.lib().knn_lsh_create(self._d, self.nbits, self._rot.ctypes.data, ctypes.byref(self._h)))
        self.metric_type = METRIC_L2
        self.is_trained = not self.train_thresholds  # (FAISS: until train() has learnt the thresholds)

    @property
    def d(self):
        return self._d

    @property
    def ntotal(self):
        return int(_lib.lib().knn_lsh_ntotal(self._h)) if self._h else 0

    @property
    def code_size(self):
        return (self.nbits + 7) // 8

    @property
    def thresholds(self):
        """float32 [nbits] copy of the trained thresholds; empty when the index has none"""
        if not (self.train_thresholds and self.is_trained):
            return np.empty(0, np.float32)
        out = np.empty(self.nbits, np.float32)
        _lib.check(_lib.lib().knn_lsh_get_thresholds(self._h, out.ctypes.data))
        return out

    def train(self, x):
        _check_matrix(x, self._d)
        if not self.train_thresholds:
            return
        _lib.check(_lib.lib().knn_lsh_train(self._h, x.ctypes.data, x.shape[0]))  # (refused: the index stays as it was)
        self.is_trained = True

    def _need_trained(self, what):
        if not self.is_trained:  # (FAISS asserts is_trained)
            raise RuntimeError(f"IndexLSH.{what}: train_thresholds=True: call train(x) first")

    def add(self, x):
        self._need_trained("add")
        _check_matrix(x, self._d)
        _lib.check(_lib.lib().knn_lsh_add(self._h, x.ctypes.data, x.shape[0]))

    def search(self, x, k):
        self._need_trained("search")
        _check_matrix(x, self._d)
        k = int(k)
        D = np.empty((x.shape[0], k), np.float32)
        I = np.empty((x.shape[0], k), np.int64)
        _lib.check(_lib.lib().knn_lsh_search(self._h, x.ctypes.data, x.shape[0], k, D.ctypes.data, I.ctypes.data))
        return D, I

    def reset(self):
        """faiss.IndexLSH.reset: drops the rows; the rotation and trained thresholds stay"""
        _lib.check(_lib.lib().knn_lsh_reset(self._h))

    def codes(self):
        out = np.empty((self.ntotal, self.code_size), np.uint8)
        _lib.check(_lib.lib().knn_lsh_get_codes(self._h, out.ctypes.data, self.code_size))
        return out

    # ---- FAISS "IxHe" layout: header, nbits, rotate_data, train_thresholds, thresholds,
    # code_size, VectorTransform "rrot" {have_bias, A, b, d_in, d_out, is_trained}, codes
    # (FAISS 1.7.2 index_write.cpp, restated from the published source; not verified against a FAISS binary).
    # thresholds: empty unless train_thresholds is set and train() has run, then nbits floats.
    def _write(self, f):
        _w_header(f, b"IxHe", self._d, self.ntotal, METRIC_L2, self.is_trained)
        f.write(struct.pack("<i??", self.nbits, self.rotate_data, self.train_thresholds))
        _w_vec(f, self.thresholds, np.float32)
        f.write(struct.pack("<i", self.code_size))
        f.write(b"rrot")
        f.write(struct.pack("<?", False))
        _w_vec(f, self._rot.reshape(-1), np.float32)
        _w_vec(f, np.empty(0, np.float32), np.float32)
        f.write(struct.pack("<ii?", self._d, self.nbits, True))
        _w_vec(f, self.codes().reshape(-1), np.uint8)

    @classmethod
    def _read(cls, f):
        d, ntotal, _metric = _r_header(f)
        from .faiss import _r_exact
        nbits, rotate, thr = struct.unpack("<i??", _r_exact(f, 6))
        thresholds = _r_vec(f, np.float32)
        (code_size,) = struct.unpack("<i", _r_exact(f, 4))
        if f.read(4) != b"rrot":
            raise RuntimeError("read_index: IndexLSH without a random rotation block")
        _r_exact(f, 1)
        A = _r_vec(f, np.float32)
        _r_vec(f, np.float32)
        d_in, d_out, _tr = struct.unpack("<ii?", _r_exact(f, 9))
        codes = _r_vec(f, np.uint8)
        if nbits <= 0 or code_size != (nbits + 7) // 8 or codes.size != ntotal * code_size or (A.size and (d_in != d or d_out < nbits or A.size != d_in * d_out)):
            raise RuntimeError("read_index: IxHe tables do not fit the header")
        # thresholds: nbits of them under the flag (a trained index), none under the flag (not trained yet: no rows
        # either), none without the flag.  FAISS ignores a vector kept without the flag; such a file is refused here
        # rather than guessed at.
        if thresholds.size not in ((0, nbits) if thr else (0,)) or (thr and not thresholds.size and ntotal):
            raise RuntimeError("read_index: IxHe tables do not fit the header (thresholds)")
        idx = cls(d, nbits, rotate_data=rotate, train_thresholds=thr, _rotation=A.reshape(d_out, d_in)[:nbits] if A.size else None)
        if thresholds.size:  # before the codes: a handle that holds rows refuses new thresholds
            t = np.ascontiguousarray(thresholds, np.float32)
            _lib.check(_lib.lib().knn_lsh_set_thresholds(idx._h, t.ctypes.data))
            idx.is_trained = True
        if ntotal:
            c = np.ascontiguousarray(codes.reshape(ntotal, code_size))
            _lib.check(_lib.lib().knn_lsh_add_codes(idx._h, c.ctypes.data, ntotal, code_size))
        return idx

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            try:
                _lib.lib().knn_lsh_free(h)
            except Exception:
                pass
            self._h = None
