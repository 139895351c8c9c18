"""Mean pooling of per-residue embeddings on the GPU: the step that produces the matrix an index stores.

The reference pools ragged ``[L, d]`` per-residue arrays in Python loops, one ``mean(axis=0)`` per protein or domain:

* pfam/embed_pfam_seqvec.py:29-40, ``embedding[start - 1 : stop].mean(axis=0)`` per Pfam domain: swap the import ::

      from knn_for_homology_amd.pooling import extract_domain_representations  # was: ..._from_embedder of the script

* ``reduce_per_protein`` of pfam/embed_pfam_t5.py:40-43, pfam/embed_t5_fp16.py:45-47 and cath/embed.py:92-94, and with
  ``normalize=True`` the body of pfam/embed_t5_l2.py:68-71 (``normalize_L2`` on every residue row, then the mean).

All of them are ``pool_ranges``: one call pools any number of row ranges of one packed residue matrix
(``knn_pool_ranges`` / ``knn_pool_ranges_dev``; the arithmetic contract is above them in include/knn355.h).  The result
has the bits of ``x[start:stop].mean(axis=0)`` of numpy on a C-contiguous float32 array.  A torch tensor on the GPU stays
there: embed -> ``pool_ranges`` -> ``knn_normalize_l2_dev`` -> ``knn_flat_add_dev`` -> search never leaves the device.

Not here: columns with a stride, d = 1 (numpy sums a single column pairwise), float64, several GPUs.
"""
import ctypes

import numpy as np

from . import _lib

MAX_LEN = 1 << 24  # a range is shorter than this (POOL_MAX_LEN)
MAX_D = 1 << 20    # KNN_POOL_MAX_D
DEFAULT_BATCH_BYTES = 256 << 20


def _is_torch(x):
    return type(x).__module__.split(".")[0] == "torch"


def _ranges(starts, stops):
    """(starts, stops) as two int64 numpy vectors of one length, or as they are when both are torch tensors"""
    if _is_torch(starts) != _is_torch(stops):
        raise ValueError("starts and stops must both be torch tensors or both be array-likes")
    if _is_torch(starts):
        if starts.dim() != 1 or starts.shape != stops.shape:
            raise ValueError(f"starts and stops must be 1-D and of one length, not {tuple(starts.shape)} and {tuple(stops.shape)}")
        return starts, stops
    out = []
    for name, v in (("starts", starts), ("stops", stops)):
        a = np.asarray(v)
        if a.size == 0:
            a = a.astype(np.int64)
        if a.ndim != 1 or a.dtype.kind not in "iu":
            raise ValueError(f"{name} must be a 1-D integer array, not {a.dtype} {a.shape}")
        out.append(np.ascontiguousarray(a, np.int64))
    if out[0].shape != out[1].shape:
        raise ValueError(f"starts and stops must have one length, not {out[0].shape[0]} and {out[1].shape[0]}")
    return out[0], out[1]


def _check_d(d):
    if d < 2 or d > MAX_D:
        raise ValueError(f"d must be in [2, {MAX_D}], not {d} (numpy sums a single column pairwise: d = 1 has another contract)")


def _pool_torch(x, starts, stops, flags):
    import torch
    if not x.is_cuda:
        raise ValueError("pool_ranges: a torch tensor must be on the GPU (pass a numpy array for host data)")
    if x.dim() != 2:
        raise ValueError(f"residues must be 2-D, [rows, d], not {x.dim()}-D")
    if x.dtype not in (torch.float32, torch.float16):
        raise ValueError(f"residues must be float32 or float16, not {x.dtype}")
    rows, d = x.shape
    _check_d(d)
    if x.stride(1) != 1:
        raise ValueError("residues: the columns of a row must be adjacent (column stride 1)")
    stride = x.stride(0) if rows > 1 else max(x.stride(0), d)
    if stride < d:
        raise ValueError(f"residues: row stride {stride} is below d = {d}")
    with torch.cuda.device(x.device):
        starts, stops = (v.to(device=x.device, dtype=torch.int64).contiguous() if _is_torch(v) else torch.from_numpy(v).to(x.device)
                         for v in (starts, stops))
        n = starts.shape[0]
        out = torch.empty((n, d), dtype=torch.float32, device=x.device)
        stream = torch.cuda.current_stream(x.device).cuda_stream
        _lib.check(_lib.lib().knn_pool_ranges_dev(x.data_ptr(), int(x.dtype == torch.float16), rows, d, stride, starts.data_ptr(), stops.data_ptr(),
                                                  n, flags, out.data_ptr(), ctypes.c_void_p(stream)))
    return out


def pool_ranges(residues, starts, stops, normalize=False):
    """float32 ``[n, d]``: row o is the mean of ``residues[starts[o]:stops[o]]`` (0-based, stop exclusive).

    ``residues`` is a float32 or float16 ``[rows, d]`` numpy array, or such a torch tensor on the GPU; then the result is
    a torch tensor on the same device, computed on torch's current stream (the call returns when it is done: it reads
    the ranges' status word).  Rows may be apart (a row stride above d: ``t[:, :d]`` of a wider tensor; a numpy array of
    that kind is copied first), columns may not.  Ranges may overlap, repeat and come in any order; each needs
    ``0 <= start < stop <= rows`` and fewer than 2^24 rows.  ``normalize=True`` scales every residue row as
    ``faiss.normalize_L2`` would before it is added; ``residues`` itself is never modified."""
    flags = 1 if normalize else 0
    starts, stops = _ranges(starts, stops)
    if _is_torch(residues):
        return _pool_torch(residues, starts, stops, flags)
    if _is_torch(starts):
        raise ValueError("pool_ranges: torch ranges need a torch residue tensor")
    if not isinstance(residues, np.ndarray):
        raise ValueError(f"residues must be a numpy array or a torch tensor, not {type(residues).__name__}")
    if residues.ndim != 2:
        raise ValueError(f"residues must be 2-D, [rows, d], not {residues.ndim}-D")
    if residues.dtype not in (np.float32, np.float16):
        raise ValueError(f"residues must be float32 or float16, not {residues.dtype}")
    rows, d = residues.shape
    _check_d(d)
    if rows > 0 and residues.strides[1] != residues.itemsize:
        raise ValueError("residues: the columns of a row must be adjacent (column stride 1)")
    x = np.ascontiguousarray(residues)
    n = starts.shape[0]
    out = np.empty((n, d), np.float32)
    _lib.check(_lib.lib().knn_pool_ranges(x.ctypes.data, int(x.dtype == np.float16), rows, d, starts.ctypes.data, stops.ctypes.data, n, flags,
                                          out.ctypes.data))
    return out


def last_ms():
    """{upload, kernel, download}: HIP-event milliseconds of this thread's last pool_ranges (tools/bench_pool.py)"""
    u, k, dn = _lib.c_float(), _lib.c_float(), _lib.c_float()
    _lib.check(_lib.lib().knn_pool_last_ms(u, k, dn))
    return {"upload": float(u.value), "kernel": float(k.value), "download": float(dn.value)}


def _pack(arrays):
    """(one [sum L_i, d] matrix, the L_i) of a non-empty sequence of [L_i, d] arrays or GPU tensors of one dtype and width"""
    arrays = list(arrays)
    if not arrays:
        raise ValueError("no embeddings to pool")
    for a in arrays:
        if len(a.shape) != 2 or a.shape[1] != arrays[0].shape[1] or a.dtype != arrays[0].dtype:
            raise ValueError("every embedding must be [L_i, d] with the same d and dtype")
    lengths = np.asarray([a.shape[0] for a in arrays], np.int64)
    if _is_torch(arrays[0]):
        import torch
        return torch.cat(arrays, 0), lengths
    return np.concatenate([np.asarray(a) for a in arrays], 0), lengths


def reduce_per_protein(embeddings, normalize=False, lengths=None):
    """float32 ``[n, d]``: the mean over the residues of every protein, the reference's ``reduce_per_protein`` applied
    to each of them; with ``normalize=True`` the body of pfam/embed_t5_l2.py:68-71.

    ``embeddings`` is a sequence of ``[L_i, d]`` arrays (or GPU tensors), or, with ``lengths``, one packed
    ``[sum L_i, d]`` matrix whose proteins follow one another.  Every L_i is 1 at least."""
    if lengths is None:
        packed, lengths = _pack(embeddings)
    else:
        packed = embeddings
        lengths = np.asarray(lengths)
        if lengths.ndim != 1 or lengths.dtype.kind not in "iu":
            raise ValueError("lengths must be a 1-D integer array")
        lengths = lengths.astype(np.int64)
        if len(packed.shape) != 2 or int(lengths.sum()) != packed.shape[0]:
            raise ValueError(f"lengths sum to {int(lengths.sum())}, the packed matrix has shape {tuple(packed.shape)}")
    if (lengths < 1).any():
        raise ValueError("every protein needs one residue at least")
    stops = np.cumsum(lengths)
    return pool_ranges(packed, stops - lengths, stops, normalize=normalize)


def extract_domain_representations(embedder, domain_ranges_test, domain_ranges_train, batch_bytes=DEFAULT_BATCH_BYTES):
    """The drop-in for ``extract_domain_representations_from_embedder`` (pfam/embed_pfam_seqvec.py:29-40).

    ``embedder`` yields ``(sequence_id, embedding [L, d])``; ``domain_ranges_*[sequence_id]`` lists
    ``(start, stop, annotation)`` with 1-based inclusive residues.  Returns ``(data_test, data_train)``: per annotation the
    float32 ``[d]`` mean of the domain's residues, in the reference's insertion order, a later duplicate of an
    annotation overwriting the value of an earlier one.  Sequences are packed up to ``batch_bytes`` of residues per
    ``pool_ranges`` call instead of being pooled one domain at a time.  Unlike a Python slice, a domain that is not
    inside its sequence (``1 <= start <= stop <= L``) is a ValueError."""
    if batch_bytes < 1:
        raise ValueError("batch_bytes must be positive")
    data_train, data_test = {}, {}
    batch, todo, base, nbytes = [], [], 0, 0  # todo: (dict, annotation, first row, stop row) in the reference's order

    def flush():
        nonlocal batch, todo, base, nbytes
        if todo:
            packed, _ = _pack(batch)
            pooled = pool_ranges(packed, np.asarray([t[2] for t in todo], np.int64), np.asarray([t[3] for t in todo], np.int64))
            if _is_torch(pooled):
                pooled = pooled.cpu().numpy()
            for row, (data, annotation, _, _) in zip(pooled, todo):
                data[annotation] = row
        batch, todo, base, nbytes = [], [], 0, 0

    for sequence_id, embedding in embedder:
        if len(embedding.shape) != 2:
            raise ValueError(f"{sequence_id}: the embedding must be [L, d], not {tuple(embedding.shape)}")
        L = embedding.shape[0]
        size = L * embedding.shape[1] * (embedding.element_size() if _is_torch(embedding) else embedding.itemsize)
        if batch and (nbytes + size > batch_bytes or embedding.dtype != batch[0].dtype or embedding.shape[1] != batch[0].shape[1]):
            flush()
        used = False
        for data, ranges in ((data_train, domain_ranges_train[sequence_id]), (data_test, domain_ranges_test[sequence_id])):
            for (start, stop, annotation) in ranges:
                if not 1 <= start <= stop <= L:
                    raise ValueError(f"{annotation}: residues {start}-{stop} are not inside the {L} residues of {sequence_id}")
                todo.append((data, annotation, base + start - 1, base + stop))
                used = True
        if used:
            batch.append(embedding)
            base += L
            nbytes += size
    flush()
    return data_test, data_train
