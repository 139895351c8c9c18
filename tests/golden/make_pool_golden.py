#!/usr/bin/env python3
"""Regenerates tests/golden/reference_pool.npz -- run ONLY in the build container (needs /root/reference).

The reference's pfam/embed_pfam_seqvec.py cannot be imported here: its module pulls in seqvec_search/utils.py, whose
matplotlib set-up the installed matplotlib refuses.  As make_pca_golden.py does, this script parses the file with `ast`,
picks out the definition of `extract_domain_representations_from_embedder` (lines 29-40) and compiles that node as it
is in a namespace that holds only the typing names its signature mentions.  So the outputs in the fixture are what the
reference's own function returned under this container's numpy (version stored in the file), driven by a synthetic
embedder: seeded float32 [L, D] arrays with lengths 1 ... 600, overlapping and unordered domains, a sequence without
domains, annotations that repeat inside a sequence and across sequences (the later one wins).  D is 16, not 3072: the
function does not look at the width, and 3072 columns of these lengths would be a hundred times the size limit.  No
reference source is copied: the fixture holds the inputs and what the function returned.

    python tests/golden/make_pool_golden.py
"""
import ast
from pathlib import Path
from typing import Dict, Tuple

import numpy
from numpy import ndarray

HERE = Path(__file__).resolve().parent
REFERENCE = Path("/root/reference/pfam/embed_pfam_seqvec.py")
OUT = HERE / "reference_pool.npz"
SEED, D, NSEQ = 4242, 16, 30
NAME = "extract_domain_representations_from_embedder"


def reference_function():
    tree = ast.parse(REFERENCE.read_text())
    nodes = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == NAME]
    assert len(nodes) == 1, "the reference's function was not found"
    ns = {"Dict": Dict, "Tuple": Tuple, "ndarray": ndarray}
    exec(compile(ast.Module(body=nodes, type_ignores=[]), str(REFERENCE), "exec"), ns)
    return ns[NAME]


def synthetic():
    """-> (ids, embeddings, train ranges, test ranges): ranges[id] = [(start, stop, annotation)], 1-based inclusive"""
    rng = numpy.random.default_rng(SEED)
    lengths = [1, 2, 600, 599, 64, 65, 129] + [int(v) for v in rng.integers(1, 420, NSEQ - 7)]
    ids = [f"SEQ{i:02d}_SYNTH" for i in range(NSEQ)]
    emb = [rng.standard_normal((L, D), dtype=numpy.float32) + numpy.float32(0.25) for L in lengths]
    train, test = {}, {}
    for i, (sid, L) in enumerate(zip(ids, lengths)):
        train[sid], test[sid] = [], []
        if i == 9:
            continue  # a sequence without domains
        for which, k in ((train, int(rng.integers(1, 5))), (test, int(rng.integers(0, 3)))):
            for j in range(k):
                start = int(rng.integers(1, L + 1))
                stop = int(rng.integers(start, L + 1))
                name = "train" if which is train else "test"
                which[sid].append((start, stop, f"{sid}/{start}-{stop} {name}{j} PF{i % 7:05d}.1;fam;"))
        train[sid].append((1, L, f"{sid}/1-{L} whole PF00000.1;whole;"))
    # the same annotation twice inside a sequence and once more in a later one: the last value wins, the first place stays
    dup = "SEQ03_SYNTH/dup PF99999.1;dup;"
    train[ids[3]] = [(5, 50, dup)] + train[ids[3]] + [(300, 599, dup)]
    test[ids[4]].append((1, 64, dup))
    test[ids[20]].append((1, 1, dup))
    return ids, emb, train, test


def flat(ids, ranges):
    rows = [(ids.index(sid), a, b, ann) for sid in ids for (a, b, ann) in ranges[sid]]
    return numpy.asarray([r[:3] for r in rows], numpy.int64).reshape(-1, 3), numpy.asarray([r[3] for r in rows])


def main():
    fn = reference_function()
    ids, emb, train, test = synthetic()
    data_test, data_train = fn(iter(zip(ids, emb)), test, train)
    arrays = {"numpy_version": numpy.asarray(numpy.__version__), "ids": numpy.asarray(ids), "packed": numpy.concatenate(emb, 0),
              "lengths": numpy.asarray([e.shape[0] for e in emb], numpy.int64)}
    for name, ranges, data in (("train", train, data_train), ("test", test, data_test)):
        arrays[f"{name}_ranges"], arrays[f"{name}_annotations"] = flat(ids, ranges)
        arrays[f"{name}_keys"] = numpy.asarray(list(data.keys()))
        values = numpy.stack(list(data.values()))
        assert values.dtype == numpy.float32
        arrays[f"{name}_values"] = values
    numpy.savez_compressed(OUT, **arrays)
    print({k: (v.shape, str(v.dtype)) for k, v in arrays.items()})
    print(f"wrote {OUT} ({OUT.stat().st_size} bytes)")
    assert OUT.stat().st_size < 1000000


if __name__ == "__main__":
    main()
