"""What a layer mix is, restated in numpy for the tests of knn_for_homology_amd/layers.py (no GPU, no library).

The reference writes ``ratio[0] * cnn + ratio[1] * lstm1 + ratio[2] * lstm2`` (cath/compare_seqvec_layer.py:56) with float64
scalars out of ``numpy.linspace`` and float32 arrays.  Under numpy 1.x, which the reference ran on, value-based casting makes
each scalar a float32 before the product, so every product and every sum is a float32 array operation.  numpy 2 (NEP 50)
keeps a numpy.float64 scalar's type and would compute in float64.  The restatement therefore casts every weight to
numpy.float32 BY HAND and is the same statement under either numpy: separate float32 products, added left to right.
"""
import itertools

import numpy as np


def mix(layers, weights):
    """((w0 * x0 + w1 * x1) + w2 * x2) + ...: one float32 array operation per product and per sum, in the reference's order"""
    w = [np.float32(v) for v in weights]
    assert all(x.dtype == np.float32 for x in layers) and len(w) == len(layers)
    acc = np.multiply(w[0], layers[0], dtype=np.float32)
    for wi, x in zip(w[1:], layers[1:]):
        acc = np.add(acc, np.multiply(wi, x, dtype=np.float32), dtype=np.float32)
    return acc


def mix_fused(layers, weights):
    """the same chain with every ``acc + w * x`` contracted into one fused multiply-add, emulated in float64: the product of
    two float32 values is exact in float64, so only the sum is rounded (to float64, then to float32 -- a double rounding that
    can differ from a true fma in rare cases, which does not matter for its use: showing that the test inputs tell a fused
    kernel from an unfused one)"""
    w = [np.float32(v) for v in weights]
    acc = np.multiply(w[0], layers[0], dtype=np.float32)
    for wi, x in zip(w[1:], layers[1:]):
        acc = (np.float64(wi) * x.astype(np.float64) + acc.astype(np.float64)).astype(np.float32)
    return acc


def reference_grid(granularity):
    """the reference's own construction of the grid (cath/compare_seqvec_layer.py:44-47), for comparing simplex_ratios with"""
    points = np.asarray(list(itertools.product(np.linspace(0, 1, granularity), repeat=3)))
    return points[np.isclose(points.sum(axis=1), 1)]


def inputs(n, d, nlayers=3, seed=0):
    """float32 [n, d] layers whose products with most weights are inexact: normal values times 1/3"""
    rng = np.random.default_rng(1000 * seed + 7 * n + d)
    return [(rng.standard_normal((n, d)) / 3.0).astype(np.float32) for _ in range(nlayers)]


# weights beside the granularity-5 grid (whose entries 0, 1/4, 1/2 and 1 give exact products: only 3/4 rounds): nothing dyadic
EXTRA_WEIGHTS = ((0.3, 0.3, 0.4), (1.0 / 3.0, 1.0 / 3.0, 1.0 / 3.0), (0.7, -0.2, 0.5))


def clustered_layers(n, d, nclasses, seed=0):
    """three layers of n rows around class centres, with a different share of noise each, and int32 labels [n, 4] whose
    finest level has nclasses classes: accuracy then differs from mix to mix"""
    rng = np.random.default_rng(seed)
    fine = rng.integers(0, nclasses, n)
    mapping = np.stack([fine, fine // 2, fine // 6, fine // 20], axis=1).astype(np.int32)
    layers = []
    for noise in (2.0, 3.0, 5.0):
        centres = rng.standard_normal((nclasses, d))
        layers.append(((centres[fine] + noise * rng.standard_normal((n, d))) / 3.0).astype(np.float32))
    return layers, mapping
