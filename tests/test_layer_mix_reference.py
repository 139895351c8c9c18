"""No GPU: the numpy restatement of a layer mix (layer_mix_reference.py) against numpy's own statement, the simplex grid
against the reference's construction, the special weights against the statements of seqvec_search/figures/layers.py:37-47,
and plan_mix / mix_args_illegal of csrc/plan.h through the stand-alone csrc/plan_check.cpp, built here with the host compiler
under ASan and UBSan (`plan_check mix`, `plan_check mixargs`)."""
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import layer_mix_reference as ref

CSRC = Path(__file__).resolve().parent.parent / "knn-for-homology_amd" / "csrc"


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_restatement_is_numpys_statement_with_float32_weights():
    a, b, c = ref.inputs(193, 1000)
    from knn_for_homology_amd.layers import simplex_ratios
    for ratio in list(simplex_ratios(5)) + list(ref.EXTRA_WEIGHTS):
        r0, r1, r2 = (np.float32(v) for v in ratio)
        want = r0 * a + r1 * b + r2 * c
        assert want.dtype == np.float32
        assert np.array_equal(bits(ref.mix([a, b, c], ratio)), bits(want)), ratio


@pytest.mark.parametrize("granularity,rows", [(5, 15), (11, 66), (21, 231)])
def test_simplex_ratios_is_the_references_grid(granularity, rows):
    from knn_for_homology_amd.layers import simplex_ratios
    got = simplex_ratios(granularity)
    assert got.shape == (rows, 3) and got.dtype == np.float64
    assert np.isclose(got.sum(axis=1), 1).all()
    assert np.array_equal(got, ref.reference_grid(granularity))  # the same points in the same order


def test_special_weights_are_the_layer_statements():
    """figures/layers.py:37-47 on a [N, 3072] matrix.  Compared as values: 1 * x + 0 * y has a zero where x is a zero, but not
    always the zero of the same sign (0 * y is -0.0 for negative y, and -0.0 + 0.0 is +0.0), and the data has zeros planted."""
    x = np.concatenate(ref.inputs(50, 1024), axis=1)
    x[::7, ::5] = 0.0
    x[3::7, 1::5] = -0.0
    layers = [x[:, :1024], x[:, 1024:2048], x[:, 2048:]]
    cases = [((0, 1, 0), x[:, 1024:2048]), ((1, 1, 1), x[:, :1024] + x[:, 1024:2048] + x[:, 2048:]), ((0, 0, 1), x[:, 2048:]),
             ((0, 1, 1), x[:, 1024:2048] + x[:, 2048:]), ((0, 1, -1), x[:, 1024:2048] - x[:, 2048:]), ((1, 0, 0), x[:, :1024])]
    for w, want in cases:
        got = ref.mix(layers, w)
        assert np.isfinite(got).all() and np.array_equal(got, want), w


def test_the_gpu_tests_inputs_tell_fused_from_unfused():
    """A kernel that contracts acc + w * x into an fma must fail tests/test_layer_mix_gpu.py: on its inputs every row has an
    element where the fused chain differs, for the grid's rows with 3/4 behind the first layer and for every extra row."""
    for d in (1024, 1000, 1001):
        layers = ref.inputs(193, d)
        for w in [(0.25, 0.75, 0.0), (0.0, 0.25, 0.75), (0.25, 0.0, 0.75)] + list(ref.EXTRA_WEIGHTS):
            differs = bits(ref.mix(layers, w)) != bits(ref.mix_fused(layers, w))
            assert differs.any(axis=1).all(), (d, w)


# ---- the planner and the argument checks, under the sanitizers ----
@pytest.fixture(scope="module")
def plan_check(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    out = tmp_path_factory.mktemp("plan_check_mix")
    subprocess.run(["make", "-C", str(CSRC), "plan_check", f"OUT_DIR={out}", f"CXX={cxx}"], check=True, capture_output=True, text=True)
    return out / "plan_check"


def run(plan_check, sub, text):
    r = subprocess.run([str(plan_check), sub], input=text, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr  # (a sanitizer report ends the program with another status)
    return r.stdout.strip().splitlines()


def mix_line(n, d, dp, layers, out_base=4096):
    """layers: (base, stride) pairs"""
    pairs = list(layers) + [(0, 0)] * (4 - len(layers))
    return f"{n} {d} {dp} {len(layers)} {out_base} " + " ".join(f"{b} {s}" for b, s in pairs[:4]) + "\n"


def test_plan_mix_picks_the_wide_build_by_bases_and_strides(plan_check):
    packed = lambda d: [(8192, d), (1 << 20, d), (2 << 20, d)]  # noqa: E731
    blocks = [(8192 + 4 * 1024 * i, 3072) for i in range(3)]  # the column blocks of a [N, 3072] matrix
    cases = [
        (mix_line(193, 1024, 1024, packed(1024)), "1 256 49408 193"),
        (mix_line(193, 1000, 1024, packed(1000)), "1 256 49408 193"),     # 4000-byte rows keep 16-byte alignment
        (mix_line(193, 1001, 1024, packed(1001)), "0 1024 197632 772"),   # an odd stride: float by float
        (mix_line(193, 1002, 1024, packed(1002)), "0 1024 197632 772"),
        (mix_line(193, 1024, 1024, blocks), "1 256 49408 193"),
        (mix_line(193, 1024, 1024, [(8192, 3072), (8192 + 4100, 3072), (8192 + 8192, 3072)]), "0 1024 197632 772"),  # a base off by 4 bytes
        (mix_line(193, 1024, 1024, packed(1024), out_base=4100), "0 1024 197632 772"),
        (mix_line(7, 6, 32, [(8192, 8)]), "1 8 56 1"),                    # a quad that straddles d, padding quads
        (mix_line(1, 1, 32, [(8192, 1)]), "0 32 32 1"),
        (mix_line(14433, 1024, 1024, packed(1024)), "1 256 3694848 2048"),  # the grid's cap: a grid-stride loop from here on
        (mix_line(8192, 1024, 1024, packed(1024)[:1]), "1 256 2097152 2048"),
        (mix_line(2049, 1024, 1024, packed(1024)[:2]), "1 256 524544 2048"),
        (mix_line(2048, 1024, 1024, packed(1024)[:2]), "1 256 524288 2048"),
        (mix_line(4294967280, 32, 32, [(8192, 32)]), f"1 8 {4294967280 * 8} 2048"),
    ]
    out = run(plan_check, "mix", "".join(c[0] for c in cases))
    assert out == [c[1] for c in cases]


def test_plan_mix_refuses_illegal_launches(plan_check):
    ok = [(8192, 1024)] * 3
    lines = [mix_line(0, 1024, 1024, ok), mix_line(4294967281, 1024, 1024, ok), mix_line(5, 0, 32, ok), mix_line(5, 1024, 1023, ok),
             mix_line(5, 1024, 1 << 30, ok), mix_line(5, 1024, 1024, []), mix_line(5, 1024, 1024, ok, out_base=0),
             mix_line(5, 1024, 1024, [(8192, 1024), (0, 1024)]), mix_line(5, 1024, 1024, [(8192, 1024), (8192, 1023)]),
             "5 1024 1024 5 4096 8192 1024 8192 1024 8192 1024 8192 1024\n"]
    assert run(plan_check, "mix", "".join(lines)) == ["refused"] * len(lines)


def test_argument_checks(plan_check):
    """d nlayers layers_set flat_d flat_is_view sweep g k column nlevels"""
    cases = [
        ("1024 3 7 1024 0 0 0 0 0 0", "ok"),
        ("1024 3 7 1024 0 1 15 2 1 4", "ok"),
        ("1024 4 15 1024 0 1 0 2048 2047 8", "ok"),
        ("1024 3 3 1024 0 1 15 2 1 4", "a layer has no rows (knn_mix_set_layer)"),
        ("1024 3 6 1024 0 0 0 0 0 0", "a layer has no rows (knn_mix_set_layer)"),
        ("1024 3 7 1000 0 1 15 2 1 4", "the index's dimension is not the layers'"),
        ("1024 3 7 1024 1 1 15 2 1 4", "a view is read-only"),
        ("1024 3 7 1024 0 1 15 2 2 4", "column must be 0 .. k - 1"),
        ("1024 3 7 1024 0 1 15 2 -1 4", "column must be 0 .. k - 1"),
        ("1024 0 0 1024 0 0 0 0 0 0", "nlayers must be 1 .. KNN_MIX_MAX_LAYERS"),
        ("1024 5 31 1024 0 0 0 0 0 0", "nlayers must be 1 .. KNN_MIX_MAX_LAYERS"),
        ("1024 3 7 1024 0 1 15 2 1 0", "nlevels must be 1 .. KNN_MIX_MAX_LEVELS"),
        ("1024 3 7 1024 0 1 15 2 1 9", "nlevels must be 1 .. KNN_MIX_MAX_LEVELS"),
        ("1024 3 7 1024 0 1 15 0 0 4", "k must be 1 .. KNN_MAX_K"),
        ("1024 3 7 1024 0 1 15 2049 1 4", "k must be 1 .. KNN_MAX_K"),
        ("1024 3 7 1024 0 1 -1 2 1 4", "negative number of mixes"),
    ]
    assert run(plan_check, "mixargs", "".join(c[0] + "\n" for c in cases)) == [c[1] for c in cases]
