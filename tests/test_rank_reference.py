"""No GPU: the host side of the ranked consumers.

  * tests/rank_reference.py == tests/golden/reference_rank.npz, the arrays the reference's own loop (pfam/pfam.py:561-598)
    saved for synthetic inputs, exactly -- both the curve read off the full recall array and the path through integer
    targets that the device takes;
  * evaluation.score_quantiles' host half (_quantile_positions, _quantile_lerp), with numpy.sort standing in for the
    device, == numpy.quantile, exactly: the arithmetic restates numpy 2.2.6, so the comparison runs under that numpy's
    major.minor and says so otherwise;
  * the target arithmetic by hand;
  * the size plan of csrc/plan.h (plan_rank) through the stand-alone, sanitizer-built csrc/plan_check.cpp."""
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import rank_reference as rr

GOLDEN = Path(__file__).resolve().parent / "golden" / "reference_rank.npz"
CSRC = Path(__file__).resolve().parent.parent / "knn-for-homology_amd" / "csrc"
TILE, SCAN_BLOCK, SCAN_TOP = 2048, 1024, 256  # RANK_TILE, RANK_SCAN_BLOCK, RANK_SCAN_TOP of csrc/plan.h


def golden_cases():
    g = np.load(GOLDEN)
    for run in g["runs"]:
        for label in g["sets"]:
            for name in g["names"]:
                yield g, str(run), str(label), str(name)


def test_fixture_covers_the_cases_the_curve_needs():
    g = np.load(GOLDEN)
    seen = set()
    for g, run, label, name in golden_cases():
        scores, limit = g[f"{run}_{label}_scores"], int(g[f"{run}_{label}_{name}_limit"])
        ties = str(g[f"{run}_{label}_{name}_ties"])
        assert ties in ("none", "one_value")
        reached = bool((g[f"{run}_{label}_{name}_recall"] >= 1).any())
        seen.add((scores.dtype.name, ties, limit < scores.shape[1], reached))
        if ties == "one_value":
            assert (scores[:, :limit] == 100000).any()  # the e-value padding
    assert any(s[0] == "float32" and s[1] == "none" for s in seen)
    assert any(s[0] == "float64" and s[1] == "one_value" for s in seen)
    assert any(s[2] for s in seen) and any(not s[2] for s in seen)  # limit < k and limit == k
    assert any(s[3] for s in seen) and any(not s[3] for s in seen)  # recall reaches 1; never does: the clip


def test_restatement_is_the_reference_exactly():
    for g, run, label, name in golden_cases():
        scores, correct = g[f"{run}_{label}_scores"], g[f"{run}_{label}_correct"]
        total, limit = int(g[f"{run}_total"]), int(g[f"{run}_{label}_{name}_limit"])
        want = g[f"{run}_{label}_{name}_recall"], g[f"{run}_{label}_{name}_precision"]
        for fn in (rr.precision_recall_direct, rr.precision_recall):
            recall, precision = fn(correct, scores, total, limit)
            assert np.array_equal(rr.bits(recall), rr.bits(want[0])), (run, label, name, fn.__name__)
            assert np.array_equal(rr.bits(precision), rr.bits(want[1])), (run, label, name, fn.__name__)


def test_product_targets_are_the_restatement():
    from knn_for_homology_amd import evaluation as ev
    levels = np.linspace(0, 1, 10000)
    for total in (1, 2, 3, 7, 10, 999, 1000, 2400, 9999, 10000, 10001, 123457):
        assert np.array_equal(ev._recall_targets(levels, total), rr.recall_targets(levels, total)), total


def test_target_arithmetic_by_hand():
    # C over 6 ranks; total 4: the levels 0, 0.25, 0.5, 0.75, 1 ask for 0, 1, 2, 3, 4 correct hits
    C = np.array([0, 1, 1, 2, 3, 3], np.int64)
    assert rr.recall_targets(np.array([0, 0.25, 0.5, 0.75, 1.0]), 4).tolist() == [0, 1, 2, 3, 4]
    idx, at = rr.lookup(C, [0, 1, 2, 3, 4, 2, -5])
    assert idx.tolist() == [0, 1, 3, 4, 6, 3, 0]  # t = 0 -> rank 0; reached exactly; 4 is never reached -> N; a repeat; below 0
    assert at.tolist() == [0, 1, 2, 3, 3, 2, 0]   # C at the rank, at N - 1 for the unreachable one
    # a level between two quotients asks for the next count: 0.3 * 4 = 1.2 -> 2
    assert rr.recall_targets(np.array([0.3]), 4).tolist() == [2]
    # total larger than the number of correct hits: the clip reads the last rank
    correct = np.array([[1, 0, 1]], bool)
    scores = np.array([[0.5, 0.25, 0.75]], np.float64)
    recall, precision = rr.precision_recall(correct, scores, 5, points=6)  # levels 0, .2, .4, .6, .8, 1 -> counts 0 .. 5
    # order: 0.25 (F), 0.5 (T), 0.75 (T): C = 0, 1, 2
    assert recall.tolist() == [0 / 5, 1 / 5, 2 / 5, 2 / 5, 2 / 5, 2 / 5]
    assert precision.tolist() == [0 / 1, 1 / 2, 2 / 3, 2 / 3, 2 / 3, 2 / 3]
    direct = rr.precision_recall_direct(correct, scores, 5, points=6)
    assert np.array_equal(direct[0], recall) and np.array_equal(direct[1], precision)


def test_order_contract_of_the_restatement():
    s = np.array([np.nan, 0.0, -0.0, -np.inf, np.inf, -np.nan, 1e-45, -1e-45, 0.0], np.float32)
    assert rr.order(s).tolist() == [3, 7, 1, 2, 8, 6, 4, 0, 5]            # zeros tie in input order; NaN last in input order
    assert rr.order(s, descending=True).tolist() == [4, 6, 1, 2, 8, 7, 3, 0, 5]  # NaN still last


def quantile_inputs():
    rng = np.random.default_rng(626)
    q_full = np.concatenate([[0.0, 1.0], np.linspace(0, 1, 301), rng.random(40), [0.5, 0.5, 1 / 3, 0.999999, 1e-9]])
    for dtype in (np.float32, np.float64):
        for n in (1, 2, 3, 259, 6000, 100001):
            yield rng.normal(0, 3, n).astype(dtype), q_full
        yield rng.integers(0, 4, 1000).astype(dtype), q_full          # repeated values
        yield np.full(77, 2.5, dtype), q_full
        yield (rng.random((50, 12)) * 1e-3).astype(dtype), q_full     # 2-D
        yield np.array([1.0, np.nan, 3.0, 2.0], dtype), q_full        # a NaN: every quantile is NaN


def host_half(scores, q, limit=None):
    """evaluation.score_quantiles with numpy.sort in the device's place"""
    from knn_for_homology_amd import evaluation as ev
    flat = np.sort((scores if scores.ndim == 1 else scores[:, :limit]).reshape(-1), kind="stable")
    q = np.asarray(q, np.float64)
    previous, following, gamma = ev._quantile_positions(flat.size, q)
    return ev._quantile_lerp(flat[previous], flat[following], gamma, flat[-1])


def test_quantile_host_half_is_numpy_quantile_exactly():
    assert np.__version__.split(".")[:2] == ["2", "2"], (
        f"the host half restates numpy 2.2's linear method; this is numpy {np.__version__}: re-derive it (evaluation._quantile_lerp)")
    for scores, q in quantile_inputs():
        want = np.quantile(scores, q)
        assert want.dtype == np.float64
        for got in (host_half(scores, q), rr.quantiles(scores, q)):
            assert got.dtype == np.float64
            assert np.array_equal(rr.bits(got), rr.bits(want)), (scores.dtype, scores.shape)
    s = np.random.default_rng(1).random((30, 9)).astype(np.float32)
    q = np.linspace(0, 1, 11)
    assert np.array_equal(host_half(s, q, 4), np.quantile(s[:, :4], q))
    assert np.array_equal(rr.quantiles(s, q, 4), np.quantile(s[:, :4], q))


def test_python_argument_checks_need_no_gpu():
    from knn_for_homology_amd import evaluation as ev
    c, s = np.zeros((3, 4), bool), np.zeros((3, 4), np.float32)
    for bad in (lambda: ev.ranked_precision_recall(c[:2], s, 5), lambda: ev.ranked_precision_recall(c, s, 5, limit=0),
                lambda: ev.ranked_precision_recall(c, s, 5, limit=5), lambda: ev.ranked_precision_recall(c, s, 0),
                lambda: ev.ranked_precision_recall(c, s[0], 5), lambda: ev.ranked_precision_recall(c, s, 5, points=0),
                lambda: ev.ranked_cumulative(c, s[:, :3]), lambda: ev.ranked_cumulative(c.reshape(3, 2, 2), s.reshape(3, 2, 2)),
                lambda: ev.score_quantiles(s, [0.5, 1.5]), lambda: ev.score_quantiles(s, [-0.1]), lambda: ev.score_quantiles(s, [np.nan]),
                lambda: ev.score_quantiles(s, [[0.5]]), lambda: ev.score_quantiles(s, [0.5], limit=9),
                lambda: ev.score_quantiles(np.zeros((0, 4), np.float32), [0.5]),
                # N too large: shapes alone decide, so a broadcast view stands in for 2^31 values
                lambda: ev.ranked_cumulative(np.broadcast_to(np.zeros(1, bool), (1 << 16, 1 << 15)),
                                             np.broadcast_to(np.zeros(1, np.float32), (1 << 16, 1 << 15)))):
        with pytest.raises(ValueError):
            bad()


@pytest.fixture(scope="module")
def plan_check(tmp_path_factory):
    cxx = next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    if cxx is None or shutil.which("make") is None:
        pytest.skip("no host C++ compiler")
    out = tmp_path_factory.mktemp("plan_check_rank")
    subprocess.run(["make", "-C", str(CSRC), "plan_check", f"OUT_DIR={out}", f"CXX={cxx}"], check=True, capture_output=True, text=True)
    return out / "plan_check"


def expected_plan(rows, k, limit, key_bytes, has_correct, want_cum, want_wide):
    """plan_rank by hand: 'refused', or the line `plan_check rank` prints"""
    n = rows * limit
    if rows < 1 or k < 1 or not 1 <= limit <= k or k > 2 ** 31 - 1 or key_bytes not in (4, 8) or n > 2 ** 31 - 1 or rows * k > (2 ** 63 - 1) // 16:
        return "refused"
    ntiles = -(-n // TILE)
    table = 256 * ntiles
    table_blocks = -(-table // SCAN_BLOCK)
    cum_blocks = -(-n // SCAN_BLOCK) if want_cum else 0
    pack = 2 * limit <= k  # the first `limit` columns are packed on the host when that at least halves the upload
    dev_k = limit if pack else k
    sizes = [rows * dev_k * key_bytes, rows * dev_k if has_correct else 0, n * key_bytes, n * 4, table * 4, max(table_blocks, cum_blocks) * 4,
             key_bytes * 256 * 4, n * 4 if want_cum else 0, n * 8 if want_wide else 0]
    resident = sum(sizes) + sizes[2] + sizes[3]  # two key and two payload buffers
    return f"{n} {ntiles} {table} {table_blocks} {cum_blocks} {key_bytes} {int(pack)} {dev_k} " + " ".join(map(str, sizes)) + f" {resident}"


def test_rank_plans_are_the_ones_worked_out_by_hand(plan_check):
    """(the sweep of tests/test_plan_cpu.py walks plan_rank's invariants under the same sanitizers)"""
    shapes = [(1, 1, 1), (TILE - 1, 1, 1), (TILE, 1, 1), (TILE + 1, 1, 1), (3 * TILE + 5, 1, 1), (SCAN_BLOCK + 1, 2, 1), (SCAN_TOP * SCAN_BLOCK + 1, 1, 1),
              ((SCAN_TOP * SCAN_BLOCK // 256 + 1) * TILE + 5, 1, 1), (200000, 300, 300), (200000, 300, 10), (200000, 300, 150), (200000, 300, 151),
              (2 ** 31 - 1, 1, 1), (1, 2 ** 31 - 1, 2 ** 31 - 1), (1, 2 ** 31, 5), (2 ** 31, 1, 1), (7158279, 300, 300), (0, 5, 5), (5, 5, 0), (5, 4, 5),
              (2 ** 62, 2 ** 62, 2 ** 62), (2 ** 40, 2 ** 30, 1)]
    cases = [(r, k, l, kb, hc, c, w) for r, k, l in shapes for kb in (4, 8) for hc, c, w in ((0, 0, 0), (1, 1, 0), (1, 1, 1), (0, 0, 1), (1, 0, 0))]
    cases += [(10, 10, 10, 2, 1, 1, 1), (10, 10, 10, 16, 1, 1, 1)]
    lines = "".join(" ".join(map(str, c)) + "\n" for c in cases)
    r = subprocess.run([str(plan_check), "rank"], input=lines, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    out = r.stdout.splitlines()
    assert len(out) == len(cases)
    wrong = {c: (got, expected_plan(*c)) for c, got in zip(cases, out) if got != expected_plan(*c)}
    assert not wrong, wrong
    assert "refused" in out and any(o != "refused" for o in out)
