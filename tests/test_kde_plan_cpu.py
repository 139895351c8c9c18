"""No GPU: plan_kde of csrc/plan.h through the stand-alone csrc/plan_check.cpp, built here with the host compiler under
ASan/UBSan (as tests/test_plan_cpu.py builds it).  Its `sweep`, which tests/test_plan_cpu.py runs, checks the invariants
over a grid; the tests below restate the counts for the shapes tests/test_kde_gpu.py uses: groups of the statistics,
chunks, tiles and both tails are those of the contract (tests/kde_reference.py)."""
import shutil
import subprocess
from pathlib import Path

import pytest

import kde_reference as ref

CSRC = Path(__file__).resolve().parent.parent / "knn-for-homology_amd" / "csrc"
NS = (2, 5, 255, 256, 257, 4097, 16384, 16385, 40000, 1048581)
MS = (1, 15, 16, 17, 1000)


@pytest.fixture(scope="module")
def plan_check(tmp_path_factory):
    cxx = next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    if cxx is None or shutil.which("make") is None:
        pytest.skip("no host C++ compiler")
    out = tmp_path_factory.mktemp("plan_check_kde")
    subprocess.run(["make", "-C", str(CSRC), "plan_check", f"OUT_DIR={out}", f"CXX={cxx}"], check=True, capture_output=True, text=True)
    return out / "plan_check"


def run(plan_check, text):
    r = subprocess.run([str(plan_check), "kde"], input=text, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout.splitlines()


def test_counts_of_the_gpu_tests_shapes(plan_check):
    cases = [(n, c, m) for n in NS for c in (1, 3) for m in MS]
    out = run(plan_check, "".join(f"{n} {c} {m}\n" for n, c, m in cases))
    assert len(out) == len(cases)
    for (n, c, m), line in zip(cases, out):
        group_rows, groups, tiles, chunks, tail_rows, tail_points, part_bytes = map(int, line.split())
        assert group_rows == ref.group_rows(n) and groups == -(-n // group_rows)
        assert chunks == -(-n // ref.CHUNK) and tail_rows == n - (chunks - 1) * ref.CHUNK and 1 <= tail_rows <= ref.CHUNK
        assert tiles == -(-m // ref.TILE) and tail_points == m - (tiles - 1) * ref.TILE and 1 <= tail_points <= ref.TILE
        assert part_bytes == c * chunks * m * 8


def test_known_cases(plan_check):
    assert run(plan_check, "40000 3 1000\n16385 1 17\n1048581 3 1\n") == ["4096 10 63 3 7232 8 72000", "4096 5 2 2 1 1 272", "8192 129 1 65 5 1 1560"]


def test_illegal_launches_are_refused(plan_check):
    top = 65535 * 16384
    lines = ["1 1 1", "0 1 1", "2 0 1", "2 4097 1", "2 1 0", f"2 1 {(1 << 24) + 1}", f"{top + 1} 1 1", "-5 1 1"]
    assert run(plan_check, "\n".join(lines) + "\n") == ["refused"] * len(lines)
    assert run(plan_check, f"{top} 4096 {1 << 24}\n") == [f"4194304 256 {1 << 20} 65535 16384 16 {4096 * 65535 * (1 << 24) * 8}"]
