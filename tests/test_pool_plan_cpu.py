"""No GPU: plan_pool and pool_assign_chunks of csrc/plan.h through the stand-alone csrc/plan_check.cpp, built here with
the host compiler under ASan/UBSan (as tests/test_plan_cpu.py builds it).  Its `sweep`, which tests/test_plan_cpu.py
runs, checks the invariants over a grid (every column owned once, the grid limits, every range in one chunk that holds
it); the tests below restate the two rules in Python for the shapes the GPU tests use: every (range, column) pair is covered exactly once, the aligned /
element-wise choice is the pointer's and the stride's, and the chunks are the ones the header describes."""
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import pool_reference as ref

CSRC = Path(__file__).resolve().parent.parent / "knn-for-homology_amd" / "csrc"
DS = (2, 8, 20, 1024, 1028, 3072)


@pytest.fixture(scope="module")
def plan_check(tmp_path_factory):
    cxx = next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    if cxx is None or shutil.which("make") is None:
        pytest.skip("no host C++ compiler")
    out = tmp_path_factory.mktemp("plan_check_pool")
    subprocess.run(["make", "-C", str(CSRC), "plan_check", f"OUT_DIR={out}", f"CXX={cxx}"], check=True, capture_output=True, text=True)
    return out / "plan_check"


def run(plan_check, sub, text):
    r = subprocess.run([str(plan_check), sub], input=text, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout.splitlines()


@pytest.mark.parametrize("normalize", [0, 1])
@pytest.mark.parametrize("d", DS)
def test_every_range_and_column_is_covered_once(plan_check, d, normalize):
    n = 37
    ncb, waves, grid_x, grid_y, aligned = map(int, run(plan_check, "pool", f"{n} {d} {d} 4096 4 {normalize}\n")[0].split())
    assert ncb == -(-d // 256) and grid_x == n
    assert waves <= (16 if normalize else 4) and (not normalize or 64 % waves == 0)
    owners = np.zeros((n, d), np.int64)
    for o in range(grid_x):
        for y in range(grid_y):
            for w in range(waves):
                c0 = (y * waves + w) * 256 + 4 * np.arange(64)
                for e in range(4):
                    c = c0 + e
                    np.add.at(owners[o], c[c < d], 1)
    assert (owners == 1).all()
    assert (grid_y - 1) * waves < ncb, "a workgroup without a column block"
    assert aligned == int(d % 4 == 0)


def test_aligned_follows_the_pointer_and_the_stride(plan_check):
    cases = []
    for elem in (4, 2):
        for base in (4096, 4096 + elem, 4096 + 2 * elem, 4096 + 4 * elem, 4096 + 8):
            for d, stride in ((20, 20), (20, 24), (20, 21), (1026, 1028), (1026, 1026), (8, 8)):
                cases.append((elem, base, d, stride))
    out = run(plan_check, "pool", "".join(f"5 {d} {s} {b} {e} 0\n" for e, b, d, s in cases))
    assert len(out) == len(cases)
    for (elem, base, d, stride), line in zip(cases, out):
        assert int(line.split()[4]) == int(base % (4 * elem) == 0 and stride % 4 == 0), (elem, base, d, stride, line)


def test_illegal_launches_are_refused(plan_check):
    lines = ["0 8 8 4096 4 0", "5 1 1 4096 4 0", "5 8 7 4096 4 0", "5 8 8 4096 8 0", f"5 {(1 << 20) + 1} {(1 << 20) + 1} 4096 4 0",
             f"{1 << 31} 8 8 4096 4 0"]
    assert run(plan_check, "pool", "\n".join(lines) + "\n") == ["refused"] * len(lines)
    assert run(plan_check, "pool", f"{(1 << 31) - 1} {1 << 20} {1 << 20} 4096 2 1\n") == [f"4096 16 {(1 << 31) - 1} 256 1"]


def chunks_of(plan_check, starts, stops, chunk_rows):
    text = f"{len(starts)} {chunk_rows}\n" + "".join(f"{a} {b}\n" for a, b in zip(starts, stops))
    out = []
    for line in run(plan_check, "poolchunks", text):
        head, _, members = line.partition(":")
        row0, row1, count = map(int, head.split())
        members = [int(v) for v in members.split()]
        assert len(members) == count
        out.append((row0, row1, members))
    return out


@pytest.mark.parametrize("chunk_rows", [1, 50, 64, 129, 700, 1500, 1 << 40])
def test_chunks_hold_their_ranges(plan_check, chunk_rows):
    starts, stops = ref.ranges(1500, 11)
    chunks = chunks_of(plan_check, starts, stops, chunk_rows)
    seen = sorted(o for _, _, members in chunks for o in members)
    assert seen == list(range(len(starts))), "every range in exactly one chunk"
    for row0, row1, members in chunks:
        assert row0 == starts[members[0]] and row1 == max(stops[o] for o in members)
        assert all(row0 <= starts[o] and stops[o] <= row1 for o in members)
        first_len = stops[members[0]] - starts[members[0]]
        assert row1 - row0 <= chunk_rows or (first_len > chunk_rows and row1 == stops[members[0]]), "only a longer range exceeds the budget"
    if chunk_rows >= 1500:
        assert len(chunks) == 1
    if chunk_rows == 700:
        assert any(row1 - row0 == 1500 for row0, row1, _ in chunks), "the range over all rows is a chunk beyond the budget"


def test_chunks_of_a_known_case(plan_check):
    #          0        1        2         3         4        5 (longer than a chunk)   6 (duplicate of 1)
    starts = [0, 5, 9, 30, 12, 2, 5]
    stops = [4, 12, 10, 31, 20, 29, 12]
    # by (start, stop, index): 0, 5, 1, 6, 2, 4, 3; ranges that end inside the budget behind the long range's start ride with it
    assert chunks_of(plan_check, starts, stops, 10) == [(0, 4, [0]), (2, 29, [5, 1, 6, 2]), (12, 20, [4]), (30, 31, [3])]
