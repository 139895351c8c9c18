"""No GPU: the planners of csrc/plan.h as the stand-alone program csrc/plan_check.cpp, built here with the host
compiler under ASan/UBSan.  `sweep` walks a grid of shapes and flags and checks the plans' invariants; `cases` plans every
case of tests/plan_cases.py, and the last piece's launch must be the one the table records (test_plan_gpu.py compares the
library's own introspection with the same table); `sym` and `range` print the symmetric self-search's and the range scan's
plans, which must be the ones of SYM_EXPECT and RANGE_EXPECT."""
import shutil
import subprocess
from pathlib import Path

import pytest

import plan_cases as pc

CSRC = Path(__file__).resolve().parent.parent / "knn-for-homology_amd" / "csrc"


@pytest.fixture(scope="module")
def plan_check(tmp_path_factory):
    cxx = next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    if cxx is None or shutil.which("make") is None:
        pytest.skip("no host C++ compiler")
    out = tmp_path_factory.mktemp("plan_check")
    subprocess.run(["make", "-C", str(CSRC), "plan_check", f"OUT_DIR={out}", f"CXX={cxx}"], check=True, capture_output=True, text=True)
    return out / "plan_check"


def test_sweep_holds_every_invariant(plan_check):
    r = subprocess.run([str(plan_check), "sweep"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 broken" in r.stdout


def _last_launch(line):
    """(kernel, query_tile, db_tile, nchunks, grid, seed_stride, stat_rank, sample_rows) of the last piece of a `cases` line"""
    f = line.split(" | ")[-1].split()
    assert f[2] == "L0", line
    name = f[3]
    qt, dt, nchunks, grid, _npairs, _cap, _lds, sstride, seed_stat, seed_j, pub_rounds, pub_m, _kslot, _qcap, _pool, sample_rows = map(int, f[4:20])
    return (name, qt, dt, nchunks, grid, -pub_rounds * pub_m if pub_rounds else sstride, seed_j if seed_stat else 0, sample_rows)


def test_cases_plan_what_the_table_records(plan_check):
    lines = "".join(f"{c.nb} {c.nq} {c.k} {c.metric} {c.flags} {c.force_qt} {c.force_chunks} {c.batch} {int(c.entry != 'stream')} {int(c.approx16)}\n"
                    for c in pc.CASES)
    r = subprocess.run([str(plan_check), "cases"], input=lines, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = r.stdout.splitlines()
    assert len(out) == len(pc.CASES)
    got = {c.name: _last_launch(line) for c, line in zip(pc.CASES, out)}
    wrong = {n: (got[n], pc.EXPECT.get(n)) for n in got if got[n] != pc.EXPECT.get(n)}
    assert not wrong, wrong
    assert set(pc.EXPECT) == set(got)


def _lines(plan_check, sub, lines, n):
    r = subprocess.run([str(plan_check), sub], input=lines, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = r.stdout.splitlines()
    assert len(out) == n
    return out


def _sym_plan(line):
    """a `sym` line as SYM_EXPECT holds it"""
    if line == "plain":
        return None
    f = line.split()
    groups = int(f[9])
    gstart, rest = f[10:11 + groups], f[11 + groups:]
    assert len(rest) == 5, line
    return (f[0], *map(int, f[1:10]), tuple(map(int, gstart)), *map(int, rest[:4]), rest[4])


def test_sym_plans_what_the_table_records(plan_check):
    lines = "".join(f"{c.n} {c.k} {c.metric} {c.flags} {c.can_stream} {c.force_qt}\n" for c in pc.SYM_CASES)
    out = _lines(plan_check, "sym", lines, len(pc.SYM_CASES))
    got = {c.name: _sym_plan(line) for c, line in zip(pc.SYM_CASES, out)}
    wrong = {n: (got[n], pc.SYM_EXPECT.get(n, "missing")) for n in got if n not in pc.SYM_EXPECT or got[n] != pc.SYM_EXPECT[n]}
    assert not wrong, wrong
    assert set(pc.SYM_EXPECT) == set(got)


def test_range_plans_what_the_table_records(plan_check):
    lines = "".join(f"{c.n} {c.nq} {c.metric} {c.batch}\n" for c in pc.RANGE_CASES)
    out = _lines(plan_check, "range", lines, len(pc.RANGE_CASES))
    got = {c.name: (line.split()[0], *map(int, line.split()[1:])) for c, line in zip(pc.RANGE_CASES, out)}
    wrong = {n: (got[n], pc.RANGE_EXPECT.get(n)) for n in got if got[n] != pc.RANGE_EXPECT.get(n)}
    assert not wrong, wrong
    assert set(pc.RANGE_EXPECT) == set(got)
