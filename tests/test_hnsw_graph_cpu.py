"""No GPU: the HIP-free host code of csrc/hnsw_graph.h as the stand-alone program csrc/hnsw_check.cpp, built here with the
host compiler under ASan/UBSan.  The level table, the link order of an add call and its batch schedule must be the ones
tests/hnsw_build_reference.py replays (the first comparison of the two that needs no GPU); the visited set's two modes and
heap_replace_top are checked by the program against each other and against the standard heap calls."""
import shutil
import subprocess
from pathlib import Path

import pytest

import hnsw_build_reference as ref

CSRC = Path(__file__).resolve().parent.parent / "knn-for-homology_amd" / "csrc"


@pytest.fixture(scope="module")
def hnsw_check(tmp_path_factory):
    cxx = next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    if cxx is None or shutil.which("make") is None:
        pytest.skip("no host C++ compiler")
    out = tmp_path_factory.mktemp("hnsw_check")
    subprocess.run(["make", "-C", str(CSRC), "hnsw_check", f"OUT_DIR={out}", f"CXX={cxx}"], check=True, capture_output=True, text=True)
    return out / "hnsw_check"


def _ints(prog, *args):
    r = subprocess.run([str(prog), *map(str, args)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return [int(v) for v in r.stdout.split()]


@pytest.mark.parametrize("M", [2, 16, 32, 42, 63])
def test_level_table_is_the_replays(hnsw_check, M):
    assert _ints(hnsw_check, "levels", M) == ref.level_table(M).tolist()


@pytest.mark.parametrize("n0,n", [(0, 1), (0, 2), (0, 33), (1000, 257), (123456, 1000)])
def test_link_order_is_the_replays(hnsw_check, n0, n):
    assert _ints(hnsw_check, "order", n0, n, 1) == ref.call_order(n0, n)
    assert _ints(hnsw_check, "order", n0, n, 0) == list(range(n0, n0 + n))


@pytest.mark.parametrize("done", [0, 100000])
@pytest.mark.parametrize("max_batch", [32, 16384])
@pytest.mark.parametrize("n", [1, 31, 32, 33, 1024, 70000])
def test_batch_schedule_is_the_replays(hnsw_check, n, max_batch, done):
    want = [len(b) for b in ref.call_batches(done, done, n, max_batch)]
    assert sum(want) == n
    assert _ints(hnsw_check, "batches", done, n, max_batch) == want


def test_visited_set_and_heap_agree_with_their_references(hnsw_check):
    r = subprocess.run([str(hnsw_check), "self"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "self ok" in r.stdout
