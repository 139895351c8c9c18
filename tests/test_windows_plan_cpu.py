"""No GPU: plan_windows and window_piece of csrc/plan.h through the stand-alone, sanitizer-built csrc/windows_check.cpp.

`windows_check sweep` walks window_chain_kernel's staging on the host -- the kernel and the checker call the same
window_piece -- for N in {1, 2, 255, 256, 2047, 2048, 2049, 70 000} and W in {1, 2, 3, N, N - 1, run - 1, run, run + 1,
2 run + 1, ...} clipped to [1, N]: every rank is staged exactly once per direction, every chain's pieces are contiguous
and in order and end at the block's other end, every 16-byte load stays inside the padded keys and every LDS slot inside
the run, the buffers add up to resident_bytes, no grid is 0 or above the launch limits, and every argument error is
refused.  `windows_check plan` prints plans that are worked out by hand here."""
import shutil
import subprocess
from pathlib import Path

import pytest

CSRC = Path(__file__).resolve().parent.parent / "knn-for-homology_amd" / "csrc"
RUN, CHAINS, SCAN_BLOCK, TILE = 2048, 256, 1024, 2048  # WINDOW_RUN, WINDOW_CHAINS, RANK_SCAN_BLOCK, RANK_TILE of csrc/plan.h


@pytest.fixture(scope="module")
def windows_check(tmp_path_factory):
    cxx = next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    if cxx is None or shutil.which("make") is None:
        pytest.skip("no host C++ compiler")
    out = tmp_path_factory.mktemp("windows_check")
    subprocess.run(["make", "-C", str(CSRC), "windows_check", f"OUT_DIR={out}", f"CXX={cxx}"], check=True, capture_output=True, text=True)
    return out / "windows_check"


def test_sweep_holds_every_invariant(windows_check):
    r = subprocess.run([str(windows_check), "sweep"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 failures" in r.stdout


def rank_resident(n, key_bytes, want_order):
    """plan_rank(n, 1, 1, key_bytes, no flags, no running count, want_order).resident_bytes (tests/test_rank_reference.py)"""
    ntiles = -(-n // TILE)
    table = 256 * ntiles
    return n * key_bytes + 2 * n * key_bytes + 2 * n * 4 + table * 4 + -(-table // SCAN_BLOCK) * 4 + key_bytes * 256 * 4 + (n * 8 if want_order else 0)


def expected(n, key_bytes, m, window, want_order, nbins):
    if not 1 <= n <= 2 ** 31 - 1 or key_bytes not in (4, 8) or not 0 <= m <= 32 or not 0 <= window <= n or not 0 <= nbins <= 2 ** 20 or (window == 0 and nbins == 0):
        return "refused"
    nout = n - window + 1 if window else 0
    nblocks = -(-n // window) if window else 0
    bpr = (min(RUN // window, CHAINS // 2) if window <= RUN else 1) if window else 0
    rpb = (-(-window // RUN) if window > RUN else 1) if window else 0
    group = bpr * window
    grid = -(-n // group) if window else 0
    lds = 2 * (RUN + RUN // 32) * 8
    scan_blocks = -(-n // SCAN_BLOCK) if m else 0
    sizes = [m * n, n * 4 if m else 0, m * n * 4, scan_blocks * 4, (n + 1) // 2 * 2 * 8 if window else 0, n * 8 if window else 0, (m + 1) * nout * 8,
             nbins * (16 + m * 8 + 3 * key_bytes)]
    resident = rank_resident(n, key_bytes, want_order) + sum(sizes) + sizes[5]
    return f"{nout} {nblocks} {RUN} {bpr} {rpb} {group} {grid} {lds} {scan_blocks} " + " ".join(map(str, sizes)) + f" {resident}"


def test_plans_are_the_ones_worked_out_by_hand(windows_check):
    shapes = [(1, 1), (300, 7), (300, 300), (2049, 1000), (4097, 1000), (3 * RUN + 5, RUN - 1), (3 * RUN + 5, RUN), (3 * RUN + 5, RUN + 1),
              (3 * RUN + 5, 2 * RUN + 1), (60_000_000, 1000), (60_000_000, 0), (2 ** 31 - 1, 1), (2 ** 31 - 1, 2 ** 31 - 1), (300, 1), (300, 16), (300, 17)]
    cases = [(n, kb, m, w, o, nb) for n, w in shapes for kb in (4, 8) for m, o, nb in ((0, 0, 0), (5, 1, 0), (32, 0, 10), (1, 1, 7))]
    # one refused case per argument error
    cases += [(0, 4, 1, 1, 0, 0), (2 ** 31, 4, 1, 1, 0, 0), (10, 2, 1, 1, 0, 0), (10, 4, -1, 1, 0, 0), (10, 4, 33, 1, 0, 0), (10, 4, 1, -1, 0, 0),
              (10, 4, 1, 11, 0, 0), (10, 4, 1, 0, 0, 0), (10, 4, 1, 1, 0, -1), (10, 4, 1, 1, 0, 2 ** 20 + 1)]
    lines = "".join(" ".join(map(str, c)) + "\n" for c in cases)
    r = subprocess.run([str(windows_check), "plan"], input=lines, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    out = r.stdout.splitlines()
    assert len(out) == len(cases)
    wrong = {c: (got, expected(*c)) for c, got in zip(cases, out) if got != expected(*c)}
    assert not wrong, wrong
    assert all(o == "refused" for o in out[-10:]) and sum(o == "refused" for o in out) == 10 + 4  # (+ the shape with neither a window nor bins)
