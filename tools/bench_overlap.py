"""compare_hits on one MI355X at the reference's size: 200 000 queries, 300 hits against 300, random ids of which a
third are shared between the lists.

    python tools/bench_overlap.py --out profiles/overlap_probe.json

pfam/pfam.py:349-363 and 602-622 walk the two lists of every query in Python loops over `set` objects; the time of those
loops is measured where the reference is available (tests/golden/make_overlap_golden.py --time, 2000 rows) and is not
part of this tool.  Two steps, each a child process of its own under its own time limit, the second only when the first
ended well: `warm` makes one call on 64 rows and compares it with plain Python sets; `full` makes --reps calls at the full
size and reports of each the wall clock and what last_overlap_ms gives by HIP events: upload, kernel, download.  This
process itself never opens the device.  Nothing is gated on a speed.  Prints one JSON line (and writes it to --out)."""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
STEP_SECONDS = {"warm": 120, "full": 420}


def inputs(rng, rows, k, nids):
    hits_a = rng.integers(0, nids, (rows, k)).astype(np.int64)
    hits_b = rng.integers(0, nids, (rows, k)).astype(np.int64)
    hits_b[:, ::3] = hits_a[:, ::3]
    labels = rng.integers(0, 2, nids).astype(np.uint8)  # a hit is correct when its id's label is 1: the lists agree about shared ids
    return hits_a, labels[hits_a], hits_b, labels[hits_b]


def python_sets(hits_a, correct_a, hits_b, correct_b):
    """the sizes compare_hits returns, from Python sets"""
    def run(h, c):
        out = set()
        for i, f in zip(h, c):
            if i < 0:
                continue
            if not f:
                break
            out.add(i)
        return out
    tp, lead = [], []
    for ha, ca, hb, cb in zip(hits_a.tolist(), correct_a.tolist(), hits_b.tolist(), correct_b.tolist()):
        ta, tb = {i for i, f in zip(ha, ca) if i >= 0 and f}, {i for i, f in zip(hb, cb) if i >= 0 and f}
        la, lb = run(ha, ca), run(hb, cb)
        tp.append([len(ta - tb), len(ta & tb), len(tb - ta)])
        lead.append([len(la - lb), len(la & lb), len(lb - la)])
    return np.asarray(tp, np.int32), np.asarray(lead, np.int32)


def step(args):
    from knn_for_homology_amd import _lib, evaluation
    rng = np.random.default_rng(349)
    if args.step == "warm":
        case = inputs(rng, 64, args.k, 2000)
        got = evaluation.compare_hits(*case)
        tp, lead = python_sets(*case)
        return {"warm_rows": 64, "warm_equal": bool(np.array_equal(got.tp, tp) and np.array_equal(got.lead, lead))}
    case = inputs(rng, args.rows, args.k, args.ids)
    evaluation.compare_hits(*(a[:64] for a in case))  # the first call of a process loads the code object
    calls = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        got = evaluation.compare_hits(*case)
        calls.append({"wall_ms": 1e3 * (time.perf_counter() - t0), **evaluation.last_overlap_ms()})
    return {"box": socket.gethostname(), "library": _lib.lib().knn_version().decode(), "numpy": np.__version__, "rows": args.rows, "k": args.k,
            "ids": args.ids, "reps": args.reps, "calls": calls, "tp_totals": got.tp.sum(axis=0, dtype=np.int64).tolist(),
            "lead_totals": got.lead.sum(axis=0, dtype=np.int64).tolist()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=200000)
    ap.add_argument("--k", type=int, default=300)
    ap.add_argument("--ids", type=int, default=200000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", choices=sorted(STEP_SECONDS), default=None, help="(internal) run one step in this process")
    args = ap.parse_args()
    if args.step:
        print(json.dumps(step(args)), flush=True)
        return 0
    rec = {}
    for name in ("warm", "full"):
        cmd = [sys.executable, os.path.abspath(__file__), "--step", name, "--rows", str(args.rows), "--k", str(args.k), "--ids", str(args.ids),
               "--reps", str(args.reps)]
        try:
            done = subprocess.run(cmd, stdout=subprocess.PIPE, timeout=STEP_SECONDS[name])
        except subprocess.TimeoutExpired:
            print(f"bench_overlap: step {name} ran past {STEP_SECONDS[name]} s", file=sys.stderr)
            return 124
        if done.returncode != 0:
            print(f"bench_overlap: step {name} ended with status {done.returncode}", file=sys.stderr)
            return 1
        rec.update(json.loads(done.stdout.decode().strip().splitlines()[-1]))
        if name == "warm" and not rec["warm_equal"]:
            print("bench_overlap: the warm call differs from the Python sets", file=sys.stderr)
            return 1
    line = json.dumps(rec)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
