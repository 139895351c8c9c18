"""GPU: a plain `bench.py` run at a small size -- one JSON line holding the headline and nothing of `--full`, `--steps`
timed steps, and `--dump-outputs` writing the last timed step's (D, I), identical from run to run."""
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


def _bench(out_dir, steps):
    p = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "2",
                        "--nb-total", "200000", "--dump-outputs", str(out_dir)],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = p.stdout.strip().splitlines()
    assert len(lines) == 1, p.stdout
    return json.loads(lines[0])


def test_plain_bench_line_and_dumped_outputs(tmp_path):
    a = _bench(tmp_path / "a", 5)
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert key in a, key
    assert a["steps"] == 5 and a["unit"] == "queries/s" and a["dtype"] == "f32" and a["higher_is_better"] is True
    assert a["ms_per_step"] > 0 and a["value"] == pytest.approx(32 * 1e3 / a["ms_per_step"], rel=1e-6)
    assert a["verification"]["planted_rows_first_on_every_rank"] and a["verification"]["sorted_and_in_range"]
    for key in ("roofline", "cpu_baseline", "batch", "all_vs_all_query_sharded", "shard_unit", "sweep", "host_buffers", "hnsw",
                "efficiency_vs_shard_sweep"):
        assert key not in a, key

    D = np.load(tmp_path / "a" / "distances.npy")
    I = np.load(tmp_path / "a" / "labels.npy")
    assert D.dtype == np.float32 and I.dtype == np.float64 and D.shape == I.shape == (32, 100)
    assert not (tmp_path / "a" / "query_rows.npy").exists()
    assert (np.diff(D, axis=1) <= 0).all() and ((I >= 0) & (I < 200000)).all() and (I == np.round(I)).all()
    planted = a["verification"]["planted"]["0"][0]  # (query 0's copy in the database: first, score 1)
    assert I[0, 0] == planted and abs(D[0, 0] - 1.0) < 1e-5

    b = _bench(tmp_path / "b", 3)
    assert b["steps"] == 3
    assert np.array_equal(np.load(tmp_path / "b" / "distances.npy").view(np.uint32), D.view(np.uint32))
    assert np.array_equal(np.load(tmp_path / "b" / "labels.npy"), I)
