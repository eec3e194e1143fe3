"""bench.py contract smoke on a real GPU (the driver's entry point)."""

import json
import os
import subprocess
import sys
from pathlib import Path

import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

REPO = Path(__file__).resolve().parent.parent


@pytest.mark.parametrize("engine", ["native", "python"])
def test_bench_single_gpu_json_contract(engine):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    env = dict(os.environ)
    env["PYTHONPATH"] = str(REPO)
    res = subprocess.run(
        [
            sys.executable,
            "bench.py",
            "--engine",
            engine,
            "--steps",
            "12",
            "--warmup",
            "3",
            "--events-per-batch",
            "4000000",
            "--batches-per-poll",
            "4",
            "--vocab",
            "20000",
        ],
        capture_output=True,
        timeout=420,
        cwd=str(REPO),
        env=env,
    )
    assert res.returncode == 0, res.stderr.decode()[-1500:]
    line = res.stdout.decode().strip().splitlines()[-1]
    d = json.loads(line)
    assert d["n_gpus"] == 1
    assert d["steps"] == 12
    assert d["higher_is_better"] is True
    assert d["value"] > 0
    assert d["ms_per_step"] > 0
    assert d["data"] == "synthetic"
    got = d["config"]["engine"]
    if engine == "python":
        assert got.startswith("dataflow")
    else:
        assert got == engine


def test_bench_dump_outputs_gpu(tmp_path):
    """--dump-outputs writes what the last timed step emitted.

    4 batches x 5 s per step, 60 s windows: poll 15 (the last of 3
    warmup + 13 timed) hands out batches 60..63, whose first batch
    moves the watermark past 300 s and closes window [240 s, 300 s):
    12 batches x 4M events over all 20000 keys."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import numpy as np

    env = dict(os.environ)
    env["PYTHONPATH"] = str(REPO)
    res = subprocess.run(
        [
            sys.executable,
            "bench.py",
            "--gpus",
            "1",
            "--steps",
            "13",
            "--warmup",
            "3",
            "--events-per-batch",
            "4000000",
            "--batches-per-poll",
            "4",
            "--vocab",
            "20000",
            "--dump-outputs",
            str(tmp_path),
        ],
        capture_output=True,
        timeout=420,
        cwd=str(REPO),
        env=env,
    )
    assert res.returncode == 0, res.stderr.decode()[-1500:]
    d = json.loads(res.stdout.decode().strip().splitlines()[-1])
    assert d["steps"] == 13
    cols = {
        n: np.load(tmp_path / f"{n}.npy")
        for n in ("keys", "window_start_ms", "counts", "n_rows")
    }
    assert all(c.dtype == np.float64 for c in cols.values())
    assert cols["n_rows"][0] == 20000
    assert np.array_equal(cols["keys"], np.arange(20000))
    t0 = 1704067200000  # 2024-01-01T00:00:00Z
    assert np.all(cols["window_start_ms"] == t0 + 240_000)
    assert cols["counts"].sum() == 12 * 4_000_000
