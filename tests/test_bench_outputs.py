"""bench.py --dump-outputs / --full contract (CPU twin, tiny sizes)."""

import json
import os
import subprocess
import sys
from pathlib import Path

import pytest

np = pytest.importorskip("numpy")
pytest.importorskip("torch")

REPO = Path(__file__).resolve().parent.parent

# 3 timed steps of 30 batches x 5 s = 2.5 windows per step: the last
# step emits exactly the two 60 s windows [720 s, 780 s) and
# [780 s, 840 s), 12 batches x 2000 events each.
E, B, VOCAB = 2000, 30, 100


def _run(dump_dir, *extra):
    env = dict(os.environ)
    env["PYTHONPATH"] = str(REPO)
    # CPU twin everywhere: bench.py picks the device by availability.
    env["HIP_VISIBLE_DEVICES"] = ""
    env["CUDA_VISIBLE_DEVICES"] = ""
    res = subprocess.run(
        [
            sys.executable,
            str(REPO / "bench.py"),
            "--gpus", "1",
            "--steps", "3",
            "--warmup", "3",
            "--events-per-batch", str(E),
            "--batches-per-poll", str(B),
            "--vocab", str(VOCAB),
            "--device", "cpu",
            "--dump-outputs", str(dump_dir),
            *extra,
        ],
        capture_output=True,
        timeout=120,
        cwd=str(REPO),
        env=env,
    )
    assert res.returncode == 0, res.stderr.decode()[-1500:]
    return json.loads(res.stdout.decode().strip().splitlines()[-1])


def test_dump_outputs_cpu(tmp_path: Path):
    a, b = tmp_path / "a", tmp_path / "b"
    d = _run(a)
    assert d["steps"] == 3
    assert d["ms_per_step"] > 0
    _run(b, "--full")
    names = sorted(p.name for p in a.iterdir())
    assert names == [
        "counts.npy", "keys.npy", "n_rows.npy", "window_start_ms.npy",
    ]
    cols = {}
    for name in names:
        x, y = np.load(a / name), np.load(b / name)
        assert x.dtype == np.float64
        assert np.array_equal(x, y), name
        cols[name[:-4]] = x
    assert sum(x.nbytes for x in cols.values()) <= 64 << 20
    n = int(cols["n_rows"][0])
    assert n == 2 * VOCAB == len(cols["keys"])
    t0 = 1704067200000  # 2024-01-01T00:00:00Z
    assert sorted(set(cols["window_start_ms"] - t0)) == [720e3, 780e3]
    assert cols["counts"].sum() == 2 * 12 * E
    # Canonical (window, key) order.
    for w in (720e3, 780e3):
        k = cols["keys"][cols["window_start_ms"] - t0 == w]
        assert np.array_equal(k, np.arange(VOCAB))
