"""bench.py's command line: what a plain run prints and what --dump-outputs writes."""

import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def test_dump_outputs_writes_every_row_or_a_fixed_sample(tmp_path, monkeypatch):
    import bench
    monkeypatch.setattr(bench, "DUMP_BYTES", 64 * 4 * 8)               # 64 rows of 8 floats
    small = torch.randn(50, 8)
    bench.dump_outputs(small, str(tmp_path / "small"))
    got = np.load(tmp_path / "small" / "out.npy")
    assert got.dtype == np.float32 and np.array_equal(got, small.numpy())

    big = torch.arange(1000 * 8, dtype=torch.float32).reshape(1000, 8)
    for run in ("a", "b"):
        bench.dump_outputs(big, str(tmp_path / run))
    a, b = np.load(tmp_path / "a" / "out.npy"), np.load(tmp_path / "b" / "out.npy")
    assert a.shape == (64, 8) and a.dtype == np.float32 and np.array_equal(a, b)
    rows = a[:, 0].astype(np.int64) // 8
    assert np.all(np.diff(rows) > 0) and np.array_equal(a, big.numpy()[rows])


def test_steps_must_be_positive():
    r = subprocess.run([sys.executable, BENCH, "--steps", "0"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and "--steps must be at least 1" in r.stderr


@pytest.mark.gpu
def test_plain_run_reports_the_headline_and_dumps_the_last_step(tmp_path):
    r = subprocess.run([sys.executable, BENCH, "--workload", "c1", "--steps", "3", "--warmup", "1",
                        "--dump-outputs", str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert key in line
    assert line["steps"] == 3 and line["ms_per_step"] > 0 and line["value"] == pytest.approx(11 / (line["ms_per_step"] * 1e-3))
    assert "roofline" not in line and "cpu_baseline" not in line, "the extra measurements belong to --full"
    out = np.load(tmp_path / "out.npy")
    assert out.shape == (8, 32) and out.dtype == np.float32 and np.isfinite(out).all()


@pytest.mark.gpu
def test_full_run_adds_the_roofline():
    r = subprocess.run([sys.executable, BENCH, "--workload", "c1", "--steps", "3", "--warmup", "1", "--full", "--no-cpu-baseline",
                        "--kernel-reps", "3"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["steps"] == 3 and line["roofline"]["ms_per_launch"] > 0 and "cpu_baseline" not in line
