"""bench.py without --full: only the headline (set-up, warm-up, timed steps, --dump-outputs, one JSON line); the side measurements,
CPU baselines, Node.js leg and parity gates run only with --full."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

FULL_ONLY = ("ops", "cpu_baseline", "parity", "gates", "pmc", "scale", "roofline_svd", "valid")


def _parse(monkeypatch, argv):
    sys.path.insert(0, ROOT)
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py"] + argv)
    return bench.parse()


def test_full_is_off_by_default(monkeypatch):
    args = _parse(monkeypatch, ["--gpus", "1", "--steps", "3", "--warmup", "1"])
    assert args.full is False and args.no_ops is False and args.no_cpu_baseline is False


def test_full_and_its_narrowing_options(monkeypatch):
    args = _parse(monkeypatch, ["--full", "--no-ops", "--no-cpu-baseline"])
    assert args.full is True and args.no_ops is True and args.no_cpu_baseline is True


@pytest.mark.gpu
def test_plain_run_prints_only_the_headline(tmp_path):
    d = tmp_path / "out"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--dump-outputs", str(d)],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["metric"] == "fp64 GFLOP/s: matmul N=4096 & SVD N=2048; % of MFMA/HBM peak"
    assert out["unit"] == "GFLOP/s" and out["higher_is_better"] is True and out["dtype"] == "f64"
    assert out["steps"] == 2 and out["warmup"] == 1 and out["n_gpus"] == 1
    assert out["value"] > 0 and out["ms_per_step"] > 0
    assert abs(out["value"] - 2.0 * 4096 ** 3 / (out["ms_per_step"] * 1e-3) / 1e9) <= 0.01 * out["value"]
    assert out["roofline"]["kernel_ms"] > 0
    assert not [k for k in FULL_ONLY if k in out]
    c = np.load(d / "C_sample.npy")
    assert c.dtype == np.float64 and c.shape == (1 << 22,) and np.isfinite(c).all()
