"""bench.py --dump-outputs and --steps, checked on CPU: what dump_outputs writes for a product that fits the bound (all of C) and for
one that does not (a fixed sample, the same from run to run), and that --steps below 1 or a negative --warmup is refused."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT


def _bench():
    sys.path.insert(0, ROOT)
    import bench
    return bench


def test_dump_whole_product(tmp_path):
    bench = _bench()
    c = torch.from_numpy(np.random.default_rng(1).standard_normal((48, 40)))
    d = tmp_path / "out"
    bench.dump_outputs(str(d), c)
    got = np.load(d / "C.npy")
    assert got.dtype == np.float64 and np.array_equal(got, c.numpy())
    assert (d / ".gitignore").read_text() == "*\n"


def test_dump_fixed_sample(tmp_path, monkeypatch):
    bench = _bench()
    monkeypatch.setattr(bench, "DUMP_MAX_ENTRIES", 100)
    c = torch.from_numpy(np.random.default_rng(2).standard_normal((32, 32)))
    for run in ("a", "b"):
        bench.dump_outputs(str(tmp_path / run), c)
    a, b = np.load(tmp_path / "a" / "C_sample.npy"), np.load(tmp_path / "b" / "C_sample.npy")
    idx = np.sort(np.random.default_rng(0).choice(c.numel(), 100, replace=False))
    assert a.dtype == np.float64 and a.shape == (100,) and np.array_equal(a, b) and np.array_equal(a, c.numpy().reshape(-1)[idx])
    assert not os.path.exists(tmp_path / "a" / "C.npy")


@pytest.mark.parametrize("argv", [["--steps", "0"], ["--warmup", "-1"]])
def test_bad_step_counts_refused(monkeypatch, argv):
    bench = _bench()
    monkeypatch.setattr(sys, "argv", ["bench.py"] + argv)
    with pytest.raises(SystemExit):
        bench.parse()
