"""eigen_herm / eigenvals_herm through the JS host and the N-API addon: tests/js/node_herm_checks.js. The GPU part hands the inputs and
the Python result (la.eigen_herm(H), with and without a subset) over as a JSON file of interleaved (re, im) doubles: the JS side
returns its bits from host arrays and from DeviceNDArrays. Skipped where node or the addon is missing."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import herm_common as X
from conftest import ROOT

NODE = shutil.which("node")
ADDON = os.path.join(ROOT, "nd4js_amd", "js", "nd4hip_napi.node")
SCRIPT = os.path.join(ROOT, "tests", "js", "node_herm_checks.js")
needs_node = pytest.mark.skipif(NODE is None or not os.path.exists(ADDON), reason="node or the N-API addon not available")


def run(*args):
    r = subprocess.run([NODE, SCRIPT] + list(args), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout
    return r.stdout


def pairs(z):
    """complex128 as the list of its interleaved doubles"""
    return np.ascontiguousarray(z, dtype=np.complex128).view(np.float64).ravel().tolist()


@needs_node
def test_js_herm_argument_errors():
    assert "node herm cpu checks ok" in run("cpu")


@needs_node
@pytest.mark.gpu
def test_js_herm_on_gpu(tmp_path):
    from nd4js_amd import la
    inputs = {"dense_33": (np.array(X.dense(33)[0]), None), "batch_5x40": (X.batch_5x40(), None), "dense_130_top8": (np.array(X.dense(130)[0]), (0, 8)),
              "batch_5x40_subset": (X.batch_5x40(), (10, 14)), "dense_1": (np.array(X.dense(1)[0]), None), "dense_1_subset": (np.array(X.dense(1)[0]), (0, 1))}
    cases = {}
    for name, (H, sub) in inputs.items():
        lam, V = la.eigen_herm(H, subset=sub)
        assert np.all(np.isfinite(lam)) and np.all(np.isfinite(V))
        case = {"shape": list(H.shape), "H": pairs(H), "lam": lam.ravel().tolist(), "V": pairs(V)}
        if sub is not None:
            case["subset"] = list(sub)
        cases[name] = case
    f = tmp_path / "herm_cases.json"
    f.write_text(json.dumps(cases))
    assert "node herm gpu checks ok %d" % len(cases) in run("gpu", str(f))
