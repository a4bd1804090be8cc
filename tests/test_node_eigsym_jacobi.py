"""eigen_sym / eigenvals_sym with {algo: 'jacobi'} through the JS host and the N-API addon: tests/js/node_eigsym_jacobi_checks.js.
The inputs and the numpy model's results (tests/eigsym_jacobi_common.py) are handed over as bit patterns in a JSON file; node has
to return the same bits from host arrays and from DeviceNDArrays. Skipped where node or the addon is missing."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import eigsym_jacobi_common as J
from conftest import ROOT

NODE = shutil.which("node")
ADDON = os.path.join(ROOT, "nd4js_amd", "js", "nd4hip_napi.node")
SCRIPT = os.path.join(ROOT, "tests", "js", "node_eigsym_jacobi_checks.js")
needs_node = pytest.mark.skipif(NODE is None or not os.path.exists(ADDON), reason="node or the N-API addon not available")
# one input per tier, an odd size, a batch with a partial workgroup and a graded positive definite matrix
CASES = ("dense_5", "dense_33", "dense_65", "mixed_7x8", "diag_ties_6", "graded_pd_24")


def run(*args):
    r = subprocess.run([NODE, SCRIPT] + list(args), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout
    return r.stdout


def _hex(a):
    return np.ascontiguousarray(a, dtype="<f8").tobytes().hex()


@needs_node
def test_js_option_errors():
    assert "node eigsym jacobi cpu checks ok" in run("cpu")


@needs_node
@pytest.mark.gpu
def test_js_has_the_models_bits_on_gpu(tmp_path):
    cases = {}
    for name in CASES:
        S, lam, V, _ = J.case(name)
        cases[name] = {"shape": list(S.shape), "S": _hex(S), "lam": _hex(lam), "V": _hex(V)}
    f = tmp_path / "eigsym_jacobi_cases.json"
    f.write_text(json.dumps(cases))
    assert "node eigsym jacobi gpu checks ok %d" % len(cases) in run("gpu", str(f))
