"""eigen_sym / eigenvals_sym with opts.subset through the JS host and the N-API addon: tests/js/node_eigsym_subset_checks.js.
The GPU part hands the inputs and the Python result (la.eigen_sym(S, subset=...)) over as a JSON file: the JS side returns its bits
from host arrays and from DeviceNDArrays. Skipped where node or the addon is missing."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import eigsym_common as C
from conftest import ROOT

NODE = shutil.which("node")
ADDON = os.path.join(ROOT, "nd4js_amd", "js", "nd4hip_napi.node")
SCRIPT = os.path.join(ROOT, "tests", "js", "node_eigsym_subset_checks.js")
needs_node = pytest.mark.skipif(NODE is None or not os.path.exists(ADDON), reason="node or the N-API addon not available")


def run(*args):
    r = subprocess.run([NODE, SCRIPT] + list(args), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout
    return r.stdout


@needs_node
def test_js_subset_argument_errors():
    assert "node eigsym subset cpu checks ok" in run("cpu")


@needs_node
@pytest.mark.gpu
def test_js_subset_on_gpu(tmp_path):
    from nd4js_amd import la
    cases = {}
    for name, sub in (("dense_33", (0, 1)), ("dense_33", (32, 33)), ("dense_70", (0, 8)), ("dense_3", (0, 3)), ("batch_5x40", (10, 14)),
                      ("identity_8", (2, 5)), ("dense_1", (0, 1))):
        S = C.reference(name)[0]
        lam, V = la.eigen_sym(S, subset=sub)
        assert np.all(np.isfinite(lam)) and np.all(np.isfinite(V))
        cases["%s_%d_%d" % ((name,) + sub)] = {"shape": list(S.shape), "subset": list(sub), "S": S.ravel().tolist(), "lam": lam.ravel().tolist(),
                                              "V": V.ravel().tolist()}
    f = tmp_path / "eigsym_subset_cases.json"
    f.write_text(json.dumps(cases))
    assert "node eigsym subset gpu checks ok %d" % len(cases) in run("gpu", str(f))
