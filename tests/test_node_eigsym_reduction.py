"""eigen_sym / eigenvals_sym with opts.reduction through the JS host and the N-API addon: tests/js/node_eigsym_reduction_checks.js.
The GPU part hands the inputs and the Python result (la.eigen_sym(S, reduction='tridiag'), with and without a subset) over as a JSON
file: the JS side returns its bits from host arrays and from DeviceNDArrays. Skipped where node or the addon is missing."""
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
SCRIPT = os.path.join(ROOT, "tests", "js", "node_eigsym_reduction_checks.js")
needs_node = pytest.mark.skipif(NODE is None or not os.path.exists(ADDON), reason="node or the N-API addon not available")


def run(*args):
    r = subprocess.run([NODE, SCRIPT] + list(args), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout
    return r.stdout


@needs_node
def test_js_reduction_argument_errors():
    assert "node eigsym reduction cpu checks ok" in run("cpu")


@needs_node
@pytest.mark.gpu
def test_js_reduction_on_gpu(tmp_path):
    from nd4js_amd import la
    cases = {}
    for name, sub in (("dense_33", None), ("dense_70", (0, 8)), ("dense_3", None), ("batch_5x40", (10, 14)), ("batch_2x130", None),
                      ("identity_8", (2, 5)), ("dense_1", None)):
        S = C.reference(name)[0]
        kw = {} if sub is None else {"subset": sub}
        lam, V = la.eigen_sym(S, reduction="tridiag", **kw)
        assert np.all(np.isfinite(lam)) and np.all(np.isfinite(V))
        case = {"shape": list(S.shape), "S": S.ravel().tolist(), "lam": lam.ravel().tolist(), "V": V.ravel().tolist()}
        if sub is None:
            case["lam0"] = la.eigenvals_sym(S).ravel().tolist()
        else:
            case["subset"] = list(sub)
        cases[name] = case
    f = tmp_path / "eigsym_reduction_cases.json"
    f.write_text(json.dumps(cases))
    assert "node eigsym reduction gpu checks ok %d" % len(cases) in run("gpu", str(f))
