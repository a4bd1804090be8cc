"""herm_cholesky_decomp / herm_cholesky_solve / eigen_herm_gen / eigenvals_herm_gen through the JS host and the N-API addon:
tests/js/node_hegv_checks.js. The GPU part hands the inputs and the Python results over as a JSON file of interleaved (re, im)
doubles: the JS side returns their bits from host arrays and from DeviceNDArrays. Skipped where node or the addon is missing."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import hegv_common as G
from conftest import ROOT

NODE = shutil.which("node")
ADDON = os.path.join(ROOT, "nd4js_amd", "js", "nd4hip_napi.node")
SCRIPT = os.path.join(ROOT, "tests", "js", "node_hegv_checks.js")
needs_node = pytest.mark.skipif(NODE is None or not os.path.exists(ADDON), reason="node or the N-API addon not available")


def run(*args):
    r = subprocess.run([NODE, SCRIPT] + list(args), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout
    return r.stdout


def pairs(z):
    """complex128 as the list of its interleaved doubles"""
    return np.ascontiguousarray(z, dtype=np.complex128).view(np.float64).ravel().tolist()


@needs_node
def test_js_hegv_names_and_argument_errors():
    assert "node hegv cpu checks ok" in run("cpu")


@needs_node
@pytest.mark.gpu
def test_js_hegv_on_gpu(tmp_path):
    from nd4js_amd import la
    inputs = {"gram_33": ("gram_33", None), "batch_5x40": ("batch_5x40", None), "shared_3x40": ("shared_3x40", None),
              "gram_130_top8": ("gram_130", (0, 8)), "shared_3x40_subset": ("shared_3x40", (10, 14)), "gram_1": ("gram_1", None),
              "gram_1_subset": ("gram_1", (0, 1))}
    cases = {}
    for name, (cat, sub) in inputs.items():
        A, B = G.inputs(cat)
        lam, Xv = la.eigen_herm_gen(A, B, subset=sub)
        assert np.all(np.isfinite(lam)) and np.all(np.isfinite(Xv))
        L = la.herm_cholesky_decomp(B)
        N = A.shape[-1]
        Y = G.cmatrix(G.SEED + 9500 + N, int(np.prod(B.shape[:-2], dtype=np.int64)) * N, 3).reshape(B.shape[:-1] + (3,))
        case = {"shape": list(A.shape), "shapeB": list(B.shape), "shapeY": list(Y.shape), "A": pairs(A), "B": pairs(B), "lam": lam.ravel().tolist(),
                "X": pairs(Xv), "L": pairs(L), "Y": pairs(Y), "S": pairs(la.herm_cholesky_solve(L, Y))}
        if name == "gram_33":
            case["Yreal"] = np.ascontiguousarray(Y.real).ravel().tolist()
            case["Sreal"] = pairs(la.herm_cholesky_solve(L, np.ascontiguousarray(Y.real)))
        if sub is not None:
            case["subset"] = list(sub)
        cases[name] = case
    f = tmp_path / "hegv_cases.json"
    f.write_text(json.dumps(cases))
    assert "node hegv gpu checks ok %d" % len(cases) in run("gpu", str(f))
