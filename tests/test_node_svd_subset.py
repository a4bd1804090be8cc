"""The selected singular triplets through the JS host and the N-API addon: tests/js/node_svd_subset_checks.js. The GPU part hands the
inputs and the Python results (la.svd_decomp(A, subset=...), la.bidiag_svd(d, e, subset=...)) over as a JSON file: the JS side
returns their bits from host arrays and from DeviceNDArrays. Skipped where node or the addon is missing."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import svd_dc_common as D
import svd_subset_common as C
from conftest import ROOT

NODE = shutil.which("node")
ADDON = os.path.join(ROOT, "nd4js_amd", "js", "nd4hip_napi.node")
SCRIPT = os.path.join(ROOT, "tests", "js", "node_svd_subset_checks.js")
needs_node = pytest.mark.skipif(NODE is None or not os.path.exists(ADDON), reason="node or the N-API addon not available")


def run(*args):
    r = subprocess.run([NODE, SCRIPT] + list(args), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout
    return r.stdout


@needs_node
def test_js_svd_subset_argument_errors():
    assert "node svd subset cpu checks ok" in run("cpu")


@needs_node
@pytest.mark.gpu
def test_js_svd_subset_on_gpu(tmp_path):
    from nd4js_amd import la
    dense, bidiag = {}, {}
    for name, sub in (("sq_33", (0, 1)), ("sq_33", (30, 33)), ("wide_33x130", (0, 8)), ("tall_70x33", (0, 33)), ("batch_3x2x9x9", (2, 6)), ("sq_1", (0, 1))):
        A = D.DENSE_CASES[name]
        U, sv, V = la.svd_decomp(A, subset=sub)
        assert all(np.all(np.isfinite(x)) for x in (U, sv, V))
        dense["%s_%d_%d" % ((name,) + sub)] = {"shape": list(A.shape), "subset": list(sub), "A": A.ravel().tolist(), "U": U.ravel().tolist(),
                                                "sv": sv.ravel().tolist(), "V": V.ravel().tolist(), "all": la.svd_vals(A).ravel().tolist()}
    for name, sub in (("rand_33_34", (0, 8)), ("rand_64_64", (56, 64)), ("graded_40", (19, 22)), ("zero_8", (3, 6)), ("rand_2_2", (0, 2))):
        d, e = C.case_input(name)
        U2, sv, V2 = la.bidiag_svd(d, e, subset=sub)
        bidiag["%s_%d_%d" % ((name,) + sub)] = {"subset": list(sub), "d": d.tolist(), "e": e.tolist(), "U2": U2.ravel().tolist(), "sv": sv.tolist(),
                                                 "V2": V2.ravel().tolist(), "all": la.bidiag_svdvals(d, e).tolist()}
    f = tmp_path / "svd_subset_cases.json"
    f.write_text(json.dumps({"dense": dense, "bidiag": bidiag}))
    assert "node svd subset gpu checks ok %d" % (len(dense) + len(bidiag)) in run("gpu", str(f))
