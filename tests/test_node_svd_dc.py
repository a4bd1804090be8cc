"""svd_decomp(A, {algo: 'dc'}) through the JS host and the N-API addon: tests/js/node_svd_dc_checks.js. The small cases of
tests/svd_dc_common.py with oracle.svd_dc's singular values, handed over as a JSON file. Skipped where node or the addon is missing."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import svd_dc_common as C
from conftest import ROOT

NODE = shutil.which("node")
ADDON = os.path.join(ROOT, "nd4js_amd", "js", "nd4hip_napi.node")
SCRIPT = os.path.join(ROOT, "tests", "js", "node_svd_dc_checks.js")
needs_node = pytest.mark.skipif(NODE is None or not os.path.exists(ADDON), reason="node or the N-API addon not available")
SMALL = ("sq_1", "sq_2", "sq_3", "sq_4", "sq_5", "sq_9", "sq_17", "sq_33", "sq_65", "wide_5x9", "tall_70x33", "batch_3x2x9x9",
         "scaled_1e+150", "rank2_16", "hilbert_12")


def run(*args):
    r = subprocess.run([NODE, SCRIPT] + list(args), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout
    return r.stdout


@needs_node
def test_js_svd_dc_validation():
    assert "node svd_dc cpu checks ok" in run("cpu")


@needs_node
@pytest.mark.gpu
def test_js_svd_dc_against_the_oracle_on_gpu(tmp_path):
    cases = {}
    for name in SMALL:
        a, _, sv, _ = C.dense_reference(name)
        cases[name] = {"shape": list(a.shape), "A": np.asarray(a).ravel().tolist(), "sv": sv.ravel().tolist()}
    f = tmp_path / "svd_dc_cases.json"
    f.write_text(json.dumps(cases))
    assert "node svd_dc gpu checks ok %d" % len(SMALL) in run("gpu", str(f))
