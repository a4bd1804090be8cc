"""eigen_sym_gen / eigenvals_sym_gen through the JS host and the N-API addon: tests/js/node_sygv_checks.js. The single-member
catalogue cases of tests/sygv_common.py up to N = 130 with their committed LAPACK values, handed over as a JSON file.
Skipped where node or the addon is missing; the install check also needs the reference bundle."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import sygv_common as G
from conftest import ROOT

NODE = shutil.which("node")
ADDON = os.path.join(ROOT, "nd4js_amd", "js", "nd4hip_napi.node")
SCRIPT = os.path.join(ROOT, "tests", "js", "node_sygv_checks.js")
needs_node = pytest.mark.skipif(NODE is None or not os.path.exists(ADDON), reason="node or the N-API addon not available")


def run(*args):
    r = subprocess.run([NODE, SCRIPT] + list(args), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout
    return r.stdout


def _reference_bundle():
    if os.environ.get("ND4_REFERENCE"):
        return os.environ["ND4_REFERENCE"]
    with open(os.path.join(ROOT, "BASELINE.json")) as f:
        return os.path.join(json.load(f)["reference_path"], "dist", "nd.js")


REF_BUNDLE = _reference_bundle()


@needs_node
def test_js_names_and_argument_errors():
    assert "node sygv cpu checks ok" in run("cpu")


@needs_node
@pytest.mark.skipif(not os.path.exists(REF_BUNDLE), reason="the reference bundle is not here")
def test_install_adds_the_names_and_keeps_the_keys():
    assert "node sygv install checks ok" in run("install", REF_BUNDLE)


@needs_node
@pytest.mark.gpu
def test_js_fixtures_on_gpu(tmp_path):
    cases = {}
    for name in G.NAMES:
        A, B = G.inputs(name)
        if A.ndim != 2 or A.shape[-1] > 130:
            continue
        sv = np.linalg.svd(B, compute_uv=False)
        cases[name] = {"N": A.shape[-1], "A": A.ravel().tolist(), "B": B.ravel().tolist(), "ref": G.golden(name).tolist(),
                       "fro_A": float(np.linalg.norm(A)), "sigma_min": float(sv[-1]), "kappa": float(sv[0] / sv[-1])}
    f = tmp_path / "sygv_cases.json"
    f.write_text(json.dumps(cases))
    assert "node sygv gpu checks ok %d" % len(cases) in run("gpu", str(f))
