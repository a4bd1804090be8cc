"""eigen_sym / eigenvals_sym through the JS host and the N-API addon: tests/js/node_eigsym_checks.js. The fixtures of
tests/golden/eigsym with their reference values (LAPACK's where the reference's were not kept), handed over as a JSON file.
Skipped where node or the addon is missing; the install check also needs the reference bundle."""
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
SCRIPT = os.path.join(ROOT, "tests", "js", "node_eigsym_checks.js")
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
    assert "node eigsym cpu checks ok" in run("cpu")


@needs_node
@pytest.mark.skipif(not os.path.exists(REF_BUNDLE), reason="the reference bundle is not here")
def test_install_adds_the_names_and_keeps_the_keys():
    assert "node eigsym install checks ok" in run("install", REF_BUNDLE)


@needs_node
@pytest.mark.gpu
def test_js_fixtures_on_gpu(tmp_path):
    cases = {}
    for name, meta in C.golden_manifest()["cases"].items():
        S = C.golden_input(name, meta)
        want = C.golden_values(name, meta)
        ref = np.sort(want.real)[::-1] if want is not None else np.linalg.eigvalsh(S)[::-1]
        cases[name] = {"N": meta["N"], "S": S.ravel().tolist(), "ref": ref.tolist()}
    f = tmp_path / "eigsym_cases.json"
    f.write_text(json.dumps(cases))
    assert "node eigsym gpu checks ok %d" % len(cases) in run("gpu", str(f))
