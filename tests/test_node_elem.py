"""la.zip_elems, DeviceNDArray.mapElems and DeviceNDArray.reduceElems through the JS host and the N-API addon:
tests/js/node_elem_checks.js. Skipped where node or the addon is missing; the install check also needs the reference bundle, the
GPU check uses it where it is present."""
import json
import os
import shutil
import subprocess

import pytest

from conftest import GOLDEN, ROOT

NODE = shutil.which("node")
ADDON = os.path.join(ROOT, "nd4js_amd", "js", "nd4hip_napi.node")
SCRIPT = os.path.join(ROOT, "tests", "js", "node_elem_checks.js")
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
def test_js_planners_and_closures_reproduce_the_fixtures_and_refusals():
    assert "node elem cpu checks ok" in run("cpu", GOLDEN)


@needs_node
@pytest.mark.skipif(not os.path.exists(REF_BUNDLE), reason="the reference bundle is not here")
def test_install_adds_zip_elems_and_leaves_the_host_modules():
    assert "node elem install checks ok" in run("install", REF_BUNDLE)


@needs_node
@pytest.mark.gpu
def test_js_elementwise_against_golden_and_the_host_module_on_gpu():
    assert "node elem gpu checks ok" in run("gpu", GOLDEN, REF_BUNDLE)
