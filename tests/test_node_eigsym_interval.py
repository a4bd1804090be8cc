"""opts.interval on eigen_sym / eigenvals_sym, opts.subset / opts.interval / opts.reduction on eigen_sym_gen / eigenvals_sym_gen and the JS
tridiag_eigen / tridiag_eigenvals / tridiag_count through the JS host and the N-API addon: tests/js/node_eigsym_interval_checks.js.
The GPU part hands the inputs and the Python results over as a JSON file (arrays as base64 of their bytes: the ragged results hold
NaN): the JS side returns their bits from host arrays and from DeviceNDArrays. Skipped where node or the addon is missing."""
import base64
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import eigsym_common as C
import eigsym_subset_common as X
import sygv_common as G
from conftest import ROOT

NODE = shutil.which("node")
ADDON = os.path.join(ROOT, "nd4js_amd", "js", "nd4hip_napi.node")
SCRIPT = os.path.join(ROOT, "tests", "js", "node_eigsym_interval_checks.js")
needs_node = pytest.mark.skipif(NODE is None or not os.path.exists(ADDON), reason="node or the N-API addon not available")


def run(*args):
    r = subprocess.run([NODE, SCRIPT] + list(args), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout
    return r.stdout


def _b64(a, dtype=np.float64):
    return base64.b64encode(np.ascontiguousarray(a, dtype=dtype).tobytes()).decode()


def _operand(a):
    return None if a is None else {"shape": list(a.shape), "data": _b64(a)}


def _side(x):
    """a bound for the JS side: a number, 'inf' / '-inf', or the base64 of one value per member"""
    if np.ndim(x):
        return _b64(np.ravel(x))
    return "inf" if x == np.inf else "-inf" if x == -np.inf else float(x)


def _case(fn, operands, result, vectors, opts=None, interval=None, info=None):
    lam, V = result if vectors else (result, None)
    c = {"fn": fn, "operands": [_operand(o) for o in operands], "opts": opts or {}, "lam": _b64(lam), "lam_shape": list(lam.shape)}
    if vectors:
        c["V"], c["V_shape"] = _b64(V), list(V.shape)
    if interval is not None:
        c["interval"] = [_side(interval[0]), _side(interval[1])]
        c["range"], c["range_shape"] = _b64(info["range"], np.int32), list(info["range"].shape)
    return c


@needs_node
def test_js_interval_argument_errors():
    assert "node eigsym interval cpu checks ok" in run("cpu")


@needs_node
@pytest.mark.gpu
def test_js_interval_on_gpu(tmp_path):
    from nd4js_amd import la
    cases = {}
    # eigen_sym / eigenvals_sym with opts.interval, both reductions, one matrix and a ragged batch
    for name, iv in (("dense_33", (0.0, np.inf)), ("dense_70", (-0.5, 0.5)), ("dense_3", (-np.inf, np.inf)), ("identity_8", (0.5, 1.0)),
                     ("batch_5x40", (np.array([0.0, 1.0, -1.0, 2.5, -9.0]), np.array([np.inf, 2.0, 0.0, 3.0, 9.0])))):
        S = C.reference(name)[0]
        for red in (None, "tridiag"):
            info, opts = {}, ({} if red is None else {"reduction": red})
            cases["sym_%s_%s" % (name, red)] = _case("eigen_sym", [S], la.eigen_sym(S, interval=iv, reduction=red, info=info), True, opts, iv, info)
            cases["symvals_%s_%s" % (name, red)] = _case("eigenvals_sym", [S], la.eigenvals_sym(S, interval=iv, reduction=red, info=info), False, opts, iv, info)
    # eigen_sym_gen with each keyword, one B and one B per member
    for name in ("gram_33", "gram_65", "shared_3x40", "batch_5x40"):
        A, B = G.inputs(name)
        N = A.shape[-1]
        for tag, kw in (("sub", {"subset": (0, 3)}), ("subtr", {"subset": (N - 3, N), "reduction": "tridiag"}), ("tr", {"reduction": "tridiag"})):
            opts = {k: (list(v) if k == "subset" else v) for k, v in kw.items()}
            cases["gen_%s_%s" % (name, tag)] = _case("eigen_sym_gen", [A, B], la.eigen_sym_gen(A, B, **kw), True, opts)
            cases["genvals_%s_%s" % (name, tag)] = _case("eigenvals_sym_gen", [A, B], la.eigenvals_sym_gen(A, B, **kw), False, opts)
        for red in (None, "tridiag"):
            info, iv, opts = {}, (0.0, np.inf), ({} if red is None else {"reduction": red})
            cases["gen_%s_iv_%s" % (name, red)] = _case("eigen_sym_gen", [A, B], la.eigen_sym_gen(A, B, interval=iv, reduction=red, info=info), True, opts, iv, info)
            cases["genvals_%s_iv_%s" % (name, red)] = _case("eigenvals_sym_gen", [A, B], la.eigenvals_sym_gen(A, B, interval=iv, reduction=red, info=info), False,
                                                          opts, iv, info)
    # the tridiagonal functions: all, a subset, an interval; N = 1 has no e; a batch
    for name in ("dense_50", "w21", "glued_w21", "diag_ties_zero"):
        d, e = (np.array(a) for a in X.tridiag_input(name))
        N = len(d)
        cases["tri_%s_all" % name] = _case("tridiag_eigen", [d, e], la.tridiag_eigen(d, e), True)
        cases["tri_%s_sub" % name] = _case("tridiag_eigen", [d, e], la.tridiag_eigen(d, e, subset=(1, 4)), True, {"subset": [1, 4]})
        cases["trivals_%s_sub" % name] = _case("tridiag_eigenvals", [d, e], la.tridiag_eigenvals(d, e, subset=(N - 2, N)), False, {"subset": [N - 2, N]})
        info, iv = {}, (float(np.median(d)), np.inf)
        cases["tri_%s_iv" % name] = _case("tridiag_eigen", [d, e], la.tridiag_eigen(d, e, interval=iv, info=info), True, None, iv, info)
        cases["trivals_%s_iv" % name] = _case("tridiag_eigenvals", [d, e], la.tridiag_eigenvals(d, e, interval=iv, info=info), False, None, iv, info)
        x = np.linspace(d.min() - 1.0, d.max() + 1.0, 7)
        cases["count_%s" % name] = {"fn": "tridiag_count", "operands": [_operand(d), _operand(e), _operand(x)], "count": _b64(la.tridiag_count(d, e, x), np.int32)}
    d1 = np.array([[-2.5], [0.0], [7.0]])
    info, iv = {}, (-3.0, 0.0)
    cases["tri_n1_iv"] = _case("tridiag_eigen", [d1, None], la.tridiag_eigen(d1, np.zeros((3, 0)), interval=iv, info=info), True, None, iv, info)
    cases["tri_n1_all"] = _case("tridiag_eigenvals", [d1, None], la.tridiag_eigenvals(d1, np.zeros((3, 0))), False)
    S = C.reference("batch_5x40")[0]
    db, eb = np.ascontiguousarray(S[:, 0]), np.ascontiguousarray(S[:, 1, :39])
    info, iv = {}, (np.array([0.0, 5.0, -9.0, 0.3, -0.2]), np.array([np.inf, 6.0, 9.0, 0.6, 0.2]))
    cases["tri_batch_iv"] = _case("tridiag_eigen", [db, eb], la.tridiag_eigen(db, eb, interval=iv, info=info), True, None, iv, info)
    assert 0 in (info["range"][:, 1] - info["range"][:, 0]) and np.isnan(la.tridiag_eigenvals(db, eb, interval=iv)).any()   # ragged, with an empty member
    f = tmp_path / "eigsym_interval_cases.json"
    f.write_text(json.dumps(cases))
    assert "node eigsym interval gpu checks ok %d" % len(cases) in run("gpu", str(f))
