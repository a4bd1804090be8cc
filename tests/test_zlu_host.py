"""zlu_decomp / zlu_solve / zsolve without a GPU: the model of tests/zlu_common.py inside its bounds and against numpy.linalg.solve, the
pivot margins, the argument rows of both forms of the C ABI, exports and build list, the argument and dtype errors of la and dev."""
import re

import numpy as np
import pytest

import zlu_common as Z
from nd4js_amd import _lib, la

NEW = ["nd4hip_zgetrf_batched", "nd4hip_zgetrs_batched", "nd4hip_zgesv_batched"]
NAMES = [str(n) for n in Z.SIZES + Z.PANEL_SIZES] + [Z.name_of(s) for s in Z.BATCHES]


@pytest.mark.parametrize("name", NAMES)
def test_model_inside_the_bounds_with_wide_pivot_margins(name):
    A, LU, P, margin = Z.catalogue(name)
    assert margin >= Z.MARGIN
    Y = Z.cmatrix(99, *(A.shape[:-1] + (3,)))
    X = Z.solve_model(LU, P, Y).reshape(Y.shape)
    s1, s3, s2 = Z.shares(A, LU, P, X, Y)
    print("%s: model shares of the bounds 1, 2, 3: %.2e %.2e %.2e, margin %.2e" % (name, s1, s2, s3, margin))
    assert s1 <= 1.0 and s2 <= 1.0 and s3 <= 1.0
    if A.shape[-1] <= 300 and A.ndim == 2:
        ref = np.linalg.solve(A, Y)
        assert np.linalg.norm(X - ref) <= 1e-9 * np.linalg.norm(ref)    # two backward-stable solves of one well-conditioned system


def test_both_forms_refuse_alike_before_the_handle():
    lib = _lib.load()
    for op in {r[0] for r in Z.ROWS}:
        assert {"extent", "limit", "empty", "null", "handle"} <= {r[1] for r in Z.ROWS if r[0] == op}
    for op, what, args, text in Z.ROWS:
        for form in ("_host", "_dev"):
            rc = getattr(lib, "nd4hip_" + op + form)(None, *args)
            assert (rc, lib.nd4hip_last_error().decode()) == (-1, text) if text else rc == 0, (op, what, form)


def test_exports_bindings_and_build_list():
    lib = _lib.load()
    for name in [b + f for b in NEW for f in ("_host", "_dev")]:
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    from nd4js_amd import build
    assert "zgetrf.hip" in build.HIP_SOURCES and build.FILE_FLAGS["zgetrf.hip"] == ["-ffp-contract=off"]


@pytest.fixture
def recorder(monkeypatch):
    """the library must not be reached"""
    monkeypatch.setattr(la._lib, "handle", lambda device=None: pytest.fail("the library was reached"))


def test_an_empty_call_reaches_nothing(recorder):
    c = np.complex128
    info = {}
    LU, P = la.zlu_decomp(np.zeros((0, 3, 3), dtype=c), info=info)
    assert LU.shape == (0, 3, 3) and P.shape == (0, 3) and info["singular"].shape == (0,)
    assert la.zlu_decomp(np.zeros((2, 0, 0), dtype=c))[1].shape == (2, 0)
    assert la.zlu_solve(np.zeros((3, 3), dtype=c), np.zeros(3, dtype=np.int32), np.zeros((3, 0), dtype=c)).shape == (3, 0)
    assert la.zlu_solve(np.zeros((0, 3, 3), dtype=c), np.zeros((0, 3), dtype=np.int32), np.zeros((3, 2))).shape == (0, 3, 2)
    assert la.zsolve(np.zeros((3, 3), dtype=c), np.zeros((0, 3, 2), dtype=c)).shape == (0, 3, 2)


def test_argument_errors(recorder):
    c = np.complex128
    A, P, Y = np.eye(4, dtype=c), np.arange(4, dtype=np.int32), np.zeros((4, 2), dtype=c)
    for fn, real_fn in ((lambda a: la.zlu_decomp(a), "lu_decomp"), (lambda a: la.zlu_solve(a, P, Y), "lu_solve"), (lambda a: la.zsolve(a, Y), r"\bsolve")):
        for bad in (np.eye(4), np.eye(4, dtype=np.int32)):
            with pytest.raises(TypeError, match=real_fn):
                fn(bad)
        with pytest.raises(TypeError, match="only complex128 runs on the GPU path"):
            fn(np.eye(4, dtype=np.complex64))
    for fn in (lambda y: la.zlu_solve(A, P, y), lambda y: la.zsolve(A, y)):
        for bad in (Y.astype(np.complex64), np.zeros((4, 2), dtype=np.int32)):
            with pytest.raises(TypeError, match="Y must be complex128 or float64"):
                fn(bad)
    for fn in (la.zlu_decomp, lambda a: la.zsolve(a, Y)):
        for bad, text in ((np.ones((4, 3), dtype=c), "quadratic"), (np.ones(4, dtype=c), "at least 2"), (np.zeros((2049, 2049), dtype=c), "N <= 2048")):
            with pytest.raises(ValueError, match=text):
                fn(bad)
    for args, text in (((np.ones(4, dtype=c), P, Y), "LU must be at least 2D."),
                       ((A, P, Y[:, 0]), "y must be at least 2D."), ((np.ones((4, 3), dtype=c), P, Y), "Last two dimensions of LU must be quadratic."),
                       ((A, P, np.zeros((5, 2), dtype=c)), "LU and y don't match."), ((A, P[:3], Y), "LU and P don't match."),
                       ((np.zeros((2, 4, 4), dtype=c), P, np.zeros((3, 4, 2), dtype=c)), "LU and y are not broadcast-compatible."),
                       ((A, np.zeros((3, 4), dtype=np.int32), np.zeros((2, 4, 2), dtype=c)), "P is not broadcast-compatible.")):
        with pytest.raises(ValueError, match=re.escape(text)):
            la.zlu_solve(*args)
    for bad, text in ((np.zeros((5, 2), dtype=c), "A and Y don't match"), (np.zeros(4, dtype=c), "Y.ndim must be at least 2"),
                      (np.zeros((3, 4, 2), dtype=c), "not broadcast-compatible")):
        with pytest.raises(ValueError, match=text):
            la.zsolve(np.zeros((2, 4, 4), dtype=c), bad)


def test_device_layer_refuses_alike():
    import torch
    from nd4js_amd import dev
    z, r, p = torch.zeros((2, 2), dtype=torch.complex128), torch.zeros((2, 2), dtype=torch.float64), torch.zeros(2, dtype=torch.int32)
    for fn, real_fn in ((dev.zlu_decomp, "lu_decomp"), (lambda a: dev.zlu_solve(a, p, z), "lu_solve"), (lambda a: dev.zsolve(a, z), r"\bsolve")):
        with pytest.raises(TypeError, match=real_fn):
            fn(r)
        with pytest.raises(TypeError, match="only complex128"):
            fn(z.to(torch.complex64))
        with pytest.raises(TypeError, match="CUDA tensor"):
            fn(z)
        with pytest.raises(TypeError, match="CUDA tensor"):
            fn(np.zeros((2, 2), dtype=np.complex128))


def test_the_real_family_still_refuses_complex_input():
    z = np.eye(3, dtype=np.complex128)
    for call in (lambda: la.lu_decomp(z), lambda: la.lu_solve(z, np.arange(3), z), lambda: la.solve(z, z), lambda: la.tril_solve(z, z),
                 lambda: la.triu_solve(z, z)):
        with pytest.raises(TypeError, match="complex"):
            call()
