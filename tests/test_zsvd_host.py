"""zbidiag_factor / zbidiag_apply_p / zsvd_decomp / zsvd_vals without a GPU: the argument rows of both forms of the C ABI, header,
exports and bindings, the argument and dtype errors of la and dev."""
import os
import re

import numpy as np
import pytest

from nd4js_amd import _lib, la

OPS = ("zgebrd_batched", "zunmbr_p_batched", "zgesdd_batched")
B = 16           # any non-NULL pointer value
SHAPE, NULL = "the shape must satisfy N <= M <= 2048", "NULL pointer"
ROWS = [  # (operation, the arguments after the handle, the error text after the operation's name or None for an empty call)
    ("zgebrd_batched", (-1, 4, 3, B, B, B, B, B, B), "negative extent"), ("zgebrd_batched", (1, 2049, 3, B, B, B, B, B, B), SHAPE),
    ("zgebrd_batched", (1, 3, 4, B, B, B, B, B, B), SHAPE), ("zgebrd_batched", (0, 4, 3, B, B, B, B, B, B), None),
    ("zgebrd_batched", (1, 4, 3, B, B, B, None, B, B), NULL), ("zgebrd_batched", (1, 4, 3, B, B, B, B, B, None), NULL),
    ("zgebrd_batched", (1, 4, 1, B, B, B, B, B, None), "NULL handle"), ("zgebrd_batched", (1, 4, 3, B, B, B, B, B, B), "NULL handle"),
    ("zunmbr_p_batched", (1, 4, 3, -2, 0, B, 12, B, 3, B), "negative extent"), ("zunmbr_p_batched", (1, 2049, 3, 2, 0, B, 6147, B, 3, B), SHAPE),
    ("zunmbr_p_batched", (1, 3, 4, 2, 0, B, 12, B, 4, B), SHAPE), ("zunmbr_p_batched", (1, 4, 3, 0, 0, B, 12, B, 3, B), None),
    ("zunmbr_p_batched", (1, 4, 3, 2, 0, B, 12, None, 3, B), NULL), ("zunmbr_p_batched", (1, 4, 3, 2, 1, B, 0, B, 0, B), "NULL handle"),
    ("zunmbr_p_batched", (2, 4, 3, 2, 0, B, 12, B, 0, B), "the strides of F and taup must be M*N and N, or both 0"),
    ("zunmbr_p_batched", (2, 4, 3, 2, 2, B, 12, B, 3, B), "adjoint must be 0 or 1"),
    ("zgesdd_batched", (-1, 4, 3, 0, 3, 1, B, B, B, B), "negative extent"), ("zgesdd_batched", (1, 2049, 3, 0, 3, 1, B, B, B, B), "M <= 2048 and N <= 2048"),
    ("zgesdd_batched", (1, 3, 2049, 0, 3, 0, B, None, B, None), "M <= 2048 and N <= 2048"),
    ("zgesdd_batched", (1, 4, 3, 2, 4, 1, B, B, B, B), "subset must satisfy 0 <= i0 <= i1 <= min(M, N)"),
    ("zgesdd_batched", (1, 3, 4, 0, 4, 1, B, B, B, B), "subset must satisfy 0 <= i0 <= i1 <= min(M, N)"),
    ("zgesdd_batched", (1, 4, 3, 1, 1, 1, B, B, B, B), None), ("zgesdd_batched", (0, 4, 3, 0, 3, 1, B, B, B, B), None),
    ("zgesdd_batched", (1, 4, 3, 0, 3, 2, B, B, B, B), "vectors must be 0 or 1"),
    ("zgesdd_batched", (1, 4, 3, 0, 3, 1, B, None, B, B), "NULL pointer, or vectors without the flag"),
    ("zgesdd_batched", (1, 4, 3, 0, 3, 0, B, B, B, B), "NULL pointer, or vectors without the flag"),
    ("zgesdd_batched", (1, 3, 4, 0, 3, 0, B, None, B, None), "NULL handle"), ("zgesdd_batched", (1, 4, 3, 0, 3, 1, B, B, B, B), "NULL handle"),
]


@pytest.mark.parametrize("form", ["_host", "_dev"])
def test_both_forms_refuse_alike_before_the_handle(form):
    lib = _lib.load()
    for op, args, text in ROWS:
        rc = getattr(lib, "nd4hip_" + op + form)(None, *args)
        assert (rc, lib.nd4hip_last_error().decode()) == (-1, "nd4hip_%s: %s" % (op, text)) if text else rc == 0, (op, args)


def test_header_exports_and_bindings_agree():
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "nd4hip.h")).read()
    lib = _lib.load()
    for op in OPS:
        for form in ("_dev", "_host"):
            name = "nd4hip_" + op + form
            proto = re.search(r"int %s\s*\(([^;]*)\);" % name, header)
            assert proto and name in _lib.SIGNATURES and hasattr(lib, name), name
            assert len(proto.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name


@pytest.fixture
def recorder(monkeypatch):
    """the library must not be reached"""
    monkeypatch.setattr(la._lib, "handle", lambda device=None: pytest.fail("the library was reached"))


def test_an_empty_call_reaches_nothing(recorder):
    c = np.complex128
    F, tauq, taup, d, e = la.zbidiag_factor(np.zeros((0, 4, 3), dtype=c))
    assert (F.shape, tauq.shape, taup.shape, d.shape, e.shape) == ((0, 4, 3), (0, 3), (0, 3), (0, 3), (0, 2)) and d.dtype == e.dtype == np.float64
    assert la.zbidiag_apply_p(np.zeros((4, 3), dtype=c), np.zeros(3, dtype=c), np.zeros((3, 0), dtype=c)).shape == (3, 0)
    U, sv, V = la.zsvd_decomp(np.zeros((0, 4, 3), dtype=c))
    assert (U.shape, sv.shape, V.shape) == ((0, 4, 3), (0, 3), (0, 3, 3)) and sv.dtype == np.float64
    U, sv, V = la.zsvd_decomp(np.ones((3, 5), dtype=c), subset=(2, 2))
    assert (U.shape, sv.shape, V.shape) == ((3, 0), (0,), (0, 5)) and la.zsvd_vals(np.ones((2, 3, 5), dtype=c), subset=(1, 1)).shape == (2, 0)


def test_argument_errors(recorder):
    c = np.complex128
    A, taup, Z = np.ones((4, 3), dtype=c), np.zeros(3, dtype=c), np.zeros((3, 2), dtype=c)
    calls = ((la.zbidiag_factor, "bidiag_decomp", True), (lambda a: la.zbidiag_apply_p(a, taup, Z), "bidiag_decomp", True),
             (la.zsvd_decomp, "svd_decomp", False), (la.zsvd_vals, "svd_decomp", False))
    for fn, real_fn, tall in calls:
        with pytest.raises(TypeError, match=real_fn):
            fn(np.ones((4, 3)))
        with pytest.raises(TypeError, match="only complex128 runs on the GPU path"):
            fn(A.astype(np.complex64))
        bad = [(np.ones(4, dtype=c), "at least 2"), (np.zeros((2049, 1), dtype=c), "M <= 2048")]
        bad.append((np.ones((3, 4), dtype=c), "M >= N") if tall else (np.zeros((1, 2049), dtype=c), "N <= 2048"))
        for a, text in bad:
            with pytest.raises(ValueError, match=text):
                fn(a)
    for fn in (la.zsvd_decomp, la.zsvd_vals):
        for subset in ((2, 1), (0, 4), (-1, 2), (0.5, 2), 3):
            with pytest.raises(ValueError, match="subset must be"):
                fn(A, subset=subset)
    with pytest.raises(TypeError, match="complex128 or float64"):
        la.zbidiag_apply_p(A, taup, Z.astype(np.complex64))
    with pytest.raises(TypeError, match="tau.dtype must be complex128"):
        la.zbidiag_apply_p(A, np.zeros(3), Z)
    with pytest.raises(ValueError, match="F and Z don't match"):
        la.zbidiag_apply_p(A, taup, np.zeros((4, 2), dtype=c))
    with pytest.raises(ValueError, match="F and taup don't match"):
        la.zbidiag_apply_p(A, np.zeros(2, dtype=c), Z)
    with pytest.raises(ValueError, match="leading dimensions"):
        la.zbidiag_apply_p(np.ones((2, 4, 3), dtype=c), np.zeros((2, 3), dtype=c), np.zeros((3, 3, 2), dtype=c))


def test_device_layer_refuses_alike():
    import torch
    from nd4js_amd import dev
    z, r, t = torch.zeros((3, 2), dtype=torch.complex128), torch.zeros((3, 2), dtype=torch.float64), torch.zeros(2, dtype=torch.complex128)
    for fn, real_fn in ((dev.zbidiag_factor, "bidiag_decomp"), (lambda a: dev.zbidiag_apply_p(a, t, z[:2]), "bidiag_decomp"),
                        (dev.zsvd_decomp, "svd_decomp"), (dev.zsvd_vals, "svd_decomp")):
        with pytest.raises(TypeError, match=real_fn):
            fn(r)
        with pytest.raises(TypeError, match="only complex128"):
            fn(z.to(torch.complex64))
        with pytest.raises(TypeError, match="CUDA tensor"):
            fn(z)


def test_the_real_family_still_refuses_complex_input():
    z = np.ones((3, 2), dtype=np.complex128)
    for call in (lambda: la.svd_decomp(z), lambda: la.svd_vals(z), lambda: la.bidiag_decomp(z)):
        with pytest.raises((TypeError, ValueError), match="complex|must be float"):
            call()
