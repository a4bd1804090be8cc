"""zhess_* / zschur_* / zeigen / zeigenvals without a GPU: the argument rows of both forms of the C ABI, header, exports and bindings,
the tier arithmetic of csrc/zgehrd.hip and csrc/zhseqr.hip, the argument and dtype errors of la."""
import ctypes
import os
import re

import numpy as np
import pytest

from nd4js_amd import _lib, la

OPS = ("zgehrd_batched", "zunmhr_batched", "zhseqr_batched", "zgees_batched", "ztrevc_batched", "zgeev_batched")
B = 16           # any non-NULL pointer value
NULL, NEG = "NULL pointer", "negative extent"
ROWS = [  # (operation, the arguments after the handle, the error text after the operation's name or None for an empty call)
    ("zgehrd_batched", (-1, 4, B, B, B), NEG), ("zgehrd_batched", (1, 2049, B, B, B), "N <= 2048"), ("zgehrd_batched", (0, 4, B, B, B), None),
    ("zgehrd_batched", (1, 4, B, B, None), NULL), ("zgehrd_batched", (1, 1, B, B, None), "NULL handle"),
    ("zunmhr_batched", (1, 4, -1, 0, B, B, B), NEG), ("zunmhr_batched", (1, 4, 2, 2, B, B, B), "adjoint must be 0 or 1"),
    ("zunmhr_batched", (1, 2049, 2, 0, B, B, B), "N <= 2048"), ("zunmhr_batched", (1, 4, 0, 0, B, B, B), None),
    ("zunmhr_batched", (1, 4, 2, 1, B, B, None), NULL), ("zunmhr_batched", (1, 4, 2, 1, B, B, B), "NULL handle"),
    ("zhseqr_batched", (1, -4, 1, B, B, B, B), NEG), ("zhseqr_batched", (1, 1025, 1, B, B, B, B), "N <= 1024"),
    ("zhseqr_batched", (1, 4, 2, B, B, B, B), "want_t must be 0 or 1"), ("zhseqr_batched", (1, 4, 0, B, B, B, B), "NULL pointer, or Q without want_t"),
    ("zhseqr_batched", (1, 4, 1, None, B, B, B), "NULL pointer, or Q without want_t"), ("zhseqr_batched", (1, 0, 1, B, B, B, B), None),
    ("zhseqr_batched", (1, 4, 0, None, B, None, B), "NULL handle"),
    ("zgees_batched", (-1, 4, B, B, B), NEG), ("zgees_batched", (1, 1025, B, B, B), "N <= 1024"), ("zgees_batched", (1, 4, B, None, B), NULL),
    ("zgees_batched", (0, 4, B, B, B), None), ("zgees_batched", (1, 4, B, B, B), "NULL handle"),
    ("ztrevc_batched", (1, 1025, B, B, B, B), "N <= 1024"), ("ztrevc_batched", (1, 4, B, B, B, None), NULL), ("ztrevc_batched", (1, 4, B, B, B, B), "NULL handle"),
    ("zgeev_batched", (1, -1, B, B, B), NEG), ("zgeev_batched", (1, 1025, B, B, None), "N <= 1024"), ("zgeev_batched", (1, 4, B, None, B), NULL),
    ("zgeev_batched", (1, 0, B, B, B), None), ("zgeev_batched", (1, 4, B, B, None), "NULL handle"),
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


def test_tier_arithmetic():
    """the edges the headers state, LDS within a CU's 163840 bytes for every N, the reduction's workspace"""
    lib = ctypes.CDLL(_lib.load()._name)
    fn = {}
    for name, res in (("15nd4_zgehrd_tier", ctypes.c_int), ("14nd4_zgehrd_lds", ctypes.c_size_t), ("19nd4_zgehrd_ws_elems", ctypes.c_int64),
                      ("15nd4_zhseqr_tier", ctypes.c_int), ("14nd4_zhseqr_lds", ctypes.c_size_t), ("20nd4_zhseqr_tile_rows", ctypes.c_int),
                      ("15nd4_ztrevc_tier", ctypes.c_int)):
        f = getattr(lib, "_Z%sl" % name)
        f.restype, f.argtypes = res, [ctypes.c_int64]
        fn[name[2:]] = f
    assert [fn["nd4_zgehrd_tier"](n) for n in (1, 95, 96, 2048)] == [0, 0, 1, 1] and fn["nd4_zgehrd_lds"](95) == 159232
    assert [fn["nd4_zhseqr_tier"](n) for n in (1, 89, 90, 1024)] == [0, 0, 1, 1] and fn["nd4_zhseqr_lds"](89) == 162664
    assert [fn["nd4_ztrevc_tier"](n) for n in (1, 64, 65, 1024)] == [0, 0, 1, 1]
    for n in range(1, 2049):
        tier = fn["nd4_zgehrd_tier"](n)
        assert fn["nd4_zgehrd_lds"](n) == (16 * (n * (n | 1) + 7 * n + 256) + 96 if tier == 0 else 48 * n) <= 163840
        assert fn["nd4_zgehrd_ws_elems"](n) == (0 if tier == 0 else 6 * n + 2 * ((n + 63) // 64) * n)
        if n <= 1024:
            rows = fn["nd4_zhseqr_tile_rows"](n)
            assert rows == (256 if fn["nd4_zhseqr_tier"](n) else 16 if n <= 16 else 32 if n <= 32 else 64)
            assert fn["nd4_zhseqr_lds"](n) == 24 * n + 528 * rows + (0 if fn["nd4_zhseqr_tier"](n) else 16 * n * (n | 1)) <= 163840


@pytest.fixture
def recorder(monkeypatch):
    """the library must not be reached"""
    monkeypatch.setattr(la._lib, "handle", lambda device=None: pytest.fail("the library was reached"))


def test_empty_calls_and_argument_errors(recorder):
    c = np.complex128
    F, tau = la.zhess_factor(np.zeros((0, 4, 4), dtype=c))
    assert (F.shape, tau.shape) == ((0, 4, 4), (0, 3)) and la.zhess_apply_q(np.zeros((4, 4), dtype=c), np.zeros(3, dtype=c), np.zeros((4, 0), dtype=c)).shape == (4, 0)
    lam, V = la.zeigen(np.zeros((2, 0, 0), dtype=c))
    assert (lam.shape, V.shape) == ((2, 0), (2, 0, 0)) and la.zeigenvals(np.zeros((0, 3, 3), dtype=c)).shape == (0, 3)
    assert [x.shape for x in la.zschur_decomp(np.zeros((0, 3, 3), dtype=c))] == [(0, 3, 3)] * 2
    for fn, real_fn, nmax in ((la.zhess_factor, "hessenberg_decomp", 2048), (la.zhess_decomp, "hessenberg_decomp", 2048), (la.zschur_decomp, "schur_decomp", 1024),
                              (la.zeigen, "eigen", 1024), (la.zeigenvals, "eigen", 1024), (lambda a: la.zschur_eigen(a, a), "schur_eigen", 1024),
                              (lambda a: la.zschur_qr(a, a), "schur_decomp", 1024)):
        with pytest.raises(TypeError, match=real_fn):
            fn(np.ones((3, 3)))
        with pytest.raises(TypeError, match="only complex128 runs on the GPU path"):
            fn(np.ones((3, 3), dtype=np.complex64))
        for a, text in ((np.ones(4, dtype=c), "at least 2"), (np.ones((3, 4), dtype=c), "must be quadratic"), (np.zeros((nmax + 1, nmax + 1), dtype=c), "N <= %d" % nmax)):
            with pytest.raises(ValueError, match=text):
                fn(a)
    with pytest.raises(ValueError, match="F and tau don't match"):
        la.zhess_apply_q(np.ones((4, 4), dtype=c), np.zeros(4, dtype=c), np.zeros((4, 2), dtype=c))
    with pytest.raises(ValueError, match="F and Z don't match"):
        la.zhess_apply_q(np.ones((4, 4), dtype=c), np.zeros(3, dtype=c), np.zeros((3, 2), dtype=c))
