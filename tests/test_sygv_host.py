"""CPU-side checks of eigen_sym_gen / eigenvals_sym_gen: the numpy model of csrc/sygv.hip's small tier (tests/sygv_common.py) meets
every bound on every catalogue case, the committed LAPACK values are sound, the argument errors of la and dev, the ABI names, and
the loud failure without a GPU.

Largest shares of the bounds seen for the model over the catalogue (numpy.linalg.eigh as the solver): values 4.9e-4 (gram_64),
residual 8.2e-5 (gram_3), B-orthonormality 1.3e-3 (eye_33, where kappa = 1 leaves the bound at 1e-12 sqrt N), reduction 3.1e-5
(gram_3). On the device (test_gpu_sygv.py, default route / Jacobi): values 4.5e-4 / 4.8e-4, residual 1.8e-4 / 1.1e-4,
B-orthonormality 1.5e-3 / 1.1e-3, reduction 3.1e-5 (small tier, the model's bits) and 5.8e-6 (large tier)."""
import os
import re

import numpy as np
import pytest

import sygv_common as G
from conftest import ROOT
from nd4js_amd import _lib, la


@pytest.mark.parametrize("name", G.NAMES)
def test_model_meets_the_bounds(name):
    A, B = G.inputs(name)
    N = A.shape[-1]
    lam, X = np.empty(A.shape[:-1]), np.empty(A.shape)
    red = 0.0
    for m, (a, b) in enumerate(G.members(A, B)):
        L, C, bad = G.reduce_model(a, b)
        assert not bad and np.all(np.triu(C, 1) == 0.0)
        red = max(red, G.reduction_share(a, L, C))
        lam.reshape(-1, N)[m], X.reshape(-1, N, N)[m] = G.model(a, b)
    sh = G.check(A, B, lam, X, G.golden(name), name)
    print("%s model shares of the bounds (values, residual, B-orthonormality, reduction): %.3g %.3g %.3g %.3g" % ((name,) + sh + (red,)))
    assert red <= 1.0


def test_model_ignores_the_upper_triangles_and_flags_bad_radicands():
    A, B = G.inputs("gram_33")
    L, C, bad = G.reduce_model(A, B)
    L2, C2, bad2 = G.reduce_model(G.with_upper(A, np.nan), G.with_upper(B, 1e300))
    assert not bad and not bad2 and G.same_bits(L, L2) and G.same_bits(C, C2)
    assert np.abs(L @ L.T - B).max() <= 64 * np.finfo(float).eps * np.abs(B).max()
    for Bb in (-np.eye(3), np.zeros((3, 3)), np.ones((3, 3)), np.diag([1.0, 1.0, 0.0]), np.diag([1.0, np.inf, 1.0]), np.diag([1.0, np.nan, 1.0])):
        assert G.chol_model(Bb)[1]
    # B = I: C is the lower triangle of A and X = Y, bit for bit
    Li, Ci, _ = G.reduce_model(A, np.eye(33))
    assert G.same_bits(Li, np.eye(33)) and G.same_bits(Ci, np.tril(A)) and G.same_bits(G.back_model(Li, np.array(A)), np.array(A))


def test_committed_values_are_sound():
    man = G.manifest()
    assert sorted(man["cases"]) == sorted(G.NAMES)
    for name, meta in man["cases"].items():
        A, B = G.inputs(name)
        assert list(A.shape) == meta["shape_A"] and list(B.shape) == meta["shape_B"]
        want = G.golden(name)
        assert want.shape == A.shape[:-1] and want.dtype == np.float64 and np.all(np.diff(want, axis=-1) <= 0)
        for m, (a, b) in enumerate(G.members(A, B)):
            assert np.linalg.norm(a) == pytest.approx(meta["fro_A"][m], rel=1e-13, abs=0)
            assert np.linalg.norm(b) == pytest.approx(meta["fro_B"][m], rel=1e-13, abs=0)


def test_committed_values_are_what_scipy_returns():
    sl = pytest.importorskip("scipy.linalg")
    for name in G.NAMES:
        A, B = G.inputs(name)
        N = A.shape[-1]
        for want, (a, b) in zip(G.golden(name).reshape(-1, N), G.members(A, B)):
            sv = np.linalg.svd(b, compute_uv=False)
            got = sl.eigh(a, b, eigvals_only=True)[::-1]
            assert np.all(np.abs(got - want) <= 1e-13 * (np.linalg.norm(a) / sv[-1] + sv[0] / sv[-1] * np.abs(want))), name


@pytest.mark.parametrize("fn, name", [(la.eigen_sym_gen, "eigen_sym_gen"), (la.eigenvals_sym_gen, "eigenvals_sym_gen")])
def test_argument_errors(fn, name):
    I3 = np.eye(3)
    for a, b, who in ((np.ones(3), I3, "A"), (I3, np.ones(3), "B")):
        with pytest.raises(ValueError, match=re.escape("%s(A,B): %s.ndim must be at least 2." % (name, who))):
            fn(a, b)
    for a, b, who in ((np.ones((2, 3, 4)), I3, "A"), (I3, np.ones((3, 4)), "B")):
        with pytest.raises(ValueError, match=re.escape("%s(A,B): %s must be quadratic." % (name, who))):
            fn(a, b)
    with pytest.raises(TypeError):
        fn(np.eye(3, dtype=np.float32), I3)
    with pytest.raises(TypeError):
        fn(I3, np.eye(3, dtype=np.float32))
    with pytest.raises(TypeError, match=re.escape("%s(A,B): A.dtype must be float." % name)):
        fn(np.eye(3, dtype=np.complex128), I3)
    with pytest.raises(TypeError, match=re.escape("%s(A,B): B.dtype must be float." % name)):
        fn(I3, np.eye(3, dtype=np.complex128))
    for a, b in ((I3, np.eye(4)), (np.zeros((2, 3, 3)), np.zeros((3, 3, 3))), (np.zeros((2, 3, 3)), np.zeros((1, 3, 3))), (I3, np.zeros((2, 3, 3)))):
        with pytest.raises(ValueError, match=re.escape("%s(A,B): B.shape must be A.shape or A.shape[-2:]" % name)):
            fn(a, b)
    with pytest.raises(ValueError, match=re.escape("%s(A,B): algo must be None, 'dc' or 'jacobi'." % name)):
        fn(I3, I3, algo="qr")


def test_dev_argument_errors():
    torch = pytest.importorskip("torch")
    from nd4js_amd import dev
    eye = torch.eye(3, dtype=torch.float64)
    for fn in (dev.eigen_sym_gen, dev.eigenvals_sym_gen):
        with pytest.raises(TypeError, match="A.dtype must be float"):
            fn(torch.eye(3, dtype=torch.float32), eye)
        with pytest.raises(TypeError, match="B.dtype must be float"):
            fn(eye, torch.eye(3, dtype=torch.float32))
        with pytest.raises(TypeError):
            fn(np.eye(3), np.eye(3))
        with pytest.raises(TypeError):
            fn(eye, eye)                                        # host tensors: the device form takes device tensors only
        with pytest.raises(ValueError, match="algo must be None, 'dc' or 'jacobi'"):
            fn(eye, eye, algo="qr")


ABI = ("nd4hip_dsygvd_batched_dev", "nd4hip_dsygvd_batched", "nd4hip_dsygst_batched_dev", "nd4hip_dsygst_batched")


def test_abi_names():
    hdr = open(os.path.join(ROOT, "include", "nd4hip.h")).read()
    lib = _lib.load()
    for n in ABI:
        assert re.search(r"\b%s\s*\(" % n, hdr) and hasattr(lib, n) and n in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["nd4hip_dsygvd_batched_dev"][1]) == 10 and len(_lib.SIGNATURES["nd4hip_dsygst_batched"][1]) == 7
    for text in ("eigen_sym_gen(A,B): B is not positive definite. (matrix <b>)", "eigen_sym_gen(A,B): L^-1 A L^-T is not finite"):
        assert text in hdr


def test_c_argument_checks_need_no_device():
    lib = _lib.load()
    for algo in (0, 1):
        assert lib.nd4hip_dsygvd_batched_dev(None, algo, 1, 4, None, None, 16, None, None, None) == -1
        assert lib.nd4hip_dsygvd_batched(None, algo, 1, 4, None, None, 0, None, None, None) == -1
    assert lib.nd4hip_dsygst_batched_dev(None, 1, 4, None, None, 16, None) == -1
    assert lib.nd4hip_dsygst_batched(None, 1, 4, None, None, 0, None) == -1
    # out-of-range arguments are refused before the handle is looked at
    for args, text in (((0, 1, 2049), b"N <= 2048"), ((1, 1, 129), b"N <= 128"), ((2, 1, 4), b"algo must be 0"), ((0, -1, 4), b"negative extent")):
        for fn in (lib.nd4hip_dsygvd_batched_dev, lib.nd4hip_dsygvd_batched):
            assert fn(None, args[0], args[1], args[2], None, None, 0, None, None, None) == -1
            assert text in lib.nd4hip_last_error()
    assert lib.nd4hip_dsygvd_batched_dev(None, 0, 1, 4, None, None, 5, None, None, None) == -1 and b"strideB" in lib.nd4hip_last_error()
    assert lib.nd4hip_dsygst_batched_dev(None, 1, 2049, None, None, 0, None) == -1 and b"N <= 2048" in lib.nd4hip_last_error()


@pytest.mark.skipif(_lib.load().nd4hip_device_count() > 0, reason="GPU present")
def test_no_cpu_fallback_without_gpu():
    for fn in (la.eigen_sym_gen, la.eigenvals_sym_gen):
        for algo in (None, "jacobi"):
            with pytest.raises(_lib.Nd4HipError) as e:
                fn(np.eye(4), np.eye(4), algo=algo)
            assert e.value.code == -4
    with pytest.raises(_lib.Nd4HipError) as e:
        la._sygst(np.eye(4), np.eye(4))
    assert e.value.code == -4
