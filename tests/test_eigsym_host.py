"""CPU-side checks of eigen_sym / eigenvals_sym: the numpy model of csrc/syev.hip's new arithmetic (tests/eigsym_common.py) meets
the device's bounds on every catalogue input, the committed reference values are sound, the argument errors, the ABI names, and
the loud failure without a GPU."""
import os
import re

import numpy as np
import pytest

import eigsym_common as C
from conftest import ROOT
from nd4js_amd import _lib, la


@pytest.mark.parametrize("name", C.NAMES)
def test_model_meets_the_bounds(name):
    """largest shares of the bounds seen over the catalogue up to N = 300: values 3.9e-3, residual 1.3e-2, orthogonality 2.6e-3;
    smallest radicand 0.075 (dense_2). Asserted: the bounds themselves, and a radicand above 2^-21, the kernel's own pivot bound
    (csrc/syev.hip) less rounding."""
    S, lam_ref, _ = C.reference(name)
    N = S.shape[-1]
    for s, lr in zip(S.reshape(-1, N, N), lam_ref.reshape(-1, N)):
        lam, V, low = C.model(s)
        order = np.argsort(-lam, kind="stable")
        C.check(s, lam[order], V[:, order], lr, name)
        assert low > 2.0 ** -21


def test_model_recurrence_is_a_cholesky_factor():
    d, e = np.zeros(9), np.ones(8)
    p, q, c, k, _ = C.shift_chol(d, e)
    B = np.diag(p) + np.diag(q, 1)
    assert np.abs(B.T @ B - (np.ldexp(C.tridiag(d, e), k) + c * np.eye(9))).max() <= 8 * C.EPS * c
    assert C.shift_chol(np.zeros(4), np.zeros(3)) is None


@pytest.mark.parametrize("name", sorted(C.golden_manifest()["cases"]))
def test_committed_reference_values_are_sound(name):
    meta = C.golden_manifest()["cases"][name]
    S = C.golden_input(name, meta)
    assert S.shape == (meta["N"], meta["N"]) and np.array_equal(S, S.T)
    nrm = np.linalg.norm(S)
    assert nrm == pytest.approx(meta["fro"], rel=1e-13, abs=0)
    want = C.golden_values(name, meta)
    if want is None:
        assert meta["lam_kept"] is False and meta["reason"]
        return
    assert np.abs(want.imag).max() <= 1e-12 * nrm and np.abs(want.imag).max() == meta["ref_max_imag"]
    assert np.abs(np.sort(want.real) - np.linalg.eigvalsh(S)).max() <= 1e-12 * nrm


def test_dense_fixtures_are_the_catalogue_inputs():
    cases = C.golden_manifest()["cases"]
    for N in (1, 2, 3, 33, 70, 127, 128):
        meta = cases["dense_%d" % N]
        assert np.array_equal(C.golden_input("dense_%d" % N, meta), C.reference("dense_%d" % N)[0])


@pytest.mark.parametrize("fn, name", [(la.eigen_sym, "eigen_sym"), (la.eigenvals_sym, "eigenvals_sym")])
def test_argument_errors(fn, name):
    with pytest.raises(ValueError, match=re.escape("%s(S): S.ndim must be at least 2." % name)):
        fn(np.ones(3))
    with pytest.raises(ValueError, match=re.escape("%s(S): S must be quadratic." % name)):
        fn(np.ones((2, 3, 4)))
    with pytest.raises(TypeError):
        fn(np.eye(3, dtype=np.float32))
    with pytest.raises(TypeError, match=re.escape("%s(S): S.dtype must be float." % name)):
        fn(np.eye(3, dtype=np.complex128))


def test_dev_argument_errors():
    torch = pytest.importorskip("torch")
    from nd4js_amd import dev
    for fn in (dev.eigen_sym, dev.eigenvals_sym):
        with pytest.raises(TypeError):
            fn(torch.eye(3, dtype=torch.float32))
        with pytest.raises(TypeError):
            fn(np.eye(3))


def test_abi_names():
    hdr = open(os.path.join(ROOT, "include", "nd4hip.h")).read()
    lib = _lib.load()
    for n in ("nd4hip_dsyevd_batched_dev", "nd4hip_dsyevd_batched", "nd4hip_dsyevd_last_stages"):
        assert re.search(r"\b%s\s*\(" % n, hdr) and hasattr(lib, n) and n in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["nd4hip_dsyevd_batched_dev"][1]) == 6


def test_c_argument_checks_need_no_device():
    lib = _lib.load()
    assert lib.nd4hip_dsyevd_batched_dev(None, 1, 4, None, None, None) == -1
    assert lib.nd4hip_dsyevd_batched(None, 1, 4, None, None, None) == -1


@pytest.mark.skipif(_lib.load().nd4hip_device_count() > 0, reason="GPU present")
def test_no_cpu_fallback_without_gpu():
    for fn in (la.eigen_sym, la.eigenvals_sym):
        with pytest.raises(_lib.Nd4HipError) as e:
            fn(np.eye(4))
        assert e.value.code == -4
