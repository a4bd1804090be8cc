"""The Hermitian tridiagonal reduction and eigenproblem (herm_tridiag_factor, herm_tridiag_apply_q, herm_tridiag_decomp, eigen_herm,
eigenvals_herm) without a GPU: the numpy model of herm_common.py against LAPACK's zhetrd, its exact cases, the argument checks of the
four new C operations in both forms, the header / exports / bindings, the argument errors of la and dev, and which entry point each
Python call reaches.

Largest shares of the bounds the model has shown (N = 3 .. 200): reconstruction 1.2e-3, unitarity 9.7e-4, values of T 1.9e-3."""
import os
import re

import numpy as np
import pytest
from scipy.linalg import eigh
from scipy.linalg.lapack import zhetrd

import herm_common as X
import tridiag_common as R
from conftest import ROOT
from nd4js_amd import _lib, la


# ---- the model --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [3, 4, 5, 17, 64, 129, 200])
def test_model_against_lapack(N):
    H, lam_ref = X.dense(N)
    F, tau, d, e = X.model(H)
    X.check_layout(F, tau, d, e)
    Q = X.form_q(F, tau)
    X.check(H, Q, d, e, lam_ref, "model N = %d" % N)
    # LAPACK's convention: zhetrd(lower) on the column-major view of the same matrix
    c, dl, el, taul, info = zhetrd(np.asfortranarray(H), lower=1)
    nrm = X.norm_of(H)
    assert info == 0
    assert np.abs(d - dl).max() <= X.TOL * nrm and np.abs(e - el).max() <= X.TOL * nrm and np.abs(tau - taul).max() <= X.TOL * nrm
    assert np.abs(np.tril(F, -2) - np.tril(c, -2)).max() <= X.TOL * nrm
    # the eigenvectors of T, taken back by Q, are those of H
    lam, W = eigh(X.tridiag(d, e))
    V = X.apply_q(F, tau, W)
    assert np.linalg.norm(H @ V - V * lam) <= X.TOL * nrm
    Z = X.rng.matrix(N, N, 3) + 1j * X.rng.matrix(N + 1, N, 3)
    assert np.linalg.norm(X.apply_q(F, tau, X.apply_q(F, tau, Z), True) - Z) <= X.TOL * np.linalg.norm(Z)


def test_model_sign_rule_with_a_real_tail():
    # x = [alpha; tail]: e = -sign(Re alpha) |x|, sign(0) = +1
    for alpha, want in ((3.0, -5.0), (-3.0, 5.0), (0.0, -4.0)):
        H = np.zeros((3, 3), dtype=np.complex128)
        H[1, 0] = H[0, 1] = alpha
        H[2, 0] = H[0, 2] = 4.0
        F, tau, d, e = X.model(H)
        assert e[0] == want and tau[0] == (want - alpha) / want and tau[0].imag == 0.0


def test_model_phase_reflector_2x2():
    H = np.array([[1.0, 99.0], [3.0 + 4.0j, 2.0]], dtype=np.complex128)
    F, tau, d, e = X.model(H)
    X.check_layout(F, tau, d, e)
    # d_1 = h_11 - 2 Re w with Re w = (1.6 - 1.6) h_11 up to one rounding of |tau|^2 / 2
    assert tau[0] == 1.6 + 0.8j and e[0] == -5.0 and d[0] == 1.0 and abs(d[1] - 2.0) <= 4 * np.finfo(float).eps
    Q = X.form_q(F, tau)
    assert np.abs(Q @ X.tridiag(d, e) @ np.conj(Q.T) - X.herm(H)).max() <= 8 * np.finfo(float).eps


def test_model_tiny_complex_coupling_stays_finite():
    X.check_tiny_coupling(X.model)
    # two dense blocks coupled by one such entry: the three bounds hold
    H = X.block_diagonal(12, 5)
    H[5, 4] = (1.0 - 2.0j) * 1e-165
    F, tau, d, e = X.model(H)
    assert np.all(np.isfinite(tau)) and np.all(np.isfinite(d)) and np.all(np.isfinite(e)) and tau[4] != 0.0
    X.check(H, X.form_q(F, tau), d, e, np.linalg.eigvalsh(X.herm(H)), "tiny coupling 12")


def test_model_complex_tridiagonal():
    H = X.complex_tridiag(9)
    F, tau, d, e = X.model(H)
    assert not np.tril(F, -2).any() and np.all(tau != 0.0)
    # d = Re diag: step k takes a (2 Re tau - |tau|^2) off d_{k+1}, which is zero up to the roundings of tau, p and w (LAPACK's
    # zhetd2 does the same), so not to the bit: 8 eps with |d| < 1
    assert np.abs(d - np.diag(H).real).max() <= 8 * np.finfo(float).eps
    # |e_k| = |h_{k+1,k}|: step k-1 multiplies h_{k+1,k} by the phase 1 - tau_{k-1} (modulus 1 within 4 eps: a division, a subtraction,
    # a complex product), then one square root of a sum of two squares (3 eps): 8 eps |h| with |h| < 2, so 16 eps. Measured: 1.5 eps
    # at most on the device (N = 2, 5, 130; tests/test_gpu_herm.py prints it), and printed here for the model
    dev_e = np.abs(np.abs(e) - np.abs(np.diag(H, -1))).max() / np.finfo(float).eps
    print("model, complex tridiagonal 9: ||e_k| - |h_k+1,k|| is %.2f eps" % dev_e)
    assert dev_e <= 16
    Q = X.form_q(F, tau)
    assert np.abs(np.abs(np.diag(Q)) - 1.0).max() <= 32 * np.finfo(float).eps and not (Q - np.diag(np.diag(Q))).any()


def test_model_real_symmetric_as_complex():
    S = R.dense(17)[0]
    F, tau, d, e = X.model(S.astype(np.complex128))
    Fr, taur, dr, er = R.model(S)
    assert not F.imag.any() and not tau.imag.any()
    # the same recurrence on the same numbers; only the order inside the sums differs (BLAS dot and gemv, real against complex), so
    # the two agree as two backward stable runs do: well inside 1e-13 at N = 17 (entries in [-1, 1))
    tol = 1e-13
    assert np.abs(tau.real - taur).max() <= tol and np.abs(d - dr).max() <= tol and np.abs(e - er).max() <= tol
    assert np.abs(F.real - Fr).max() <= tol
    # the extra reflector: the real route leaves e_{N-2} = alpha with tau = 0, here too (sigma = 0, Im alpha = 0)
    assert tau[-1] == 0.0


def test_model_block_diagonal():
    H = X.block_diagonal(12, 5)
    F, tau, d, e = X.model(H)
    # column 3 has only its alpha inside the first block (complex: a phase reflector), column 4 nothing at all below the diagonal
    assert tau[3] != 0.0 and not F[5:, 3].any() and e[3] != 0.0 and tau[4] == 0.0 and e[4] == 0.0 and tau[2] != 0.0 and tau[5] != 0.0
    X.check(H, X.form_q(F, tau), d, e, np.linalg.eigvalsh(H), "block diagonal 12")


def test_model_power_of_two_scaling():
    H, _ = X.dense(17)
    F, tau, d, e = X.model(H)
    for k in (-500, 500):
        F2, tau2, d2, e2 = X.model(X._ldexp(np.array(H), k))
        assert X.same_bits(tau2, tau) and X.same_bits(np.tril(F2, -2), np.tril(F, -2))
        assert np.array_equal(d2, np.ldexp(d, k)) and np.array_equal(e2, np.ldexp(e, k))


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------
def test_both_forms_refuse_alike_before_the_handle():
    assert {r[0] for r in X.ROWS} == {n[len("nd4hip_"):] for n in X.NEW}
    for op in {r[0] for r in X.ROWS}:
        assert {"extent", "empty", "null"} <= {r[1] for r in X.ROWS if r[0] == op}
    assert X.mismatches(None) == []


def test_a_valid_call_without_a_handle_is_refused():
    lib = _lib.load()
    for name, args in X.VALID.items():
        for form in ("_host", "_dev"):
            assert getattr(lib, "nd4hip_" + name + form)(None, *args) == -1
            assert lib.nd4hip_last_error().decode() == "nd4hip_%s: NULL handle" % name


def test_header_exports_bindings_and_build_list():
    src = open(os.path.join(ROOT, "include", "nd4hip.h")).read()
    lib = _lib.load()
    for base in X.NEW:
        for form in ("_host", "_dev"):
            assert re.search(r"\bint %s%s\s*\(" % (base, form), src), base + form
            assert hasattr(lib, base + form) and base + form in _lib.SIGNATURES
        assert base not in _lib.SIGNATURES and not hasattr(lib, base)    # the pair is (X_host, X_dev), as for the tridiag_* operations
    assert _lib.SIGNATURES["nd4hip_zhetrd_batched_dev"] == _lib.SIGNATURES["nd4hip_dsytrd_batched_dev"]
    assert _lib.SIGNATURES["nd4hip_zunmtr_batched_host"] == _lib.SIGNATURES["nd4hip_dormtr_batched_host"]
    assert _lib.SIGNATURES["nd4hip_zheevd_batched_dev"] == _lib.SIGNATURES["nd4hip_dsyevd_tr_batched_dev"]
    assert _lib.SIGNATURES["nd4hip_zheevx_batched_host"] == _lib.SIGNATURES["nd4hip_dsyevx_tr_batched_host"]
    from nd4js_amd import build
    assert "hetrd.hip" in build.HIP_SOURCES and os.path.exists(os.path.join(build.CSRC, "hetrd.hip"))


# ---- the Python layers ----------------------------------------------------------------------------------------------------------
class _Recorder:
    """stands in for the handle: records the entry points that are called with their arguments, answers 0"""

    def __init__(self):
        self.calls, self.args, self.ptr, self.lib = [], [], None, self

    def __getattr__(self, name):
        if not name.startswith("nd4hip_"):
            raise AttributeError(name)
        return lambda *a: (self.calls.append(name), self.args.append(a)) and 0


@pytest.fixture
def recorder(monkeypatch):
    rec = _Recorder()
    monkeypatch.setattr(la._lib, "handle", lambda device=None: rec)
    return rec


def test_the_calls_reach_the_new_entries(recorder):
    H = np.zeros((3, 4, 4), dtype=np.complex128)
    lam, V = la.eigen_herm(H)
    assert lam.shape == (3, 4) and lam.dtype == np.float64 and V.shape == (3, 4, 4) and V.dtype == np.complex128
    assert la.eigenvals_herm(H).shape == (3, 4)
    assert recorder.calls == ["nd4hip_zheevd_batched_host"] * 2
    assert recorder.args[0][:3] == (None, 3, 4) and recorder.args[0][5] is not None and recorder.args[1][5] is None
    del recorder.calls[:], recorder.args[:]
    lam, V = la.eigen_herm(H, subset=(1, 3))
    assert lam.shape == (3, 2) and V.shape == (3, 4, 2) and V.dtype == np.complex128
    assert la.eigenvals_herm(H, subset=(0, 4)).shape == (3, 4)
    assert recorder.calls == ["nd4hip_zheevx_batched_host"] * 2
    assert recorder.args[0][:5] == (None, 3, 4, 1, 3) and recorder.args[1][7] is None
    del recorder.calls[:]
    F, tau, d, e = la.herm_tridiag_factor(H)
    assert F.shape == (3, 4, 4) and tau.shape == (3, 3) and d.shape == (3, 4) and e.shape == (3, 3)
    assert F.dtype == tau.dtype == np.complex128 and d.dtype == e.dtype == np.float64
    Z = np.ones((3, 4, 2))                                                  # float64: promoted
    out = la.herm_tridiag_apply_q(F, tau, Z, adjoint=True)
    assert out.shape == (3, 4, 2) and out.dtype == np.complex128 and recorder.args[-1][4] == 1
    Q, d, e = la.herm_tridiag_decomp(H)
    assert Q.shape == (3, 4, 4) and np.array_equal(Q[1], np.eye(4))             # (the recorder leaves the identity it was given)
    assert recorder.calls == ["nd4hip_zhetrd_batched_host", "nd4hip_zunmtr_batched_host", "nd4hip_zhetrd_batched_host", "nd4hip_zunmtr_batched_host"]
    F1, tau1, d1, e1 = la.herm_tridiag_factor(np.zeros((1, 1), dtype=np.complex128))
    assert tau1.shape == (0,) and e1.shape == (0,) and d1.shape == (1,)


def test_an_empty_call_reaches_nothing(recorder):
    lam, V = la.eigen_herm(np.eye(4, dtype=np.complex128), subset=(2, 2))
    assert lam.shape == (0,) and V.shape == (4, 0)
    assert la.eigenvals_herm(np.zeros((2, 4, 4), dtype=np.complex128), subset=(4, 4)).shape == (2, 0)
    F, tau, d, e = la.herm_tridiag_factor(np.zeros((0, 3, 3), dtype=np.complex128))
    assert F.shape == (0, 3, 3) and tau.shape == (0, 2)
    c = np.complex128
    assert la.herm_tridiag_apply_q(np.zeros((3, 3), dtype=c), np.zeros(2, dtype=c), np.zeros((3, 0), dtype=c)).shape == (3, 0)
    assert recorder.calls == []


def test_argument_errors(recorder):
    H = np.eye(4, dtype=np.complex128)
    for fn in (la.eigen_herm, la.eigenvals_herm):
        with pytest.raises(TypeError, match="eigen_sym"):
            fn(np.eye(4))
        with pytest.raises(TypeError, match="eigen_sym"):
            fn(np.eye(4, dtype=np.int32))
        with pytest.raises(TypeError, match="only complex128"):
            fn(np.eye(4, dtype=np.complex64))
        with pytest.raises(ValueError, match="quadratic"):
            fn(np.ones((2, 3), dtype=np.complex128))
        with pytest.raises(ValueError, match="at least 2"):
            fn(np.ones(3, dtype=np.complex128))
        # eigen_sym's subset errors
        for bad in ((3, 2), (0, 5), (-1, 2), (0.5, 2), (1,), 3, "ab"):
            with pytest.raises(ValueError, match=r"subset must be \(i0, i1\) with 0 <= i0 <= i1 <= N"):
                fn(H, subset=bad)
    for fn in (la.herm_tridiag_factor, la.herm_tridiag_decomp):
        with pytest.raises(ValueError, match="quadratic"):
            fn(np.ones((2, 3), dtype=np.complex128))
        with pytest.raises(ValueError, match="at least 2"):
            fn(np.ones(3, dtype=np.complex128))
        with pytest.raises(TypeError, match="eigen_sym"):
            fn(np.ones((2, 2)))
        with pytest.raises(ValueError, match="N <= 2048"):
            fn(np.zeros((2049, 2049), dtype=np.complex128))
    c = np.complex128
    F, tau, Z = np.zeros((2, 4, 4), dtype=c), np.zeros((2, 3), dtype=c), np.zeros((2, 4, 5), dtype=c)
    for bad in ((np.zeros((2, 4, 3), dtype=c), tau, Z), (F, np.zeros((2, 4), dtype=c), Z), (F, np.zeros((3, 3), dtype=c), Z), (F, np.zeros(3, dtype=c), Z),
                (F, tau, np.zeros((2, 5, 4))), (F, tau, np.zeros((4, 5))), (F, tau, np.zeros((3, 4, 5))), (F, tau, np.zeros(4))):
        with pytest.raises(ValueError, match="herm_tridiag_apply_q"):
            la.herm_tridiag_apply_q(*bad)
    with pytest.raises(TypeError, match="F and tau must be complex128"):
        la.herm_tridiag_apply_q(F.real, tau, Z)
    with pytest.raises(TypeError, match="Z must be"):
        la.herm_tridiag_apply_q(F, tau, np.zeros((2, 4, 5), dtype=np.int32))
    assert recorder.calls == []


def test_device_layer_refuses_alike():
    import torch
    from nd4js_amd import dev
    for fn in (dev.eigen_herm, dev.eigenvals_herm, dev.herm_tridiag_factor, dev.herm_tridiag_decomp):
        with pytest.raises(TypeError, match="eigen_sym"):
            fn(torch.zeros((2, 2), dtype=torch.float64))
        with pytest.raises(TypeError, match="CUDA tensor"):
            fn(torch.zeros((2, 2), dtype=torch.complex128))
        with pytest.raises(TypeError, match="CUDA tensor"):
            fn(np.zeros((2, 2), dtype=np.complex128))
    z = torch.zeros((2, 2), dtype=torch.complex128)
    with pytest.raises(TypeError, match="F and tau must be"):
        dev.herm_tridiag_apply_q(z, torch.zeros(1, dtype=torch.complex128), z)
    with pytest.raises(TypeError, match="F and tau must be"):
        dev.herm_tridiag_apply_q(torch.zeros((2, 2), dtype=torch.float64), torch.zeros(1, dtype=torch.float64), z)


def test_the_symmetric_family_still_refuses_complex_input():
    for fn in (la.eigen_sym, la.eigenvals_sym, la.tridiag_factor):
        with pytest.raises(TypeError, match="must be float"):
            fn(np.eye(3, dtype=np.complex128))
