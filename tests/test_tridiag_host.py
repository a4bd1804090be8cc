"""The symmetric tridiagonal reduction (tridiag_factor, tridiag_apply_q, tridiag_decomp, eigen_sym(S, reduction='tridiag')) without a
GPU: the numpy model of tridiag_common.py against LAPACK, the argument checks of the four new C operations in both forms, the
header / exports / bindings, the argument errors of la and dev, and which entry point each Python call reaches."""
import os
import re

import numpy as np
import pytest
from scipy.linalg import eigh, eigvalsh

import tridiag_common as X
from conftest import ROOT
from nd4js_amd import _lib, la


# ---- the model --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [3, 4, 5, 17, 64, 129, 200])
def test_model_against_lapack(N):
    S, _ = X.dense(N)
    F, tau, d, e = X.model(S)
    X.check_layout(F, tau, d, e)
    Q = X.form_q(F, tau)
    sh = X.check(S, Q, d, e, eigvalsh(S), "model N = %d" % N)
    print("model N = %d shares (reconstruction, orthogonality, values): %.3g %.3g %.3g" % ((N,) + sh))
    # the eigenvectors of T, taken back by Q, are those of S
    lam, W = eigh(X.tridiag(d, e))
    V = X.apply_q(F, tau, W)
    assert np.linalg.norm(S @ V - V * lam) <= X.TOL * np.linalg.norm(S)
    Z = X.rng.matrix(N, N, 3)
    assert np.linalg.norm(X.apply_q(F, tau, X.apply_q(F, tau, Z), True) - Z) <= X.TOL * np.linalg.norm(Z)


def test_model_sign_rule_and_exact_cases():
    # x = [alpha; tail]: e = -sign(alpha) |x|, sign(0) = +1
    for alpha, want in ((3.0, -5.0), (-3.0, 5.0), (0.0, -4.0)):
        S = np.zeros((3, 3))
        S[1, 0] = S[0, 1] = alpha
        S[2, 0] = S[0, 2] = 4.0
        F, tau, d, e = X.model(S)
        assert e[0] == want and tau[1] == 0.0 and tau[0] == (want - alpha) / want
    # a zero tail changes nothing: tau = 0, e = alpha
    T = X.tridiag(np.arange(1.0, 7.0), -np.arange(1.0, 6.0))
    F, tau, d, e = X.model(T)
    assert np.array_equal(d, np.diag(T)) and np.array_equal(e, np.diag(T, -1)) and not tau.any() and np.array_equal(X.form_q(F, tau), np.eye(6))
    S = X.block_diagonal(12, 5)
    F, tau, d, e = X.model(S)
    # column 3 has only its alpha inside the first block, column 4 nothing at all below the diagonal
    assert tau[3] == 0.0 and e[3] != 0.0 and tau[4] == 0.0 and e[4] == 0.0 and tau[2] != 0.0 and tau[5] != 0.0
    # 2^k S: the same tails and tau, d and e scaled
    S, _ = X.dense(17)
    F, tau, d, e = X.model(S)
    for k in (-500, 500):
        F2, tau2, d2, e2 = X.model(np.ldexp(S, k))
        assert np.array_equal(tau2, tau) and np.array_equal(np.tril(F2, -2), np.tril(F, -2))
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


def test_header_exports_bindings_and_napi_table():
    src = open(os.path.join(ROOT, "include", "nd4hip.h")).read()
    lib = _lib.load()
    for base in X.NEW:
        for form in ("_host", "_dev"):
            assert re.search(r"\bint %s%s\s*\(" % (base, form), src), base + form
            assert hasattr(lib, base + form) and base + form in _lib.SIGNATURES
        assert base not in _lib.SIGNATURES and not hasattr(lib, base)    # the pair is (X_host, X_dev), as for the selected eigenpairs
    assert len(_lib.SIGNATURES["nd4hip_dsytrd_batched_dev"][1]) == 8 and len(_lib.SIGNATURES["nd4hip_dormtr_batched_host"][1]) == 8
    assert _lib.SIGNATURES["nd4hip_dsyevd_tr_batched_dev"] == _lib.SIGNATURES["nd4hip_dsyevd_batched_dev"]
    assert _lib.SIGNATURES["nd4hip_dsyevx_tr_batched_host"] == _lib.SIGNATURES["nd4hip_dsyevx_batched_host"]
    # the JS layer reaches the two eigen routes (opts.reduction) in both forms; the tridiag_* JS forms are not built
    shim = open(os.path.join(ROOT, "nd4js_amd", "csrc", "napi_shim.c")).read()
    for base in ("nd4hip_dsyevd_tr_batched", "nd4hip_dsyevx_tr_batched"):
        assert '"%s_host"' % base in shim and '"%s_dev"' % base in shim
    for name in ("dsyevd_tr_batched", "dsyevdals_tr_batched", "dsyevx_tr_batched", "dsyevxals_tr_batched"):
        assert '{"%s",' % name in shim


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


def test_without_the_keyword_the_calls_are_todays(recorder):
    S = np.zeros((3, 4, 4))
    la.eigen_sym(S), la.eigenvals_sym(S), la.eigen_sym(S, reduction=None), la.eigen_sym(S, reduction="hessenberg"), la.eigen_sym(S, algo="dc")
    assert recorder.calls == ["nd4hip_dsyevd_batched"] * 5
    for a in recorder.args:
        assert a[:3] == (None, 3, 4) and len(a) == 6 and (a[5] is None) == (a is recorder.args[1])
    del recorder.calls[:], recorder.args[:]
    la.eigen_sym(S, subset=(1, 3)), la.eigenvals_sym(S, subset=(1, 3), reduction="hessenberg")
    assert recorder.calls == ["nd4hip_dsyevx_batched_host"] * 2
    assert recorder.args[0][:5] == (None, 3, 4, 1, 3) and recorder.args[0][7] is not None and recorder.args[1][7] is None
    del recorder.calls[:]
    la.eigen_sym(S, algo="jacobi")
    assert recorder.calls == ["nd4hip_dsyevj_batched"]


def test_the_keyword_calls_the_new_entries(recorder):
    S = np.zeros((3, 4, 4))
    lam, V = la.eigen_sym(S, reduction="tridiag")
    assert lam.shape == (3, 4) and V.shape == (3, 4, 4)
    assert la.eigenvals_sym(S, reduction="tridiag", algo="dc").shape == (3, 4)
    assert recorder.calls == ["nd4hip_dsyevd_tr_batched_host"] * 2
    assert recorder.args[0][:3] == (None, 3, 4) and recorder.args[0][5] is not None and recorder.args[1][5] is None
    del recorder.calls[:], recorder.args[:]
    lam, V = la.eigen_sym(S, reduction="tridiag", subset=(1, 3))
    assert lam.shape == (3, 2) and V.shape == (3, 4, 2)
    assert la.eigenvals_sym(S, reduction="tridiag", subset=(0, 4)).shape == (3, 4)
    assert recorder.calls == ["nd4hip_dsyevx_tr_batched_host"] * 2
    assert recorder.args[0][:5] == (None, 3, 4, 1, 3) and recorder.args[1][7] is None
    del recorder.calls[:]
    F, tau, d, e = la.tridiag_factor(S)
    assert F.shape == (3, 4, 4) and tau.shape == (3, 3) and d.shape == (3, 4) and e.shape == (3, 3)
    Z = np.ones((3, 4, 2))
    out = la.tridiag_apply_q(F, tau, Z, transpose=True)
    assert out.shape == (3, 4, 2) and out is not Z and recorder.args[-1][4] == 1
    Q, d, e = la.tridiag_decomp(S)
    assert Q.shape == (3, 4, 4) and np.array_equal(Q[1], np.eye(4))             # (the recorder leaves the identity it was given)
    assert recorder.calls == ["nd4hip_dsytrd_batched_host", "nd4hip_dormtr_batched_host", "nd4hip_dsytrd_batched_host", "nd4hip_dormtr_batched_host"]
    F1, tau1, d1, e1 = la.tridiag_factor(np.zeros((1, 1)))
    assert tau1.shape == (0,) and e1.shape == (0,) and d1.shape == (1,)


def test_an_empty_call_reaches_nothing(recorder):
    lam, V = la.eigen_sym(np.eye(4), subset=(2, 2), reduction="tridiag")
    assert lam.shape == (0,) and V.shape == (4, 0)
    assert la.eigenvals_sym(np.zeros((2, 4, 4)), subset=(4, 4), reduction="tridiag").shape == (2, 0)
    F, tau, d, e = la.tridiag_factor(np.zeros((0, 3, 3)))
    assert F.shape == (0, 3, 3) and tau.shape == (0, 2)
    assert la.tridiag_apply_q(np.zeros((3, 3)), np.zeros(2), np.zeros((3, 0))).shape == (3, 0)
    assert recorder.calls == []


def test_argument_errors(recorder):
    S = np.eye(4)
    for fn in (la.eigen_sym, la.eigenvals_sym):
        for bad in ("tri", "sytrd", 1, True, ("tridiag",)):
            with pytest.raises(ValueError, match="reduction must be None, 'hessenberg' or 'tridiag'"):
                fn(S, reduction=bad)
        with pytest.raises(ValueError, match="reduction is not available with algo='jacobi'"):
            fn(S, algo="jacobi", reduction="tridiag")
        with pytest.raises(ValueError, match="quadratic"):
            fn(np.ones((2, 3)), reduction="tridiag")
        with pytest.raises(TypeError, match="must be float"):
            fn(np.ones((2, 2), dtype=np.complex128), reduction="tridiag")
        with pytest.raises(ValueError, match="subset must be"):
            fn(S, reduction="tridiag", subset=(3, 2))
    for fn in (la.tridiag_factor, la.tridiag_decomp):
        with pytest.raises(ValueError, match="quadratic"):
            fn(np.ones((2, 3)))
        with pytest.raises(ValueError, match="at least 2"):
            fn(np.ones(3))
        with pytest.raises(TypeError, match="must be float"):
            fn(np.ones((2, 2), dtype=np.complex128))
        with pytest.raises(ValueError, match="N <= 2048"):
            fn(np.zeros((2049, 2049)))
    F, tau, Z = np.zeros((2, 4, 4)), np.zeros((2, 3)), np.zeros((2, 4, 5))
    for bad in ((np.zeros((2, 4, 3)), tau, Z), (F, np.zeros((2, 4)), Z), (F, np.zeros((3, 3)), Z), (F, np.zeros(3), Z), (F, tau, np.zeros((2, 5, 4))),
                (F, tau, np.zeros((4, 5))), (F, tau, np.zeros((3, 4, 5))), (F, tau, np.zeros(4))):
        with pytest.raises(ValueError, match="tridiag_apply_q"):
            la.tridiag_apply_q(*bad)
    with pytest.raises(TypeError, match="must be float"):
        la.tridiag_apply_q(F, tau, Z.astype(np.complex128))
    assert recorder.calls == []


def test_device_layer_refuses_alike():
    import torch
    from nd4js_amd import dev
    for fn in (dev.eigen_sym, dev.eigenvals_sym):
        with pytest.raises(ValueError, match="reduction is not available with algo='jacobi'"):
            fn(None, algo="jacobi", reduction="tridiag")
        with pytest.raises(ValueError, match="reduction must be None, 'hessenberg' or 'tridiag'"):
            fn(None, reduction="householder")
    for fn in (dev.tridiag_factor, dev.tridiag_decomp):
        with pytest.raises(TypeError, match="must be float"):
            fn(torch.zeros((2, 2), dtype=torch.complex128))
        with pytest.raises(TypeError, match="CUDA tensor"):
            fn(torch.zeros((2, 3), dtype=torch.float64))
    with pytest.raises(TypeError, match="must be float"):
        dev.tridiag_apply_q(torch.zeros((2, 2)), torch.zeros(1), torch.zeros((2, 2)))
    with pytest.raises(TypeError, match="CUDA tensor"):
        dev.tridiag_apply_q(torch.zeros((2, 2), dtype=torch.float64), torch.zeros(1, dtype=torch.float64), torch.zeros((2, 2), dtype=torch.float64))
