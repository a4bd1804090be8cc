"""Selected eigenpairs (eigen_sym(S, subset), tridiag_eigen, tridiag_count) without a GPU: the numpy model of csrc/syevx.hip
(eigsym_subset_common.py) against LAPACK, the termination and scaling properties of the bisection, and the argument contract of
the three new operations in the C ABI and in the Python layers."""
import os
import re

import numpy as np
import pytest
import scipy.linalg

import eigsym_subset_common as X
from conftest import ROOT
from nd4js_amd import _lib, la

NAMES = tuple(X.TRIDIAGS) + tuple(X.LARGE_TRIDIAGS)


def _subsets(N):
    out = [(0, N)]
    if N >= 200:
        out += [(0, 16), (N // 2 - 32, N // 2 + 32)]
    return out


@pytest.mark.parametrize("name", NAMES)
def test_model_meets_the_bounds_against_lapack(name):
    d, e = X.tridiag_input(name)
    ref, T = X.tridiag_reference(name), X.tridiag(*X.tridiag_input(name))
    for sub in _subsets(len(d)):
        lam, Z, info = X.tridiag_model(name, None if sub == (0, len(d)) else sub)
        sh = X.check_subset(T, lam, Z, ref[sub[0]:sub[1]], "%s %s" % (name, sub))
        print("%s %s: shares %.3g %.3g %.3g, %d halvings" % ((name, sub) + sh + (info["halvings"],)))
        assert info["halvings"] <= 65
        assert X.signs_ok(Z)


def test_model_vectors_agree_with_lapack_where_isolated():
    d, e = X.tridiag_input("dense_50")
    w, v = scipy.linalg.eigh_tridiagonal(d, e)
    lam, Z, _ = X.tridiag_model("dense_50")
    v = v[:, ::-1]
    v = v * np.sign(np.einsum("ik,ik->k", v, Z))
    assert np.abs(v - Z).max() <= 1e-10                       # the smallest gap of this input is 1e-3 of its norm


def test_dense_model_against_eigh_subset_by_index():
    S = X.sym_uniform(7100 + 70, 70)
    for sub in ((0, 1), (69, 70), (0, 8), (20, 40)):
        w = scipy.linalg.eigh(S, eigvals_only=True, subset_by_index=[70 - sub[1], 70 - sub[0] - 1])[::-1]
        lam, V = X.eigen_sym_model(S, sub)
        X.check_subset(S, lam, V, w, "dense_70 %s" % (sub,))


def _halvings(d, e, force_bisection=False):
    p = X.prepare(np.asarray(d, dtype=np.float64), np.asarray(e, dtype=np.float64))
    if force_bisection:
        p["diag"] = False
    lams, lam, halvings = X.bisect(p, 0, p["N"])
    return lam, halvings, p


def test_bisection_terminates_within_the_cap():
    # the zero matrix and a diagonal with a zero eigenvalue take no bisection on the device; the recurrence is run on them all
    # the same: without the absolute floor eps g of the stop rule the zero eigenvalue takes 1054 halvings
    lam, n, p = _halvings(np.zeros(6), np.zeros(5), True)
    assert n == 0 and np.all(lam == 0.0) and p["g"] == 0.0
    lam, n, _ = _halvings([3.0, 0.0, -2.0, 1.0], np.zeros(3), True)
    assert n <= 65 and np.abs(lam - [3.0, 1.0, 0.0, -2.0]).max() <= 4 * X.EPS * 3.0
    d, e = np.ldexp(np.array([3.0, -5.0, 1.0, 7.0]), -1074), np.ldexp(np.array([2.0, 1.0, 4.0]), -1074)      # subnormal input
    lam, n, _ = _halvings(d, e)
    ref = np.linalg.eigvalsh(X.tridiag(np.ldexp(d, 1074), np.ldexp(e, 1074)))[::-1]
    assert n <= 65 and np.abs(np.ldexp(lam, 1074) - ref).max() <= 1.0                                       # one unit of 2^-1074
    N = 65
    d, e = np.full(N, np.ldexp(0.625, 1024)), np.full(N - 1, np.ldexp(0.125, 1024))                            # the top of the range
    assert np.all(np.isfinite(d))
    lam, n, _ = _halvings(d, e)
    ref = 0.625 + 0.25 * np.cos(np.arange(1, N + 1) * np.pi / (N + 1))
    assert n <= 65 and np.all(np.isfinite(lam)) and np.abs(np.ldexp(lam, -1024) - ref).max() <= 1e-12 * np.sqrt(N)
    for name in X.TRIDIAGS:
        assert X.tridiag_model(name)[2]["halvings"] <= 65, name


@pytest.mark.parametrize("m", [500, -500])
def test_power_of_two_scaling_is_exact(m):
    d, e = X.tridiag_input("dense_50")
    lam, Z, info = X.tridiag_model("dense_50")
    lam2, Z2, info2 = X.tridiag_eigen_model(np.ldexp(d, m), np.ldexp(e, m))
    assert X.same_bits(lam2, np.ldexp(lam, m)) and X.same_bits(Z2, Z)
    assert X.same_bits(info2["shift"], info["shift"]) and np.array_equal(info2["head"], info["head"])
    x = np.concatenate((lam[:5], [0.0, 1.0, -1.0]))
    assert np.array_equal(X.count(d, e, x), X.count(np.ldexp(d, m), np.ldexp(e, m), np.ldexp(x, m)))


def test_count_model_counts():
    d, e = X.tridiag_input("diag_ties_zero")                    # 3, 2, 2, 0.5, 0.5, 0, -1, -1
    x = np.array([3.0, 2.5, 2.0, 0.5, 0.0, -0.5, -1.0, -2.0, np.inf, -np.inf])
    assert X.count(d, e, x).tolist() == [0, 1, 1, 3, 5, 6, 6, 8, 0, 8]     # a probe on an eigenvalue does not count it
    d, e = X.tridiag_input("dense_50")
    ref = X.tridiag_reference("dense_50")
    mid = 0.5 * (ref[:-1] + ref[1:])
    assert X.count(d, e, mid).tolist() == list(range(1, 50))
    p = X.prepare(d, e)
    g = np.ldexp(p["g"], p["lexp"])                             # the Gershgorin bound of the unscaled member
    assert X.count(d, e, np.array([-2.0 * g, 2.0 * g])).tolist() == [50, 0]


def test_clusters_model():
    lams = np.array([1.0, 1.0 - 1e-4, 1.0 - 1e-4, 0.5, 0.5 - 2e-3, 0.5 - 2e-3 - 1e-18])
    head, shift = X.clusters(lams, 1.0)
    assert head.tolist() == [0, 0, 0, 3, 4, 4]
    assert shift[1] == lams[1] and shift[2] == lams[1] - X.PERT and shift[5] == lams[4] - X.PERT and shift[3] == 0.5


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------
P, Q, Z, ROWS, NEW, mismatches = X.P, X.Q, X.Z, X.ROWS, X.NEW, X.mismatches


def test_both_forms_refuse_alike_before_the_handle():
    assert {r[0] for r in ROWS} == {n[len("nd4hip_"):] for n in NEW}
    for op in {r[0] for r in ROWS}:
        assert {"extent", "empty", "null"} <= {r[1] for r in ROWS if r[0] == op}
    assert mismatches(None) == []


def test_a_valid_call_without_a_handle_is_refused():
    lib = _lib.load()
    for name, args in (("dstcnt_batched", (1, 1, 1, P, Z, P, Q)), ("dstevx_batched", (1, 1, 0, 1, P, Z, P, Z)), ("dsyevx_batched", (1, 1, 0, 1, P, P, Z))):
        for form in ("_host", "_dev"):
            assert getattr(lib, "nd4hip_" + name + form)(None, *args) == -1
            assert lib.nd4hip_last_error().decode() == "nd4hip_%s: NULL handle" % name


def test_header_exports_and_bindings():
    src = open(os.path.join(ROOT, "include", "nd4hip.h")).read()
    lib = _lib.load()
    for base in NEW:
        for form in ("_host", "_dev"):
            assert re.search(r"\bint %s%s\s*\(" % (base, form), src), base + form
            assert hasattr(lib, base + form) and base + form in _lib.SIGNATURES
        assert base not in _lib.SIGNATURES                      # the pair is (X_host, X_dev), not (X, X_dev): see the header
    assert "end in _host" in src and "nd4hip_dsyevx_last_stages" in _lib.SIGNATURES


# ---- the Python layers ----------------------------------------------------------------------------------------------------------
class _Recorder:
    """stands in for the handle: records the entry points that are called, answers 0"""

    def __init__(self):
        self.calls, self.ptr, self.lib = [], None, self

    def __getattr__(self, name):
        if not name.startswith("nd4hip_"):
            raise AttributeError(name)
        return lambda *a: self.calls.append(name) or 0


@pytest.fixture
def recorder(monkeypatch):
    rec = _Recorder()
    monkeypatch.setattr(la._lib, "handle", lambda device=None: rec)
    return rec


def test_the_default_call_keeps_its_entry_point(recorder):
    S = np.eye(4)
    la.eigen_sym(S), la.eigenvals_sym(S), la.eigen_sym(S, algo="dc"), la.eigen_sym(S, subset=None)
    assert recorder.calls == ["nd4hip_dsyevd_batched"] * 4
    del recorder.calls[:]
    lam, V = la.eigen_sym(np.zeros((3, 4, 4)), subset=(1, 3))
    assert recorder.calls == ["nd4hip_dsyevx_batched_host"] and lam.shape == (3, 2) and V.shape == (3, 4, 2)
    assert la.eigenvals_sym(S, subset=(0, 4)).shape == (4,) and recorder.calls[-1] == "nd4hip_dsyevx_batched_host"
    del recorder.calls[:]
    lam, Zv = la.tridiag_eigen(np.ones((2, 5)), np.ones((2, 4)), subset=(0, 3))
    assert lam.shape == (2, 3) and Zv.shape == (2, 5, 3) and la.tridiag_eigenvals(np.ones(5), np.ones(4)).shape == (5,)
    assert la.tridiag_count(np.ones(5), np.ones(4), np.zeros(7)).shape == (7,)
    assert recorder.calls == ["nd4hip_dstevx_batched_host"] * 2 + ["nd4hip_dstcnt_batched_host"]


def test_an_empty_subset_makes_no_device_call(recorder):
    lam, V = la.eigen_sym(np.eye(4), subset=(2, 2))
    assert lam.shape == (0,) and V.shape == (4, 0)
    assert la.eigenvals_sym(np.zeros((2, 4, 4)), subset=(4, 4)).shape == (2, 0)
    lam, Zv = la.tridiag_eigen(np.ones(5), np.ones(4), subset=(0, 0))
    assert lam.shape == (0,) and Zv.shape == (5, 0) and recorder.calls == []


def test_argument_errors(recorder):
    S = np.eye(4)
    for fn in (la.eigen_sym, la.eigenvals_sym):
        for bad in ((3, 2), (-1, 2), (0, 5), (0,), (0, 1, 2), 3, (0.5, 2), "ab"):
            with pytest.raises(ValueError, match="subset must be"):
                fn(S, subset=bad)
        with pytest.raises(ValueError, match="subset is not available with algo='jacobi'"):
            fn(S, algo="jacobi", subset=(0, 1))
        with pytest.raises(ValueError, match="quadratic"):
            fn(np.ones((2, 3)), subset=(0, 1))
    for fn in (la.tridiag_eigen, la.tridiag_eigenvals):
        with pytest.raises(ValueError, match="same leading dimensions"):
            fn(np.ones((2, 5)), np.ones((3, 4)))
        with pytest.raises(ValueError, match=r"e must have len\(d\) - 1 entries"):
            fn(np.ones(5), np.ones(5))
        with pytest.raises(ValueError, match="subset must be"):
            fn(np.ones(5), np.ones(4), subset=(2, 6))
        with pytest.raises(ValueError, match="N <= 2048"):
            fn(np.ones(2049), np.ones(2048))
    with pytest.raises(ValueError, match="x must have the leading dimensions of d"):
        la.tridiag_count(np.ones((2, 5)), np.ones((2, 4)), np.zeros(3))
    with pytest.raises(ValueError, match="x contains NaN"):
        la.tridiag_count(np.ones(5), np.ones(4), np.array([0.0, np.nan]))
    assert recorder.calls == []


def test_device_layer_refuses_subset_with_jacobi():
    from nd4js_amd import dev
    for fn in (dev.eigen_sym, dev.eigenvals_sym):
        with pytest.raises(ValueError, match="subset is not available with algo='jacobi'"):
            fn(None, algo="jacobi", subset=(0, 1))
