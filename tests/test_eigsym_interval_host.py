"""interval=(lo, hi) of eigen_sym / eigenvals_sym / tridiag_eigen / tridiag_eigenvals (csrc/syevx.hip) without a GPU:
the numpy interval model against LAPACK, the argument rows of the four new C operations in both forms, the header / exports /
bindings / N-API table, the argument errors of la and dev, and which entry point each Python call reaches."""
import os
import re

import numpy as np
import pytest

import eigsym_interval_common as I
import eigsym_subset_common as X
from conftest import ROOT
from nd4js_amd import _lib, la


# ---- the model --------------------------------------------------------------------------------------------------------------------
def test_the_count_at_infinity():
    # what interval=(x, inf) and (-inf, x) rest on: nothing is greater than +inf, everything is greater than -inf
    for name in ("dense_3", "dense_50", "identity_8", "diag_ties_zero", "zeros_in_e_40", "scaled_p500", "scaled_m500"):
        d, e = X.tridiag_input(name)
        assert X.count(d, e, [np.inf, -np.inf]).tolist() == [0, len(d)], name
        assert I.model_range(d, e, -np.inf, np.inf) == (0, len(d))


@pytest.mark.parametrize("name", tuple(X.TRIDIAGS))
def test_model_ranges_against_lapack(name):
    d, e = X.tridiag_input(name)
    ref, N = X.tridiag_reference(name), len(d)
    cuts = I.cuts(ref, I.gershgorin(d, e))
    assert cuts or name in ("identity_8",), name
    # the count at every unambiguous boundary is the number of LAPACK's values above it
    js = sorted(cuts)
    assert X.count(d, e, [cuts[j] for j in js]).tolist() == js if js else True
    for a in js[:: max(1, len(js) // 6)]:
        for b in js[:: max(1, len(js) // 5)]:
            if a <= b:                                         # x_a >= x_b: the interval (x_b, x_a] holds the values a .. b - 1
                assert I.model_range(d, e, cuts[b], cuts[a]) == (a, b), (name, a, b)
        assert I.model_range(d, e, cuts[a], np.inf) == (0, a) and I.model_range(d, e, -np.inf, cuts[a]) == (a, N)
        assert I.model_range(d, e, cuts[a], cuts[a]) == (a, a)


def test_model_values_are_those_of_the_subset_model():
    d, e = X.tridiag_input("dense_50")
    ref = X.tridiag_reference("dense_50")
    cuts = I.cuts(ref, I.gershgorin(d, e))
    a, b = sorted(cuts)[2], sorted(cuts)[-3]
    rng_, lam, Z = I.model(d, e, cuts[b], cuts[a])
    assert rng_ == (a, b) and lam.shape == (b - a,) and Z.shape == (50, b - a)
    want = X.tridiag_eigen_model(d, e, (a, b))
    assert X.same_bits(lam, want[0]) and X.same_bits(Z, want[1])
    X.check_subset(X.tridiag(d, e), lam, Z, ref[a:b], "interval model")
    assert np.all(lam > cuts[b]) and np.all(lam <= cuts[a])
    rng_, lam, Z = I.model(d, e, 1e9, np.inf)
    assert rng_ == (0, 0) and lam.shape == (0,) and Z.shape == (50, 0)


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------
def test_both_forms_refuse_alike_before_the_handle():
    assert {r[0] for r in I.ROWS} == {n[len("nd4hip_"):] for n in I.NEW}
    for op in {r[0] for r in I.ROWS}:
        assert {"extent", "empty", "null", "kcap"} <= {r[1] for r in I.ROWS if r[0] == op}
    assert I.mismatches(None) == []


def test_a_valid_call_without_a_handle_is_refused():
    lib = _lib.load()
    for name, lists in I.VALID.items():
        for args in lists:
            for form in ("_host", "_dev"):
                assert getattr(lib, "nd4hip_" + name + form)(None, *args) == -1
                assert lib.nd4hip_last_error().decode() == "nd4hip_%s: NULL handle" % name


def test_gen_entry_refuses_alike_before_the_handle():
    assert {"selector", "extent", "kcap", "stride", "empty", "null"} <= {r[0] for r in I.GEN_ROWS}
    assert I.gen_mismatches(None) == []
    lib = _lib.load()
    for args in I.GEN_VALID:
        for form in ("_host", "_dev"):
            assert getattr(lib, "nd4hip_dsygvx_batched" + form)(None, *args) == -1
            assert lib.nd4hip_last_error().decode() == "nd4hip_dsygvx_batched: NULL handle"


def test_header_exports_and_bindings():
    src = open(os.path.join(ROOT, "include", "nd4hip.h")).read()
    lib = _lib.load()
    for base in I.NEW:
        for form in ("_host", "_dev"):
            assert re.search(r"\bint %s%s\s*\(" % (base, form), src), base + form
            assert hasattr(lib, base + form) and base + form in _lib.SIGNATURES
        assert base not in _lib.SIGNATURES and not hasattr(lib, base)    # the pair is (X_host, X_dev), as for the selected eigenpairs
        assert _lib.SIGNATURES[base + "_host"] == _lib.SIGNATURES[base + "_dev"]
    assert len(_lib.SIGNATURES["nd4hip_dstevxv_batched_dev"][1]) == 11 and len(_lib.SIGNATURES["nd4hip_dsyevxv_batched_dev"][1]) == 10
    assert _lib.SIGNATURES["nd4hip_dsyevxv_tr_batched_host"] == _lib.SIGNATURES["nd4hip_dsyevxv_batched_host"]
    for name in ("nd4hip_dsygvx_batched_host", "nd4hip_dsygvx_batched_dev"):
        assert re.search(r"\bint %s\s*\(" % name, src) and hasattr(lib, name) and len(_lib.SIGNATURES[name][1]) == 16
    assert _lib.SIGNATURES["nd4hip_dsygvx_batched_host"] == _lib.SIGNATURES["nd4hip_dsygvx_batched_dev"] and "nd4hip_dsygvx_batched" not in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["nd4hip_dsygvd_batched"][1]) == 10          # untouched
    # the JS layer reaches every new operation, and the tridiagonal solver of DESIGN.md 4.20, in both forms
    shim = open(os.path.join(ROOT, "nd4js_amd", "csrc", "napi_shim.c")).read()
    for base in I.NEW + ("nd4hip_dsygvx_batched", "nd4hip_dstcnt_batched", "nd4hip_dstevx_batched"):
        assert '"%s_host"' % base in shim and '"%s_dev"' % base in shim, base
    for name in ("dstcnt_batched", "dstevx_batched", "dstevxv_batched", "dsyevxv_batched", "dsygvx_batched"):
        assert '{"%s",' % name in shim, name
    js = open(os.path.join(ROOT, "nd4js_amd", "js", "index.js")).read()
    for name in ("dstcnt_batched", "dstevx_batched", "dstevxv_batched", "dsyevxv_batched", "dsygvx_batched"):
        assert "native().%s(" % name in js, name
    # one checker per operation in nd4hip_args.h, called by both forms
    args = open(os.path.join(ROOT, "nd4js_amd", "csrc", "nd4hip_args.h")).read()
    api = open(os.path.join(ROOT, "nd4js_amd", "csrc", "nd4hip_api.hip")).read()
    host = open(os.path.join(ROOT, "nd4js_amd", "csrc", "nd4hip_host.hip")).read()
    assert "inline int nd4_args_sygvx(" in args and "ND4_ARGS(nd4_args_sygvx(" in api and "ND4_ARGS(nd4_args_sygvx(" in host
    for checker in ("nd4_args_stevxv", "nd4_args_syevxv"):
        assert "inline int %s(" % checker in args and "ND4_ARGS(%s(" % checker in api and "ND4_ARGS(%s(" % checker in host


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
    la.eigen_sym(S), la.eigenvals_sym(S), la.eigen_sym(S, interval=None), la.eigen_sym(S, reduction="hessenberg", interval=None)
    assert recorder.calls == ["nd4hip_dsyevd_batched"] * 4
    for a in recorder.args:
        assert a[:3] == (None, 3, 4) and len(a) == 6 and (a[5] is None) == (a is recorder.args[1])
    del recorder.calls[:], recorder.args[:]
    la.eigen_sym(S, subset=(1, 3)), la.eigenvals_sym(S, subset=(1, 3), interval=None)
    la.eigen_sym(S, subset=(1, 3), reduction="tridiag"), la.eigen_sym(S, reduction="tridiag")
    assert recorder.calls == ["nd4hip_dsyevx_batched_host"] * 2 + ["nd4hip_dsyevx_tr_batched_host", "nd4hip_dsyevd_tr_batched_host"]
    assert recorder.args[0][:5] == (None, 3, 4, 1, 3) and len(recorder.args[0]) == 8 and recorder.args[0][7] is not None
    assert recorder.args[1][7] is None and len(recorder.args[2]) == 8 and len(recorder.args[3]) == 6
    del recorder.calls[:], recorder.args[:]
    d, e = np.zeros((3, 4)), np.zeros((3, 3))
    lam, Z = la.tridiag_eigen(d, e)
    assert lam.shape == (3, 4) and Z.shape == (3, 4, 4)
    assert la.tridiag_eigenvals(d, e, subset=(1, 2), interval=None).shape == (3, 1)
    la.tridiag_count(d, e, np.zeros((3, 2)))
    assert recorder.calls == ["nd4hip_dstevx_batched_host"] * 2 + ["nd4hip_dstcnt_batched_host"]
    assert recorder.args[0][:5] == (None, 3, 4, 0, 4) and len(recorder.args[0]) == 9 and recorder.args[1][:5] == (None, 3, 4, 1, 2)
    assert recorder.args[1][8] is None and len(recorder.args[2]) == 8


def test_the_keyword_calls_the_new_entries(recorder):
    S = np.zeros((3, 4, 4))
    info = {}
    lam, V = la.eigen_sym(S, interval=(-1.0, 2.0), info=info)
    # (the recorder leaves kmax = 0: an empty selection)
    assert lam.shape == (3, 0) and V.shape == (3, 4, 0) and info["range"].shape == (3, 2) and info["range"].dtype == np.int32
    assert la.eigenvals_sym(S, interval=(-np.inf, np.inf)).shape == (3, 0)
    la.eigen_sym(S, interval=([0.0, 1.0, 2.0], 5.0), reduction="tridiag"), la.eigenvals_sym(S, interval=(0, 0), reduction="tridiag", algo="dc")
    assert recorder.calls == ["nd4hip_dsyevxv_batched_host"] * 2 + ["nd4hip_dsyevxv_tr_batched_host"] * 2
    for a, vectors in zip(recorder.args, (True, False, True, False)):
        # (handle, batch, N, kcap = N, bounds, S, lambda, V, range, kmax)
        assert len(a) == 10 and a[:4] == (None, 3, 4, 4) and (a[7] is not None) == vectors and a[8] is not None and a[9] is not None
    del recorder.calls[:], recorder.args[:]
    d, e = np.zeros((2, 3, 5)), np.zeros((2, 3, 4))
    lam, Z = la.tridiag_eigen(d, e, interval=(np.zeros((3,)), np.ones((2, 1))), info=info)
    assert lam.shape == (2, 3, 0) and Z.shape == (2, 3, 5, 0) and info["range"].shape == (2, 3, 2)
    assert la.tridiag_eigenvals(d, e, interval=(0.0, np.inf)).shape == (2, 3, 0)
    assert recorder.calls == ["nd4hip_dstevxv_batched_host"] * 2
    for a, vectors in zip(recorder.args, (True, False)):
        # (handle, batch, N, kcap = N, bounds, d, e, lambda, Z, range, kmax)
        assert len(a) == 11 and a[:4] == (None, 6, 5, 5) and (a[8] is not None) == vectors


def test_gen_routing(recorder):
    A, B = np.zeros((3, 4, 4)), np.zeros((4, 4))
    la.eigen_sym_gen(A, B), la.eigenvals_sym_gen(A, np.zeros((3, 4, 4))), la.eigen_sym_gen(A, B, subset=None, interval=None, reduction="hessenberg")
    la.eigen_sym_gen(A, B, algo="jacobi")
    assert recorder.calls == ["nd4hip_dsygvd_batched"] * 4
    for a, (algo, sb, vectors) in zip(recorder.args, ((0, 0, True), (0, 16, False), (0, 0, True), (1, 0, True))):
        assert len(a) == 10 and a[:4] == (None, algo, 3, 4) and a[6] == sb and (a[8] is not None) == vectors and (a[9] is not None) == (algo == 1)
    del recorder.calls[:], recorder.args[:]
    info = {}
    lam, X = la.eigen_sym_gen(A, B, subset=(1, 3))
    assert lam.shape == (3, 2) and X.shape == (3, 4, 2)
    assert la.eigenvals_sym_gen(A, B, subset=(0, 4), reduction="tridiag").shape == (3, 4)
    lam, X = la.eigen_sym_gen(A, np.zeros((3, 4, 4)), reduction="tridiag")
    assert lam.shape == (3, 4) and X.shape == (3, 4, 4)
    lam, X = la.eigen_sym_gen(A, B, interval=(0.0, [1.0, 2.0, 3.0]), info=info)
    assert lam.shape == (3, 0) and X.shape == (3, 4, 0) and info["range"].shape == (3, 2)
    assert la.eigenvals_sym_gen(A, B, interval=(0.0, 1.0), reduction="tridiag").shape == (3, 0)
    assert recorder.calls == ["nd4hip_dsygvx_batched_host"] * 5
    # (handle, reduction, select, batch, N, i0, i1, kcap, bounds, A, B, strideB, lambda, X, range, kmax)
    heads = [a[:8] + (a[11],) for a in recorder.args]
    assert heads == [(None, 0, 1, 3, 4, 1, 3, 0, 0), (None, 1, 1, 3, 4, 0, 4, 0, 0), (None, 1, 0, 3, 4, 0, 0, 0, 16), (None, 0, 2, 3, 4, 0, 0, 4, 0),
                     (None, 1, 2, 3, 4, 0, 0, 4, 0)]
    for a, (vectors, interval) in zip(recorder.args, ((True, False), (False, False), (True, False), (True, True), (False, True))):
        assert len(a) == 16 and (a[13] is not None) == vectors
        assert (a[8] is not None) == interval and (a[14] is not None) == interval and (a[15] is not None) == interval
    del recorder.calls[:]
    # an empty input reaches nothing
    assert la.eigen_sym_gen(np.zeros((0, 4, 4)), B, subset=(0, 2))[1].shape == (0, 4, 2)
    assert la.eigenvals_sym_gen(A, B, subset=(2, 2)).shape == (3, 0)
    assert la.eigen_sym_gen(np.zeros((2, 0, 0)), np.zeros((0, 0)), reduction="tridiag")[1].shape == (2, 0, 0)
    assert la.eigen_sym_gen(np.zeros((0, 4, 4)), B, interval=(0.0, 1.0))[0].shape == (0, 0)
    assert recorder.calls == []


def test_gen_argument_errors(recorder):
    from nd4js_amd import dev
    A, B = np.zeros((3, 4, 4)), np.eye(4)
    for fn in (la.eigen_sym_gen, la.eigenvals_sym_gen):
        for kw, text in (({"subset": (0, 1)}, "subset is not available with algo='jacobi'"),
                         ({"interval": (0.0, 1.0)}, "interval is not available with algo='jacobi'"),
                         ({"reduction": "tridiag"}, "reduction is not available with algo='jacobi'")):
            with pytest.raises(ValueError, match=text):
                fn(A, B, algo="jacobi", **kw)
        with pytest.raises(ValueError, match="interval and subset exclude each other"):
            fn(A, B, subset=(0, 1), interval=(0.0, 1.0))
        with pytest.raises(ValueError, match="subset must be"):
            fn(A, B, subset=(3, 2))
        with pytest.raises(ValueError, match="interval must satisfy lo <= hi"):
            fn(A, B, interval=(1.0, 0.0))
        with pytest.raises(ValueError, match="interval contains NaN"):
            fn(A, B, interval=(np.nan, 0.0), reduction="tridiag")
        with pytest.raises(ValueError, match="interval must broadcast"):
            fn(A, B, interval=(np.zeros(2), 0.0))
        with pytest.raises(ValueError, match="reduction must be None, 'hessenberg' or 'tridiag'"):
            fn(A, B, reduction="sytrd")
        with pytest.raises(ValueError, match="quadratic"):
            fn(np.zeros((2, 3)), B, subset=(0, 1))
    for fn in (dev.eigen_sym_gen, dev.eigenvals_sym_gen):
        for kw in ({"subset": (0, 1)}, {"interval": (0.0, 1.0)}, {"reduction": "tridiag"}):
            with pytest.raises(ValueError, match="not available with algo='jacobi'"):
                fn(None, None, algo="jacobi", **kw)
        with pytest.raises(ValueError, match="interval and subset exclude each other"):
            fn(None, None, subset=(0, 1), interval=(0.0, 1.0))
    assert recorder.calls == []


def test_the_bounds_that_reach_the_entry_point(monkeypatch):
    seen = []

    class Rec(_Recorder):
        def __getattr__(self, name):
            def call(*a):
                import ctypes
                seen.append(np.ctypeslib.as_array(ctypes.cast(a[4], ctypes.POINTER(ctypes.c_double)), shape=(a[1], 2)).copy())
                return 0
            return call if name.startswith("nd4hip_") else super().__getattr__(name)
    rec = Rec()
    monkeypatch.setattr(la._lib, "handle", lambda device=None: rec)
    la.eigenvals_sym(np.zeros((2, 3, 4, 4)), interval=([[1.0], [-np.inf]], [2.0, 3.0, np.inf]))
    want = [[1, 2], [1, 3], [1, np.inf], [-np.inf, 2], [-np.inf, 3], [-np.inf, np.inf]]
    assert np.array_equal(seen[0], np.array(want, dtype=np.float64))
    la.tridiag_eigenvals(np.zeros(4), np.zeros(3), interval=(-0.5, 0.5))
    assert np.array_equal(seen[1], [[-0.5, 0.5]])


def test_an_empty_call_reaches_nothing(recorder):
    info = {}
    lam, V = la.eigen_sym(np.zeros((0, 4, 4)), interval=(0.0, 1.0), info=info)
    assert lam.shape == (0, 0) and V.shape == (0, 4, 0) and info["range"].shape == (0, 2)
    lam, V = la.eigen_sym(np.zeros((2, 0, 0)), interval=(0.0, 1.0), reduction="tridiag")
    assert lam.shape == (2, 0) and V.shape == (2, 0, 0)
    lam, Z = la.tridiag_eigen(np.zeros((0, 4)), np.zeros((0, 3)), interval=(0.0, 1.0))
    assert lam.shape == (0, 0) and Z.shape == (0, 4, 0)
    assert recorder.calls == []


def test_argument_errors(recorder):
    S, d, e = np.zeros((3, 4, 4)), np.zeros((3, 4)), np.zeros((3, 3))
    calls = [lambda **kw: la.eigen_sym(S, **kw), lambda **kw: la.eigenvals_sym(S, **kw), lambda **kw: la.eigen_sym(S, reduction="tridiag", **kw),
             lambda **kw: la.tridiag_eigen(d, e, **kw), lambda **kw: la.tridiag_eigenvals(d, e, **kw)]
    for fn in calls:
        with pytest.raises(ValueError, match="interval and subset exclude each other"):
            fn(interval=(0.0, 1.0), subset=(0, 1))
        with pytest.raises(ValueError, match="interval must satisfy lo <= hi"):
            fn(interval=(1.0, 0.5))
        with pytest.raises(ValueError, match="interval must satisfy lo <= hi"):
            fn(interval=([0.0, 0.0, 2.0], [1.0, 1.0, 1.0]))
        for bad in ((np.nan, 1.0), (0.0, np.nan), ([0.0, np.nan, 0.0], 1.0)):
            with pytest.raises(ValueError, match="interval contains NaN"):
                fn(interval=bad)
        for bad in ((np.zeros(2), 1.0), (0.0, np.ones((3, 2))), (np.zeros((2, 3)), 1.0)):
            with pytest.raises(ValueError, match="interval must broadcast to the leading dimensions"):
                fn(interval=bad)
        for bad in (1.0, (1.0,), (0.0, 1.0, 2.0), "ab", ("a", "b")):
            with pytest.raises(ValueError, match="interval must be \\(lo, hi\\)"):
                fn(interval=bad)
    for fn in (la.eigen_sym, la.eigenvals_sym):
        with pytest.raises(ValueError, match="interval is not available with algo='jacobi'"):
            fn(S, algo="jacobi", interval=(0.0, 1.0))
        with pytest.raises(ValueError, match="quadratic"):
            fn(np.ones((2, 3)), interval=(0.0, 1.0))
        with pytest.raises(TypeError, match="must be float"):
            fn(np.ones((2, 2), dtype=np.complex128), interval=(0.0, 1.0))
    with pytest.raises(ValueError, match="e must have len\\(d\\) - 1 entries"):
        la.tridiag_eigen(d, d, interval=(0.0, 1.0))
    assert recorder.calls == []


def test_device_layer_refuses_alike():
    from nd4js_amd import dev
    for fn in (dev.eigen_sym, dev.eigenvals_sym):
        with pytest.raises(ValueError, match="interval is not available with algo='jacobi'"):
            fn(None, algo="jacobi", interval=(0.0, 1.0))
        with pytest.raises(ValueError, match="interval and subset exclude each other"):
            fn(None, subset=(0, 1), interval=(0.0, 1.0))
        with pytest.raises(TypeError, match="CUDA tensor"):
            fn(np.zeros((2, 2)), interval=(0.0, 1.0))
    for fn in (dev.tridiag_eigen, dev.tridiag_eigenvals):
        with pytest.raises(ValueError, match="interval and subset exclude each other"):
            fn(None, None, subset=(0, 1), interval=(0.0, 1.0))
        with pytest.raises(TypeError, match="CUDA tensor"):
            fn(np.zeros(2), np.zeros(1), interval=(0.0, 1.0))
