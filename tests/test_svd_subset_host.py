"""CPU checks of the selected-singular-triplet route: the numpy model of tests/svd_subset_common.py inside its bounds on the
catalogue sweep, the fallback rule, the argument contract of the two operations in both forms with a NULL handle, header, exports
and bindings, and what the Python layers call (the binding replaced by a recorder)."""
import os
import re

import numpy as np
import pytest

import svd_dc_common as D
import svd_subset_common as C
from nd4js_amd import _lib, la

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUNS = C.sweep_runs()
# the runs the rule sends to the full solver: every run of the sweep that violates a bound without it is among them
FLAGGED_NAMES = {"rand_64_64", "rand_129_129", "rand_129_130", "rand_257_257", "rand_257_258", "eqdiag_e0", "eqdiag_e1e-3", "zero_8",
                 "quad_16_weak", "quad_16_singular", "sing_69", "twin_34_zeros", "twin_34_zeros_b2", "zero_middle_69", "graded_40"}


# ---- the model ----------------------------------------------------------------------------------------------------------------------
def test_interleave_and_the_golub_kahan_spectrum():
    d, e = np.array([3.0, -2.0, 1.0]), np.array([0.5, 0.25, -4.0])
    assert C.interleave(d, e).tolist() == [3.0, 0.5, -2.0, 0.25, 1.0, -4.0] and C.interleave(d, e[:2]).tolist() == [3.0, 0.5, -2.0, 0.25, 1.0]
    for ee in (e, e[:2]):
        b = C.interleave(d, ee)
        T = np.diag(b, 1) + np.diag(b, -1)
        sv = np.linalg.svd(D.bidiag_dense(d, ee), compute_uv=False)
        assert np.allclose(np.linalg.eigvalsh(T)[::-1][:3], sv, rtol=0, atol=1e-14)


def test_the_sweep_has_every_catalogue_entry_but_one():
    names = {n for n, _ in RUNS}
    assert names == set(D.BIDIAG_CASES) | set(D.PATH_CASES) - {"max_2048"} and 140 <= len(RUNS) <= 150
    for K in (1, 2, 3, 10, 300):
        subs = C.subsets_of(K)
        assert (0, min(8, K)) in subs and (0, K) in subs and (max(K - 8, 0), K) in subs and all(0 <= a < b <= K for a, b in subs)
    assert (149, 152) in C.subsets_of(300)


@pytest.mark.parametrize("name", sorted({n for n, _ in RUNS}))
def test_model_inside_the_bounds(name):
    B, ref = C.case_reference(name)
    for n, sub in RUNS:
        if n != name:
            continue
        U2, sv, V2, info = C.case_model(name, sub)
        sh = C.check_triplets(B, U2, sv, V2, ref[sub[0]:sub[1]], "%s %r" % (name, sub))
        print("%s %r fallback %d: shares %s" % (name, sub, info["fallback"], " ".join("%.3g" % s for s in sh)))
        assert C.same_bits(C.case_model(name, sub, False)[1], sv)
        if not info["fallback"]:
            assert max(sh) <= 2e-2                              # an unflagged run is nowhere near a bound
            assert np.abs(np.sum(U2 * U2, axis=0) - 1.0).max() <= 1e-14 and np.abs(np.sum(V2 * V2, axis=1) - 1.0).max() <= 1e-14


def test_the_rule_flags_the_predicted_runs():
    flagged = [(n, s) for n, s in RUNS if C.case_model(n, s)[3]["fallback"]]
    assert len(flagged) <= 32
    assert {n for n, _ in flagged} == FLAGGED_NAMES
    for hard in (("graded_40", (0, 8)), ("graded_40", (19, 22)), ("eqdiag_e0", (2, 10)), ("zero_8", (3, 6)), ("rand_64_64", (56, 64)),
                 ("rand_64_64", (0, 64))):
        assert hard in flagged
    # what each part of the rule catches: B = 0; two small values; a lopsided split with well separated values
    assert C.case_model("zero_8", (3, 6))[3]["split_min"] is None
    _, _, _, info = C.case_model("rand_64_64", (56, 64))
    assert C.values_flag(info["lams"], info["prepared"]) and info["split_min"] > 0.49
    _, _, _, info = C.case_model("graded_40", (19, 22))
    assert not C.values_flag(info["lams"], info["prepared"]) and info["split_min"] < 0.5 - 1e-3 or C.values_flag(info["lams"], info["prepared"])


def test_without_the_rule_the_flagged_runs_break_the_bounds():
    """the rule is needed: the iteration's own vectors of a flagged run miss a bound for at least graded_40, eqdiag_e0 and zero_8"""
    import eigsym_subset_common as S
    for name, sub in (("graded_40", (0, 40)), ("eqdiag_e0", (0, 10))):
        d, e = C.case_input(name)
        B, ref = C.case_reference(name)
        sv, lams, p = C.values(d, e, sub)
        head, shift = S.clusters(lams, p["g"])
        Z = S.start_vectors(len(d) + len(e) + 1, *sub)
        for r in range(3):
            Z = S.orth(S.factor_solve(p, shift, Z), head, r == 2)
        U2, V2, _ = C.split(Z)
        assert max(C.shares(B, U2, sv, V2, ref[sub[0]:sub[1]])) > 1.0, name


def test_values_contract():
    for name in ("zero_8", "quad_16_singular", "identity_16", "graded_40"):
        sv = C.case_model(name, (0, len(C.case_input(name)[0])), False)[1]
        assert np.all(sv >= 0.0) and not np.any(np.signbit(sv)) and np.all(np.diff(sv) <= 0)
    U2, sv, V2, _ = C.bidiag_svd_model(np.ones(4), np.ones(3), (2, 2))
    assert U2.shape == (4, 0) and sv.shape == (0,) and V2.shape == (0, 4)
    d, e = C.case_input("rand_17_18")
    for m in (500, -500):                                       # exact scaling by a power of two
        a, b = C.values(d, e, (3, 9))[0], C.values(np.ldexp(d, m), np.ldexp(e, m), (3, 9))[0]
        assert C.same_bits(np.ldexp(a, m), b)


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------
P, Q, Z, ROWS, NEW = C.P, C.Q, C.Z, C.ROWS, C.NEW


def test_both_forms_refuse_alike_before_the_handle():
    assert {"nd4hip_" + r[0] for r in ROWS} == set(NEW[:2])
    for op in {r[0] for r in ROWS}:
        assert {"extent", "selector", "empty", "null"} <= {r[1] for r in ROWS if r[0] == op}
    assert C.mismatches(None) == []


def test_a_valid_call_without_a_handle_is_refused():
    lib = _lib.load()
    for name, args in (("dbdsvdx_batched", (1, 1, 1, 0, 1, P, Z, Z, P, Z, Z)), ("dbdsvdx_batched", (1, 2, 3, 0, 2, P, P, P, P, P, Q)),
                       ("dgesvdx_batched", (1, 2, 3, 0, 1, P, Z, P, Z, Z)), ("dgesvdx_batched", (1, 3, 2, 1, 2, P, P, P, P, Q))):
        for form in ("_host", "_dev"):
            assert getattr(lib, "nd4hip_" + name + form)(None, *args) == -1
            assert lib.nd4hip_last_error().decode() == "nd4hip_%s: NULL handle" % name
    assert lib.nd4hip_dgesvdx_last_stages(None, None, 0) == -1


def test_header_exports_and_bindings():
    src = open(os.path.join(ROOT, "include", "nd4hip.h")).read()
    lib = _lib.load()
    for base in NEW[:2]:
        for form in ("_host", "_dev"):
            assert re.search(r"\bint %s%s\s*\(" % (base, form), src), base + form
            assert hasattr(lib, base + form) and base + form in _lib.SIGNATURES
        assert base not in _lib.SIGNATURES                      # the pair is (X_host, X_dev), not (X, X_dev): see the header
    assert re.search(r"\bint nd4hip_dgesvdx_last_stages\s*\(", src) and "nd4hip_dgesvdx_last_stages" in _lib.SIGNATURES
    assert "#define ND4HIP_SVDX_STAGES %d" % len(_lib.Handle.SVD_SUBSET_STAGES) in src
    shim = open(os.path.join(ROOT, "nd4js_amd", "csrc", "napi_shim.c")).read()
    for base in NEW[:2]:                                        # the N-API table binds both forms and exports one function each
        assert '"%s_host"' % base in shim and '"%s_dev"' % base in shim and '{"%s", NULL' % base[len("nd4hip_"):] in shim


# ---- the Python layers ----------------------------------------------------------------------------------------------------------
class _Recorder:
    """stands in for the handle: records the entry points that are called with their arguments, answers 0"""

    def __init__(self):
        self.calls, self.args, self.ptr, self.lib = [], [], None, self

    def __getattr__(self, name):
        if not name.startswith("nd4hip_"):
            raise AttributeError(name)
        return lambda *a: (self.calls.append(name), self.args.append(a)) and 0

    def svd_last_info(self):
        return {"rotations": 0}


@pytest.fixture
def recorder(monkeypatch):
    rec = _Recorder()
    monkeypatch.setattr(la._lib, "handle", lambda device=None: rec)
    return rec


def test_calls_without_the_keyword_keep_their_entry_points(recorder):
    A, d, e = np.zeros((3, 4, 6)), np.ones((2, 5)), np.ones((2, 5))
    la.svd_decomp(A), la.svd_decomp(A, algo="jacobi"), la.svd_decomp(A, algo="dc"), la.svd_decomp(A, subset=None), la.svd_dc(A)
    assert recorder.calls == ["nd4hip_dgesvdj_batched"] * 2 + ["nd4hip_dgesdd_batched"] + ["nd4hip_dgesvdj_batched"] * 2
    assert recorder.args[2][1:4] == (3, 4, 6) and len(recorder.args[2]) == 8 and len(recorder.args[0]) == 10
    del recorder.calls[:], recorder.args[:]
    U2, sv, V2 = la.bidiag_svd(d, e)
    assert recorder.calls == ["nd4hip_dbdsdc_batched"] and recorder.args[0][1:4] == (2, 5, 6) and len(recorder.args[0]) == 9
    assert U2.shape == (2, 5, 5) and sv.shape == (2, 5) and V2.shape == (2, 6, 6)
    la.bidiag_svd(d, e, None, None)                             # device and subset by position: still today's call
    assert recorder.calls == ["nd4hip_dbdsdc_batched"] * 2


def test_calls_with_the_keyword_reach_the_new_entry_points(recorder):
    A, d, e = np.zeros((3, 4, 6)), np.ones((2, 5)), np.ones((2, 5))
    info = {}
    U, sv, V = la.svd_decomp(A, subset=(1, 3), info=info)
    assert U.shape == (3, 4, 2) and sv.shape == (3, 2) and V.shape == (3, 2, 6) and info["fallback"].shape == (3,)
    assert la.svd_decomp(A, subset=(0, 4), algo="dc")[1].shape == (3, 4)
    assert la.svd_vals(A).shape == (3, 4) and la.svd_vals(A.transpose(0, 2, 1), subset=(0, 1)).shape == (3, 1)
    assert recorder.calls == ["nd4hip_dgesvdx_batched_host"] * 4
    assert recorder.args[0][1:6] == (3, 4, 6, 1, 3) and recorder.args[0][10].value is not None and recorder.args[1][10] is None
    assert recorder.args[2][7] is None and recorder.args[2][9] is None and recorder.args[3][1:6] == (3, 6, 4, 0, 1)
    del recorder.calls[:], recorder.args[:]
    U2, sv, V2 = la.bidiag_svd(d, e, subset=(0, 3))
    assert U2.shape == (2, 5, 3) and sv.shape == (2, 3) and V2.shape == (2, 3, 6)
    assert la.bidiag_svdvals(d, e).shape == (2, 5) and la.bidiag_svdvals(d, e[:, :4], subset=(4, 5)).shape == (2, 1)
    assert recorder.calls == ["nd4hip_dbdsvdx_batched_host"] * 3
    assert recorder.args[0][1:6] == (2, 5, 6, 0, 3) and recorder.args[1][1:6] == (2, 5, 6, 0, 5) and recorder.args[2][1:6] == (2, 5, 5, 4, 5)
    assert recorder.args[1][8] is None and recorder.args[1][10] is None


def test_an_empty_subset_makes_no_device_call(recorder):
    U, sv, V = la.svd_decomp(np.eye(4), subset=(2, 2))
    assert U.shape == (4, 0) and sv.shape == (0,) and V.shape == (0, 4)
    U2, sv, V2 = la.bidiag_svd(np.ones(5), np.ones(4), subset=(0, 0))
    assert U2.shape == (5, 0) and sv.shape == (0,) and V2.shape == (0, 5)
    assert la.svd_vals(np.zeros((2, 0, 3))).shape == (2, 0) and recorder.calls == []


def test_argument_errors(recorder):
    A = np.eye(4)
    for fn in (la.svd_decomp, la.svd_vals):
        for bad in ((3, 2), (-1, 2), (0, 5), (0,), (0, 1, 2), 3, (0.5, 2), "ab"):
            with pytest.raises(ValueError, match="subset must be"):
                fn(A, subset=bad)
        with pytest.raises(TypeError, match="A.dtype must be float"):
            fn(A + 1j, subset=(0, 1))
        with pytest.raises(ValueError, match="A.ndim must be at least 2"):
            fn(np.ones(3), subset=(0, 1))
        with pytest.raises(ValueError, match=r"min\(M, N\) <= 2048"):
            fn(np.zeros((2049, 2049)), subset=(0, 1))
    with pytest.raises(ValueError, match="subset is not available with algo='jacobi'"):
        la.svd_decomp(A, algo="jacobi", subset=(0, 1))
    with pytest.raises(ValueError, match="algo must be"):
        la.svd_decomp(A, algo="qr", subset=(0, 1))
    for fn in (la.bidiag_svd, la.bidiag_svdvals):
        with pytest.raises(ValueError, match="same leading dimensions"):
            fn(np.ones((2, 5)), np.ones((3, 4)), subset=(0, 1))
        with pytest.raises(ValueError, match=r"e must have len\(d\) - 1 or len\(d\) entries"):
            fn(np.ones(5), np.ones(6), subset=(0, 1))
        with pytest.raises(ValueError, match="subset must be"):
            fn(np.ones(5), np.ones(4), subset=(2, 6))
        with pytest.raises(ValueError, match="K <= 2048"):
            fn(np.ones(2049), np.ones(2048), subset=(0, 1))
    assert recorder.calls == []


def test_device_layer_refuses_before_it_touches_a_tensor():
    from nd4js_amd import dev
    with pytest.raises(ValueError, match="subset is not available with algo='jacobi'"):
        dev.svd_decomp(None, algo="jacobi", subset=(0, 1))
    with pytest.raises(ValueError, match="algo must be"):
        dev.svd_decomp(None, algo="qr", subset=(0, 1))
    for fn in (dev.svd_vals, lambda A: dev.svd_decomp(A, subset=(0, 1))):
        with pytest.raises(TypeError, match="contiguous float64 CUDA tensor"):
            fn(np.eye(3))
    for fn in (dev.bidiag_svdvals, lambda d, e: dev.bidiag_svd(d, e, subset=(0, 1))):
        with pytest.raises(TypeError, match="contiguous float64 CUDA tensor"):
            fn(np.ones(3), np.ones(2))
