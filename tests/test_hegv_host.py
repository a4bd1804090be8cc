"""The Hermitian Cholesky factorisation, the complex triangular solves and the generalised Hermitian-definite eigenproblem
(herm_cholesky_decomp, herm_cholesky_solve, ztril_solve, herm_gen_reduce, eigen_herm_gen, eigenvals_herm_gen) without a GPU: the numpy
model of hegv_common.py inside the six bounds on the catalogue and against numpy's Cholesky, its exact cases, the committed LAPACK
values, the argument checks of the six new C operations in both forms, the header / exports / bindings, the argument and dtype errors
of la and dev, and which entry point each Python call reaches.

Largest shares of the six 1e-12 bounds the model has shown on the catalogue (N = 1 .. 300), in order: 2.9e-4, 1.1e-4, 8.3e-4, 1.2e-4,
7.0e-4, 9.9e-5."""
import os
import re

import numpy as np
import pytest

import hegv_common as G
import herm_common as X
from conftest import ROOT
from nd4js_amd import _lib, la


# ---- the model --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", G.SINGLES)
def test_model_inside_the_six_bounds(name):
    A, B = G.inputs(name)
    N = A.shape[-1]
    L, bad = G.chol_model(B)
    assert not bad
    s5 = G.chol_share(B, L)
    ref = np.linalg.cholesky(B)
    assert np.linalg.norm(L - ref) <= 1e-12 * np.linalg.cond(B) * np.linalg.norm(ref)   # two backward stable factors of the same B
    assert np.linalg.norm(ref @ np.conj(ref.T) - B) <= G.TOL * np.linalg.norm(B)          # numpy's own factor inside bound 5
    C = G.hegst_model(A, L)
    s4 = G.reduction_share(A, L, C)
    Y = G.rhs(name, 3)
    s6 = G.solve_share(B, G.potrs_model(L, Y), Y)
    lam, Xv = G.model(np.array(A), np.array(B))
    sh = G.check(A, B, lam, Xv, G.golden(name), "model " + name)
    print("model %s: shares of bounds 4-6: %.3g %.3g %.3g" % (name, s4, s5, s6))
    assert s4 <= 1.0 and s5 <= 1.0 and s6 <= 1.0 and max(sh) <= 1.0
    if N >= 7:
        G.check(A, B, lam[2:7], Xv[:, 2:7], G.golden(name), "model %s subset" % name, subset=(2, 7))


def test_goldens_are_sound_and_what_scipy_returns():
    assert sorted(f[:-len(".Lam.npy")] for f in os.listdir(G.GOLDEN)) == sorted(G.NAMES)
    for name in G.NAMES:
        A, B = G.inputs(name)
        lam = G.golden(name)
        assert lam.shape == A.shape[:-1] and lam.dtype == np.float64 and np.all(np.isfinite(lam)) and np.all(np.diff(lam, axis=-1) <= 0)
    try:
        import scipy.linalg
    except ImportError:
        return
    for name in ("gram_33", "graded_65", "shared_3x40"):
        A, B = G.inputs(name)
        N = A.shape[-1]
        for got, (a, b) in zip(G.golden(name).reshape(-1, N), G.members(A, B)):
            ref = scipy.linalg.eigh(a, b, eigvals_only=True)[::-1]
            sv = np.linalg.svd(b, compute_uv=False)
            assert np.all(np.abs(got - ref) <= G.TOL * (np.linalg.norm(a) / sv[-1] + sv[0] / sv[-1] * np.abs(ref)))


def test_model_product_and_division_orders():
    # s - a conj(b) with a = 1 + 2i, b = 3 + 4i: a conj(b) = 11 + 2i
    assert G.nmsc(0.0, 0.0, 1.0, 2.0, 3.0, 4.0) == (-11.0, -2.0)
    # the order: Re (s - a_re b_re) - a_im b_im; 2^53 + 1 is not representable, so the first subtraction decides
    big = 2.0 ** 53
    assert G.nmsc(big, 0.0, -1.0, 1.0, 1.0, big)[0] == (big + 1.0) - big and G.nmsc(big, 0.0, -1.0, 1.0, 1.0, big)[0] == 0.0
    assert G.div(3.0, -0.0, 2.0, 0.0) == (1.5, -0.0) and np.signbit(G.div(3.0, -0.0, 2.0, 0.0)[1])
    xr, xi = G.div(1.0, 2.0, 3.0, 4.0)                                       # Smith's other branch: (1 + 2i) / (3 + 4i) = 0.44 + 0.08i
    assert abs(xr - 0.44) <= 1e-16 and abs(xi - 0.08) <= 1e-16
    xr, xi = G.div(1.0, 2.0, 4.0, 3.0)
    assert abs(complex(xr, xi) - (1 + 2j) / (4 + 3j)) <= 1e-16


@pytest.mark.parametrize("N", [1, 5, 33, 70])
def test_model_identity_b_is_exact(N):
    A = np.array(X.dense(N)[0]) if N > 1 else np.array([[0.75 + 0j]])
    I = np.eye(N, dtype=np.complex128)
    L, C, bad = G.reduce_model(A, I)
    assert not bad and X.same_bits(L, I) and X.same_bits(C, np.tril(G.mirror(A)))
    Y = G.cmatrix(77 + N, N, N)
    assert X.same_bits(G.solve_model(L, Y, True), Y) and X.same_bits(G.solve_model(L, Y), Y)


def test_model_diagonal_b_with_powers_of_two():
    N = 33
    A, B = np.array(X.dense(N)[0]), G.diag2(N)
    s = np.sqrt(np.diagonal(B).real)                                        # exact for even exponents only: the entries take two roundings
    L, C, bad = G.reduce_model(A, B)
    assert not bad and X.same_bits(L, np.diag(np.sqrt(np.diagonal(B).real)).astype(np.complex128))
    T = np.tril(G.mirror(A))                                                # c_ic = conj(conj(a_ic) / l_cc) / l_ii: the column's divisor first,
    want = G._join(T.real / s[None, :] / s[:, None], T.imag / s[None, :] / s[:, None])   # each part on its own (not numpy's complex division)
    assert X.same_bits(C, want)


def test_model_power_of_two_scaling():
    N = 17
    A, B = (np.array(m) for m in G.inputs("gram_17"))
    L, C, _ = G.reduce_model(A, B)
    for k in (-500, 500):
        L2, C2, bad = G.reduce_model(X._ldexp(A, k), B)
        assert not bad and X.same_bits(L2, L) and X.same_bits(C2, X._ldexp(C, k))
    for j in (-200, 200):
        L2, C2, bad = G.reduce_model(A, X._ldexp(B, 2 * j))
        assert not bad and X.same_bits(L2, X._ldexp(L, j)) and X.same_bits(C2, X._ldexp(C, -2 * j))
        Y = G.cmatrix(5, N, N)
        assert X.same_bits(G.solve_model(L2, Y, True), X._ldexp(G.solve_model(L, Y, True), -j))
    assert G.model(np.array([[3.0 + 9j]]), np.array([[4.0 - 2j]]))[0][0] == 0.75 and G.model(np.array([[3.0 + 0j]]), np.array([[4.0 + 0j]]))[1][0, 0] == 0.5


@pytest.mark.parametrize("fill", [np.nan, 1e300])
def test_model_reads_only_the_lower_triangles_and_real_diagonals(fill):
    A, B = (np.array(m) for m in G.inputs("gram_17"))
    L, C, _ = G.reduce_model(A, B)
    L2, C2, bad = G.reduce_model(G.with_unread(A, fill), G.with_unread(B, fill))
    assert not bad and X.same_bits(L, L2) and X.same_bits(C, C2)


def test_model_flags_every_bad_radicand():
    B = np.array(G.inputs("gram_17")[1])
    for spoil in (lambda b: b.__setitem__((8, 8), -1.0), lambda b: b.__setitem__((0, 0), 0.0), lambda b: b.__setitem__((16, 0), np.nan)):
        b = np.array(B)
        spoil(b)
        assert G.chol_model(b)[1]
    b = np.eye(5, dtype=np.complex128)
    b[4, 4] = 0.0                                                           # the exact zero in the last pivot: no NaN anywhere
    L, bad = G.chol_model(b)
    assert bad and np.all(np.isfinite(L))


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------
def test_both_forms_refuse_alike_before_the_handle():
    assert {r[0] for r in G.ROWS} == {n[len("nd4hip_"):] for n in G.NEW}
    for op in {r[0] for r in G.ROWS}:
        assert {"extent", "empty", "null"} <= {r[1] for r in G.ROWS if r[0] == op}
    assert G.mismatches(None) == []


def test_a_valid_call_without_a_handle_is_refused():
    lib = _lib.load()
    for name, args in G.VALID.items():
        for form in ("_host", "_dev"):
            assert getattr(lib, "nd4hip_" + name + form)(None, *args) == -1
            assert lib.nd4hip_last_error().decode() == "nd4hip_%s: NULL handle" % name


def test_header_exports_bindings_and_build_list():
    src = open(os.path.join(ROOT, "include", "nd4hip.h")).read()
    lib = _lib.load()
    for base in G.NEW:
        for form in ("_host", "_dev"):
            assert re.search(r"\bint %s%s\s*\(" % (base, form), src), base + form
            assert hasattr(lib, base + form) and base + form in _lib.SIGNATURES
        assert _lib.SIGNATURES[base + "_host"] == _lib.SIGNATURES[base + "_dev"]
        assert base not in _lib.SIGNATURES and not hasattr(lib, base)
    from nd4js_amd import build
    assert "hegv.hip" in build.HIP_SOURCES and os.path.exists(os.path.join(build.CSRC, "hegv.hip"))
    assert build.FILE_FLAGS["hegv.hip"] == ["-ffp-contract=off"]


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
    c = np.complex128
    A, B, B1 = np.zeros((3, 4, 4), dtype=c), np.zeros((3, 4, 4), dtype=c), np.zeros((4, 4), dtype=c)
    L = la.herm_cholesky_decomp(B)
    assert L.shape == (3, 4, 4) and L.dtype == c and recorder.calls == ["nd4hip_zpotrf_batched_host"] and recorder.args[0][:3] == (None, 3, 4)
    del recorder.calls[:], recorder.args[:]
    Y = np.ones((3, 4, 2))                                                  # float64: promoted
    for fn, name, lead in ((la.herm_cholesky_solve, "nd4hip_zpotrs_batched_host", (None, 3, 4, 2)),
                           (la.ztril_solve, "nd4hip_ztrsm_batched_host", (None, 3, 4, 2, 0)),
                           (lambda l, y: la.ztril_solve(l, y, adjoint=True), "nd4hip_ztrsm_batched_host", (None, 3, 4, 2, 1))):
        for l, stride in ((B, 16), (B1, 0)):                               # a stacked L, and one for all
            out = fn(l, Y)
            assert out.shape == (3, 4, 2) and out.dtype == c and np.array_equal(out, Y)
            assert recorder.calls == [name] and recorder.args[0][:len(lead)] == lead and recorder.args[0][len(lead) + 1] == stride
            assert len(recorder.args[0]) == len(lead) + (4 if "zpotrs" in name else 3)   # zpotrs: (Y, X), the same array here
            del recorder.calls[:], recorder.args[:]
    for l, stride in ((B, 16), (B1, 0)):
        assert la.herm_gen_reduce(A, l).shape == (3, 4, 4)
        assert recorder.calls == ["nd4hip_zhegst_batched_host"] and recorder.args[0][:3] == (None, 3, 4) and recorder.args[0][5] == stride
        del recorder.calls[:], recorder.args[:]
    for b, stride in ((B, 16), (B1, 0)):
        lam, Xv = la.eigen_herm_gen(A, b)
        assert lam.shape == (3, 4) and lam.dtype == np.float64 and Xv.shape == (3, 4, 4) and Xv.dtype == c
        assert la.eigenvals_herm_gen(A, b).shape == (3, 4)
        assert recorder.calls == ["nd4hip_zhegvd_batched_host"] * 2
        assert recorder.args[0][:3] == (None, 3, 4) and recorder.args[0][5] == stride and recorder.args[0][7] is not None and recorder.args[1][7] is None
        del recorder.calls[:], recorder.args[:]
        lam, Xv = la.eigen_herm_gen(A, b, subset=(1, 3))
        assert lam.shape == (3, 2) and Xv.shape == (3, 4, 2)
        assert la.eigenvals_herm_gen(A, b, subset=(0, 4)).shape == (3, 4)
        assert recorder.calls == ["nd4hip_zhegvx_batched_host"] * 2
        assert recorder.args[0][:5] == (None, 3, 4, 1, 3) and recorder.args[0][7] == stride and recorder.args[0][9] is not None
        assert recorder.args[1][:5] == (None, 3, 4, 0, 4) and recorder.args[1][9] is None
        del recorder.calls[:], recorder.args[:]


def test_an_empty_call_reaches_nothing(recorder):
    c = np.complex128
    lam, Xv = la.eigen_herm_gen(np.eye(4, dtype=c), np.eye(4, dtype=c), subset=(2, 2))
    assert lam.shape == (0,) and Xv.shape == (4, 0)
    assert la.eigenvals_herm_gen(np.zeros((0, 4, 4), dtype=c), np.zeros((4, 4), dtype=c)).shape == (0, 4)
    assert la.herm_cholesky_decomp(np.zeros((0, 3, 3), dtype=c)).shape == (0, 3, 3)
    assert la.herm_cholesky_decomp(np.zeros((2, 0, 0), dtype=c)).shape == (2, 0, 0)
    assert la.herm_cholesky_solve(np.zeros((3, 3), dtype=c), np.zeros((3, 0), dtype=c)).shape == (3, 0)
    assert la.ztril_solve(np.zeros((3, 3), dtype=c), np.zeros((0, 3, 2), dtype=c)).shape == (0, 3, 2)
    assert la.herm_gen_reduce(np.zeros((0, 3, 3), dtype=c), np.zeros((3, 3), dtype=c)).shape == (0, 3, 3)
    assert recorder.calls == []


def test_argument_errors(recorder):
    c = np.complex128
    H = np.eye(4, dtype=c)
    for fn in (la.eigen_herm_gen, la.eigenvals_herm_gen, la.herm_gen_reduce):
        for bad in ((np.eye(4), H), (H, np.eye(4)), (np.eye(4, dtype=np.int32), H)):
            with pytest.raises(TypeError, match="eigen_sym_gen"):
                fn(*bad)
        for bad in ((H.astype(np.complex64), H), (H, H.astype(np.complex64))):
            with pytest.raises(TypeError, match="only complex128"):
                fn(*bad)
        for bad in ((np.ones((2, 3), dtype=c), H), (H, np.ones((4, 3), dtype=c))):
            with pytest.raises(ValueError, match="quadratic"):
                fn(*bad)
        for bad in ((np.ones(3, dtype=c), H), (H, np.ones(4, dtype=c))):
            with pytest.raises(ValueError, match="at least 2"):
                fn(*bad)
        for bad in ((H, np.eye(3, dtype=c)), (np.zeros((2, 4, 4), dtype=c), np.zeros((3, 4, 4), dtype=c)), (H, np.zeros((2, 4, 4), dtype=c))):
            with pytest.raises(ValueError, match=r"shape must be A.shape or A.shape\[-2:\]"):
                fn(*bad)
        with pytest.raises(ValueError, match="N <= 2048"):
            fn(np.zeros((2049, 2049), dtype=c), np.zeros((2049, 2049), dtype=c))
    for fn in (la.eigen_herm_gen, la.eigenvals_herm_gen):
        for bad in ((3, 2), (0, 5), (-1, 2), (0.5, 2), (1,), 3, "ab"):
            with pytest.raises(ValueError, match=r"subset must be \(i0, i1\) with 0 <= i0 <= i1 <= N"):
                fn(H, H, subset=bad)
    with pytest.raises(TypeError, match="cholesky_decomp"):
        la.herm_cholesky_decomp(np.eye(4))
    with pytest.raises(TypeError, match="only complex128"):
        la.herm_cholesky_decomp(np.eye(4, dtype=np.complex64))
    with pytest.raises(ValueError, match="quadratic"):
        la.herm_cholesky_decomp(np.ones((2, 3), dtype=c))
    with pytest.raises(ValueError, match="at least 2"):
        la.herm_cholesky_decomp(np.ones(3, dtype=c))
    with pytest.raises(ValueError, match="N <= 2048"):
        la.herm_cholesky_decomp(np.zeros((2049, 2049), dtype=c))
    Y = np.zeros((2, 4, 3), dtype=c)
    for fn in (la.herm_cholesky_solve, la.ztril_solve):
        with pytest.raises(TypeError, match="cholesky_solve / tril_solve"):
            fn(np.eye(4), Y)
        with pytest.raises(TypeError, match="only complex128"):
            fn(np.eye(4, dtype=np.complex64), Y)
        with pytest.raises(TypeError, match="Y must be complex128 or float64"):
            fn(H, Y.astype(np.complex64))
        with pytest.raises(TypeError, match="Y must be complex128 or float64"):
            fn(H, np.zeros((4, 3), dtype=np.int32))
        for bad in ((np.ones((4, 3), dtype=c), Y), (H, np.zeros((2, 5, 3), dtype=c)), (H, np.zeros(4, dtype=c)), (np.ones(4, dtype=c), Y),
                    (np.zeros((3, 4, 4), dtype=c), Y), (np.zeros((2, 4, 4), dtype=c), np.zeros((4, 3), dtype=c))):
            with pytest.raises(ValueError, match=fn.__name__):
                fn(*bad)
    assert recorder.calls == []


def test_device_layer_refuses_alike():
    import torch
    from nd4js_amd import dev
    z, r = torch.zeros((2, 2), dtype=torch.complex128), torch.zeros((2, 2), dtype=torch.float64)
    for fn in (dev.eigen_herm_gen, dev.eigenvals_herm_gen, dev.herm_gen_reduce):
        with pytest.raises(TypeError, match="eigen_sym_gen"):
            fn(r, z)
        with pytest.raises(TypeError, match="eigen_sym_gen"):
            fn(r, r)
        with pytest.raises(TypeError, match="only complex128"):
            fn(z.to(torch.complex64), z)
        with pytest.raises(TypeError, match="CUDA tensor"):
            fn(z, z)
        with pytest.raises(TypeError, match="CUDA tensor"):
            fn(np.zeros((2, 2), dtype=np.complex128), z)
    with pytest.raises(TypeError, match="cholesky_decomp"):
        dev.herm_cholesky_decomp(r)
    with pytest.raises(TypeError, match="only complex128"):
        dev.herm_cholesky_decomp(z.to(torch.complex64))
    with pytest.raises(TypeError, match="CUDA tensor"):
        dev.herm_cholesky_decomp(z)
    for fn in (dev.herm_cholesky_solve, dev.ztril_solve):
        with pytest.raises(TypeError, match="cholesky_solve / tril_solve"):
            fn(r, z)
        with pytest.raises(TypeError, match="CUDA tensor"):
            fn(z, z)


def test_the_real_family_still_refuses_complex_input():
    z = np.eye(3, dtype=np.complex128)
    for call in (lambda: la.cholesky_decomp(z), lambda: la.cholesky_solve(z, z), lambda: la.tril_solve(z, z), lambda: la.triu_solve(z, z)):
        with pytest.raises(TypeError, match="complex"):
            call()
    for fn in (la.eigen_sym_gen, la.eigenvals_sym_gen):
        with pytest.raises(TypeError, match="must be float"):
            fn(z, z)
