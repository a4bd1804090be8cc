"""CPU tests of the DGEMM checker itself (tests/gemm_common.py): a check that cannot fail is worth nothing.

The reference is pinned to exact rational arithmetic, correct float64 products (numpy's and the oracle's) must pass the bound check,
and a list of wrong products, each of the kind a kernel edge bug produces, must be rejected by it. The last tests pin a Python model
of the tiled kernel's workgroup -> tile map and the coverage of the rank-k case selection that test_gpu_gemm_paths.py runs."""
from fractions import Fraction

import numpy as np
import pytest

import oracle
import gemm_common as gc
from gemm_common import LD, U

TRANSPOSES = [(0, 0), (1, 0), (0, 1), (1, 1)]


def _operands(seed, ta, tb, M, N, K, family=gc.uniform):
    A = family(seed, K, M) if ta else family(seed, M, K)
    B = family(seed + 1, N, K) if tb else family(seed + 1, K, N)
    return A, B, family(seed + 2, M, N)


# --------------------------------------------------------------------------------------------------------------------- reference
def _fraction_gemm(ta, tb, alpha, A, B, beta, C0):
    a, b = gc.op(ta, A), gc.op(tb, B)
    M, K = a.shape
    N = b.shape[1]
    fa = [[Fraction(float(a[i, k])) for k in range(K)] for i in range(M)]
    fb = [[Fraction(float(b[k, j])) for j in range(N)] for k in range(K)]
    al, be = Fraction(alpha), Fraction(beta)
    ref = [[al * sum(fa[i][k] * fb[k][j] for k in range(K)) + be * Fraction(float(C0[i, j])) for j in range(N)] for i in range(M)]
    env = [[abs(al) * sum(abs(fa[i][k] * fb[k][j]) for k in range(K)) + abs(be) * abs(Fraction(float(C0[i, j]))) for j in range(N)]
           for i in range(M)]
    return ref, env


def _to_fraction(x):
    """exact value of a longdouble (64-bit mantissa: two float64 pieces hold it) or of a float64"""
    hi = float(x)
    return Fraction(hi) + Fraction(float(x - LD(hi)))


@pytest.mark.parametrize("force_dot2", [False, True], ids=["longdouble", "dot2"])
@pytest.mark.parametrize("ta,tb", TRANSPOSES)
@pytest.mark.parametrize("M,N,K,alpha,beta", [(12, 11, 40, 0.75, -0.5), (3, 5, 1, -1.0, 1.0), (7, 2, 17, 1.0, 0.0), (1, 1, 33, -1.25, 0.5)])
def test_reference_against_exact_rationals(ta, tb, M, N, K, alpha, beta, force_dot2):
    """|ref - exact| <= 2^-60 E elementwise, for the longdouble product and for the Dot2 pair that replaces it on a host whose
    longdouble is only a double; the envelope to the same accuracy"""
    A, B, C0 = _operands(900 + K, ta, tb, M, N, K)
    ref, E = gc.ref_gemm(ta, tb, alpha, A, B, beta, C0, force_dot2=force_dot2)
    want, env = _fraction_gemm(ta, tb, alpha, A, B, beta, C0)
    assert isinstance(ref, gc.Pair) == (force_dot2 or not gc.HAVE_LD)
    for i in range(M):
        for j in range(N):
            got = Fraction(float(ref[i, j])) + Fraction(float(ref.lo[i, j])) if isinstance(ref, gc.Pair) else _to_fraction(ref[i, j])
            assert abs(got - want[i][j]) <= Fraction(1, 2 ** 60) * env[i][j], (i, j)
            assert abs(_to_fraction(E[i, j]) - env[i][j]) <= Fraction(1, 2 ** 50) * env[i][j], (i, j)


def test_reference_does_not_read_c_when_beta_is_zero():
    A, B, _ = _operands(77, 0, 0, 5, 6, 9)
    ref, E = gc.ref_gemm(0, 0, 2.0, A, B, 0.0, np.full((5, 6), np.nan))
    ref2, E2 = gc.ref_gemm(0, 0, 2.0, A, B, 0.0, None)
    assert np.isfinite(ref).all() and np.array_equal(ref, ref2) and np.array_equal(E, E2)


# ------------------------------------------------------------------------------------------- correct products pass the bound check
SHAPES = [(129, 17, 255), (300, 300, 700), (64, 200, 4096)]          # (I, J, K)


@pytest.mark.parametrize("I,J,K", SHAPES)
def test_float64_products_pass_the_bound_check(I, J, K):
    A, B = gc.uniform(100 + I, I, K), gc.uniform(200 + J, K, J)
    ref, E = gc.ref_gemm(0, 0, 1.0, A, B, 0.0, None)
    r_np = gc.assert_within_bound(A @ B, ref, E, K)
    r_or = gc.assert_within_bound(oracle.matmul2(A, B), ref, E, K)
    print("I, J, K = %d, %d, %d: |err| / (gamma E) numpy %.4f oracle %.4f" % (I, J, K, r_np, r_or))
    assert max(r_np, r_or) < 0.5                            # (the margin of a correct product; the assertion stays the bound itself)


def test_integer_family_is_exact_in_float64():
    A, B, C0 = _operands(31, 1, 1, 70, 50, 333, gc.integers)
    assert set(np.unique(A)) == set(range(-4, 5))
    for alpha in gc.ALPHAS:
        for beta in gc.BETAS:
            want = gc.exact_gemm(1, 1, alpha, A, B, beta, C0)
            gc.assert_exact(alpha * (A.T @ B.T) + beta * C0, want)
            gc.assert_exact(gc.exact_gemm(1, 1, alpha, A, B, beta, C0, blas=True), want)
            ref, E = gc.ref_gemm(1, 1, alpha, A, B, beta, C0)
            assert np.array_equal(ref, want.astype(LD))


# ------------------------------------------------------------------------------------------------------ wrong products are rejected
def _mutants(A, B):
    """(name, wrong product) of float64 A @ B, each what one kind of kernel bug gives"""
    I, K = A.shape
    J = B.shape[1]
    C = A @ B
    i, j, k = I // 2, J // 3, K // 2
    m = C.copy(); m[i, j] -= A[i, k] * B[k, j]
    yield "one k-term missing from one element", m
    yield "last k of the whole product omitted", A[:, :K - 1] @ B[:K - 1]
    m = C.copy(); m[i, j], m[i, j + 1] = C[i, j + 1], C[i, j]
    yield "two neighbouring elements swapped", m
    yield "float32-rounded operands", A.astype(np.float32).astype(np.float64) @ B.astype(np.float32).astype(np.float64)
    m = C.copy(); m[i, :] = A[i, 1:] @ B[1:]
    yield "one row computed with K - 1 terms", m
    m = C.copy(); m[I - 1, J - 1] += 64 * K * U * float((np.abs(A[I - 1]) @ np.abs(B[:, J - 1])))
    yield "one element off by 64 K ulps of E", m
    m = C.copy(); m[i, j] = np.nan
    yield "a NaN where the reference is finite", m
    m = C.copy(); m[0, J - 1] = 0.0
    yield "one element never written", m


@pytest.mark.parametrize("I,J,K", SHAPES)
def test_bound_check_rejects_mutants(I, J, K):
    A, B = gc.uniform(100 + I, I, K), gc.uniform(200 + J, K, J)
    ref, E = gc.ref_gemm(0, 0, 1.0, A, B, 0.0, None)
    gc.assert_within_bound(A @ B, ref, E, K)
    names = []
    for name, wrong in _mutants(A, B):
        with pytest.raises(AssertionError):
            gc.assert_within_bound(wrong, ref, E, K)
        names.append(name)
    assert len(names) == 8


def test_bound_check_compares_non_finite_by_kind():
    A, B = gc.uniform(5, 20, 30), gc.uniform(6, 30, 25)
    A[3, 7], B[5, 9] = np.inf, np.nan
    with np.errstate(invalid="ignore"):
        C = A @ B
    ref, E = gc.ref_gemm(0, 0, 1.0, A, B, 0.0, None)
    gc.assert_within_bound(C, ref, E, 30)
    assert np.isnan(C[:, 9]).all() and np.isinf(C[3, :9]).all()
    for i, j, v in ((3, 2, -C[3, 2]), (3, 2, np.nan), (0, 9, 1.0), (1, 1, np.inf)):
        m = C.copy(); m[i, j] = v
        with pytest.raises(AssertionError):
            gc.assert_within_bound(m, ref, E, 30)


def test_exact_check_rejects_one_unit():
    A, B, C0 = _operands(41, 0, 1, 33, 65, 48, gc.integers)
    want = gc.exact_gemm(0, 1, -0.5, A, B, 2.0, C0)
    gc.assert_exact(want.copy(), want)
    for i, j, d in ((0, 0, 1.0), (32, 64, -1.0), (17, 31, 0.25)):
        m = want.copy(); m[i, j] += d
        with pytest.raises(AssertionError, match=r"1 element\(s\), first at \[\(%d, %d\)\]" % (i, j)):
            gc.assert_exact(m, want)


def test_padded_buffer_layout():
    p = gc.padded(5, 3, 4, lead_rows=2, tail_rows=1, offset=1)
    assert p.start == 9 and p.win.shape == (5, 3) and np.isnan(p.buf).all()
    p.win[...] = 1.0
    assert np.isfinite(p.buf).sum() == 15 and p.buf[9] == 1.0 and np.isnan(p.buf[12]) and p.buf[13] == 1.0 and np.isnan(p.buf[8])
    q = gc.Padded(2, 3, 3, batch=3, stride=10)
    q.win[...] = 2.0
    assert q.win.shape == (3, 2, 3) and np.isfinite(q.buf).sum() == 18 and q.buf[q.start + 10] == 2.0 and np.isnan(q.buf[q.start + 6])


# ----------------------------------------------------------------------------------------------------------------------- tile map
def test_tile_map_model_is_bijective():
    """gemm.hip, dgemm_kernel, "XCD-aware tile assignment (bijective for any tile count)": the model of gemm_common.tile_of maps the
    workgroups onto every tile exactly once, short last groups and tile counts that are not multiples of 8 included"""
    for tiles_m in range(1, 41):
        for tiles_n in range(1, 41):
            seen = {gc.tile_of(b, tiles_m, tiles_n) for b in range(tiles_m * tiles_n)}
            assert seen == {(m, n) for m in range(tiles_m) for n in range(tiles_n)}, (tiles_m, tiles_n)


def test_rank_k_selection_covers_every_pair():
    cases = gc.smallk_cases()
    assert cases == gc.smallk_cases() and len(cases) < 150          # the same list in every process
    axes = gc.SMALLK_AXES
    for i in range(5):
        for j in range(i + 1, 5):
            assert {(c[i], c[j]) for c in cases} == {(a, b) for a in axes[i] for b in axes[j]}, (i, j)
