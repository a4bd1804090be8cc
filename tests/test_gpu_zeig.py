"""zhess_* / zschur_* / zeigen / zeigenvals on the GPU (csrc/zgehrd.hip, csrc/zhseqr.hip): la and dev give the same bits and leave their
operands untouched; the norm-wise bounds of DESIGN.md 4.29 with TOL = 1e-12, products formed in np.clongdouble, on the smallest shapes
at which each path can go wrong (the reduction's LDS tier ends at N = 95, the iteration's at N = 89)."""
import numpy as np
import pytest

import zlu_common as Z
from nd4js_amd import la
from test_gpu_zlu import _up, both

pytestmark = pytest.mark.gpu
TOL, L = 1e-12, np.clongdouble
SHAPES = [(1, 1), (2, 2), (3, 3), (5, 5), (95, 95), (96, 96), (130, 130), (3, 40, 40)]


def gauss(shape, seed=1):
    r = np.random.default_rng(seed)
    return r.standard_normal(shape) + 1j * r.standard_normal(shape)


def fro(x):
    return float(np.sqrt(np.sum(np.abs(np.asarray(x, dtype=L)) ** 2)))


def H(x):
    return np.conj(np.swapaxes(x, -1, -2))


def check_similarity(name, A, Q, T):
    """fro(A - Q T Q^H) <= TOL fro(A) and fro(Q^H Q - I) <= TOL sqrt(N), member by member"""
    N = A.shape[-1]
    for m in np.ndindex(A.shape[:-2]):
        Qm, Tm = Q[m].astype(L), T[m].astype(L)
        s1 = fro(A[m] - Qm @ Tm @ H(Qm)) / (TOL * max(fro(A[m]), 1e-300))
        s2 = fro(H(Qm) @ Qm - np.eye(N)) / (TOL * np.sqrt(N))
        print("%s %s: shares of the residual and unitarity bounds: %.2e %.2e" % (name, A.shape, s1, s2))
        assert max(s1, s2) <= 1.0


def check_pairs(A, lam, V):
    """fro(A V - V diag(lam)) <= TOL sqrt(N) fro(A), unit columns, |sum lam - tr A| <= TOL N fro(A)"""
    N = A.shape[-1]
    assert np.isfinite(V).all() and np.isfinite(lam).all()
    for m in np.ndindex(A.shape[:-2]):
        Vm = V[m].astype(L)
        s1 = fro(A[m].astype(L) @ Vm - Vm * lam[m]) / (TOL * np.sqrt(N) * fro(A[m]))
        s2 = float(np.max(np.abs(np.sqrt(np.sum(np.abs(Vm) ** 2, axis=0)) - 1))) / TOL
        s3 = float(abs(np.sum(lam[m].astype(L)) - np.trace(A[m].astype(L)))) / (TOL * N * fro(A[m]))
        print("zeigen %s: shares of the residual, unit-norm and trace bounds: %.2e %.2e %.2e" % (A.shape, s1, s2, s3))
        assert max(s1, s2, s3) <= 1.0


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_hessenberg(shape):
    A = gauss(shape)
    N = shape[-1]
    Q, Hs = both("zhess_decomp", A)
    check_similarity("zhess_decomp", A, Q, Hs)
    assert not np.tril(Hs, -2).any() and not np.diagonal(Hs, -1, -2, -1).imag.any()
    F, tau = both("zhess_factor", A)
    assert tau.shape == shape[:-2] + (max(N - 1, 0),) and Z.same_bits(np.triu(F, -1), Hs)
    Zc = gauss(shape[:-1] + (3,), 5)
    Zc /= np.sqrt(np.sum(np.abs(Zc) ** 2, axis=-2, keepdims=True))
    back = both("zhess_apply_q", F, tau, both("zhess_apply_q", F, tau, Zc), True)
    for m in np.ndindex(shape[:-2]):
        s3 = fro(back[m] - Zc[m]) / (TOL * np.sqrt(3))
        print("zhess_apply_q %s: share of the bound on Q^H (Q Z): %.2e" % (shape, s3))
        assert s3 <= 1.0


@pytest.mark.parametrize("shape", SHAPES + [(89, 89), (90, 90), (200, 200)], ids=str)
def test_schur(shape):
    A = gauss(shape, 2)
    Q, T = both("zschur_decomp", A)
    check_similarity("zschur_decomp", A, Q, T)
    assert not np.tril(T, -1).any()
    assert Z.same_bits(both("zeigenvals", A), np.diagonal(T, 0, -2, -1))
    Qh, Hs = both("zhess_decomp", A)
    Q2, T2 = both("zschur_qr", Qh, Hs)
    assert Z.same_bits(Q2, Q) and Z.same_bits(T2, T)


@pytest.mark.parametrize("shape", [(7, 7), (64, 64), (65, 65), (200, 200), (4, 33, 33)], ids=str)
def test_eigenpairs(shape):
    A = gauss(shape, 3)
    lam, V = both("zeigen", A)
    check_pairs(A, lam, V)
    Q, T = both("zschur_decomp", A)
    l2, V2 = both("zschur_eigen", Q, T)
    assert Z.same_bits(l2, lam) and Z.same_bits(V2, V)


@pytest.mark.parametrize("N", [48, 150])
def test_known_spectrum(N):
    j = np.arange(N)
    want = (j % 16) + 1j * (j // 16)
    U = np.linalg.qr(gauss((N, N), 4))[0].astype(L)
    A = ((U * want) @ H(U)).astype(np.complex128)
    lam = both("zeigenvals", A)
    share = float(np.max(np.abs(lam - np.round(lam)))) / (TOL * float(np.max(np.abs(want))))
    print("zeigenvals known spectrum N = %d: share of the bound: %.2e" % (N, share))
    key = lambda z: (np.round(z.real), np.round(z.imag))
    assert sorted(map(key, lam)) == sorted(map(key, want)) and share <= 1.0


def cyclic(N):
    return np.roll(np.eye(N, dtype=np.complex128), 1, axis=0)


@pytest.mark.parametrize("case", ["triangular", "cyclic8", "cyclic70", "jordan", "coupled"])
def test_sharp_inputs(case):
    if case == "triangular":
        A = np.triu(gauss((20, 20), 6))
        Q, T = both("zschur_decomp", A)
        F, tau = both("zhess_factor", A)
        assert Z.same_bits(T, A) and Z.same_bits(Q, np.eye(20, dtype=np.complex128)) and not tau.any()
    elif case.startswith("cyclic"):
        N = int(case[6:])
        lam = both("zeigenvals", cyclic(N))
        k = np.round(np.angle(lam) * N / (2 * np.pi)).astype(int) % N
        assert sorted(k) == list(range(N)) and np.max(np.abs(lam - np.exp(2j * np.pi * k / N))) <= TOL
        check_pairs(cyclic(N), *both("zeigen", cyclic(N)))
    elif case == "jordan":
        U = np.linalg.qr(gauss((12, 12), 7))[0].astype(L)
        J = (1 + 2j) * np.eye(12) + np.eye(12, k=1)
        A = (U @ J @ H(U)).astype(np.complex128)
        check_pairs(A, *both("zeigen", A))
    else:
        A = np.zeros((20, 20), dtype=np.complex128)
        A[:10, :10], A[10:, 10:], A[10, 9] = gauss((10, 10), 8), gauss((10, 10), 9), 1e-300 * (1 + 1j)
        check_similarity("zhess_decomp", A, *both("zhess_decomp", A))
        check_similarity("zschur_decomp", A, *both("zschur_decomp", A))
        check_pairs(A, *both("zeigen", A))


def test_exact_scaling():
    A = gauss((33, 33), 10)
    lam, V = both("zeigen", A)
    for p in (300, -300):
        l2, V2 = both("zeigen", np.ldexp(A.real, p) + 1j * np.ldexp(A.imag, p))
        assert Z.same_bits(V2, V) and Z.same_bits(l2, np.ldexp(lam.real, p) + 1j * np.ldexp(lam.imag, p))


def test_nan_member_and_isolation():
    import torch
    from nd4js_amd import dev
    A = gauss((3, 12, 12), 11)
    lam, V = both("zeigen", A)
    Ab = A.copy()
    Ab[1, 3, 4], Ab[2, 0, 0] = np.nan, np.inf                 # two members: the lowest is named
    for run in (lambda: la.zeigen(Ab), lambda: dev.zeigen(_up(Ab)), lambda: la.zeigenvals(Ab), lambda: la.zschur_decomp(Ab), lambda: la.zhess_factor(Ab)):
        with pytest.raises(ValueError, match=r"\(A\): A contains NaN or Infinity\. \(matrix 1\)"):
            run()
    up = _up(Ab)
    lo, Vo = torch.zeros(3, 12, dtype=torch.complex128, device="cuda"), torch.zeros(3, 12, 12, dtype=torch.complex128, device="cuda")
    h = dev._h(up)
    assert h.lib.nd4hip_zgeev_batched_dev(h.ptr, 3, 12, dev._p(up), dev._p(lo), dev._p(Vo)) == -3
    for m in (0,):
        assert Z.same_bits(lo[m].cpu().numpy(), lam[m]) and Z.same_bits(Vo[m].cpu().numpy(), V[m])
    Q, T = both("zschur_decomp", A)
    Q[2, 1, 1] = np.nan
    with pytest.raises(ValueError, match=r"zschur_eigen\(Q,T\): Q or T contains NaN or Infinity\. \(matrix 2\)"):
        la.zschur_eigen(Q, T)
    with pytest.raises(ValueError, match="N <= 1024"):
        la.zeigen(np.zeros((1025, 1025), dtype=np.complex128))
