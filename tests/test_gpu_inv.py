"""inv, tril_inv, triu_inv and cholesky_inv on the device (csrc/getri.hip) through la and dev, which must give the same bits and leave
their operands untouched. The reference X_hp is numpy.linalg.inv refined by two Newton-Schulz steps in longdouble; the gates hold the
device's forward error and two-sided residual to 8 x those of plain numpy.linalg.inv on the same input (the same algorithm class in
another summation order). The largest ratios seen are in DESIGN.md 4.30."""
import numpy as np
import pytest

from nd4js_amd import _lib, la

pytestmark = pytest.mark.gpu

LD, EPS = np.longdouble, np.finfo(np.float64).eps
NAMES = ("inv", "tril_inv", "triu_inv", "cholesky_inv")
ORDERS = [1, 2, 3, 8, 15, 16, 17, 33, 64, 65, 127, 128, 129, 130, 192, 193, 257]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def both(name, A, info=False):
    """la.<name> and dev.<name> on the same operand: the same bits, the operand untouched; la's result (with the flags if info)"""
    import torch
    from nd4js_amd import dev
    keep, up, ih, idv = A.copy(), torch.from_numpy(A.copy()).cuda(), {}, {}
    X = getattr(la, name)(A, **({"info": ih} if info else {}))
    Xd = getattr(dev, name)(up, **({"info": idv} if info else {}))
    assert same_bits(A, keep) and same_bits(up.cpu().numpy(), keep), name + ": the operand was written"
    assert same_bits(X, Xd.cpu().numpy()), name + ": la and dev differ"
    if info:
        assert np.array_equal(ih["singular"], idv["singular"].cpu().numpy()) and ih["singular"].dtype == np.int32
        return X, ih["singular"]
    return X


def operand(name, seed, *shape):
    """(the operand of la.<name> with NaN where it must not be read, the well-conditioned matrices M whose inverses are wanted)"""
    rng, N = np.random.default_rng(seed), shape[-1]
    G = rng.standard_normal(shape)
    if name == "inv":
        # kappa_2 = 100 by construction: a plain Gaussian draw can have kappa ~ 1e5 (seed 65 at N = 65 has), where numpy's own forward
        # error on that draw happened to be 0.004 kappa eps and the device's ordinary 0.3 kappa eps missed the gate at equal residuals
        A = (np.linalg.qr(G)[0] * np.logspace(0, -2, N)) @ np.linalg.qr(rng.standard_normal(shape))[0]
        return A, A
    if name == "cholesky_inv":
        L = np.linalg.cholesky(G @ np.swapaxes(G, -1, -2) / N + np.eye(N))
        M = mm(L, np.swapaxes(L, -1, -2))
    else:
        L = M = np.tril(G, -1) / (4 * np.sqrt(N)) + np.eye(N) * (1 + rng.random(shape[:-1])[..., None])   # ||strict part|| ~ 1/2
    op = np.where(np.tri(N, dtype=bool), L, np.nan)
    return (np.ascontiguousarray(np.swapaxes(op, -1, -2)), np.swapaxes(M, -1, -2)) if name == "triu_inv" else (op, M)


def ninf(M):
    return np.abs(M).sum(axis=-1).max()


def mm(A, B):
    """A B in longdouble; above 512 columns by splitting both factors into three slices of 17 bits whose float64 products are exact"""
    if A.shape[-1] <= 512:
        return A.astype(LD) @ B.astype(LD)
    import torch

    def slices(M):
        s, out = 2.0 ** np.ceil(np.log2(np.abs(M).max())), []
        for bits in (17, 34):
            out.append(np.round((M - sum(out)) / s * 2.0 ** bits) / 2.0 ** bits * s)
        return [torch.from_numpy(np.ascontiguousarray(p)).cuda() for p in out + [M - sum(out)]]
    return sum((a @ b).cpu().numpy().astype(LD) for a in slices(A) for b in slices(B))


def gates(M, X, forward=True):
    """both gates for one member: the larger of the two ratios, each at most 8"""
    N, eye = M.shape[-1], np.eye(M.shape[-1], dtype=LD)
    Xn = np.linalg.inv(np.asarray(M, dtype=np.float64))

    def res(Y):
        return max(ninf(mm(M, Y) - eye), ninf(mm(Y, M) - eye))
    ratio = res(X) / max(res(Xn), N * EPS)
    if forward:
        Xhp = Xn.astype(LD)
        for _ in range(2):
            Xhp = Xhp + Xhp @ (eye - M.astype(LD) @ Xhp)
        ratio = max(ratio, (ninf(X - Xhp) / ninf(Xhp)) / max(ninf(Xn - Xhp) / ninf(Xhp), EPS))
    assert np.isfinite(X).all() and ratio <= 8.0, ratio
    return float(ratio)


@pytest.mark.parametrize("N", ORDERS)
@pytest.mark.parametrize("name", NAMES)
def test_orders(name, N):
    """every tier and block edge; the triangle that must not be read holds NaN, the other triangle of a triangular result is +0"""
    op, M = operand(name, N, N, N)
    X = both(name, op)
    print("%s %d: largest ratio %.2f" % (name, N, gates(M, X)))
    if name == "cholesky_inv":
        assert same_bits(X, X.T)
    elif name != "inv":
        other = ~np.tri(N, dtype=bool) if name == "tril_inv" else np.tri(N, k=-1, dtype=bool)
        assert not X.view(np.uint64)[other].any()


def test_the_largest_order_and_the_refusal_of_a_larger_one():
    """N = 2048: the residual gate only; N = 2049: refused before anything is written"""
    A = operand("inv", 2048, 2048, 2048)[0]
    print("inv 2048: residual ratio %.2f" % gates(A, la.inv(A), forward=False))
    h, N, ptr = _lib.handle(None), 2049, la._ptr
    A, X, info = np.zeros((N, N)), np.full((N, N), 7.0), np.full(1, -3, np.int32)
    for rc in (h.lib.nd4hip_dgetri_batched_host(h.ptr, 1, N, ptr(A), ptr(X), ptr(info)), h.lib.nd4hip_dtrtri_batched_host(h.ptr, 1, 1, N, ptr(A), ptr(X)),
               h.lib.nd4hip_dpotri_batched_host(h.ptr, 1, N, ptr(A), ptr(X))):
        assert rc == -1 and "N <= 2048" in h.lib.nd4hip_last_error().decode()
    assert np.all(X == 7.0) and info[0] == -3


@pytest.mark.parametrize("kind,N", [(k, n) for k in ("reversed", "ties") for n in (16, 40, 130)] + [("graded", n) for n in (16, 64, 130)])
def test_pivoting_and_conditioning(kind, N):
    """every column interchanges; every column's maxima are tied; kappa ~ 1e10 from a graded scaling between two orthogonal factors"""
    rng = np.random.default_rng(N)
    if kind == "reversed":
        A = (rng.standard_normal((N, N)) + 2 * N * np.eye(N))[::-1].copy()
    elif kind == "ties":
        A = rng.choice([-1.0, 1.0], (N, N))
    else:
        A = (np.linalg.qr(rng.standard_normal((N, N)))[0] * np.logspace(0, -10, N)) @ np.linalg.qr(rng.standard_normal((N, N)))[0]
    print("%s %d: largest ratio %.2f" % (kind, N, gates(A, both("inv", A))))


@pytest.mark.parametrize("shape", [(70000, 4, 4), (301, 8, 8), (5, 17, 17), (3, 130, 130)], ids=lambda s: "%dx%d" % s[:2])
@pytest.mark.parametrize("name", NAMES)
def test_batches(name, shape):
    """more members than one pass or one workgroup holds, counts that fill no wave: every member has the bits it has alone"""
    op, M = operand(name, 7, *shape)
    X = both(name, op)
    for m in sorted({0, 1, 15, 16, 63, 64, shape[0] // 2, shape[0] - 2, shape[0] - 1} & set(range(shape[0]))):   # lane-row and wave edges too
        assert same_bits(X[m], getattr(la, name)(op[m]))
    gates(M[-1], X[-1])


@pytest.mark.parametrize("name", NAMES)
def test_members_with_long_sums(name):
    """2 x 640^2: the products of the blocked tier run over K >= 512, where a split of K chosen from the size of the launch would
    give a member other bits in a batch than alone"""
    op = operand(name, 9, 2, 640, 640)[0]
    X = both(name, op)
    assert np.isfinite(X).all() and all(same_bits(X[m], getattr(la, name)(op[m])) for m in range(2))


@pytest.mark.parametrize("N", [8, 40, 130])
def test_singular_and_nan_members(N):
    """member 1 of 3 with a zero column j, then with a NaN as its first pivot: flagged, all NaN, the others as alone; a raise without info"""
    A, j = operand("inv", N + 1, 3, N, N)[0], N // 2
    for col, value, flag in ((j, 0.0, j + 1), (0, np.nan, 1)):
        B = A.copy()
        B[1, :1 if flag == 1 else N, col] = value
        X, flags = both("inv", B, info=True)
        assert flags.tolist() == [0, flag, 0] and np.isnan(X[1]).all()
        assert same_bits(X[0], la.inv(B[0])) and same_bits(X[2], la.inv(B[2]))
        with pytest.raises(_lib.Nd4HipError, match=r"inv\(A\): A is singular\. \(matrix 1\)") as err:
            la.inv(B)
        assert err.value.code == -5
        import torch
        from nd4js_amd import dev
        with pytest.raises(_lib.Nd4HipError, match=r"\(matrix 1\)"):
            dev.inv(torch.from_numpy(B).cuda())


@pytest.mark.parametrize("N", [8, 40, 130])
@pytest.mark.parametrize("name", ["tril_inv", "triu_inv"])
def test_zero_on_the_diagonal(name, N):
    """no raise; inside the triangle the result is finite exactly where tril_solve(L, I) / triu_solve(U, I) is (the rows that the
    substitution reaches before the zero); the other triangle stays +0"""
    T = np.nan_to_num(operand(name, N, N, N)[0])
    T[N // 2, N // 2] = 0.0
    X, want = both(name, T), getattr(la, name.replace("inv", "solve"))(T, np.eye(N))
    tri = np.tri(N, dtype=bool) if name == "tril_inv" else np.tri(N, dtype=bool).T
    assert np.array_equal(np.isfinite(X)[tri], np.isfinite(want)[tri]) and not np.isfinite(X).all() and not X.view(np.uint64)[~tri].any()


@pytest.mark.parametrize("N", [16, 64, 130])
@pytest.mark.parametrize("m", [-200, 200])
def test_power_of_two_scaling(m, N):
    """pivoting is scale-invariant and the divisions are true divisions: inv(2^m A) = 2^-m inv(A) bit for bit"""
    A = operand("inv", N + 2, N, N)[0]
    assert same_bits(both("inv", np.ldexp(A, m)), np.ldexp(la.inv(A), -m))


@pytest.mark.parametrize("name", NAMES)
def test_shape_edges(name):
    """no members: an empty array without a launch; N = 1: 1 / a ((1 / a)^2 from a Cholesky factor: W^T W of W = L^-1)"""
    assert both(name, np.zeros((0, 5, 5))).shape == (0, 5, 5) and both(name, np.zeros((2, 0, 3, 3))).shape == (2, 0, 3, 3)
    X, w = both(name, np.array([[[3.0]], [[-0.7]]])), 1.0 / np.array([[[3.0]], [[-0.7]]])
    assert same_bits(X, w * w if name == "cholesky_inv" else w)
