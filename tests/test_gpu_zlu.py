"""zlu_decomp, zlu_solve and zsolve on the device (csrc/zgetrf.hip) through la and dev, which must give the same bits and leave their
operands untouched, against the model and bounds of tests/zlu_common.py. The largest shares seen are in DESIGN.md 4.26."""
import numpy as np
import pytest

import zlu_common as Z
from nd4js_amd import _lib, la

pytestmark = pytest.mark.gpu

SINGULAR = r"zsolve\(A,Y\): A is singular\. \(matrix %d\)"


def _up(a):
    import torch
    return torch.from_numpy(np.array(a, order="C")).cuda()


def both(name, *args, info=False):
    """la.<name> and dev.<name> on the same operands: the same bits, the operands untouched; la's result (with the flags if info)"""
    from nd4js_amd import dev
    keep = [np.array(a) for a in args]
    ih, idv, ups = {}, {}, [_up(a) for a in args]
    out = getattr(la, name)(*args, **({"info": ih} if info else {}))
    outd = getattr(dev, name)(*ups, **({"info": idv} if info else {}))
    for a, k, u in zip(args, keep, ups):
        assert Z.same_bits(np.array(a), k) and Z.same_bits(u.cpu().numpy(), k), name + ": an operand was written"
    for a, b in zip(out if isinstance(out, tuple) else (out,), outd if isinstance(outd, tuple) else (outd,)):
        assert Z.same_bits(a, b.cpu().numpy()), name + ": la and dev differ"
    if info:
        assert Z.same_bits(ih["singular"], idv["singular"].cpu().numpy())
        return out + (ih["singular"],)
    return out


def check(name, K=3, model_bits=None):
    """a catalogue input through zlu_decomp, zlu_solve and zsolve: P, the bounds, the bits where they are promised"""
    A, LUm, Pm, _ = Z.catalogue(name)
    N = A.shape[-1]
    LU, P, flags = both("zlu_decomp", A, info=True)
    assert not flags.any() and np.array_equal(P, Pm)
    Y = Z.cmatrix(99, *(A.shape[:-1] + (K,)))
    X = both("zlu_solve", LU, P, Y)
    assert Z.same_bits(X, both("zsolve", A, Y))
    s1, s3, s2 = Z.shares(A, LU, P, X, Y)
    print("%s K=%d: shares of the bounds 1, 2, 3: %.2e %.2e %.2e" % (name, K, s1, s2, s3))
    assert s1 <= 1.0 and s2 <= 1.0 and s3 <= 1.0
    if N <= 64 if model_bits is None else model_bits:
        assert Z.same_bits(LU, LUm) and Z.same_bits(X, Z.solve_model(LUm, Pm, Y).reshape(X.shape))
    return LU, P


@pytest.mark.parametrize("N", Z.SIZES + Z.PANEL_SIZES)
def test_sizes(N):
    check(str(N))


def test_the_largest_order_and_the_refusal_of_a_larger_one():
    """N = 2048: bounds 1 and 2 only; N = 2049: refused before anything is written"""
    A, Y = Z.cmatrix(2048, 2048, 2048), Z.cmatrix(7, 2048, 2)
    LU, P = la.zlu_decomp(A)
    s1, _, s2 = Z.shares(A, LU, P, la.zsolve(A, Y), Y)
    print("2048: shares of the bounds 1, 2: %.2e %.2e" % (s1, s2))
    assert sorted(P.tolist()) == list(range(2048)) and s1 <= 1.0 and s2 <= 1.0
    h, N, ptr = _lib.handle(None), 2049, la._ptr
    A, LU, P, X = np.zeros((N, N), np.complex128), np.full((N, N), 7 + 7j), np.full(N, -3, np.int32), np.full((N, 1), 7 + 7j)
    for rc in (h.lib.nd4hip_zgetrf_batched_host(h.ptr, 1, N, ptr(A), ptr(LU), ptr(P), None),
               h.lib.nd4hip_zgetrs_batched_host(h.ptr, 1, N, 1, ptr(A), 0, ptr(P), 0, ptr(X), 0, ptr(X)),
               h.lib.nd4hip_zgesv_batched_host(h.ptr, 1, N, 1, ptr(A), ptr(X), ptr(X))):
        assert rc == -1 and "N <= 2048" in h.lib.nd4hip_last_error().decode()
    assert np.all(LU == 7 + 7j) and np.all(P == -3) and np.all(X == 7 + 7j)


@pytest.mark.parametrize("N", [17, 40, 130])
def test_right_hand_sides(N):
    """K = 1, 64 and 65 as columns of one solve, bit for bit; a float64 Y; one factorisation against a stack of Y"""
    A, LU, P, _ = Z.catalogue(str(N))
    Y, Ys = Z.cmatrix(98, N, 65), Z.cmatrix(6, 3, N, 2)
    X, Xs = both("zsolve", A, Y), both("zlu_solve", LU, P, Ys)
    assert Z.shares(A, LU, P, X, Y)[2] <= 1.0 and Z.shares(A, LU, P, Xs, Ys)[2] <= 1.0
    for K in (1, 64):
        assert Z.same_bits(both("zsolve", A, Y[:, :K]), X[:, :K])
    assert all(Z.same_bits(Xs[m], la.zlu_solve((LU, P), Ys[m])) for m in range(3))
    assert Z.same_bits(both("zlu_solve", LU, P, Y.real), la.zlu_solve(LU, P, Y.real + 0j)) and Z.same_bits(both("zsolve", A, Y.real), la.zsolve(A, Y.real + 0j))


@pytest.mark.parametrize("shape", Z.BATCHES, ids=Z.name_of)
def test_batches(shape):
    """every member has the bits it has alone (70000 x 4^2: more than one pass of members)"""
    LU, P = check(Z.name_of(shape), K=2, model_bits=False)
    A = Z.catalogue(Z.name_of(shape))[0]
    for m in sorted({0, 1, shape[0] // 2, 32767 % shape[0], 32768 % shape[0], shape[0] - 1}):
        LU1, P1 = la.zlu_decomp(A[m])
        assert Z.same_bits(LU[m], LU1) and np.array_equal(P[m], P1)


@pytest.mark.parametrize("N,rows", [(8, (2, 3, 5, 7)), (16, (3, 7, 8, 15)), (17, (8, 9, 15, 16)), (130, (3, 10, 20, 40)), (130, (5, 70, 100, 129)),
                                    (520, (2, 514, 515, 519))], ids=["reg-8", "reg-16", "lds-17", "one-wave", "two-waves", "two-slots"])
def test_exact_ties_go_to_the_first_row(N, rows):
    A = Z.tie_input(N, rows, 31)
    LUm, Pm, info, _ = Z.lu_model(A)
    LU, P = both("zlu_decomp", A)
    assert P[0] == rows[0] and np.array_equal(P, Pm) and Z.shares(A, LU, P)[0] <= 1.0


@pytest.mark.parametrize("N", [3, 16, 32, 40, 64, 65, 130, 300, 520, 1030])
def test_exact_inputs_have_the_exact_factors(N):
    A, LUx, Px = Z.exact_input(N, 17)
    LU, P = both("zlu_decomp", A)
    a, b = np.array(LU).view(np.float64), np.array(LUx).view(np.float64)     # (an exact zero may carry either sign from the matrix cores)
    assert np.array_equal(P, Px) and Z.same_bits(a[b != 0], b[b != 0]) and not a[b == 0].any()
    Y = A @ (np.arange(N * 2).reshape(N, 2) % 5 - 2.0)                  # an integer solution, an exact right-hand side
    assert np.array_equal(both("zsolve", A, Y), np.arange(N * 2).reshape(N, 2) % 5 - 2.0)


@pytest.mark.parametrize("N", [17, 130])
@pytest.mark.parametrize("k", [-500, 500])
def test_scaling_by_a_power_of_two_is_exact(N, k):
    A, LUm, Pm, _ = Z.catalogue(str(N))
    LU0, P0 = la.zlu_decomp(A)
    LU, P = both("zlu_decomp", np.ldexp(A.real, k) + 1j * np.ldexp(A.imag, k))
    low, up = np.tril(np.ones((N, N), bool), -1), np.triu(np.ones((N, N), bool))
    assert np.array_equal(P, P0) and Z.same_bits(LU[low], LU0[low])
    assert Z.same_bits(LU[up], np.ldexp(LU0[up].real, k) + 1j * np.ldexp(LU0[up].imag, k))


@pytest.mark.parametrize("N", [3, 40, 130])
def test_singular_and_non_finite_members(N):
    M, expected = Z.singular_members(N, 23)
    LU, P, flags = both("zlu_decomp", M, info=True)
    info = Z.lu_model(M)[2]
    assert np.array_equal(flags, info) and all(flags[m] == f for m, f in expected.items()) and flags[3] > 0 and flags[4] > 0
    for m in (0, 5):                                                       # the neighbours' bits
        LU1, P1 = la.zlu_decomp(M[m])
        assert Z.same_bits(LU[m], LU1) and np.array_equal(P[m], P1)
    Y = Z.cmatrix(3, 6, N, 2)
    from nd4js_amd import dev
    for call, lowest in ((lambda: la.zsolve(M, Y), 1), (lambda: dev.zsolve(_up(M), _up(Y)), 1), (lambda: la.zsolve(M[[0, 5, 0, 4, 2]], Y[:5]), 3),
                         (lambda: la.zsolve(M[2], Y[2]), 0)):
        with pytest.raises(_lib.Nd4HipError, match=SINGULAR % lowest) as e:
            call()
        assert e.value.code == -5
    assert Z.same_bits(la.zsolve(M[5], Y[5]), la.zlu_solve(LU[5], P[5], Y[5]))   # the handle afterwards


def test_the_profile_record():
    from nd4js_amd import dev
    A, Y = _up(Z.catalogue("5x40x40")[0]), _up(Z.cmatrix(1, 5, 40, 3))
    h, recs = _lib.handle(0), []
    h.profile_enable(True)
    try:
        for call in (lambda: dev.zlu_decomp(A), lambda: dev.zlu_solve(dev.zlu_decomp(A), Y), lambda: dev.zsolve(A, Y)):
            call()
            recs.append(h.profile_last()[0])
    finally:
        h.profile_enable(False)
    f, s = 5 * 8.0 / 3.0 * 40 ** 3, 5 * 8.0 * 40 * 40 * 3
    for rec, (op, flops) in zip(recs, (("zgetrf_batched", f), ("zgetrs_batched", s), ("zgesv_batched", f + s))):
        assert rec["valid"] and rec["op"] == op and rec["flops"] == pytest.approx(flops) and rec["kernel_ms"] > 0
