"""zqr_factor, zqr_apply_q, zqr_decomp and zqr_lstsq on the device (csrc/zgeqrf.hip) through la and dev, which must give the same bits and
leave their operands untouched, against the model and bounds of tests/zqr_common.py. The largest shares seen are in DESIGN.md 4.27."""
import numpy as np
import pytest

import zqr_common as Q
from nd4js_amd import _lib, la
from test_gpu_zlu import _up, both

pytestmark = pytest.mark.gpu

DEFICIENT = r"zqr_lstsq\(A,Y\): A is rank-deficient\. \(matrix %d\)"


def factored(F, tau, Y):
    """zqr_lstsq((F, tau), Y) through la and dev: the same bits"""
    from nd4js_amd import dev
    X = la.zqr_lstsq((F, tau), Y)
    assert Q.same_bits(X, dev.zqr_lstsq((_up(F), _up(tau)), _up(Y)).cpu().numpy())
    return X


def check(A, K=3, model=False):
    """A through the four functions: the bounds 1 - 5, the thin Q against zqr_apply_q, the model's bits where they are promised"""
    M, N = A.shape[-2:]
    F, tau = both("zqr_factor", A)
    Qd, R = both("zqr_decomp", A)
    eye = np.array(np.broadcast_to(np.eye(M, N), A.shape))
    assert Q.same_bits(Qd, both("zqr_apply_q", F, tau, eye)) and Q.same_bits(R, np.triu(F[..., :N, :]))
    Zm, Y = Q.rhs(A, K, 5), Q.rhs(A, K)
    QZ = both("zqr_apply_q", F, tau, Zm)
    X = both("zqr_lstsq", A, Y)
    assert Q.same_bits(X, factored(F, tau, Y))
    s1, s2, b3 = Q.shares_qr(A, Qd, R)
    from nd4js_amd import dev
    back = la.zqr_apply_q(F, tau, QZ, adjoint=True)
    assert Q.same_bits(back, dev.zqr_apply_q(_up(F), _up(tau), _up(QZ), adjoint=True).cpu().numpy())
    s4, s5 = Q.share_apply(Zm, back), Q.share_lstsq(A, X, Y)
    print("%s K=%d: shares of the bounds 1, 2, 4, 5: %.2e %.2e %.2e %.2e" % (Q.name_of(A.shape), K, s1, s2, s4, s5))
    assert max(s1, s2, s4, s5) <= 1.0 and b3
    if model:
        Fm, taum = Q.factor_model(A)
        assert Q.same_bits(F, Fm) and Q.same_bits(tau, taum) and Q.same_bits(QZ, Q.apply_model(Fm, taum, Zm))
        assert Q.same_bits(Qd, Q.apply_model(Fm, taum, eye))
        if N <= 64:                                                          # (above, the upper sweep runs on the matrix cores)
            assert Q.same_bits(X, Q.lstsq_model(Fm, taum, Y))
    return F, tau


@pytest.mark.parametrize("shape", Q.LDS_SHAPES + Q.BLOCKED_SHAPES, ids=Q.name_of)
def test_shapes_of_both_tiers(shape):
    """the LDS tier has the bits of the model"""
    check(Q.catalogue(*shape), model=shape in Q.LDS_SHAPES)


def test_the_largest_shape_and_the_refusals():
    """2048 x 2048: bounds 1 and 2 on 32 fixed rows and columns; 2049 rows or columns and M < N: refused with the outputs intact"""
    A = Q.catalogue(2048, 2048)
    Qd, R = la.zqr_decomp(A)
    pick = np.sort(np.random.default_rng(2048).choice(2048, 32, replace=False))
    s1, s2, b3 = Q.shares_qr(A, Qd, R, pick, pick)
    print("2048x2048: shares of the bounds 1, 2: %.2e %.2e" % (s1, s2))
    assert s1 <= 1.0 and s2 <= 1.0 and b3
    h, ptr = _lib.handle(None), la._ptr
    for M, N in ((2049, 1), (2049, 2049), (3, 4)):
        A, F, tau = np.zeros((M, N), np.complex128), np.full((M, N), 7 + 7j), np.full(max(M, N), 7 + 7j)
        for rc in (h.lib.nd4hip_zgeqrf_batched_host(h.ptr, 1, M, N, ptr(A), ptr(F), ptr(tau)),
                   h.lib.nd4hip_zunmqr_batched_host(h.ptr, 1, M, N, 1, 0, ptr(A), M * N, ptr(A), N, ptr(tau)),
                   h.lib.nd4hip_zungqr_batched_host(h.ptr, 1, M, N, ptr(A), ptr(F), ptr(tau)),
                   h.lib.nd4hip_zgels_batched_host(h.ptr, 1, M, N, 1, ptr(A), M * N, None, ptr(A), ptr(tau), None)):
            assert rc == -1 and "N <= M <= 2048" in h.lib.nd4hip_last_error().decode()
        assert np.all(F == 7 + 7j) and np.all(tau == 7 + 7j)


@pytest.mark.parametrize("shape", [(33, 5), (153, 17)], ids=Q.name_of)
def test_right_hand_sides(shape):
    """K = 1, 3, 64 as columns of one call with K = 65, bit for bit; a float64 Y; one (F, tau) against a stack of Y"""
    A = Q.catalogue(*shape)
    F, tau = la.zqr_factor(A)
    Y, Ys = Q.rhs(A, 65), Q.cmatrix(6, 3, shape[0], 2)
    X, QZ = both("zqr_lstsq", A, Y), both("zqr_apply_q", F, tau, Y)
    assert Q.share_lstsq(A, X, Y) <= 1.0
    for K in (1, 3, 64):
        assert Q.same_bits(both("zqr_lstsq", A, Y[:, :K]), X[:, :K]) and Q.same_bits(both("zqr_apply_q", F, tau, Y[:, :K]), QZ[:, :K])
    Xs = factored(F, tau, Ys)
    assert all(Q.same_bits(Xs[m], la.zqr_lstsq(A, Ys[m])) for m in range(3))
    assert Q.same_bits(both("zqr_apply_q", F, tau, Ys), np.stack([la.zqr_apply_q(F, tau, Ys[m]) for m in range(3)]))
    assert Q.same_bits(both("zqr_lstsq", A, Y.real), la.zqr_lstsq(A, Y.real + 0j))


@pytest.mark.parametrize("shape", Q.BATCHES, ids=Q.name_of)
def test_batches(shape):
    """every member has the bits it has alone (70000 x 4^2: more than one pass of members)"""
    A = Q.catalogue(*shape)
    F, tau = check(A, K=2, model=shape[1] <= 152)
    Y = Q.rhs(A, 2)
    X = la.zqr_lstsq(A, Y)
    for m in sorted({0, shape[0] // 2, 32768 % shape[0], shape[0] - 1}):
        F1, tau1 = la.zqr_factor(A[m])
        assert Q.same_bits(F[m], F1) and Q.same_bits(tau[m], tau1) and Q.same_bits(X[m], la.zqr_lstsq(A[m], Y[m]))


@pytest.mark.parametrize("shape", [(8, 5), (40, 40), (200, 40), (160, 160)], ids=Q.name_of)
def test_degenerate_columns(shape):
    from nd4js_amd import dev
    M, N = shape
    S = Q.degenerate(M, N)
    if M == N:                                                              # the last reflector has an empty tail: a phase
        S[0][:, N - 1] += 0.5j
    F, tau = both("zqr_factor", S)
    assert not np.ascontiguousarray(np.diagonal(F, axis1=-2, axis2=-1).imag).view(np.uint64).any()
    assert tau[1, N // 2] == 0 and F[1, N // 2, N // 2] == 0 and tau[2, 1] == 0 and F[2, 1, 1] == 3.0 and abs(abs(tau[3, 1] - 1) - 1) <= 8 * Q.Z.EPS
    assert M != N or abs(abs(tau[0, N - 1] - 1) - 1) <= 8 * Q.Z.EPS
    Qd, R = both("zqr_decomp", S)
    s1, s2, b3 = Q.shares_qr(S, Qd, R)
    assert s1 <= 1.0 and s2 <= 1.0 and b3
    Y, info = Q.rhs(S, 2), {}
    idev = {}
    assert Q.same_bits(la.zqr_lstsq(S, Y, info=info), dev.zqr_lstsq(_up(S), _up(Y), info=idev).cpu().numpy())
    assert info["singular"].tolist() == [0, N // 2 + 1, 0, 0] == idev["singular"].cpu().tolist()
    for call, lowest in ((lambda: la.zqr_lstsq(S, Y), 1), (lambda: dev.zqr_lstsq(_up(S), _up(Y)), 1), (lambda: la.zqr_lstsq(S[[0, 2, 1, 1]], Y), 2),
                         (lambda: la.zqr_lstsq(S[1], Y[1]), 0)):
        with pytest.raises(_lib.Nd4HipError, match=DEFICIENT % lowest) as e:
            call()
        assert e.value.code == -5
    assert Q.same_bits(la.zqr_lstsq(S[0], Y[0]), la.zqr_lstsq(la.zqr_factor(S[0]), Y[0]))   # the handle afterwards


@pytest.mark.parametrize("shape", [(33, 5), (200, 40)], ids=Q.name_of)
@pytest.mark.parametrize("k", [-500, 500])
def test_scaling_by_a_power_of_two_is_exact(shape, k):
    A = np.array(Q.catalogue(*shape))
    down = -600 if k > 0 else -500          # a column that is lifted (below 2^-450); 2^-600 2^-500 would underflow in the input itself
    A[:, 2] = np.ldexp(A[:, 2].real, down) + 1j * np.ldexp(A[:, 2].imag, down)
    F0, tau0 = la.zqr_factor(A)
    F, tau = both("zqr_factor", np.ldexp(A.real, k) + 1j * np.ldexp(A.imag, k))
    low = np.tril(np.ones(shape, bool), -1)
    assert Q.same_bits(tau, tau0) and Q.same_bits(F[low], F0[low])
    assert Q.same_bits(F[~low], np.ldexp(F0[~low].real, k) + 1j * np.ldexp(F0[~low].imag, k))
    Qd, R = la.zqr_decomp(A)
    s1, s2, b3 = Q.shares_qr(A, Qd, R)
    assert s1 <= 1.0 and s2 <= 1.0 and b3


@pytest.mark.parametrize("shape", [(40, 24), (200, 40)], ids=Q.name_of)
def test_nan_and_inf_members_leave_their_neighbours_alone(shape):
    S = np.array(np.broadcast_to(Q.catalogue(*shape), (4,) + shape))
    S[1][shape[0] // 2, 3], S[2][shape[0] - 1, 0] = np.nan, np.inf
    F, tau = both("zqr_factor", S)
    Qd, R = both("zqr_decomp", S)
    F1, tau1 = la.zqr_factor(S[0])
    Q1, R1 = la.zqr_decomp(S[0])
    for m in (0, 3):
        assert Q.same_bits(F[m], F1) and Q.same_bits(tau[m], tau1) and Q.same_bits(Qd[m], Q1) and Q.same_bits(R[m], R1)
    assert np.isnan(F[1]).any() and not np.isfinite(F[2]).all()

