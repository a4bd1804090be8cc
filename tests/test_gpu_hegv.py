"""The Hermitian Cholesky factorisation, the complex triangular solves and the generalised Hermitian-definite eigenproblem on the
device (csrc/hegv.hip) through la (host arrays) and dev (device tensors): herm_cholesky_decomp, herm_cholesky_solve, ztril_solve,
herm_gen_reduce, eigen_herm_gen and eigenvals_herm_gen, inside the six bounds of tests/hegv_common.py and, for L, C, the solves and
the back-transformation, bit for bit against its numpy model at every size (the LDS tier is N <= 64, with the factorisation fused into
the reduction up to N = 32; above 64 blocks of 64). Every
call goes through both layers and must give the same bits with the inputs untouched. The shares of the 1e-12 bounds are printed per
case; the largest seen on the device (also in DESIGN.md 4.25), bounds 1 to 6 in order: 5.9e-4, 1.7e-4, 1.0e-3, 1.2e-4, 7.0e-4 (1.7e-3
at N = 2048), 1.1e-4; with subset, bounds 1 to 3: 6.0e-4, 0.32, 1.0e-3 (the residual of the smallest pair of graded_2, kappa = 1e6,
from eigen_herm's bisection route on a C of norm 1e6; every other subset case stays below 2e-4).

Mutants considered, and the test that catches each:
  a missing conjugate in the trailing update (l_ik l_jk for l_ik conj(l_jk))  test_catalogue (L's bits and bound 5, every N >= 3)
  L^T for L^H in the back-transformation                                      test_catalogue (X's bits, bounds 2 and 3), test_right_hand_sides
  Im of the diagonal kept (of H, A or B)                                      test_what_is_not_read_changes_nothing
  the pitch N for N | 1 (a tile overlapping the next)                         test_sizes (N = 2, 8, 32, 64: even N, bits of L, C and X)
  the last block's remainder dropped                                          test_sizes (N = 65, 97, 129, 193), test_right_hand_sides (K = 65)
  the shared-B stride ignored (members read past the one B or L)              test_one_shared_b_against_the_stacked_call"""
import numpy as np
import pytest

import hegv_common as G
import herm_common as X
from nd4js_amd import _lib, la

pytestmark = pytest.mark.gpu

NOT_PD = r"eigen_herm_gen\(A,B\): B is not positive definite\. \(matrix %d\)"
NOT_PD_H = r"herm_cholesky_decomp\(H\): H is not positive definite\. \(matrix %d\)"
NOT_FINITE = r"eigen_herm_gen\(A,B\): L\^-1 A L\^-H is not finite \(NaN or Infinity in the lower triangle of A, or overflow\)\."


def _dev():
    import torch
    from nd4js_amd import dev
    return torch, dev


def _up(a):
    torch, _ = _dev()
    return torch.from_numpy(np.array(a, order="C")).cuda()


def both(name, *args, **kw):
    """la.<name> and dev.<name> on the same operands: the same bits, the operands untouched; returns la's result"""
    _, dev = _dev()
    keep = [np.array(a) for a in args]
    out = getattr(la, name)(*args, **kw)
    ups = [_up(a) for a in args]
    outd = getattr(dev, name)(*ups, **kw)
    for a, k, u in zip(args, keep, ups):
        assert X.same_bits(np.array(a), k) and X.same_bits(u.cpu().numpy(), k), name + ": an operand was written"
    for a, b in zip(out if isinstance(out, tuple) else (out,), outd if isinstance(outd, tuple) else (outd,)):
        assert X.same_bits(a, b.cpu().numpy()), name + ": la and dev differ"
    return out


def eigen(A, B, subset=None):
    lam, Xv = both("eigen_herm_gen", A, B, subset=subset)
    assert X.same_bits(lam, both("eigenvals_herm_gen", A, B, subset=subset))
    return lam, Xv


def per_member(fn, *stacks):
    """fn on every member; a 2-D operand serves every member"""
    lead = max((s.shape[:-2] for s in stacks), key=len)
    n = int(np.prod(lead, dtype=np.int64))
    parts = [s.reshape((-1,) + s.shape[-2:]) if s.ndim > 2 else [s] * n for s in stacks]
    outs = [fn(*(p[m] for p in parts)) for m in range(n)]
    return np.stack(outs).reshape(lead + outs[0].shape)


def chol_model(B):
    def one(b):
        L, bad = G.chol_model(b)
        assert not bad
        return L
    return per_member(one, B)


def model_checks(A, B, what):
    """L, C, the solve and the eigenpairs of (A, B) against the model's bits and bounds 2-6; returns (lam, X)"""
    N = A.shape[-1]
    L = both("herm_cholesky_decomp", B)
    s5 = G.chol_share(B, L)
    assert X.same_bits(L, chol_model(B)), what + ": L is not the model's"
    C = both("herm_gen_reduce", A, L)
    s4 = G.reduction_share(A, L, C)
    assert X.same_bits(C, per_member(G.hegst_model, A, L)), what + ": C is not the model's"
    assert not np.triu(C, 1).any() and not np.diagonal(C, axis1=-2, axis2=-1).imag.any()
    Y = G.cmatrix(G.SEED + 5000 + N, int(np.prod(A.shape[:-2], dtype=np.int64)) * N, 3).reshape(A.shape[:-1] + (3,))
    S = both("herm_cholesky_solve", L, Y)
    s6 = G.solve_share(B, S, Y)
    assert X.same_bits(S, per_member(G.potrs_model, L, Y)), what + ": the solve is not the model's"
    print("%s: shares of bounds 4-6: %.3g %.3g %.3g" % (what, s4, s5, s6))
    assert s4 <= 1.0 and s5 <= 1.0 and s6 <= 1.0
    lam, Xv = eigen(A, B)
    if N > 1:
        # composed with the device's own eigen_herm on the model's C (= the device's C): the back-transformation is the model's
        lam2, Yv = la.eigen_herm(C)
        assert X.same_bits(lam, lam2), what + ": lambda is not eigen_herm's of C"
        assert X.same_bits(Xv, per_member(lambda l, y: G.solve_model(l, y, True), L, Yv)), what + ": X is not the model's"
    return lam, Xv


# 1. the catalogue: six bounds, the model's bits, subsets
@pytest.mark.parametrize("name", G.NAMES)
def test_catalogue(name):
    A, B = G.inputs(name)
    N = A.shape[-1]
    lam, Xv = model_checks(A, B, name)
    ref = G.golden(name)
    G.check(A, B, lam, Xv, ref, name)
    for sub in ((0, 1), (N - 1, N), (2, 7), (0, N)):
        if sub[1] > N or sub[0] >= sub[1]:
            continue
        ls, Xs = eigen(A, B, subset=sub)
        G.check(A, B, ls, Xs, ref, "%s subset %r" % (name, sub), subset=sub)


# 2. B = I: eigen_herm's bits, in both tiers
@pytest.mark.parametrize("N", [33, 130])
def test_identity_b_gives_eigen_herm(N):
    A = np.array(X.dense(N)[0])
    lam, V = la.eigen_herm(A)
    lg, Xg = eigen(A, np.eye(N, dtype=np.complex128))
    assert X.same_bits(lam, lg) and X.same_bits(V, Xg)
    ls, Xs = eigen(A, np.eye(N, dtype=np.complex128), subset=(1, 5))
    l2, V2 = la.eigen_herm(A, subset=(1, 5))
    assert X.same_bits(ls, l2) and X.same_bits(Xs, V2)


# 3. the sizes at which the kernels can go wrong: tile pitch, the fused kernel's edge (32), the LDS tier's edge (64), hetrd's tier edge
# (96), block edges and remainders
@pytest.mark.parametrize("N", [1, 2, 3, 8, 31, 32, 33, 63, 64, 65, 96, 97, 127, 128, 129, 193])
def test_sizes(N):
    import scipy.linalg
    A, B = G.herm_uniform(G.SEED + 6000 + N, N), G.gram(G.SEED + 6500 + N, N)
    lam, Xv = model_checks(A, B, "N = %d" % N)
    ref = scipy.linalg.eigh(A, B, eigvals_only=True)[::-1]
    G.check(A, B, lam, Xv, ref, "N = %d" % N)


# 4. right-hand sides: K = 1, 3, 64, 65 (a tile of 64 and its remainder), both substitutions, a complex diagonal
@pytest.mark.parametrize("N", [40, 130])
@pytest.mark.parametrize("K", [1, 3, 64, 65])
def test_right_hand_sides(N, K):
    H = np.stack([G.gram(G.SEED + 7000 + N + b, N) for b in range(2)])
    L = both("herm_cholesky_decomp", H)
    Y = G.cmatrix(G.SEED + 7100 + N + K, 2 * N, K).reshape(2, N, K)
    S = both("herm_cholesky_solve", L, Y)
    assert X.same_bits(S, per_member(G.potrs_model, L, Y))
    share = G.solve_share(H, S, Y)
    print("N = %d, K = %d: share of bound 6: %.3g" % (N, K, share))
    assert share <= 1.0
    # a float64 Y is promoted
    assert X.same_bits(both("herm_cholesky_solve", L, np.ascontiguousarray(Y.real)), per_member(G.potrs_model, L, Y.real.astype(np.complex128)))
    # a general lower triangular T with a complex diagonal; what stands above the diagonal is not read
    T = np.tril(G.cmatrix(G.SEED + 7200 + N, 2 * N, N).reshape(2, N, N)) + (2.0 + 1.0j) * np.eye(N)
    for adjoint in (False, True):
        Z = both("ztril_solve", T, Y, adjoint=adjoint)
        assert X.same_bits(Z, per_member(lambda t, y: G.solve_model(t, y, adjoint), T, Y))
        Tn = np.array(T)
        Tn[..., np.triu_indices(N, 1)[0], np.triu_indices(N, 1)[1]] = complex(np.nan, np.nan)
        assert X.same_bits(Z, la.ztril_solve(Tn, Y, adjoint=adjoint))
        op = np.conj(np.swapaxes(T, -1, -2)) if adjoint else T
        assert np.linalg.norm(op @ Z - Y) <= 1e-12 * N * (np.linalg.norm(op) * np.linalg.norm(Z) + np.linalg.norm(Y))
    # the two substitutions in turn are the solve
    assert X.same_bits(S, la.ztril_solve(L, la.ztril_solve(L, Y), adjoint=True))
    # one L for every member
    assert X.same_bits(both("herm_cholesky_solve", L[1], Y)[0], la.herm_cholesky_solve(L[1], Y[0]))
    assert X.same_bits(both("ztril_solve", T[0], Y, adjoint=True)[1], la.ztril_solve(T[0], Y[1], adjoint=True))


# 5. batches
@pytest.mark.parametrize("name", ["shared_4x17", "shared_3x40", "shared_2x130"])   # the fused kernel, the LDS tier above it, the blocked tier
def test_one_shared_b_against_the_stacked_call(name):
    A, B = G.inputs(name)
    lam, Xv = eigen(A, B)
    Bs = np.ascontiguousarray(np.broadcast_to(B, A.shape))
    ls, Xs = eigen(A, Bs)
    assert X.same_bits(lam, ls) and X.same_bits(Xv, Xs)
    l7, X7 = eigen(A, B, subset=(2, 7))
    ls7, Xs7 = eigen(A, Bs, subset=(2, 7))
    assert X.same_bits(l7, ls7) and X.same_bits(X7, Xs7)
    L = la.herm_cholesky_decomp(B)
    assert X.same_bits(both("herm_gen_reduce", A, L), la.herm_gen_reduce(A, np.ascontiguousarray(np.broadcast_to(L, A.shape))))


def test_70000_members_of_order_4():
    base_a = np.stack([G.herm_uniform(G.SEED + 8000 + b, 4) for b in range(7)])
    base_b = np.stack([G.gram(G.SEED + 8100 + b, 4) for b in range(7)])
    idx = np.arange(70000) % 7
    lam, Xv = la.eigen_herm_gen(base_a[idx], base_b[idx])
    l7, X7 = la.eigen_herm_gen(base_a, base_b)
    assert X.same_bits(lam, l7[idx]) and X.same_bits(Xv, X7[idx])
    L = la.herm_cholesky_decomp(base_b[idx])
    assert X.same_bits(L, chol_model(base_b)[idx])
    _, dev = _dev()
    assert X.same_bits(dev.eigenvals_herm_gen(_up(base_a[idx]), _up(base_b[idx])).cpu().numpy(), lam)


@pytest.mark.parametrize("N", [40, 130])
def test_member_isolation_and_exact_scaling_in_a_mixed_batch(N):
    a0, a1 = G.herm_uniform(G.SEED + 8200 + N, N), G.herm_uniform(G.SEED + 8201 + N, N)
    b0, b1 = G.gram(G.SEED + 8210 + N, N), G.graded(G.SEED + 8211 + N, N)
    A = np.stack([a0, X._ldexp(a0, 500), a1, X._ldexp(a0, -500), a0, a0])
    B = np.stack([b0, b0, b1, b0, X._ldexp(b0, 400), X._ldexp(b0, -400)])
    lam, Xv = eigen(A, B)
    l0, X0 = eigen(a0, b0)
    l1, X1 = eigen(a1, b1)
    assert X.same_bits(lam[0], l0) and X.same_bits(Xv[0], X0) and X.same_bits(lam[2], l1) and X.same_bits(Xv[2], X1)
    assert X.same_bits(lam[1], np.ldexp(l0, 500)) and X.same_bits(Xv[1], X0)
    assert X.same_bits(lam[3], np.ldexp(l0, -500)) and X.same_bits(Xv[3], X0)
    assert X.same_bits(lam[4], np.ldexp(l0, -400)) and X.same_bits(Xv[4], X._ldexp(X0, -200))
    assert X.same_bits(lam[5], np.ldexp(l0, 400)) and X.same_bits(Xv[5], X._ldexp(X0, 200))


@pytest.mark.parametrize("N", [5, 40, 130])
def test_what_is_not_read_changes_nothing(N):
    A, B = G.herm_uniform(G.SEED + 8300 + N, N), G.gram(G.SEED + 8310 + N, N)
    lam, Xv = eigen(A, B)
    for fill in (np.nan, 1e300):
        l2, X2 = eigen(G.with_unread(A, fill), G.with_unread(B, fill))
        assert X.same_bits(lam, l2) and X.same_bits(Xv, X2)
        assert X.same_bits(both("herm_cholesky_decomp", G.with_unread(B, fill)), la.herm_cholesky_decomp(B))
    L = la.herm_cholesky_decomp(B)
    assert X.same_bits(la.herm_gen_reduce(G.with_unread(A), L), la.herm_gen_reduce(A, L))


# 6. B not positive definite, A not finite
def _spoil(B, kind):
    B = np.array(B)
    N = B.shape[-1]
    if kind == "negative":
        B[N // 2, N // 2] = -1.0
    elif kind == "zero first":
        B[0, 0] = 0.0
    elif kind == "zero last":                                                # the radicand of the last pivot is exactly 0: no NaN anywhere
        B[:] = np.eye(N)
        B[N - 1, N - 1] = 0.0
    else:
        B[N - 1, 0] = complex(np.nan, 0.0)
        if N == 1:
            B[0, 0] = np.nan
    return B


@pytest.mark.parametrize("N", [1, 3, 40, 130])
@pytest.mark.parametrize("kind", ["negative", "zero first", "zero last", "nan"])
def test_b_not_positive_definite(N, kind):
    _, dev = _dev()
    A = np.stack([G.herm_uniform(G.SEED + 8400 + N + b, N) for b in range(4)])
    good = G.gram(G.SEED + 8410 + N, N)
    bad = _spoil(good, kind)
    want = eigen(A[0], good)
    for member, B in ((1, np.stack([good, bad, bad, good])), (3, np.stack([good, good, good, bad]))):
        for call in (lambda: la.eigen_herm_gen(A, B), lambda: dev.eigenvals_herm_gen(_up(A), _up(B)), lambda: la.eigen_herm_gen(A, B, subset=(0, 1))):
            with pytest.raises(_lib.Nd4HipError, match=NOT_PD % member) as e:
                call()
            assert e.value.code == -5
        for call in (lambda: la.herm_cholesky_decomp(B), lambda: dev.herm_cholesky_decomp(_up(B))):
            with pytest.raises(_lib.Nd4HipError, match=NOT_PD_H % member) as e:
                call()
            assert e.value.code == -5
    with pytest.raises(_lib.Nd4HipError, match=NOT_PD % 0):                   # one shared B
        la.eigen_herm_gen(A, bad)
    got = la.eigen_herm_gen(A[0], good)                                     # the handle computes correctly afterwards
    assert X.same_bits(got[0], want[0]) and X.same_bits(got[1], want[1])


@pytest.mark.parametrize("N", [1, 3, 40, 130])
@pytest.mark.parametrize("fill", [np.nan, np.inf])
def test_a_not_finite(N, fill):
    _, dev = _dev()
    A = np.stack([G.herm_uniform(G.SEED + 8500 + N + b, N) for b in range(3)])
    B = G.gram(G.SEED + 8510 + N, N)
    want = eigen(A[2], B)
    A[1, N - 1, 0] = fill
    for call in (lambda: la.eigen_herm_gen(A, B), lambda: dev.eigen_herm_gen(_up(A), _up(B)), lambda: la.eigenvals_herm_gen(A, B, subset=(0, 1)),
                 lambda: la.eigen_herm_gen(A, np.stack([B, B, B]))):
        with pytest.raises(_lib.Nd4HipError, match=NOT_FINITE) as e:
            call()
        assert e.value.code == -3
    got = la.eigen_herm_gen(A[2], B)
    assert X.same_bits(got[0], want[0]) and X.same_bits(got[1], want[1])


# 7. the limits
def test_2048_cholesky_and_solve():
    N = 2048
    H = G.gram(G.SEED + 9000, N)
    L = la.herm_cholesky_decomp(H)
    s5 = G.chol_share(H, L)
    Y = G.cmatrix(G.SEED + 9001, N, 3)
    S = la.herm_cholesky_solve(L, Y)
    s6 = G.solve_share(H, S, Y)
    print("N = 2048: shares of bounds 5 and 6: %.3g %.3g" % (s5, s6))
    assert s5 <= 1.0 and s6 <= 1.0


def test_600_values_against_lapack():
    import scipy.linalg
    N = 600
    A, B = G.herm_uniform(G.SEED + 9100, N), G.gram(G.SEED + 9101, N)
    lam = la.eigenvals_herm_gen(A, B)
    G.check(A, B, lam, None, scipy.linalg.eigh(A, B, eigvals_only=True)[::-1], "N = 600")


def test_the_2049_refusal_leaves_the_outputs_untouched_and_both_forms_refuse_alike():
    torch, dev = _dev()
    h = _lib.handle(None)
    assert G.mismatches(h.ptr) == []
    src = np.ones(64, dtype=np.complex128)
    outs = [np.full(64, 7.0 + 7.0j) for _ in range(2)]
    p = lambda a: a.ctypes.data  # noqa: E731
    for name, args in (("zpotrf_batched", (1, 2049, p(src), p(outs[0]))), ("zpotrs_batched", (1, 2049, 1, p(src), 0, p(src), p(outs[0]))),
                       ("ztrsm_batched", (1, 2049, 1, 0, p(src), 0, p(outs[0]))), ("zhegst_batched", (1, 2049, p(src), p(src), 0, p(outs[0]))),
                       ("zhegvd_batched", (1, 2049, p(src), p(src), 0, p(outs[0]), p(outs[1]))),
                       ("zhegvx_batched", (1, 2049, 0, 1, p(src), p(src), 0, p(outs[0]), p(outs[1])))):
        assert getattr(h.lib, "nd4hip_" + name + "_host")(h.ptr, *args) == -1
        assert h.lib.nd4hip_last_error().decode() == "nd4hip_%s: N <= 2048" % name
        assert all(np.all(o == 7.0 + 7.0j) for o in outs)
    for call in (lambda: la.herm_cholesky_decomp(np.zeros((2049, 2049), dtype=np.complex128)),
                 lambda: dev.eigen_herm_gen(torch.zeros((2049, 2049), dtype=torch.complex128, device="cuda"), torch.zeros((2049, 2049), dtype=torch.complex128, device="cuda"))):
        with pytest.raises(ValueError, match="N <= 2048"):
            call()


def test_empty_calls():
    _, dev = _dev()
    c = np.complex128
    lam, Xv = la.eigen_herm_gen(np.zeros((0, 4, 4), dtype=c), np.zeros((4, 4), dtype=c))
    assert lam.shape == (0, 4) and Xv.shape == (0, 4, 4)
    lam, Xv = dev.eigen_herm_gen(_up(np.eye(4, dtype=c)), _up(np.eye(4, dtype=c)), subset=(2, 2))
    assert tuple(lam.shape) == (0,) and tuple(Xv.shape) == (4, 0)
    assert la.herm_cholesky_solve(np.eye(3, dtype=c), np.zeros((3, 0), dtype=c)).shape == (3, 0)


def test_profile_record():
    torch, dev = _dev()
    A, B = (_up(m) for m in G.inputs("batch_5x40"))
    h = _lib.handle(0)
    h.profile_enable(True)
    try:
        recs = []
        for call in (lambda: dev.herm_cholesky_decomp(B), lambda: dev.eigen_herm_gen(A, B), lambda: dev.eigenvals_herm_gen(A, B),
                     lambda: dev.eigen_herm_gen(A, B, subset=(0, 8)), lambda: dev.eigenvals_herm_gen(A, B, subset=(0, 8))):
            call()
            recs.append(h.profile_last()[0])
    finally:
        h.profile_enable(False)
    n2, n3 = 40.0 ** 2, 40.0 ** 3
    herm = [16.0 / 3.0 + 2.0 + 8.0, 16.0 / 3.0 + 2.0]                        # eigen_herm's counts, with and without vectors
    red = 4.0 / 3.0 + 8.0
    want = [("zpotrf_batched", 4.0 / 3.0 * n3), ("zhegvd_batched", (herm[0] + red) * n3 + 4.0 * n2 * 40), ("zhegvd_batched", (herm[1] + red) * n3),
            ("zhegvx_batched", (16.0 / 3.0 + red) * n3 + (8.0 + 4.0) * n2 * 8), ("zhegvx_batched", (16.0 / 3.0 + red) * n3)]
    for rec, (op, flops) in zip(recs, want):
        assert rec["op"] == op and rec["valid"] and rec["kernel_ms"] > 0
        assert rec["flops"] == pytest.approx(5 * flops, rel=1e-12)
