"""The Hermitian tridiagonal reduction and eigenproblem on the device (csrc/hetrd.hip) through la (host arrays) and dev (device
tensors): herm_tridiag_factor, herm_tridiag_apply_q, herm_tridiag_decomp, eigen_herm and eigenvals_herm, inside the bounds of
tests/herm_common.py. Every call goes through both layers and must give the same bits with the input untouched. Tier A is N <= 96
(one workgroup per member), tier B one launch per column with 64 rows per workgroup; herm_tridiag_apply_q works reflector by
reflector for N <= 96 and in blocks of 64 reflectors above. The shares of the 1e-12 bounds are printed per case; the largest seen on
the device (also in DESIGN.md 4.24): reconstruction 1.5e-3, unitarity 1.6e-3, eigenvalues of T 2.0e-3; under eigen_herm: values
9.6e-4, residual 3.7e-3, orthonormality 4.4e-3 (with subset: 5.5e-4, 3.4e-3, 4.4e-3)."""
import numpy as np
import pytest

import herm_common as X
from nd4js_amd import _lib, la

pytestmark = pytest.mark.gpu

TEXT = "herm_tridiag_decomp(H): H contains NaN or Infinity in its lower triangle."
TEXT_EIG = "eigen_herm(H): H contains NaN or Infinity in its lower triangle."
CAP = X.CAP


def _dev():
    import torch
    from nd4js_amd import dev
    return torch, dev


def _up(a):
    torch, _ = _dev()
    return torch.from_numpy(np.array(a, order="C")).cuda()


def factor(H):
    """herm_tridiag_factor through la and through dev: the same bits, the input untouched; returns la's (F, tau, d, e)"""
    torch, dev = _dev()
    keep = np.array(H)
    out = la.herm_tridiag_factor(H)
    assert X.same_bits(np.array(H), keep)
    t = _up(H)
    before = t.clone()
    outd = dev.herm_tridiag_factor(t)
    assert X.same_bits(t.cpu().numpy(), before.cpu().numpy())
    for a, b in zip(out, outd):
        assert X.same_bits(a, b.cpu().numpy())
    return out


def decomp(H):
    _, dev = _dev()
    out = la.herm_tridiag_decomp(H)
    for a, b in zip(out, dev.herm_tridiag_decomp(_up(H))):
        assert X.same_bits(a, b.cpu().numpy())
    return out


def apply_q(F, tau, Z, adjoint=False):
    _, dev = _dev()
    out = la.herm_tridiag_apply_q(F, tau, Z, adjoint)
    assert X.same_bits(out, dev.herm_tridiag_apply_q(_up(F), _up(tau), _up(Z), adjoint).cpu().numpy())
    return out


def eigen(H, subset=None):
    """eigen_herm and eigenvals_herm through la and dev: the same bits, the values alone the bits of the pairs'; returns la's (lam, V)"""
    _, dev = _dev()
    keep = np.array(H)
    lam, V = la.eigen_herm(H, subset=subset)
    assert X.same_bits(np.array(H), keep)
    t = _up(H)
    lamd, Vd = dev.eigen_herm(t, subset=subset)
    assert X.same_bits(t.cpu().numpy(), keep)
    assert X.same_bits(lam, lamd.cpu().numpy()) and X.same_bits(V, Vd.cpu().numpy())
    assert X.same_bits(lam, la.eigenvals_herm(H, subset=subset)) and X.same_bits(lam, dev.eigenvals_herm(t, subset=subset).cpu().numpy())
    return lam, V


# 1. tier A and its cap; tier B: 127 / 128 / 129 and 191 / 192 / 193 around the edges of its row blocks; 65, 66 (64 and 65 reflectors) and
# 130 (129: two blocks and one) where the reflector count crosses a WY block
@pytest.mark.parametrize("N", [1, 2, 3, 4, 5, 65, 66, CAP - 1, CAP, CAP + 1, 127, 128, 129, 130, 191, 192, 193])
def test_reduction_q_and_the_three_bounds(N):
    H, lam = X.dense(N)
    F, tau, d, e = factor(H)
    X.check_layout(F, tau, d, e, "N = %d" % N)
    Q, d2, e2 = decomp(H)
    assert X.same_bits(d2, d) and X.same_bits(e2, e)
    assert X.same_bits(Q, apply_q(F, tau, np.eye(N))), "Q must have the bits of herm_tridiag_apply_q(F, tau, I)"
    X.check(H, Q, d, e, lam, "N = %d" % N)
    Fm, taum, dm, em = X.model(H)
    tol = X.TOL * X.norm_of(H)
    assert np.abs(d - dm).max() <= tol
    if N > 1:
        assert np.abs(e - em).max() <= tol and np.abs(tau - taum).max() <= tol and np.abs(np.tril(F, -2) - np.tril(Fm, -2)).max() <= tol


# 2. a Z that is not square, one N per tier
@pytest.mark.parametrize("N", [40, 150])
@pytest.mark.parametrize("K", [1, 127, 129])
def test_apply_q_on_a_non_square_z(N, K):
    H, _ = X.dense(N)
    F, tau, d, e = la.herm_tridiag_factor(H)
    Z = X.rng.matrix(X.SEED + 9000 + K, N, K) + 1j * X.rng.matrix(X.SEED + 9500 + K, N, K)
    QZ = apply_q(F, tau, Z)
    back = apply_q(F, tau, QZ, True)
    share = np.linalg.norm(back - Z) / (X.TOL * np.linalg.norm(Z))
    print("N = %d K = %d: ||Q^H (Q Z) - Z|| is %.3g of its bound" % (N, K, share))
    assert share <= 1.0
    # against the model's reflector-by-reflector product, and Q^H Z the other way
    assert np.linalg.norm(QZ - X.apply_q(F, tau, Z)) <= X.TOL * np.linalg.norm(Z)
    assert np.linalg.norm(apply_q(F, tau, Z, True) - X.apply_q(F, tau, Z, True)) <= X.TOL * np.linalg.norm(Z)
    # a float64 Z is promoted
    assert X.same_bits(apply_q(F, tau, Z.real), apply_q(F, tau, Z.real.astype(np.complex128)))


# 3. the path that only the complex case has
@pytest.mark.parametrize("N", [2, 5, 130])
def test_complex_tridiagonal_pure_phase_reflectors(N):
    H = X.complex_tridiag(N)
    F, tau, d, e = factor(H)
    X.check_layout(F, tau, d, e)
    assert not np.tril(F, -2).any() and np.all(tau != 0.0)
    eps = np.finfo(float).eps
    dev_e, dev_d = np.abs(np.abs(e) - np.abs(np.diag(H, -1))).max() / eps, np.abs(d - np.diag(H).real).max() / eps
    print("complex tridiagonal %d: ||e_k| - |h_k+1,k|| is %.2f eps, |d - Re diag| %.2f eps" % (N, dev_e, dev_d))
    # the bounds and their reasoning: test_herm_host.py. Measured on the device: 0.5 / 0.5 / 1.5 eps for e and 0 / 0 / 2 eps for d
    # at N = 2 / 5 / 130
    assert dev_e <= 16 and dev_d <= 8
    Q, _, _ = decomp(H)
    X.check(H, Q, d, e, np.linalg.eigvalsh(H), "complex tridiagonal %d" % N)


def test_the_2x2_phase_case():
    F, tau, d, e = factor(np.array([[1.0, 99.0], [3.0 + 4.0j, 2.0]], dtype=np.complex128))
    assert tau[0] == 1.6 + 0.8j and e[0] == -5.0 and d[0] == 1.0 and abs(d[1] - 2.0) <= 4 * np.finfo(float).eps


def test_a_tiny_complex_coupling_stays_finite():
    X.check_tiny_coupling(factor)
    H = X.block_diagonal(12, 5)
    H[5, 4] = (1.0 - 2.0j) * 1e-165
    F, tau, d, e = factor(H)
    assert np.all(np.isfinite(tau)) and tau[4] != 0.0
    X.check(H, decomp(H)[0], d, e, np.linalg.eigvalsh(X.herm(H)), "tiny coupling 12")
    for sub in (None, (0, 3)):
        lam, V = eigen(H, subset=sub)
        X.eig_check(H, lam, V, X.descending(H), None if sub is None else slice(*sub), "tiny coupling 12 %s" % (sub,))


@pytest.mark.parametrize("N", [5, CAP, 130])
def test_diagonal_zero_and_real_symmetric(N):
    D = np.diag(X.C.half_steps(X.SEED + N, N)).astype(np.complex128)
    F, tau, d, e = factor(D)
    assert X.same_bits(F, D) and not tau.any() and not e.any() and np.array_equal(d, np.diag(D).real)
    assert X.same_bits(decomp(D)[0], np.eye(N, dtype=np.complex128))
    Zr = np.zeros((N, N), dtype=np.complex128)
    F, tau, d, e = factor(Zr)
    assert not F.any() and not tau.any() and not d.any() and not e.any()
    S = X.real_symmetric(N)
    F, tau, d, e = factor(S)
    assert not F.imag.any() and not tau.imag.any() and tau[-1] == 0.0
    Q, _, _ = decomp(S)
    assert not Q.imag.any()
    X.check(S, Q, d, e, np.linalg.eigvalsh(S.real), "real symmetric %d" % N)
    Fs, taus, ds, es = la.tridiag_factor(np.ascontiguousarray(S.real))
    tol = X.TOL * X.norm_of(S)
    assert np.abs(d - ds).max() <= tol and np.abs(e - es).max() <= tol and np.abs(tau.real - taus).max() <= tol


# 4. what is not read, and what is refused
@pytest.mark.parametrize("N", [7, CAP, 130])
def test_the_upper_triangle_and_the_diagonals_imaginary_part_are_not_read(N):
    H, _ = X.dense(N)
    clean = factor(H)
    dirty = factor(X.with_unread(H))
    for a, b in zip(clean, dirty):
        assert X.same_bits(a, b)
    lam, V = eigen(H)
    lam2, V2 = eigen(X.with_unread(H))
    assert X.same_bits(lam, lam2) and X.same_bits(V, V2)
    lam3, V3 = eigen(X.with_unread(H), subset=(0, 3))
    lam4, V4 = eigen(H, subset=(0, 3))
    assert X.same_bits(lam3, lam4) and X.same_bits(V3, V4)


@pytest.mark.parametrize("N", [1, 6, CAP + 4])
@pytest.mark.parametrize("bad", [np.nan, np.inf, 1j * np.inf])
def test_nan_or_inf_in_the_lower_triangle_is_refused_and_the_handle_stays_usable(N, bad):
    torch, dev = _dev()
    H, _ = X.dense(N if N > 1 else 2)
    H = np.array(H[:N, :N])
    before = la.herm_tridiag_factor(H)
    lam_before = la.eigen_herm(H)
    B = np.array(H)
    B[N - 1, 0] = bad if N > 1 else np.real(bad) if np.isreal(bad) else np.inf
    calls = [(lambda: la.herm_tridiag_factor(B), TEXT), (lambda: dev.herm_tridiag_factor(_up(B)), TEXT),
             (lambda: la.eigen_herm(B), TEXT_EIG), (lambda: dev.eigenvals_herm(_up(B)), TEXT_EIG),
             (lambda: la.eigen_herm(B, subset=(0, 1)), TEXT_EIG), (lambda: dev.eigen_herm(_up(B), subset=(0, 1)), TEXT_EIG)]
    for call, text in calls:
        with pytest.raises(_lib.Nd4HipError) as err:
            call()
        assert err.value.code == -3 and text in str(err.value)
        after = la.herm_tridiag_factor(H)
        for a, b in zip(before, after):
            assert X.same_bits(a, b)
    for a, b in zip(lam_before, la.eigen_herm(H)):
        assert X.same_bits(a, b)


# 5. member isolation and the exact scaling
@pytest.mark.parametrize("N", [24, 130])
def test_members_of_a_mixed_batch_have_the_bits_they_have_alone(N):
    B = X.mixed_batch(N, 500)
    out = factor(B)
    Q = decomp(B)[0]
    lam, V = eigen(B)
    lams, Vs = eigen(B, subset=(1, 4))
    for b in range(B.shape[0]):
        alone = factor(B[b])
        for a, o in zip(alone, out):
            assert X.same_bits(a, o[b]), "member %d" % b
        assert X.same_bits(decomp(B[b])[0], Q[b])
        l1, v1 = eigen(B[b])
        assert X.same_bits(l1, lam[b]) and X.same_bits(v1, V[b])
        l2, v2 = eigen(B[b], subset=(1, 4))
        assert X.same_bits(l2, lams[b]) and X.same_bits(v2, Vs[b])
    # the eigen routes at an extreme exponent. The full route works on the scaled d and e, which are the dense member's: its values
    # scale exactly and its vectors keep their bits. The subset route hands the unscaled d and e to the tridiagonal solver: the bounds
    ref = np.ldexp(X.descending(B[0]), 500)
    assert np.array_equal(lam[4], np.ldexp(lam[0], 500)) and X.same_bits(V[4], V[0])
    X.eig_check(B[4], lams[4], Vs[4], ref, slice(1, 4), "2^500 dense %d subset (1, 4)" % N)
    F, tau, d, e = out
    assert X.same_bits(tau[4], tau[0]) and X.same_bits(np.tril(F[4], -2), np.tril(F[0], -2)) and X.same_bits(Q[4], Q[0])
    assert np.array_equal(d[4], np.ldexp(d[0], 500)) and np.array_equal(e[4], np.ldexp(e[0], 500))
    down = factor(X._ldexp(B[0], -500))
    assert X.same_bits(down[1], tau[0]) and X.same_bits(np.tril(down[0], -2), np.tril(F[0], -2))
    assert np.array_equal(down[2], np.ldexp(d[0], -500)) and np.array_equal(down[3], np.ldexp(e[0], -500))


# 6. the eigenproblem
EIGEN_INPUTS = {
    "dense_1": lambda: np.array(X.dense(1)[0]), "dense_2": lambda: np.array(X.dense(2)[0]), "dense_3": lambda: np.array(X.dense(3)[0]),
    "dense_33": lambda: np.array(X.dense(33)[0]), "dense_cap": lambda: np.array(X.dense(CAP)[0]), "dense_130": lambda: np.array(X.dense(130)[0]),
    "dense_600": lambda: np.array(X.dense(600)[0]), "batch_5x40": X.batch_5x40, "kron_pairs_60": lambda: X.kron_pairs(30),
    "kron_pairs_140": lambda: X.kron_pairs(70), "rank5_50": lambda: X.rank5(50), "negdef_50": lambda: X.negdef(50),
    "complex_tridiag_130": lambda: X.complex_tridiag(130),
}


@pytest.mark.parametrize("name", list(EIGEN_INPUTS))
def test_eigen_herm_inside_the_three_bounds(name):
    H = EIGEN_INPUTS[name]()
    lam, V = eigen(H)
    assert lam.shape == H.shape[:-1] and V.shape == H.shape
    X.eig_check(H, lam, V, X.descending(H), None, name)
    if H.shape[-1] == 1:
        assert lam[0] == H[0, 0].real and V[0, 0] == 1.0


# 7. subsets
@pytest.mark.parametrize("name", ["dense_40", "dense_130", "dense_600", "batch_5x40"])
def test_subset_inside_the_bounds(name):
    H = X.batch_5x40() if name == "batch_5x40" else np.array(X.dense(int(name[6:]))[0])
    N = H.shape[-1]
    full = la.eigenvals_herm(H)
    ref = X.descending(H)
    for i0, i1 in ((0, 8), (N - 3, N), (0, N)):
        lam, V = eigen(H, subset=(i0, i1))
        assert lam.shape == H.shape[:-2] + (i1 - i0,) and V.shape == H.shape[:-1] + (i1 - i0,)
        X.eig_check(H, lam, V, ref, slice(i0, i1), "%s subset (%d, %d)" % (name, i0, i1))
        # within the bound of the full call's values
        nrm = np.array([X.norm_of(h) for h in H.reshape(-1, N, N)]).reshape(H.shape[:-2] + (1,))
        assert np.all(np.abs(lam - full[..., i0:i1]) <= X.TOL * nrm)


def test_empty_and_ill_formed_subsets():
    _, dev = _dev()
    H = np.array(X.dense(12)[0])
    lam, V = la.eigen_herm(H, subset=(5, 5))
    assert lam.shape == (0,) and V.shape == (12, 0)
    lamd, Vd = dev.eigen_herm(_up(H), subset=(5, 5))
    assert tuple(lamd.shape) == (0,) and tuple(Vd.shape) == (12, 0)
    for bad in ((3, 2), (0, 13), (-1, 2), (1,), "ab"):
        for call in (lambda: la.eigen_herm(H, subset=bad), lambda: dev.eigenvals_herm(_up(H), subset=bad)):
            with pytest.raises(ValueError, match=r"subset must be \(i0, i1\) with 0 <= i0 <= i1 <= N"):
                call()
    assert X.mismatches(_lib.handle(None).ptr) == []


# 8. at the limit
def test_2048_values_against_lapack_and_the_2049_refusal():
    H, lam = X.dense(2048)
    F, tau, d, e = la.herm_tridiag_factor(H)
    X.check_layout(F, tau, d, e)
    X.check(H, None, d, e, lam, "N = 2048")
    torch, dev = _dev()
    with pytest.raises(ValueError, match="N <= 2048"):
        la.herm_tridiag_factor(np.zeros((2049, 2049), dtype=np.complex128))
    with pytest.raises(ValueError, match="N <= 2048"):
        dev.herm_tridiag_factor(torch.zeros((2049, 2049), dtype=torch.complex128, device="cuda"))
    with pytest.raises(_lib.Nd4HipError, match="N <= 2048"):
        la.eigenvals_herm(np.zeros((2049, 2049), dtype=np.complex128))
