"""The symmetric tridiagonal reduction on the device (csrc/sytrd.hip) through la (host arrays) and dev (device tensors):
tridiag_factor, tridiag_apply_q, tridiag_decomp and eigen_sym / eigenvals_sym with reduction='tridiag', inside the bounds of
tests/tridiag_common.py and tests/eigsym_common.py. Tier A is N <= 128 (one workgroup per member), tier B one launch per column
with 64 rows per workgroup; tridiag_apply_q works reflector by reflector for N <= 128 and in blocks of 64 reflectors above.
Largest shares of the 1e-12 bounds on the device (printed per case): reconstruction 1.2e-3, orthogonality 1.3e-3, eigenvalues of T
1.6e-3; under eigen_sym(reduction='tridiag'): values 6.7e-4, residual 2.9e-3, orthogonality 4.2e-3 (with subset: 9.1e-4, 2.1e-3,
4.0e-3)."""
import numpy as np
import pytest

import eigsym_common as C
import eigsym_subset_common as XS
import tridiag_common as X
from nd4js_amd import _lib, la

pytestmark = pytest.mark.gpu

TEXT = "tridiag_decomp(S): S contains NaN or Infinity in its lower triangle."


def _dev():
    import torch
    from nd4js_amd import dev
    return torch, dev


def _up(a):
    torch, _ = _dev()
    return torch.from_numpy(np.array(a, dtype=np.float64, order="C")).cuda()


def factor(S):
    """tridiag_factor through la and through dev: the same bits, the input untouched; returns la's (F, tau, d, e)"""
    torch, dev = _dev()
    keep = np.array(S)
    out = la.tridiag_factor(S)
    assert np.array_equal(S, keep, equal_nan=True)
    t = _up(S)
    before = t.clone()
    outd = dev.tridiag_factor(t)
    assert torch.equal(t, before) or np.isnan(keep).any()
    for a, b in zip(out, outd):
        assert X.same_bits(a, b.cpu().numpy())
    return out


def decomp(S):
    """tridiag_decomp through la and dev, the same bits; returns la's (Q, d, e)"""
    _, dev = _dev()
    out = la.tridiag_decomp(S)
    for a, b in zip(out, dev.tridiag_decomp(_up(S))):
        assert X.same_bits(a, b.cpu().numpy())
    return out


def apply_q(F, tau, Z, transpose=False):
    _, dev = _dev()
    out = la.tridiag_apply_q(F, tau, Z, transpose)
    assert X.same_bits(out, dev.tridiag_apply_q(_up(F), _up(tau), _up(Z), transpose).cpu().numpy())
    return out


# tier A and its cap; tier B: its first size, and 191 / 192 / 193 around the edge of the third block of 64 rows
@pytest.mark.parametrize("N", [1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129, 191, 192, 193])
def test_the_three_bounds(N):
    S, lam = X.dense(N)
    F, tau, d, e = factor(S)
    X.check_layout(F, tau, d, e, "N = %d" % N)
    Q, d2, e2 = decomp(S)
    assert X.same_bits(d2, d) and X.same_bits(e2, e)
    assert X.same_bits(Q, apply_q(F, tau, np.eye(N))), "Q must have the bits of tridiag_apply_q(F, tau, I)"
    sh = X.check(S, Q, d, e, lam, "N = %d" % N)
    print("N = %d shares (reconstruction, orthogonality, values): %.3g %.3g %.3g" % ((N,) + sh))


def test_2048_values_against_lapack():
    S, lam = X.dense(2048)
    F, tau, d, e = la.tridiag_factor(S)
    X.check_layout(F, tau, d, e)
    sh = X.check(S, None, d, e, lam, "N = 2048")
    print("N = 2048 share of the eigenvalue bound: %.3g" % sh[2])


@pytest.mark.parametrize("N", [3, 4, 5])
def test_agrees_with_the_model(N):
    S, _ = X.dense(N)
    F, tau, d, e = factor(S)
    Fm, taum, dm, em = X.model(S)
    tol = X.TOL * np.linalg.norm(S)
    assert np.abs(d - dm).max() <= tol and np.abs(e - em).max() <= tol and np.abs(tau - taum).max() <= tol
    assert np.abs(np.tril(F, -2) - np.tril(Fm, -2)).max() <= tol
    assert np.all(np.sign(e[:N - 2]) == np.sign(em[:N - 2]))


@pytest.mark.parametrize("N", [5, 65, 130])
def test_exact_cases(N):
    eye, zero = np.eye(N), np.zeros(N - 1)
    dd = C.half_steps(X.SEED + 10 + N, N)
    ee = X.rng.fill_uniform(X.SEED + 11 + N, N - 1)
    for S, dw, ew in ((np.diag(dd), dd, zero), (X.tridiag(dd, ee), dd, ee), (np.zeros((N, N)), np.zeros(N), zero)):
        F, tau, d, e = factor(S)
        assert np.array_equal(d, dw) and np.array_equal(e, ew) and not tau.any() and not np.tril(F, -2).any()
        Q, _, _ = decomp(S)
        assert np.array_equal(Q, eye)
    # a block-diagonal S whose second block starts mid-way: column cut-2 keeps its alpha, column cut-1 is zero
    cut = N // 2 + 1
    S = X.block_diagonal(N, cut)
    F, tau, d, e = factor(S)
    assert tau[cut - 2] == 0.0 and e[cut - 2] != 0.0 and tau[cut - 1] == 0.0 and e[cut - 1] == 0.0 and not F[cut:, cut - 2].any()
    if cut >= 4:
        assert tau[cut - 3] != 0.0
    assert tau[cut] != 0.0 or N - cut < 3
    Q, _, _ = decomp(S)
    X.check(S, Q, d, e, np.linalg.eigvalsh(S), "block diagonal %d" % N)


@pytest.mark.parametrize("N", [40, 130])
def test_power_of_two_scaling_is_exact(N):
    S, _ = X.dense(N)
    F, tau, d, e = factor(S)
    Q, _, _ = decomp(S)
    for k in (-500, 500):
        F2, tau2, d2, e2 = factor(np.ldexp(S, k))
        assert X.same_bits(tau2, tau) and X.same_bits(np.tril(F2, -2), np.tril(F, -2))
        assert X.same_bits(d2, np.ldexp(d, k)) and X.same_bits(e2, np.ldexp(e, k))
        assert X.same_bits(decomp(np.ldexp(S, k))[0], Q)


@pytest.mark.parametrize("N,k", [(65, 500), (130, -500)])
def test_batch_members_have_the_bits_of_their_single_runs(N, k):
    B = X.mixed_batch(N, k)
    out = factor(B)
    Q = decomp(B)[0]
    again = la.tridiag_factor(B)
    for a, b in zip(out, again):
        assert X.same_bits(a, b), "two runs of the same call differ"
    assert X.same_bits(Q, la.tridiag_decomp(B)[0])
    for m in range(B.shape[0]):
        single = la.tridiag_factor(B[m])
        for a, b in zip(out, single):
            assert X.same_bits(a[m], b), "member %d differs from its single run" % m
        assert X.same_bits(Q[m], la.tridiag_decomp(B[m])[0])
    order = [3, 0, 4, 2, 1]
    for a, b in zip(out, la.tridiag_factor(B[order])):
        assert X.same_bits(a[order], b), "the order of the members matters"
    assert X.same_bits(Q[order], la.tridiag_decomp(B[order])[0])
    # the dense member and its 2^k multiple
    assert X.same_bits(out[1][4], out[1][0]) and X.same_bits(out[2][4], np.ldexp(out[2][0], k)) and X.same_bits(Q[4], Q[0])
    for m in range(B.shape[0]):
        X.check(B[m], Q[m], out[2][m], out[3][m], None, "member %d" % m)


@pytest.mark.parametrize("N", [40, 130])
def test_upper_triangle_is_ignored_and_s_is_untouched(N):
    S, _ = X.dense(N)
    want = factor(S)
    for fill in (np.nan, 1e300, -np.inf):
        got = factor(C.with_upper(S, fill))
        for a, b in zip(want, got):
            assert X.same_bits(a, b), "upper triangle %r changed the result" % fill


@pytest.mark.parametrize("N", [40, 130])
def test_nan_or_inf_is_noconv_and_the_handle_stays_usable(N):
    torch, dev = _dev()
    S, _ = X.dense(N)
    before = la.tridiag_factor(S)
    for bad in (np.nan, np.inf, -np.inf):
        for at in ((0, 0), (N // 2, N // 2 - 1), (N - 1, N // 3), (N - 1, N - 1)):
            Xb = np.array(S)
            Xb[at] = bad
            for arg in (Xb, np.stack([S, Xb, S])):
                for fn in (la.tridiag_factor, la.tridiag_decomp):
                    with pytest.raises(_lib.Nd4HipError) as err:
                        fn(arg)
                    assert err.value.code == -3 and TEXT in str(err.value)
            with pytest.raises(_lib.Nd4HipError) as err:
                dev.tridiag_factor(_up(np.stack([S, Xb, S])))
            assert err.value.code == -3 and TEXT in str(err.value)
        after = la.tridiag_factor(S)
        for a, b in zip(before, after):
            assert X.same_bits(a, b)


@pytest.mark.parametrize("N", [5, 64, 128, 129, 200])
@pytest.mark.parametrize("K", [1, 8, 0])
def test_apply_q(N, K):
    K = K or N
    S, _ = X.dense(N)
    F, tau, d, e = la.tridiag_factor(S)
    Q = apply_q(F, tau, np.eye(N))
    assert X.same_bits(Q, la.tridiag_decomp(S)[0])
    Z = X.rng.matrix(X.SEED + 50 + N + K, N, K)
    keep = Z.copy()
    QZ = apply_q(F, tau, Z)
    assert np.array_equal(Z, keep)
    nz = np.linalg.norm(Z)
    assert np.linalg.norm(QZ - Q @ Z) <= X.TOL * nz
    assert np.linalg.norm(apply_q(F, tau, QZ, True) - Z) <= X.TOL * nz
    assert np.linalg.norm(apply_q(F, tau, Z, True) - Q.T @ Z) <= X.TOL * nz


def test_apply_q_on_a_batch_and_wide_z():
    B = X.mixed_batch(130, -500)[:4]
    F, tau, d, e = la.tridiag_factor(B)
    Z = np.stack([X.rng.matrix(X.SEED + 70 + m, 130, 300) for m in range(4)])
    QZ = apply_q(F, tau, Z)
    for m in range(4):
        assert X.same_bits(QZ[m], la.tridiag_apply_q(F[m], tau[m], Z[m]))
        assert np.linalg.norm(QZ[m] - X.form_q(F[m], tau[m]) @ Z[m]) <= X.TOL * np.linalg.norm(Z[m])
    S, _ = X.dense(64)
    F, tau, d, e = la.tridiag_factor(S)
    Z = X.rng.matrix(X.SEED + 80, 64, 300)                           # three column tiles of tier A's kernel, the last one partial
    assert np.linalg.norm(apply_q(F, tau, Z) - X.form_q(F, tau) @ Z) <= X.TOL * np.linalg.norm(Z)


def test_both_forms_refuse_every_row_alike():
    h = _lib.handle()
    assert X.mismatches(h.ptr) == []
    h.synchronize()


# ---- eigen_sym(S, reduction='tridiag') --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", C.NAMES)
def test_catalogue_under_the_keyword(name):
    torch, dev = _dev()
    S, lam_ref, V_ref = C.reference(name)
    lam0 = la.eigenvals_sym(S)
    lam, V = la.eigen_sym(S, reduction="tridiag")
    sh = C.check(S, lam, V, lam_ref, name)
    print("%s shares of the bounds (values, residual, orthogonality): %.3g %.3g %.3g" % ((name,) + sh))
    C.check_vectors(S, V, lam_ref, V_ref, name)
    assert np.array_equal(la.eigenvals_sym(S, reduction="tridiag"), lam), "eigenvals_sym must have eigen_sym's bits"
    t = _up(S)
    keep = t.clone()
    ld, vd = dev.eigen_sym(t, reduction="tridiag")
    assert torch.equal(t, keep)
    assert np.array_equal(ld.cpu().numpy(), lam) and np.array_equal(vd.cpu().numpy(), V)
    assert np.array_equal(dev.eigenvals_sym(t, reduction="tridiag").cpu().numpy(), lam)
    X2 = C.with_upper(S, np.nan)
    l2, v2 = la.eigen_sym(X2, reduction="tridiag")
    assert np.array_equal(l2, lam) and np.array_equal(v2, V), "%s: the upper triangle changed the result" % name
    # the default route is the one of before, in the same process
    assert np.array_equal(la.eigenvals_sym(S), lam0) and np.array_equal(la.eigenvals_sym(S, reduction="hessenberg"), lam0)


def _check_subset(S, sub, lam_ref, what):
    """the three bounds of the subset route (eigsym_subset_common.check_subset) per member, through la and dev"""
    _, dev = _dev()
    N, k = S.shape[-1], sub[1] - sub[0]
    lam, V = la.eigen_sym(S, subset=sub, reduction="tridiag")
    assert lam.shape == S.shape[:-2] + (k,) and V.shape == S.shape[:-1] + (k,)
    worst = np.zeros(3)
    for s, l, v, r in zip(S.reshape(-1, N, N), lam.reshape(-1, k), V.reshape(-1, N, k), lam_ref.reshape(-1, N)):
        worst = np.maximum(worst, XS.check_subset(s, l, v, r[sub[0]:sub[1]], what))
    print("%s shares of the bounds (values, residual, orthogonality): %.3g %.3g %.3g" % ((what,) + tuple(worst)))
    assert X.same_bits(la.eigenvals_sym(S, subset=sub, reduction="tridiag"), lam), "eigenvals_sym must have eigen_sym's bits"
    ld, vd = dev.eigen_sym(_up(S), subset=sub, reduction="tridiag")
    assert X.same_bits(ld.cpu().numpy(), lam) and X.same_bits(vd.cpu().numpy(), V)
    return lam, V


@pytest.mark.parametrize("name", C.SMALL)
def test_subset_under_the_keyword(name):
    S, lam_ref, _ = C.reference(name)
    N = S.shape[-1]
    for sub in sorted({(0, 1), (N - 1, N), (0, min(8, N)), (0, N)}):
        lam, V = _check_subset(S, sub, lam_ref, "%s %r" % (name, sub))
        if sub == (0, N):
            C.check(S, lam, V, lam_ref, name)


def test_subset_512_under_the_keyword():
    S, lam = X.dense(512)
    _check_subset(np.array(S), (0, 8), lam[::-1].copy(), "dense 512 (0, 8)")


@pytest.mark.parametrize("k", [-500, 500])
def test_eigen_scaling_is_exact_under_the_keyword(k):
    S = C.reference("batch_2x130")[0][0]
    lam, V = la.eigen_sym(S, reduction="tridiag")
    l2, v2 = la.eigen_sym(np.ldexp(S, k), reduction="tridiag")
    assert np.array_equal(l2, np.ldexp(lam, k)) and np.array_equal(v2, V)
    S = C.reference("batch_5x40")[0][0]
    lam, V = la.eigen_sym(S, reduction="tridiag", subset=(0, 8))
    l2, v2 = la.eigen_sym(np.ldexp(S, k), reduction="tridiag", subset=(0, 8))
    assert np.array_equal(l2, np.ldexp(lam, k)) and np.array_equal(v2, V)


def test_eigen_small_sizes_nan_and_empty_subset_under_the_keyword():
    lam, V = la.eigen_sym(np.array([[[-2.5]], [[0.0]]]), reduction="tridiag")
    assert np.array_equal(lam, [[-2.5], [0.0]]) and np.array_equal(V, np.ones((2, 1, 1)))
    S = np.array([[2.0, 7.0], [1.0, -1.0]])                           # the upper 7 is not read
    lam, V = la.eigen_sym(S, reduction="tridiag")
    l0, V0 = la.eigen_sym(S)
    assert np.array_equal(lam, l0) and np.array_equal(V, V0)       # N = 2 runs no reflector: the same T, the same solver
    assert np.array_equal(la.eigen_sym(S, reduction="tridiag", subset=(0, 2))[0], la.eigen_sym(S, subset=(0, 2))[0])
    lam, V = la.eigen_sym(np.eye(4), subset=(2, 2), reduction="tridiag")
    assert lam.shape == (0,) and V.shape == (4, 0)
    for N in (40, 130):
        S = np.array(X.dense(N)[0])
        before = la.eigen_sym(S, reduction="tridiag")
        B = np.stack([S, S, S])
        B[1, N - 1, N // 2] = np.nan
        for kw in ({}, {"subset": (0, 3)}):
            for fn in (la.eigen_sym, la.eigenvals_sym):
                with pytest.raises(_lib.Nd4HipError) as err:
                    fn(B, reduction="tridiag", **kw)
                assert err.value.code == -3 and "eigen_sym(S): S contains NaN or Infinity in its lower triangle." in str(err.value)
        after = la.eigen_sym(S, reduction="tridiag")
        assert np.array_equal(after[0], before[0]) and np.array_equal(after[1], before[1])


@pytest.mark.parametrize("r", [1, 5, 20])
def test_rank_deficient_inputs_under_the_keyword(r):
    """the reduction works from the top, so the rounding noise of a rank-deficient S fills the tail of T; without syev_tr_deflate the
    solver's own assertion (svd_dc.js:206) failed on 6 of these 18 inputs"""
    for seed in range(6):
        x = X.rng.matrix(9000 + 100 * 50 + 10 * r + seed, 50, r)
        S = X.sym(x @ x.T)
        lam, V = la.eigen_sym(S, reduction="tridiag")
        C.check(S, lam, V, np.linalg.eigvalsh(S)[::-1], "rank %d seed %d" % (r, seed))


def test_profile_records():
    torch, dev = _dev()
    S = _up(C.reference("dense_70")[0])
    h = _lib.handle(0)
    h.profile_enable(True)
    try:
        F, tau, d, e = dev.tridiag_factor(S)
        rec_f = h.profile_last()[0]
        dev.tridiag_apply_q(F, tau, torch.eye(70, dtype=torch.float64, device="cuda")[:, :8].contiguous())
        rec_q = h.profile_last()[0]
        dev.eigen_sym(S, reduction="tridiag")
        rec = h.profile_last()[0]
        stages = h.eigsym_last_stages()
        dev.eigenvals_sym(S, reduction="tridiag")
        rec2 = h.profile_last()[0]
        dev.eigen_sym(S, reduction="tridiag", subset=(0, 8))
        rec3 = h.profile_last()[0]
        stages3 = h.eigsym_subset_last_stages()
    finally:
        h.profile_enable(False)
    n3 = 70.0 ** 3
    assert rec_f["op"] == "dsytrd_batched" and rec_f["flops"] == pytest.approx(4.0 / 3.0 * n3, rel=1e-12)
    assert rec_q["op"] == "dormtr_batched" and rec_q["flops"] == pytest.approx(2.0 * 70.0 ** 2 * 8, rel=1e-12)
    assert rec["op"] == "dsyevd_tr_batched" and rec["flops"] == pytest.approx((4.0 / 3.0 + 4.0) * n3, rel=1e-12)
    assert rec2["op"] == "dsyevd_tr_batched" and rec2["flops"] == pytest.approx((4.0 / 3.0 + 2.0) * n3, rel=1e-12)
    assert rec3["op"] == "dsyevx_tr_batched" and rec3["flops"] == pytest.approx(4.0 / 3.0 * n3 + 2.0 * 70.0 ** 2 * 8, rel=1e-12)
    assert rec["valid"] and rec["kernel_ms"] > 0
    assert set(stages) == set(h.EIGSYM_STAGES) and stages["symm"] == 0.0 and all(v > 0 for k, v in stages.items() if k != "symm")
    assert set(stages3) == set(h.EIGSYM_SUBSET_STAGES) and stages3["symm"] == 0.0 and stages3["reduce"] > 0 and stages3["bisect"] > 0
