"""Selected eigenpairs on the device (csrc/syevx.hip) through la (host arrays) and dev (device tensors): tridiag_count and
tridiag_eigenvals return the bits of the numpy model of tests/eigsym_subset_common.py; tridiag_eigen and eigen_sym(S, subset) are
held to the project's three 1e-12 bounds against LAPACK, tridiag_eigen inside 4 x max(the model's share, N 2^-52 / 1e-12) as well."""
import numpy as np
import pytest

import eigsym_common as C
import eigsym_subset_common as X
from nd4js_amd import _lib, la, rng

pytestmark = pytest.mark.gpu
SIZES = (1, 2, 3, 64, 65, 257)


def _dev():
    import torch
    from nd4js_amd import dev
    return torch, dev


def _tri(N, seed=7700):
    return rng.fill_uniform(seed + N, N), rng.fill_uniform(seed + 5000 + N, N - 1)


def _up(a):
    import torch
    return torch.from_numpy(np.array(a)).cuda()


# ---- tridiag_count ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", SIZES)
def test_count_has_the_bits_of_the_model(N):
    torch, dev = _dev()
    d, e = _tri(N)
    p = X.prepare(d, e)
    g = np.ldexp(p["g"], p["lexp"])
    for M in (1, 64, 65):
        x = 1.5 * g * rng.fill_uniform(7800 + N, M, offset=M)
        x[:2] = (g, -g)[:min(M, 2)]
        want = X.count(d, e, x)
        got = la.tridiag_count(d, e, x)
        assert got.dtype == np.int32 and np.array_equal(got, want), (N, M)
        assert np.array_equal(dev.tridiag_count(_up(d), _up(e), _up(x)).cpu().numpy(), want), (N, M)
    # probes exactly on the eigenvalues of a diagonal T, and a batch whose members have probes of their own
    dd, ee = np.rint(4.0 * d), np.zeros(max(N - 1, 0))
    x = np.concatenate((dd, [dd.max() + 1.0, dd.min() - 1.0]))
    want = X.count(dd, ee, x)
    assert want.tolist() == [int((dd > v).sum()) for v in x]
    assert np.array_equal(la.tridiag_count(dd, ee, x), want)
    x2 = np.stack((x, x[::-1] * 0.5))
    got = la.tridiag_count(np.stack((dd, d)), np.stack((ee, e)), x2)
    assert np.array_equal(got[0], want) and np.array_equal(got[1], X.count(d, e, x2[1]))


# ---- tridiag_eigenvals --------------------------------------------------------------------------------------------------------------
def _value_subsets(N):
    subs = {(0, 1), (N - 1, N), (0, N)}
    if N == 65:
        subs |= {(0, 64), (1, 65)}
    if N > 65:
        subs |= {(N // 2 - 32, N // 2 + 32), (N // 2 - 32, N // 2 + 33)}
    return sorted(subs)


@pytest.mark.parametrize("N", SIZES)
def test_eigenvals_have_the_bits_of_the_model(N):
    torch, dev = _dev()
    d, e = _tri(N)
    p = X.prepare(d, e)
    for sub in _value_subsets(N):
        want = X.bisect(p, *sub)[1]
        assert X.same_bits(la.tridiag_eigenvals(d, e, subset=sub), want), (N, sub)
        assert X.same_bits(dev.tridiag_eigenvals(_up(d), _up(e), subset=sub).cpu().numpy(), want), (N, sub)
    assert X.same_bits(la.tridiag_eigenvals(d, e), X.bisect(p, 0, N)[1])
    assert X.same_bits(la.tridiag_eigen(d, e, subset=(0, 1))[0], X.bisect(p, 0, 1)[1])


def test_eigenvals_at_the_lds_cap():
    d, e = _tri(2048)
    p = X.prepare(d, e)
    for sub in ((0, 4), (1022, 1026)):
        assert X.same_bits(la.tridiag_eigenvals(d, e, subset=sub), X.bisect(p, *sub)[1]), sub
    x = X.bisect(p, 0, 4)[1] + 1e-9
    assert la.tridiag_count(d, e, x).tolist() == [0, 1, 2, 3]
    lam, Z = la.tridiag_eigen(d, e, subset=(2044, 2048))
    X.check_subset(X.tridiag(d, e), lam, Z, np.linalg.eigvalsh(X.tridiag(d, e))[::-1][2044:], "N = 2048")


# ---- tridiag_eigen ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", tuple(X.TRIDIAGS))
def test_eigen_inside_the_gate_of_the_model(name):
    torch, dev = _dev()
    d, e = X.tridiag_input(name)
    N, T, ref = len(d), X.tridiag(*X.tridiag_input(name)), X.tridiag_reference(name)
    lam_m, Z_m, _ = X.tridiag_model(name)
    model = X.subset_shares(T, lam_m, Z_m, ref)
    lam, Z = la.tridiag_eigen(d, e)
    device = X.check_subset(T, lam, Z, ref, name)
    assert X.same_bits(lam, lam_m) and X.signs_ok(Z)
    floor = N * X.EPS / X.TOL
    for what, dv, md in zip(("values", "residual", "orthogonality"), device, model):
        gate = 4.0 * max(md, floor)
        print("%s %s: device %.3g model %.3g gate %.3g" % (name, what, dv, md, gate))
        assert dv <= gate, "%s %s: the device's share %.3g exceeds 4 x max(model %.3g, floor %.3g)" % (name, what, dv, md, floor)
    # the same bits from the device form, from a second run and from the values alone
    ld, Zd = dev.tridiag_eigen(_up(d), _up(e))
    assert X.same_bits(ld.cpu().numpy(), lam) and X.same_bits(Zd.cpu().numpy(), Z)
    l2, Z2 = la.tridiag_eigen(d, e)
    assert X.same_bits(l2, lam) and X.same_bits(Z2, Z)
    assert X.same_bits(la.tridiag_eigenvals(d, e), lam)


@pytest.mark.parametrize("m", [500, -500])
def test_eigen_power_of_two_scaling_is_exact(m):
    d, e = X.tridiag_input("dense_50")
    lam, Z = la.tridiag_eigen(d, e, subset=(3, 20))
    lam2, Z2 = la.tridiag_eigen(np.ldexp(d, m), np.ldexp(e, m), subset=(3, 20))
    assert X.same_bits(lam2, np.ldexp(lam, m)) and X.same_bits(Z2, Z)


def test_a_subset_that_cuts_a_cluster():
    d, e = X.tridiag_input("clusters_40")                       # 2 twenty times, then 1 twenty times
    T, ref = X.tridiag(d, e), X.tridiag_reference("clusters_40")
    for sub in ((10, 30), (0, 5), (19, 21), (35, 40)):
        lam, Z = la.tridiag_eigen(d, e, subset=sub)
        X.check_subset(T, lam, Z, ref[sub[0]:sub[1]], "clusters_40 %s" % (sub,))
        assert X.signs_ok(Z)
        assert X.same_bits(lam, la.tridiag_eigenvals(d, e)[sub[0]:sub[1]])


def _mixed_batch():
    d0, e0 = X.tridiag_input("clusters_40")
    d1, e1 = _tri(40)
    d = np.stack((d1, np.rint(4.0 * d1), np.zeros(40), d0, np.ldexp(d1, 300), np.ldexp(d1, -700)))
    e = np.stack((e1, np.zeros(39), np.zeros(39), e0, np.ldexp(e1, 300), np.ldexp(e1, -700)))
    return d, e


@pytest.mark.parametrize("sub", [(0, 40), (5, 13)])
def test_members_of_a_mixed_batch_equal_their_single_runs(sub):
    d, e = _mixed_batch()
    lam, Z = la.tridiag_eigen(d, e, subset=sub)
    assert lam.shape == (6, sub[1] - sub[0]) and Z.shape == (6, 40, sub[1] - sub[0])
    for b in range(len(d)):
        l1, Z1 = la.tridiag_eigen(d[b], e[b], subset=sub)
        assert X.same_bits(lam[b], l1) and X.same_bits(Z[b], Z1), b
        T = X.tridiag(d[b], e[b])
        X.check_subset(T, l1, Z1, np.linalg.eigvalsh(T)[::-1][sub[0]:sub[1]], "member %d" % b)
    assert X.same_bits(lam[4], np.ldexp(lam[0], 300)) and X.same_bits(Z[4], Z[0]) and X.same_bits(Z[5], Z[0])
    assert np.array_equal(Z[2], np.eye(40)[:, sub[0]:sub[1]]) and not lam[2].any()          # the zero member: the unit vectors in order


def test_tridiag_nan_or_inf_is_noconv_and_the_handle_stays_usable():
    d, e = _mixed_batch()
    before = la.tridiag_eigen(d, e, subset=(0, 3))
    for where, value in (("d", np.nan), ("e", np.inf), ("d", -np.inf)):
        bad_d, bad_e = d.copy(), e.copy()
        (bad_d if where == "d" else bad_e)[3, 7] = value
        for fn in (la.tridiag_eigen, la.tridiag_eigenvals):
            with pytest.raises(_lib.Nd4HipError) as err:
                fn(bad_d, bad_e, subset=(0, 3))
            assert err.value.code == -3 and "tridiag_eigen(d,e): d or e contains NaN or Infinity." in str(err.value)
        after = la.tridiag_eigen(d, e, subset=(0, 3))
        assert X.same_bits(after[0], before[0]) and X.same_bits(after[1], before[1])


# ---- eigen_sym(S, subset) and eigenvals_sym(S, subset) ---------------------------------------------------------------------------------
def _dense_512():
    return C.sym_uniform(7100 + 512, 512)


_REF_512 = []


def _reference(name):
    if name != "dense_512":
        return C.reference(name)[:2]
    if not _REF_512:
        S = _dense_512()
        _REF_512.extend((S, np.linalg.eigvalsh(S)[::-1].copy()))
    return _REF_512


@pytest.mark.parametrize("name", C.SMALL + ("dense_512",))
def test_catalogue_subsets_through_la_and_dev(name):
    torch, dev = _dev()
    S, lam_ref = _reference(name)
    N = S.shape[-1]
    t = _up(S)
    keep = t.clone()
    for sub in sorted({(0, 1), (N - 1, N), (0, min(8, N)), (0, N)}):
        k = sub[1] - sub[0]
        lam, V = la.eigen_sym(S, subset=sub)
        assert lam.shape == S.shape[:-2] + (k,) and V.shape == S.shape[:-1] + (k,)
        worst = np.zeros(3)
        for s, l, v, r in zip(S.reshape(-1, N, N), lam.reshape(-1, k), V.reshape(-1, N, k), lam_ref.reshape(-1, N)):
            worst = np.maximum(worst, X.check_subset(s, l, v, r[sub[0]:sub[1]], "%s %s" % (name, sub)))
        print("%s %s shares of the bounds (values, residual, orthogonality): %.3g %.3g %.3g" % ((name, sub) + tuple(worst)))
        if sub == (0, N):
            C.check(S, lam, V, lam_ref, name)
        assert X.same_bits(la.eigenvals_sym(S, subset=sub), lam), "eigenvals_sym must have eigen_sym's bits"
        ld, vd = dev.eigen_sym(t, subset=sub)
        assert X.same_bits(ld.cpu().numpy(), lam) and X.same_bits(vd.cpu().numpy(), V)
        assert X.same_bits(dev.eigenvals_sym(t, subset=sub).cpu().numpy(), lam) and torch.equal(t, keep)
    # the upper triangle is ignored: NaN and garbage there change no bit; S itself is never written
    sub = (0, min(8, N))
    lam, V = la.eigen_sym(S, subset=sub)
    for fill in (np.nan, 1e300):
        A = C.with_upper(S, fill)
        before = A.copy()
        l2, v2 = la.eigen_sym(A, subset=sub)
        assert np.array_equal(A, before, equal_nan=True)
        assert X.same_bits(l2, lam) and X.same_bits(v2, V), "%s: upper triangle %r changed the result" % (name, fill)


@pytest.mark.parametrize("N", [2, 5, 64, 65, 130])
def test_a_diagonal_matrix_returns_the_slice_of_the_default_route(N):
    for S in (C.diag_half(N), C.diag_among_dense(N)):
        lam, V = la.eigen_sym(S)
        for sub in sorted({(0, 1), (N - 1, N), (N // 3, N // 3 + min(N, 7) - 1), (0, N)}):
            l2, V2 = la.eigen_sym(S, subset=sub)
            b = 1 if S.ndim == 3 else Ellipsis
            assert X.same_bits(l2[b], lam[b][..., sub[0]:sub[1]]) and X.same_bits(V2[b], np.ascontiguousarray(V[b][..., sub[0]:sub[1]])), (N, sub)
    lam, V = la.eigen_sym(np.zeros((3, 3)), subset=(1, 3))
    assert not lam.any() and np.array_equal(V, np.eye(3)[:, 1:3])


def test_n_1_n_2_and_the_empty_subset():
    torch, dev = _dev()
    lam, V = la.eigen_sym(np.array([[[-2.5]], [[0.0]], [[7.0]]]), subset=(0, 1))
    assert lam.tolist() == [[-2.5], [0.0], [7.0]] and np.array_equal(V, np.ones((3, 1, 1)))
    S = np.array([[2.0, 99.0], [1.0, 2.0]])
    lam, V = la.eigen_sym(S, subset=(0, 2))
    X.check_subset(np.array([[2.0, 1.0], [1.0, 2.0]]), lam, V, np.array([3.0, 1.0]))
    l1, V1 = la.eigen_sym(S, subset=(1, 2))
    assert X.same_bits(l1, lam[1:]) and X.same_bits(V1, np.ascontiguousarray(V[:, 1:]))
    t = _up(C.reference("batch_5x40")[0])
    ld, vd = dev.eigen_sym(t, subset=(7, 7))
    assert tuple(ld.shape) == (5, 0) and tuple(vd.shape) == (5, 40, 0) and tuple(dev.eigenvals_sym(t, subset=(0, 0)).shape) == (5, 0)
    lz, Zz = dev.tridiag_eigen(t[0, 0], t[0, 1, :39], subset=(3, 3))
    assert tuple(lz.shape) == (0,) and tuple(Zz.shape) == (40, 0)
    for bad in ((3, 2), (0, 41), (-1, 2)):
        with pytest.raises(ValueError, match="subset must be"):
            dev.eigen_sym(t, subset=bad)
        with pytest.raises(ValueError, match="subset must be"):
            dev.tridiag_eigenvals(t[0, 0], t[0, 1, :39], subset=bad)
    with pytest.raises(ValueError, match="same leading dimensions"):
        dev.tridiag_eigen(t[0, :2], t[0, :3, :39].contiguous())
    with pytest.raises(ValueError, match="x contains NaN"):
        dev.tridiag_count(t[0, 0], t[0, 1, :39], _up(np.array([np.nan])))


@pytest.mark.parametrize("N", [1, 40, 130])
def test_nan_or_inf_in_the_lower_triangle_is_noconv_and_the_handle_stays_usable(N):
    S = np.array(C.reference("batch_2x130" if N == 130 else "batch_5x40")[0][0][:N, :N])
    sub = (0, min(3, N))
    before = la.eigen_sym(S, subset=sub)
    for value in (np.nan, np.inf, -np.inf):
        bad = S.copy()
        bad[N - 1, N // 2] = value
        for stack in (bad, np.stack((S, bad, S))):              # alone, and as the middle member of three
            for fn in (la.eigen_sym, la.eigenvals_sym):
                with pytest.raises(_lib.Nd4HipError) as err:
                    fn(stack, subset=sub)
                assert err.value.code == -3 and "eigen_sym(S): S contains NaN or Infinity in its lower triangle." in str(err.value)
            after = la.eigen_sym(S, subset=sub)
            assert X.same_bits(after[0], before[0]) and X.same_bits(after[1], before[1])


def test_profile_record():
    torch, dev = _dev()
    S = _up(C.reference("dense_70")[0])
    h = _lib.handle(0)
    h.profile_enable(True)
    try:
        dev.eigen_sym(S, subset=(0, 8))
        rec, stages = h.profile_last()[0], h.eigsym_subset_last_stages()
        dev.eigenvals_sym(S, subset=(0, 8))
        rec2, stages2 = h.profile_last()[0], h.eigsym_subset_last_stages()
        dev.tridiag_eigen(S[0], S[1, :69], subset=(0, 8))
        rec3, stages3 = h.profile_last()[0], h.eigsym_subset_last_stages()
    finally:
        h.profile_enable(False)
    assert rec["op"] == "dsyevx_batched" and rec["flops"] == pytest.approx(10.0 / 3.0 * 70.0 ** 3 + 2.0 * 70.0 ** 2 * 8, rel=1e-12)
    assert rec2["op"] == "dsyevx_batched" and rec2["flops"] == pytest.approx(10.0 / 3.0 * 70.0 ** 3, rel=1e-12)
    assert rec3["op"] == "dstevx_batched" and rec["valid"] and rec["kernel_ms"] > 0 and rec3["kernel_ms"] > 0
    assert set(stages) == set(h.EIGSYM_SUBSET_STAGES) and all(v > 0 for v in stages.values())
    assert stages2["bisect"] > 0 and stages2["reduce"] > 0 and stages3["bisect"] > 0 and stages3["invit"] > 0 and stages3["reduce"] == 0


def test_both_forms_refuse_alike():
    h = _lib.handle()
    assert X.mismatches(h.ptr) == []
    h.synchronize()
