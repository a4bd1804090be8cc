"""Selected singular triplets on the device (csrc/bdsvdx.hip) through la (host arrays) and dev (device tensors).
bidiag_svdvals and the sv of every subset call return the bits of the numpy model of tests/svd_subset_common.py; the vectors are
held to the five 1e-12 bounds against LAPACK; flagged members are the full solver's bits, sliced; svd_decomp(A, subset) and
svd_vals(A) are held to the same bounds with A in place of B, and to the bounds of the divide & conquer tests."""
import numpy as np
import pytest

import svd_dc_common as D
import svd_subset_common as C
from nd4js_amd import _lib, la

pytestmark = pytest.mark.gpu
SMALL = [(1, 1), (1, 2), (2, 2), (2, 3), (3, 3)] + [(K, J) for K in (31, 32, 33, 64, 65) for J in (K, K + 1)]
CROSSING = [(K, J) for K in (1023, 1024, 1025) for J in (K, K + 1)]
FLAGGED = (("graded_40", (0, 8)), ("graded_40", (19, 22)), ("eqdiag_e0", (2, 10)), ("zero_8", (3, 6)), ("rand_64_64", (56, 64)))


def _dev():
    import torch
    from nd4js_amd import dev
    return torch, dev


def _up(a):
    import torch
    return torch.from_numpy(np.array(a)).cuda()


def _bidiag(K, J, seed=9900):
    g = np.random.default_rng(seed + 2 * K + J)
    return g.uniform(-1, 1, K), g.uniform(-1, 1, J - 1)


def _subsets(K):
    return sorted({(0, 1), (K - 1, K), (0, K), (K // 2, min(K // 2 + 3, K))})


# ---- values: the bits of the model -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,J", SMALL)
def test_values_have_the_bits_of_the_model(K, J):
    torch, dev = _dev()
    d, e = _bidiag(K, J)
    b = C.interleave(d, e)
    for sub in _subsets(K):
        want = C.values(d, e, sub)[0]
        got = la.bidiag_svdvals(d, e, subset=sub)
        assert C.same_bits(got, want), (K, J, sub)
        assert C.same_bits(dev.bidiag_svdvals(_up(d), _up(e), subset=sub).cpu().numpy(), want), (K, J, sub)
        # the tridiagonal solver on the Golub-Kahan matrix itself: the same bits apart from the clamp
        tri = dev.tridiag_eigenvals(_up(np.zeros(K + J)), _up(b), subset=sub).cpu().numpy()
        assert C.same_bits(C.clamp(tri), want), (K, J, sub)
    assert C.same_bits(la.bidiag_svdvals(d, e), C.values(d, e)[0])
    assert C.same_bits(la.bidiag_svd(d, e, subset=(0, 1))[1], C.values(d, e, (0, 1))[0])


@pytest.mark.parametrize("K,J", CROSSING)
def test_values_where_the_order_crosses_2048(K, J):
    d, e = _bidiag(K, J)
    want = C.values(d, e, (0, 8))[0]
    assert C.same_bits(la.bidiag_svdvals(d, e, subset=(0, 8)), want)
    if K + J <= 2048:
        torch, dev = _dev()
        tri = dev.tridiag_eigenvals(_up(np.zeros(K + J)), _up(C.interleave(d, e)), subset=(0, 8)).cpu().numpy()
        assert C.same_bits(C.clamp(tri), want)


def test_values_at_the_lds_cap():
    d, e = C.case_input("max_2048")                            # K = 2048, J = 2049: order 4097, 4096 squares staged
    assert C.same_bits(la.bidiag_svdvals(d, e, subset=(0, 8)), C.values(d, e, (0, 8))[0])
    want = C.values(d, e)[0]
    got = la.bidiag_svdvals(d, e)
    assert C.same_bits(got, want) and np.all(got >= 0) and np.all(np.diff(got) <= 0)


# ---- vectors: the bounds -----------------------------------------------------------------------------------------------------------
def _held(name, sub, d, e, U2, sv, V2):
    B, ref = C.case_reference(name)
    sh = C.check_triplets(B, U2, sv, V2, ref[sub[0]:sub[1]], "%s %r" % (name, sub))
    print("%s %r: shares %s" % (name, sub, " ".join("%.3g" % s for s in sh)))
    return sh


@pytest.mark.parametrize("k", [255, 256, 257])
def test_lane_and_workgroup_edges(k):
    d, e = _bidiag(300, 301)
    B = D.bidiag_dense(d, e)
    ref = np.linalg.svd(B, compute_uv=False)
    info = {}
    U2, sv, V2 = la.bidiag_svd(d, e, subset=(20, 20 + k), info=info)
    assert C.same_bits(sv, C.values(d, e, (20, 20 + k))[0])
    C.check_triplets(B, U2, sv, V2, ref[20:20 + k], "k = %d" % k)


@pytest.mark.parametrize("name", [n for n in C.catalogue() if n not in C.SWEEP_SKIP])
def test_catalogue_inside_the_bounds(name):
    torch, dev = _dev()
    d, e = C.case_input(name)
    for sub in C.subsets_of(len(d)):
        info = {}
        U2, sv, V2 = la.bidiag_svd(d, e, subset=sub, info=info)
        _held(name, sub, d, e, U2, sv, V2)
        _, sv_m, _, info_m = C.case_model(name, sub)
        assert C.same_bits(sv, sv_m), (name, sub)
        assert info["fallback"].dtype == np.int32 and bool(info["fallback"]) == info_m["fallback"], (name, sub, info_m["split_min"])
        assert C.same_bits(la.bidiag_svdvals(d, e, subset=sub), sv), (name, sub)
    sub = C.subsets_of(len(d))[0]                               # the device form, and a second run: the same bits
    U2, sv, V2 = la.bidiag_svd(d, e, subset=sub)
    for Ux, sx, Vx in (la.bidiag_svd(d, e, subset=sub), [t.cpu().numpy() for t in dev.bidiag_svd(_up(d), _up(e), subset=sub)]):
        assert C.same_bits(Ux, U2) and C.same_bits(sx, sv) and C.same_bits(Vx, V2), name


def test_largest_member_top_eight():
    d, e = C.case_input("max_2048")
    U2, sv, V2 = la.bidiag_svd(d, e, subset=(0, 8))
    _held("max_2048", (0, 8), d, e, U2, sv, V2)
    assert C.same_bits(sv, C.values(d, e, (0, 8))[0])


def test_an_empty_subset_returns_empty_arrays():
    torch, dev = _dev()
    d, e = _bidiag(5, 6)
    U2, sv, V2 = la.bidiag_svd(d, e, subset=(2, 2))
    assert U2.shape == (5, 0) and sv.shape == (0,) and V2.shape == (0, 6) and la.bidiag_svdvals(d, e, subset=(5, 5)).shape == (0,)
    U2, sv, V2 = dev.bidiag_svd(_up(d), _up(e), subset=(0, 0))
    assert tuple(U2.shape) == (5, 0) and tuple(sv.shape) == (0,) and tuple(V2.shape) == (0, 6)
    U, s, V = la.svd_decomp(np.ones((3, 4)), subset=(1, 1))
    assert U.shape == (3, 0) and s.shape == (0,) and V.shape == (0, 4) and la.svd_vals(np.ones((3, 4)), subset=(3, 3)).shape == (0,)


# ---- fallback ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,sub", FLAGGED)
def test_a_flagged_member_is_the_full_solver_sliced(name, sub):
    torch, dev = _dev()
    d, e = C.case_input(name)
    assert C.case_model(name, sub)[3]["fallback"]
    Uf, _, Vf = la.bidiag_svd(d, e)
    info = {}
    U2, sv, V2 = la.bidiag_svd(d, e, subset=sub, info=info)
    assert int(info["fallback"]) == 1
    assert C.same_bits(U2, Uf[:, sub[0]:sub[1]]) and C.same_bits(V2, Vf[sub[0]:sub[1]])
    assert C.same_bits(sv, C.values(d, e, sub)[0]) and C.same_bits(la.bidiag_svdvals(d, e, subset=sub), sv)
    info = {}
    Ud, sd, Vd = dev.bidiag_svd(_up(d), _up(e), subset=sub, info=info)
    assert int(info["fallback"].cpu()) == 1
    assert C.same_bits(Ud.cpu().numpy(), U2) and C.same_bits(sd.cpu().numpy(), sv) and C.same_bits(Vd.cpu().numpy(), V2)
    _held(name, sub, d, e, U2, sv, V2)


def test_a_flagged_member_between_two_others():
    torch, dev = _dev()
    members = [_bidiag(64, 64, 200), C.case_input("rand_64_64"), _bidiag(64, 64, 400)]
    sub = (56, 64)
    d, e = np.stack([m[0] for m in members]), np.stack([m[1] for m in members])
    alone = [la.bidiag_svd(m[0], m[1], subset=sub, info=i) + (i,) for m, i in ((m, {}) for m in members)]
    want = [C.bidiag_svd_model(m[0], m[1], sub)[3]["fallback"] for m in members]
    assert want == [False, True, False]
    info = {}
    U2, sv, V2 = la.bidiag_svd(d, e, subset=sub, info=info)
    assert info["fallback"].tolist() == [int(w) for w in want]
    for b, (Ua, sa, Va, ia) in enumerate(alone):
        assert int(ia["fallback"]) == int(want[b])
        assert C.same_bits(U2[b], Ua) and C.same_bits(sv[b], sa) and C.same_bits(V2[b], Va), b
        B = D.bidiag_dense(*members[b])
        C.check_triplets(B, U2[b], sv[b], V2[b], np.linalg.svd(B, compute_uv=False)[sub[0]:sub[1]], "member %d" % b)
    order = [2, 0, 1]                                           # reordered, and run twice: the same bits
    for _ in range(2):
        info2 = {}
        Ur, sr, Vr = [t.cpu().numpy() for t in dev.bidiag_svd(_up(d[order]), _up(e[order]), subset=sub, info=info2)]
        assert info2["fallback"].cpu().tolist() == [int(want[b]) for b in order]
        assert C.same_bits(Ur, U2[order]) and C.same_bits(sr, sv[order]) and C.same_bits(Vr, V2[order])


# ---- errors ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", range(4))
def test_nan_and_inf_are_refused_and_the_handle_stays_usable(which):
    torch, dev = _dev()
    good = _bidiag(20, 21)
    bad = D.error_inputs()[which]
    before = la.bidiag_svd(*good, subset=(0, 5))
    for d, e in (bad, (np.stack((good[0], bad[0], good[0])), np.stack((good[1], bad[1], good[1])))):
        for fn in (lambda: la.bidiag_svd(d, e, subset=(0, 5)), lambda: la.bidiag_svdvals(d, e),
                   lambda: dev.bidiag_svd(_up(d), _up(e), subset=(0, 5))):
            with pytest.raises(_lib.Nd4HipError, match=r"bidiag_svd\(d,e\): d or e contains NaN or Infinity"):
                fn()
        after = la.bidiag_svd(*good, subset=(0, 5))
        assert all(C.same_bits(a, b) for a, b in zip(before, after))


def test_both_forms_refuse_alike_with_a_handle():
    assert C.mismatches(_lib.handle().ptr) == []


# ---- dense -------------------------------------------------------------------------------------------------------------------------
DENSE = ["sq_%d" % n for n in D.SQUARE_SIZES if n <= 65] + list(D.DENSE_SHAPES)


def _dense_subsets(L):
    return sorted({(0, 1), (0, min(8, L)), (0, L), (max(L - 3, 0), L)})


def _dense_held(a, U, sv, V, sub, what):
    """one matrix: check_values on the slice, the five bounds with A in place of B, check_vectors against LAPACK"""
    ur, ref, vr = np.linalg.svd(a, full_matrices=False)
    i0, i1 = sub
    D.check_values(sv, ref[i0:i1])
    sh = C.check_triplets(a, U, sv, V, ref[i0:i1], what)
    D.check_vectors(U, V, ur[:, i0:i1], vr[i0:i1], ref)
    return sh


@pytest.mark.parametrize("name", DENSE)
def test_dense_subsets(name):
    torch, dev = _dev()
    A = D.DENSE_CASES[name]
    M, N = A.shape[-2:]
    L = min(M, N)
    for sub in _dense_subsets(L):
        U, sv, V = la.svd_decomp(A, subset=sub)
        k = sub[1] - sub[0]
        assert U.shape == A.shape[:-2] + (M, k) and sv.shape == A.shape[:-2] + (k,) and V.shape == A.shape[:-2] + (k, N)
        for a, u, s, v in zip(A.reshape(-1, M, N), U.reshape(-1, M, k), sv.reshape(-1, k), V.reshape(-1, k, N)):
            sh = _dense_held(a, u, s, v, sub, "%s %r" % (name, sub))
            print("%s %r: shares %s" % (name, sub, " ".join("%.3g" % x for x in sh)))
        assert C.same_bits(la.svd_vals(A, subset=sub), sv) and C.same_bits(la.svd_decomp(A, subset=sub, algo="dc")[1], sv)
        Ud, sd, Vd = dev.svd_decomp(_up(A), subset=sub)
        assert C.same_bits(Ud.cpu().numpy(), U) and C.same_bits(sd.cpu().numpy(), sv) and C.same_bits(Vd.cpu().numpy(), V)
        assert C.same_bits(dev.svd_vals(_up(A), subset=sub).cpu().numpy(), sv)
    assert C.same_bits(la.svd_vals(A), la.svd_decomp(A, subset=(0, L))[1])


def test_dense_512_top_eight():
    A = D.DENSE_CASES["sq_513"][:512, :512]
    U, sv, V = la.svd_decomp(A, subset=(0, 8))
    _dense_held(A, U, sv, V, (0, 8), "512^2")
    assert C.same_bits(la.svd_vals(A, subset=(0, 8)), sv)


@pytest.mark.parametrize("m", [500, -500])
def test_dense_power_of_two_scaling_is_exact(m):
    A = D.DENSE_CASES["wide_33x130"]
    U, sv, V = la.svd_decomp(A, subset=(2, 12))
    U2, sv2, V2 = la.svd_decomp(np.ldexp(A, m), subset=(2, 12))
    assert C.same_bits(sv2, np.ldexp(sv, m)) and C.same_bits(U2, U) and C.same_bits(V2, V)


def test_the_full_routes_keep_their_bits_around_subset_calls():
    A = D.DENSE_CASES["sq_65"]
    before = la.svd_decomp(A), la.svd_decomp(A, algo="dc")
    la.svd_decomp(A, subset=(0, 8)), la.svd_vals(A), la.bidiag_svd(*_bidiag(40, 41), subset=(0, 40))
    after = la.svd_decomp(A), la.svd_decomp(A, algo="dc")
    for b, a in zip(before, after):
        assert all(C.same_bits(x, y) for x, y in zip(b, a))


def test_subset_with_jacobi_is_refused():
    torch, dev = _dev()
    for fn, A in ((la.svd_decomp, np.eye(4)), (dev.svd_decomp, _up(np.eye(4)))):
        with pytest.raises(ValueError, match="subset is not available with algo='jacobi'"):
            fn(A, algo="jacobi", subset=(0, 1))


def test_dense_nan_is_refused():
    A = D.DENSE_CASES["sq_17"].copy()
    good = la.svd_decomp(A, subset=(0, 4))
    A[3, 5] = np.nan
    with pytest.raises(_lib.Nd4HipError):
        la.svd_decomp(A, subset=(0, 4))
    assert all(C.same_bits(x, y) for x, y in zip(good, la.svd_decomp(D.DENSE_CASES["sq_17"], subset=(0, 4))))


# ---- the profile -------------------------------------------------------------------------------------------------------------------
def test_profile_ops_and_stages():
    h = _lib.handle()
    d, e = _bidiag(64, 65)
    h.profile_enable(True)
    try:
        la.bidiag_svd(d, e, subset=(0, 8))
        rec = h.profile_last()[0]
        st = h.svd_subset_last_stages()
        assert rec["op"] == "dbdsvdx_batched" and rec["valid"] and st["bidiag"] == 0.0 and st["gemm"] == 0.0 and st["bisect"] > 0.0
        la.svd_decomp(D.DENSE_CASES["sq_65"], subset=(0, 8))
        rec = h.profile_last()[0]
        st = h.svd_subset_last_stages()
        assert rec["op"] == "dgesvdx_batched" and rec["valid"] and st["bidiag"] > 0.0 and st["bisect"] > 0.0 and st["invit"] > 0.0
    finally:
        h.profile_enable(False)
