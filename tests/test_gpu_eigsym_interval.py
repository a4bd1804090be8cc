"""interval=(lo, hi) on the device (csrc/syevx.hip) through la (host arrays) and dev (device tensors): the range of
every member is the numpy model's, its pairs are bit for bit those of the subset call with that range, the padding is NaN / 0 up to
kmax and nothing is written from kmax on; dense matrices are held to the project's three 1e-12 bounds against LAPACK.
eigen_sym_gen(A, B) with subset, interval and reduction (csrc/sygv.hip): sygv_common's bounds on the selected columns against
scipy.linalg.eigh(A, B, subset_by_index=...), the small tier bit for bit, the error cases with each keyword."""
import ctypes

import numpy as np
import pytest

import eigsym_common as C
import eigsym_interval_common as I
import eigsym_subset_common as X
import sygv_common as G
from nd4js_amd import _lib, la, rng

pytestmark = pytest.mark.gpu
INF = np.inf


def _dev():
    import torch
    from nd4js_amd import dev
    return torch, dev


def _up(a):
    import torch
    return torch.from_numpy(np.array(a)).cuda()


def _tri(N, seed=7700):
    return rng.fill_uniform(seed + N, N), rng.fill_uniform(seed + 5000 + N, N - 1)


TRIDIAGS = {
    "N1": lambda: _tri(1), "N2": lambda: _tri(2), "N3": lambda: _tri(3), "w21": lambda: X.tridiag_input("w21"),
    "zeros_in_e_40": lambda: X.tridiag_input("zeros_in_e_40"), "graded_48": lambda: X.tridiag_input("graded_48"), "N64": lambda: _tri(64),
    "N65": lambda: _tri(65), "glued_w21": lambda: X.tridiag_input("glued_w21"), "N257": lambda: _tri(257),
}


def _intervals(d, e):
    """a handful of (lo, hi): empty, everything, half lines and inner intervals at unambiguous cuts of LAPACK's spectrum"""
    N = len(d)
    ref = np.linalg.eigvalsh(X.tridiag(d, e))[::-1] if N > 1 else np.array(d)
    g = I.gershgorin(d, e)
    cuts = I.cuts(ref, g)
    js = sorted(cuts)
    out = [(-INF, INF), (2.0 * g, 3.0 * g), (-INF, -2.0 * g), (ref[0] - 0.5 * g, INF)]
    if js:
        a, m, b = js[0], js[len(js) // 2], js[-1]
        out += [(cuts[a], INF), (-INF, cuts[b]), (cuts[b], cuts[a]), (cuts[m], cuts[m]), (cuts[m], cuts[a]), (cuts[b], cuts[m])]
    return out, cuts


def _single(d, e, lo, hi):
    """what a user does today, in two calls: (range, lambda, Z) by tridiag_count and tridiag_eigen(subset)"""
    c = la.tridiag_count(d, e, np.array([hi, lo]))
    sub = (int(c[0]), int(c[1]))
    if sub[0] == sub[1]:
        return sub, np.zeros(0), np.zeros((len(d), 0))
    return (sub,) + tuple(la.tridiag_eigen(d, e, subset=sub))


# ---- tridiag_eigen(d, e, interval) ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", tuple(TRIDIAGS))
def test_tridiagonal_interval_is_count_then_subset_bit_for_bit(name):
    torch, dev = _dev()
    d, e = TRIDIAGS[name]()
    td, te = _up(d), _up(e)
    intervals, cuts = _intervals(d, e)
    for lo, hi in intervals:
        sub, lam, Z = _single(d, e, lo, hi)
        assert sub == I.model_range(d, e, lo, hi), (name, lo, hi)
        info = {}
        l1, Z1 = la.tridiag_eigen(d, e, interval=(lo, hi), info=info)
        assert info["range"].dtype == np.int32 and tuple(info["range"]) == sub, (name, lo, hi)
        assert X.same_bits(l1, lam) and X.same_bits(Z1, Z), (name, lo, hi, sub)
        assert X.same_bits(la.tridiag_eigenvals(d, e, interval=(lo, hi)), lam)
        l2, Z2 = dev.tridiag_eigen(td, te, interval=(lo, hi), info=info)
        assert tuple(info["range"].cpu().numpy()) == sub and info["range"].dtype == torch.int32
        assert X.same_bits(l2.cpu().numpy(), lam) and X.same_bits(Z2.cpu().numpy(), Z), (name, lo, hi, sub)
        assert X.same_bits(dev.tridiag_eigenvals(td, te, interval=(lo, hi)).cpu().numpy(), lam)
        assert np.all(lam > lo) and np.all(lam <= hi)
    # the cuts are unambiguous: the range is what LAPACK's spectrum says
    for j in sorted(cuts)[:: max(1, len(cuts) // 4)]:
        info = {}
        assert la.tridiag_eigenvals(d, e, interval=(cuts[j], INF), info=info).shape == (j,) and tuple(info["range"]) == (0, j)


def test_a_bound_with_the_bits_of_an_eigenvalue():
    d, e = X.tridiag_input("dense_50")
    lam = la.tridiag_eigenvals(d, e)
    for j in (0, 7, 49):
        for lo, hi in ((lam[j], INF), (-INF, lam[j]), (lam[j], lam[j]), (lam[49], lam[j])):
            sub, want, Zw = _single(d, e, lo, hi)
            assert sub == I.model_range(d, e, lo, hi)          # whatever the model's count says of a probe on an eigenvalue
            info = {}
            got, Z = la.tridiag_eigen(d, e, interval=(lo, hi), info=info)
            assert tuple(info["range"]) == sub and X.same_bits(got, want) and X.same_bits(Z, Zw), (j, lo, hi)
    # a diagonal member: a probe exactly on an eigenvalue does not count it, so (lo, hi] is exact there
    dd, ee = np.array([2.0, -1.0, 0.0, 2.0, 0.5, -1.0, 0.5, 3.0]), np.zeros(7)
    info = {}
    got, Z = la.tridiag_eigen(dd, ee, interval=(-1.0, 2.0), info=info)
    assert tuple(info["range"]) == (1, 6) and got.tolist() == [2.0, 2.0, 0.5, 0.5, 0.0]
    assert np.array_equal(Z, np.eye(8)[:, [0, 3, 4, 6, 2]])


def test_a_bound_inside_a_cluster_of_the_glued_wilkinson():
    d, e = X.tridiag_input("glued_w21")
    lam = la.tridiag_eigenvals(d, e)
    assert lam[0] - lam[4] < 1e-3 * I.gershgorin(d, e)          # the five copies of the largest value are one cluster
    for lo, hi in ((lam[2], INF), (lam[7], lam[2]), (0.5 * (lam[1] + lam[2]), INF)):
        sub, want, Zw = _single(d, e, lo, hi)
        assert sub == I.model_range(d, e, lo, hi)
        info = {}
        got, Z = la.tridiag_eigen(d, e, interval=(lo, hi), info=info)
        assert tuple(info["range"]) == sub and X.same_bits(got, want) and X.same_bits(Z, Zw)
        if len(want):
            X.check_subset(X.tridiag(d, e), got, Z, X.tridiag_reference("glued_w21")[sub[0]:sub[1]], "glued_w21 %r" % (sub,))


@pytest.mark.parametrize("m", [500, -500])
def test_power_of_two_scaling_of_input_and_interval_is_exact(m):
    d, e = X.tridiag_input("dense_50")
    cuts = I.cuts(X.tridiag_reference("dense_50"), I.gershgorin(d, e))
    a, b = sorted(cuts)[3], sorted(cuts)[20]
    info, info2 = {}, {}
    lam, Z = la.tridiag_eigen(d, e, interval=(cuts[b], cuts[a]), info=info)
    lam2, Z2 = la.tridiag_eigen(np.ldexp(d, m), np.ldexp(e, m), interval=(np.ldexp(cuts[b], m), np.ldexp(cuts[a], m)), info=info2)
    assert tuple(info["range"]) == (a, b) == tuple(info2["range"])
    assert X.same_bits(lam2, np.ldexp(lam, m)) and X.same_bits(Z2, Z)


# ---- ragged batches -----------------------------------------------------------------------------------------------------------------
def _ragged_batch():
    """five members of N = 40 with k_b = 1, N, 0, a diagonal member and a dense one: (d, e, lo, hi, k_b)"""
    d1, e1 = _tri(40)
    ref = np.linalg.eigvalsh(X.tridiag(d1, e1))[::-1]
    cuts = I.cuts(ref, I.gershgorin(d1, e1))
    a, b = sorted(cuts)[4], sorted(cuts)[-6]
    dd = np.rint(4.0 * d1)
    d = np.stack((d1, d1, d1, dd, d1))
    e = np.stack((e1, e1, e1, np.zeros(39), e1))
    lo = np.array([cuts[1], -INF, 10.0, -0.5, cuts[b]])
    hi = np.array([INF, INF, 11.0, 2.0, cuts[a]])
    return d, e, lo, hi, [1, 40, 0, int(((dd > -0.5) & (dd <= 2.0)).sum()), b - a]


@pytest.mark.parametrize("order", [(0, 1, 2, 3, 4), (4, 2, 0, 3, 1), (2, 2, 3, 2, 2)])
def test_members_of_a_ragged_batch_equal_their_single_calls(order):
    torch, dev = _dev()
    d, e, lo, hi, kb = (np.array(a)[list(order)] for a in _ragged_batch())
    info = {}
    lam, Z = la.tridiag_eigen(d, e, interval=(lo, hi), info=info)
    ranges, kmax = info["range"], int(kb.max())
    assert (ranges[:, 1] - ranges[:, 0]).tolist() == kb.tolist() and lam.shape == (5, kmax) and Z.shape == (5, 40, kmax)
    assert I.padded(lam, Z, ranges)
    for m in range(5):
        sub, l1, Z1 = _single(d[m], e[m], lo[m], hi[m])
        assert tuple(ranges[m]) == sub and X.same_bits(lam[m, :kb[m]], l1) and X.same_bits(Z[m][:, :kb[m]], Z1), (order, m)
    # the same bits a second time, from the values alone and through dev
    l2, Z2 = la.tridiag_eigen(d, e, interval=(lo, hi))
    assert X.same_bits(l2, lam) and X.same_bits(Z2, Z) and X.same_bits(la.tridiag_eigenvals(d, e, interval=(lo, hi)), lam)
    ld, Zd = dev.tridiag_eigen(_up(d), _up(e), interval=(_up(lo), _up(hi)), info=info)
    assert X.same_bits(ld.cpu().numpy(), lam) and X.same_bits(Zd.cpu().numpy(), Z) and np.array_equal(info["range"].cpu().numpy(), ranges)
    ld, Zd = dev.tridiag_eigen(_up(d), _up(e), interval=(lo, hi))             # host arrays for the bounds of a device call
    assert X.same_bits(ld.cpu().numpy(), lam) and X.same_bits(Zd.cpu().numpy(), Z)


def _raw_dev(name, kcap, bounds, operands, N, vshape, poison=7.5):
    """the _dev entry point itself on poisoned outputs: (rc, lambda, vectors, range, kmax)"""
    torch, dev = _dev()
    lead = tuple(bounds.shape[:-1])
    L = torch.full(lead + (kcap,), poison, dtype=torch.float64, device="cuda")
    V = torch.full(vshape, poison, dtype=torch.float64, device="cuda")
    ranges = torch.full(lead + (2,), -9, dtype=torch.int32, device="cuda")
    kmax = ctypes.c_int64(-1)
    h = dev._h(L)
    rc = getattr(h.lib, name)(h.ptr, int(np.prod(lead)), N, kcap, dev._p(bounds), *[dev._p(a) for a in operands], dev._p(L), dev._p(V),
                              dev._p(ranges), ctypes.byref(kmax))
    return rc, L.cpu().numpy(), V.cpu().numpy(), ranges.cpu().numpy(), kmax.value


def test_nothing_is_written_from_kmax_on_and_kcap_below_kmax_is_refused():
    torch, dev = _dev()
    d, e, lo, hi, kb = _ragged_batch()
    sel = [0, 2, 3, 4]                                          # without the member that takes everything: kmax < N
    d, e, lo, hi, kb = d[sel], e[sel], lo[sel], hi[sel], np.array(kb)[sel]
    kmax = int(kb.max())
    assert 1 < kmax < 30
    want_l, want_Z = la.tridiag_eigen(d, e, interval=(lo, hi))
    bounds = _up(np.stack((lo, hi), axis=-1))
    lib = _lib.load()
    for kcap in (kmax, kmax + 1, 40):
        rc, L, Zr, ranges, km = _raw_dev("nd4hip_dstevxv_batched_dev", kcap, bounds, (_up(d), _up(e)), 40, (4, kcap, 40))
        assert rc == 0 and km == kmax and (ranges[:, 1] - ranges[:, 0]).tolist() == kb.tolist()
        assert X.same_bits(L[:, :kmax], want_l) and X.same_bits(np.swapaxes(Zr[:, :kmax], -1, -2), want_Z)
        assert np.all(L[:, kmax:] == 7.5) and np.all(Zr[:, kmax:] == 7.5), kcap
    rc, L, Zr, ranges, km = _raw_dev("nd4hip_dstevxv_batched_dev", kmax - 1, bounds, (_up(d), _up(e)), 40, (4, kmax - 1, 40))
    assert rc == -1 and "kcap = %d is less than the %d eigenvalues" % (kmax - 1, kmax) in lib.nd4hip_last_error().decode()
    assert np.all(L == 7.5) and np.all(Zr == 7.5)               # refused after the count, before anything else is launched
    # the host form refuses alike, and the handle is usable afterwards
    hl, hr, hk = np.full((4, kmax - 1), 7.5), np.zeros((4, 2), dtype=np.int32), ctypes.c_int64(-1)
    h = _lib.handle()
    hb = np.ascontiguousarray(np.stack((lo, hi), axis=-1))
    rc = h.lib.nd4hip_dstevxv_batched_host(h.ptr, 4, 40, kmax - 1, la._ptr(hb), la._ptr(d), la._ptr(e), la._ptr(hl), None, la._ptr(hr), ctypes.byref(hk))
    assert rc == -1 and "kcap = %d is less than" % (kmax - 1) in lib.nd4hip_last_error().decode() and np.all(hl == 7.5)
    l2, Z2 = la.tridiag_eigen(d, e, interval=(lo, hi))
    assert X.same_bits(l2, want_l) and X.same_bits(Z2, want_Z)
    # the host form with room to spare: the same results, nothing from kmax on
    hl, hz = np.full((4, 33), 7.5), np.full((4, 33, 40), 7.5)
    rc = h.lib.nd4hip_dstevxv_batched_host(h.ptr, 4, 40, 33, la._ptr(hb), la._ptr(d), la._ptr(e), la._ptr(hl), la._ptr(hz), la._ptr(hr), ctypes.byref(hk))
    assert rc == 0 and hk.value == kmax and X.same_bits(hl[:, :kmax], want_l) and X.same_bits(np.swapaxes(hz[:, :kmax], -1, -2), want_Z)
    assert np.all(hl[:, kmax:] == 7.5) and np.all(hz[:, kmax:] == 7.5)
    # lo > hi in device memory is seen after the count
    rc = _raw_dev("nd4hip_dstevxv_batched_dev", 40, _up(np.stack((hi, lo), axis=-1)), (_up(d), _up(e)), 40, (4, 40, 40))[0]
    assert rc == -1 and "interval must satisfy lo <= hi" in lib.nd4hip_last_error().decode()


def _raw_host(name, kcap, bounds, operands, N, lead, extra=(), poison=7.5):
    """the _host entry point itself on poisoned outputs: (rc, lambda, vectors [..., N, kcap], range, kmax)"""
    L, V = np.full(lead + (kcap,), poison), np.full(lead + (N, kcap), poison)
    ranges, kmax = np.full(lead + (2,), -9, dtype=np.int32), ctypes.c_int64(-1)
    h = _lib.handle()
    ops = [la._ptr(np.ascontiguousarray(a)) for a in operands]
    rc = getattr(h.lib, name)(h.ptr, *extra[:2], int(np.prod(lead)), N, *extra[2:4], kcap, la._ptr(bounds), *ops, *extra[4:], la._ptr(L), la._ptr(V),
                              la._ptr(ranges), ctypes.byref(kmax))
    return rc, L, V, ranges, kmax.value


@pytest.mark.parametrize("N", [40, 130])
def test_dense_and_gen_forms_write_nothing_from_kmax_on(N):
    """every interval entry with V / X: the GEMM that writes V with rows kcap apart, nd4_ormtr and stx_ragged, the 2-D download of
    the _host forms, and the copy - solve - copy back of eigen_sym_gen's large tier (N = 130), on poisoned outputs with
    kcap = kmax, kmax + 1 and N; kcap < kmax is refused and leaves the outputs alone"""
    torch, dev = _dev()
    name = "batch_2x130" if N == 130 else "batch_5x40"
    S = C.reference(name)[0]
    A, B = G.inputs(name)
    nb = len(S)
    lo = np.linspace(0.2, 1.5, nb)                             # a different k_b for every member
    hi = np.full(nb, INF)
    bounds = np.ascontiguousarray(np.stack((lo, hi), axis=-1))
    lib = _lib.load()
    entries = [("nd4hip_dsyevxv_batched", (S,), (), la.eigen_sym(S, interval=(lo, hi))),
               ("nd4hip_dsyevxv_tr_batched", (S,), (), la.eigen_sym(S, interval=(lo, hi), reduction="tridiag"))]
    for red in (0, 1):
        want = la.eigen_sym_gen(A, B, interval=(lo, hi), reduction="tridiag" if red else None)
        entries.append(("nd4hip_dsygvx_batched", (A, B), (red, 2, 0, 0, N * N), want))
    for base, operands, extra, (want_l, want_v) in entries:
        kmax = want_l.shape[-1]
        assert 1 < kmax < N - 1 and np.isnan(want_l).any(), base
        for kcap in (kmax, kmax + 1, N):
            rc, L, V, ranges, km = _raw_host(base + "_host", kcap, bounds, operands, N, (nb,), extra)
            assert rc == 0 and km == kmax and X.same_bits(L[:, :kmax], want_l) and X.same_bits(V[:, :, :kmax], want_v), (base, kcap)
            assert np.all(L[:, kmax:] == 7.5) and np.all(V[:, :, kmax:] == 7.5), (base, kcap)
            ops = [_up(a) for a in operands]
            tl, tv = torch.full((nb, kcap), 7.5, dtype=torch.float64, device="cuda"), torch.full((nb, N, kcap), 7.5, dtype=torch.float64, device="cuda")
            tr_, tk, h = torch.full((nb, 2), -9, dtype=torch.int32, device="cuda"), ctypes.c_int64(-1), dev._h(ops[0])
            rc = getattr(h.lib, base + "_dev")(h.ptr, *extra[:2], nb, N, *extra[2:4], kcap, dev._p(_up(bounds)), *[dev._p(a) for a in ops], *extra[4:],
                                               dev._p(tl), dev._p(tv), dev._p(tr_), ctypes.byref(tk))
            L, V = tl.cpu().numpy(), tv.cpu().numpy()
            assert rc == 0 and tk.value == kmax and np.array_equal(tr_.cpu().numpy(), ranges), (base, kcap)
            assert X.same_bits(L[:, :kmax], want_l) and X.same_bits(V[:, :, :kmax], want_v), (base, kcap)
            assert np.all(L[:, kmax:] == 7.5) and np.all(V[:, :, kmax:] == 7.5), (base, kcap)
        rc, L, V, ranges, km = _raw_host(base + "_host", kmax - 1, bounds, operands, N, (nb,), extra)
        assert rc == -1 and "kcap = %d is less than the %d eigenvalues" % (kmax - 1, kmax) in lib.nd4hip_last_error().decode(), base
        assert np.all(L == 7.5) and np.all(V == 7.5), base


# ---- eigen_sym(S, interval) ---------------------------------------------------------------------------------------------------------
_REF_512 = []


def _reference(name):
    if name != "dense_512":
        return C.reference(name)[:2]
    if not _REF_512:
        S = C.sym_uniform(7100 + 512, 512)
        _REF_512.extend((S, np.linalg.eigvalsh(S)[::-1].copy()))
    return _REF_512


def _dense_intervals(S, lam_ref):
    """[(lo [batch], hi [batch], ranges [batch, 2])]: bounds at midpoints of well-separated LAPACK gaps of each member, so that its
    range is known: about 8 values at the top, about a quarter in the middle, a half line, everything"""
    N = S.shape[-1]
    Sm, Lm = S.reshape(-1, N, N), lam_ref.reshape(-1, N)
    picks = []
    for want in ((0, min(8, N)), (N // 3, N // 3 + max(N // 4, 1)), (N // 2, N), (0, N)):
        lo, hi, ranges = [], [], []
        for s, ref in zip(Sm, Lm):
            cuts = I.cuts(ref, max(N * np.abs(s).max(), 1e-300))   # N max|s_ij| >= rho(S), and no square to overflow at 2^500
            cuts[0], cuts[N] = INF, -INF
            a = min(cuts, key=lambda j: (abs(j - want[0]), j))
            b = min((j for j in cuts if j >= a), key=lambda j: (abs(j - want[1]), j))
            hi.append(cuts[a]), lo.append(cuts[b]), ranges.append((a, b))
        picks.append((np.array(lo).reshape(S.shape[:-2]), np.array(hi).reshape(S.shape[:-2]), np.array(ranges)))
    return picks


@pytest.mark.parametrize("reduction", [None, "tridiag"])
@pytest.mark.parametrize("name", C.SMALL + ("dense_512",))
def test_catalogue_intervals_through_la_and_dev(name, reduction):
    torch, dev = _dev()
    S, lam_ref = _reference(name)
    N = S.shape[-1]
    t = _up(S)
    keep = t.clone()
    for lo, hi, ranges in _dense_intervals(S, lam_ref):
        info = {}
        lam, V = la.eigen_sym(S, interval=(lo, hi), info=info, reduction=reduction)
        got = info["range"].reshape(-1, 2)
        assert np.array_equal(got, ranges), "%s: ranges %r, LAPACK says %r" % (name, got.tolist(), ranges.tolist())
        kb = ranges[:, 1] - ranges[:, 0]
        kmax = int(kb.max())
        assert lam.shape == S.shape[:-2] + (kmax,) and V.shape == S.shape[:-1] + (kmax,)
        nb = len(ranges)
        assert I.padded(lam.reshape(nb, kmax), V.reshape(nb, N, kmax), ranges)
        worst = np.zeros(3)
        members = list(zip(S.reshape(nb, N, N), lam.reshape(nb, kmax), V.reshape(nb, N, kmax), lam_ref.reshape(nb, N), ranges))
        for s, l, v, r, (a, b) in members:
            if b > a:
                worst = np.maximum(worst, X.check_subset(s, l[:b - a], np.ascontiguousarray(v[:, :b - a]), r[a:b], "%s %s" % (name, (a, b))))
            # the bits of the subset call with the returned range, the member alone (N <= 512: no sum depends on the batch)
            if b > a:
                l1, v1 = la.eigen_sym(s, subset=(int(a), int(b)), reduction=reduction)
                assert X.same_bits(l[:b - a], l1) and X.same_bits(np.ascontiguousarray(v[:, :b - a]), v1), (name, reduction, a, b)
        print("%s %s %s shares of the bounds (values, residual, orthogonality): %.3g %.3g %.3g" % ((name, reduction, ranges[0].tolist()) + tuple(worst)))
        assert X.same_bits(la.eigenvals_sym(S, interval=(lo, hi), reduction=reduction), lam), "eigenvals_sym must have eigen_sym's bits"
        ld, vd = dev.eigen_sym(t, interval=(lo, hi), info=info, reduction=reduction)
        assert X.same_bits(ld.cpu().numpy(), lam) and X.same_bits(vd.cpu().numpy(), V)
        assert np.array_equal(info["range"].cpu().numpy().reshape(-1, 2), ranges)
        assert X.same_bits(dev.eigenvals_sym(t, interval=(lo, hi), reduction=reduction).cpu().numpy(), lam) and torch.equal(t, keep)


def test_n_1_n_2_and_the_empty_selection():
    torch, dev = _dev()
    info = {}
    S1 = np.array([[[-2.5]], [[0.0]], [[7.0]]])
    for reduction in (None, "tridiag"):
        lam, V = la.eigen_sym(S1, interval=(-3.0, 0.0), info=info, reduction=reduction)
        assert info["range"].tolist() == [[0, 1], [0, 1], [1, 1]]
        assert lam[:2, 0].tolist() == [-2.5, 0.0] and np.isnan(lam[2, 0]) and V[:, 0, 0].tolist() == [1.0, 1.0, 0.0]
        S = np.array([[2.0, 99.0], [1.0, 2.0]])
        lam, V = la.eigen_sym(S, interval=(-INF, INF), reduction=reduction)
        X.check_subset(np.array([[2.0, 1.0], [1.0, 2.0]]), lam, V, np.array([3.0, 1.0]))
        l1, V1 = la.eigen_sym(S, interval=(0.0, 2.0), info=info, reduction=reduction)
        assert tuple(info["range"]) == (1, 2) and X.same_bits(l1, lam[1:]) and X.same_bits(V1, np.ascontiguousarray(V[:, 1:]))
        t = _up(C.reference("batch_5x40")[0])
        ld, vd = dev.eigen_sym(t, interval=(1e6, INF), info=info, reduction=reduction)
        assert tuple(ld.shape) == (5, 0) and tuple(vd.shape) == (5, 40, 0) and info["range"].cpu().tolist() == [[0, 0]] * 5
        assert tuple(dev.eigenvals_sym(t, interval=(-INF, -1e6), info=info).shape) == (5, 0) and info["range"].cpu().tolist() == [[40, 40]] * 5
    for bad, text in (((1.0, 0.0), "lo <= hi"), ((np.nan, 0.0), "NaN"), ((np.zeros(4), 1.0), "broadcast"), ((_up(np.array([0.0, 2.0, 0, 0, 0])), 1.0), "lo <= hi")):
        with pytest.raises(ValueError, match=text):
            dev.eigen_sym(t, interval=bad)
        with pytest.raises(ValueError, match=text):
            dev.tridiag_eigenvals(t[:, 0].contiguous(), t[:, 1, :39].contiguous(), interval=bad)


@pytest.mark.parametrize("N", [1, 40, 130])
def test_nan_or_inf_is_noconv_and_the_handle_stays_usable(N):
    S = np.array(C.reference("batch_2x130" if N == 130 else "batch_5x40")[0][0][:N, :N])
    iv = (-INF, INF) if N == 1 else (0.0, INF)
    for reduction in (None, "tridiag"):
        before = la.eigen_sym(S, interval=iv, reduction=reduction)
        for value in (np.nan, np.inf):
            bad = S.copy()
            bad[N - 1, N // 2] = value
            for stack in (bad, np.stack((S, bad, S))):          # alone, and as the middle member of three
                for fn in (la.eigen_sym, la.eigenvals_sym):
                    with pytest.raises(_lib.Nd4HipError) as err:
                        fn(stack, interval=iv, reduction=reduction)
                    assert err.value.code == -3 and "eigen_sym(S): S contains NaN or Infinity in its lower triangle." in str(err.value)
                after = la.eigen_sym(S, interval=iv, reduction=reduction)
                assert X.same_bits(after[0], before[0]) and X.same_bits(after[1], before[1])
    if N > 1:
        d, e = np.array(S[0]), np.array(S[1, :N - 1])
        before = la.tridiag_eigen(d, e, interval=iv)
        bad = d.copy()
        bad[3] = np.nan
        for stack_d, stack_e in ((bad, e), (np.stack((d, bad, d)), np.stack((e, e, e)))):
            with pytest.raises(_lib.Nd4HipError) as err:
                la.tridiag_eigen(stack_d, stack_e, interval=iv)
            assert err.value.code == -3 and "tridiag_eigen(d,e): d or e contains NaN or Infinity." in str(err.value)
        after = la.tridiag_eigen(d, e, interval=iv)
        assert X.same_bits(after[0], before[0]) and X.same_bits(after[1], before[1])


def test_nothing_else_moved():
    torch, dev = _dev()
    S = C.reference("batch_5x40")[0]
    A = S[0]
    B = S[1] @ S[1].T + 40.0 * np.eye(40)
    t = _up(S)

    def today():
        out = list(la.eigen_sym(S)) + list(la.eigen_sym(S, subset=(2, 9))) + list(la.eigen_sym(S, subset=(2, 9), reduction="tridiag"))
        out += list(la.eigen_sym_gen(A, B)) + list(la.tridiag_eigen(S[2, 0], S[2, 1, :39], subset=(0, 5)))
        out += list(la.eigen_sym_gen(S, B)) + list(la.eigen_sym_gen(*G.inputs("batch_2x130"))) + list(la.eigen_sym_gen(A, B, algo="jacobi"))
        out += [x.cpu().numpy() for x in dev.eigen_sym(t)] + [x.cpu().numpy() for x in dev.eigen_sym(t, subset=(2, 9))]
        return out
    before = today()
    for reduction in (None, "tridiag"):
        la.eigen_sym(S, interval=(0.0, INF), reduction=reduction), dev.eigenvals_sym(t, interval=(-1.0, 1.0), reduction=reduction)
    la.tridiag_eigen(S[:, 0], S[:, 1, :39], interval=(-0.5, 0.5)), dev.tridiag_eigen(t[:, 0].contiguous(), t[:, 1, :39].contiguous(), interval=(5.0, 6.0))
    A130, B130 = G.inputs("batch_2x130")
    for a, b in ((A, B), (S, B), (A130, B130)):                # the small tier, one B for a stack, the large tier
        for kw in ({"subset": (0, 3)}, {"interval": (0.0, INF)}, {"reduction": "tridiag"}, {"reduction": "tridiag", "subset": (1, 2)},
                   {"reduction": "tridiag", "interval": (-1.0, 1.0)}):
            la.eigen_sym_gen(a, b, **kw), dev.eigenvals_sym_gen(_up(a), _up(b), **kw)
    for a, b in zip(before, today()):
        assert X.same_bits(a, b)


def test_profile_record():
    torch, dev = _dev()
    S = _up(C.reference("dense_70")[0])
    h = _lib.handle(0)
    h.profile_enable(True)
    try:
        dev.eigen_sym(S, interval=(0.0, INF))
        rec, stages = h.profile_last()[0], h.eigsym_subset_last_stages()
        dev.eigenvals_sym(S, interval=(0.0, INF), reduction="tridiag")
        rec2, stages2 = h.profile_last()[0], h.eigsym_subset_last_stages()
        dev.tridiag_eigen(S[0], S[1, :69], interval=(0.0, INF))
        rec3, stages3 = h.profile_last()[0], h.eigsym_subset_last_stages()
    finally:
        h.profile_enable(False)
    assert (rec["op"], rec2["op"], rec3["op"]) == ("dsyevxv_batched", "dsyevxv_tr_batched", "dstevxv_batched")
    assert rec["valid"] and rec["kernel_ms"] > 0 and rec2["kernel_ms"] > 0 and rec3["kernel_ms"] > 0
    assert set(stages) == set(h.EIGSYM_SUBSET_STAGES) and all(v > 0 for v in stages.values())
    assert stages2["symm"] == 0 and stages2["bisect"] > 0 and stages2["reduce"] > 0
    assert stages3["bisect"] > 0 and stages3["invit"] > 0 and stages3["reduce"] == 0


def test_both_forms_refuse_alike():
    h = _lib.handle()
    assert I.mismatches(h.ptr) == []
    h.synchronize()


# ---- eigen_sym_gen(A, B) with subset, interval and reduction ------------------------------------------------------------------------
GEN_NAMES = tuple("%s_%d" % (kind, N) for N in G.SMALL_N + G.LARGE_N for kind in ("gram", "graded")) + ("shared_3x40", "batch_5x40", "batch_2x130")
MSG_B = "eigen_sym_gen(A,B): B is not positive definite. (matrix %d)"
MSG_C = "eigen_sym_gen(A,B): L^-1 A L^-T is not finite"


def _gen_gate(a, b, lam, X, i0, i1, what):
    """sygv_common's three bounds on the selected columns i0 .. i1 - 1 of one member, the values against LAPACK's of that index range;
    the residual and B-orthonormality do not depend on the signs of the columns. X may be None.
    The residual bound keeps max|lambda| of the WHOLE spectrum, as sygv_common.check has it for a full call: the error of a column
    x = L^-T y is that of C = L^-1 A L^-T, eps kappa ||C|| with ||C|| = max|lambda| (sygv_common's docstring), whichever columns are
    selected; a selected column of small lambda does not have a smaller one."""
    from scipy.linalg import eigh
    N, k = a.shape[0], i1 - i0
    assert lam.shape == (k,) and np.all(np.isfinite(lam)) and np.all(np.diff(lam) <= 0), what
    if k == 0:
        return
    ref = eigh(a, b, eigvals_only=True, subset_by_index=[N - i1, N - i0 - 1])[::-1]
    lam_max = np.abs(eigh(a, b, eigvals_only=True)).max()
    sv = np.linalg.svd(b, compute_uv=False)
    kappa, na, nb = sv[0] / sv[-1], np.linalg.norm(a), np.linalg.norm(b)
    share = (np.abs(lam - ref) / (G.TOL * (na / sv[-1] + kappa * np.abs(ref)))).max()
    assert share <= 1.0, "%s: max|dlambda| is %.3g of its bound" % (what, share)
    if X is not None:
        assert X.shape == (N, k) and np.all(np.isfinite(X)), what
        share = np.linalg.norm(a @ X - (b @ X) * lam) / (G.TOL * (na + nb * lam_max) * np.linalg.norm(X))
        assert share <= 1.0, "%s: ||A X - B X L||_F is %.3g of its bound" % (what, share)
        share = np.linalg.norm(X.T @ b @ X - np.eye(k)) / (G.TOL * kappa * np.sqrt(k))
        assert share <= 1.0, "%s: ||X^T B X - I||_F is %.3g of its bound" % (what, share)


def _small_tier_bits(a, b, lam, X, sub, reduction, what):
    """N <= 64: lambda has the bits of eigen_sym(_sygst(A, L), subset), X those of back_model(L, Y), column by column"""
    N, k = a.shape[0], sub[1] - sub[0]
    L = G.chol_model(b)[0]
    l2, Y = la.eigen_sym(la._sygst(a, L), subset=sub, reduction=reduction)
    Yp = np.zeros((N, N))
    Yp[:, :k] = Y
    assert G.same_bits(lam, l2) and G.same_bits(X, G.back_model(L, Yp)[:, :k]), what


@pytest.mark.parametrize("reduction", [None, "tridiag"])
@pytest.mark.parametrize("name", GEN_NAMES)
def test_gen_subsets_through_la_and_dev(name, reduction):
    torch, dev = _dev()
    A, B = G.inputs(name)
    N = A.shape[-1]
    ta, tb = _up(A), _up(B)
    for sub in sorted({(0, 1), (0, min(8, N)), (max(N - 3, 0), N), (0, N)}):
        k = sub[1] - sub[0]
        lam, X = la.eigen_sym_gen(A, B, subset=sub, reduction=reduction)
        assert lam.shape == A.shape[:-2] + (k,) and X.shape == A.shape[:-1] + (k,)
        for m, (a, b) in enumerate(G.members(A, B)):
            l1, x1 = lam.reshape(-1, k)[m], X.reshape(-1, N, k)[m]
            _gen_gate(a, b, l1, x1, sub[0], sub[1], "%s %s member %d" % (name, sub, m))
            if N <= G.SMALL_MAX:
                _small_tier_bits(a, b, l1, x1, sub, reduction, "%s %s member %d" % (name, sub, m))
        assert G.same_bits(la.eigenvals_sym_gen(A, B, subset=sub, reduction=reduction), lam)
        ld, xd = dev.eigen_sym_gen(ta, tb, subset=sub, reduction=reduction)
        assert G.same_bits(ld.cpu().numpy(), lam) and G.same_bits(xd.cpu().numpy(), X)
        assert G.same_bits(dev.eigenvals_sym_gen(ta, tb, subset=sub, reduction=reduction).cpu().numpy(), lam)
    if reduction == "tridiag":                                 # the keyword alone: every pair, inside the bounds of the default call
        lam, X = la.eigen_sym_gen(A, B, reduction="tridiag")
        G.check(A, B, lam, X, G.golden(name), name + " tridiag")
        assert G.same_bits(la.eigenvals_sym_gen(A, B, reduction="tridiag"), lam)
        ld, xd = dev.eigen_sym_gen(ta, tb, reduction="tridiag")
        assert G.same_bits(ld.cpu().numpy(), lam) and G.same_bits(xd.cpu().numpy(), X)
    else:                                                      # reduction None / 'hessenberg' without a selection is today's call
        want = la.eigen_sym_gen(A, B)
        got = la.eigen_sym_gen(A, B, reduction="hessenberg", subset=None, interval=None)
        assert G.same_bits(got[0], want[0]) and G.same_bits(got[1], want[1])


@pytest.mark.parametrize("reduction", [None, "tridiag"])
@pytest.mark.parametrize("name", GEN_NAMES)
def test_gen_intervals_through_la_and_dev(name, reduction):
    torch, dev = _dev()
    A, B = G.inputs(name)
    N = A.shape[-1]
    lead = A.shape[:-2]
    ref = G.golden(name).reshape(-1, N)
    mem = G.members(A, B)
    ta, tb = _up(A), _up(B)
    for want in ((0, min(8, N)), (N // 3, N // 3 + max(N // 4, 1)), (0, N), (N, N)):
        lo, hi, ranges = [], [], []
        for (a, b), r in zip(mem, ref):
            cuts = I.cuts(r, max(np.abs(r).max(), 1e-300))
            cuts[0], cuts[N] = INF, -INF
            i0 = min(cuts, key=lambda j: (abs(j - want[0]), j))
            i1 = min((j for j in cuts if j >= i0), key=lambda j: (abs(j - want[1]), j))
            hi.append(cuts[i0]), lo.append(cuts[i1]), ranges.append((i0, i1))
        lo, hi, ranges = np.array(lo).reshape(lead), np.array(hi).reshape(lead), np.array(ranges)
        info = {}
        lam, X = la.eigen_sym_gen(A, B, interval=(lo, hi), reduction=reduction, info=info)
        assert np.array_equal(info["range"].reshape(-1, 2), ranges), (name, info["range"].tolist(), ranges.tolist())
        kb = ranges[:, 1] - ranges[:, 0]
        kmax, nb = int(kb.max()), len(mem)
        assert lam.shape == lead + (kmax,) and X.shape == lead + (N, kmax) and I.padded(lam.reshape(nb, kmax), X.reshape(nb, N, kmax), ranges)
        for m, (a, b) in enumerate(mem):
            i0, i1 = (int(v) for v in ranges[m])
            l1, x1 = lam.reshape(nb, kmax)[m, :kb[m]], np.ascontiguousarray(X.reshape(nb, N, kmax)[m][:, :kb[m]])
            _gen_gate(a, b, l1, x1, i0, i1, "%s %s member %d" % (name, (i0, i1), m))
            if kb[m] and (N <= G.SMALL_MAX or nb == 1):         # the bits of the subset call with the returned range
                l2, x2 = la.eigen_sym_gen(a, b, subset=(i0, i1), reduction=reduction)
                assert G.same_bits(l1, l2) and G.same_bits(x1, x2), (name, reduction, i0, i1)
        assert G.same_bits(la.eigenvals_sym_gen(A, B, interval=(lo, hi), reduction=reduction), lam)
        ld, xd = dev.eigen_sym_gen(ta, tb, interval=(lo, hi), reduction=reduction, info=info)
        assert G.same_bits(ld.cpu().numpy(), lam) and G.same_bits(xd.cpu().numpy(), X)
        assert np.array_equal(info["range"].cpu().numpy().reshape(-1, 2), ranges)
        assert G.same_bits(dev.eigenvals_sym_gen(ta, tb, interval=(lo, hi), reduction=reduction).cpu().numpy(), lam)


def _keyword_sets(N):
    return ({"subset": (0, min(2, N))}, {"interval": (-INF, INF)}, {"reduction": "tridiag"}, {"reduction": "tridiag", "subset": (0, min(2, N))},
            {"reduction": "tridiag", "interval": (0.0, INF)})


@pytest.mark.parametrize("N", [3, 40, 130])
def test_gen_errors_keep_their_codes_and_members_with_each_keyword(N):
    torch, dev = _dev()
    A = np.array(G.inputs("gram_300")[0][:N, :N])
    good = np.array(G.inputs("gram_300")[1][:N, :N])
    before = la.eigen_sym_gen(A, good, subset=(0, 2))
    As, Bs = np.stack([A, A, A, A]), np.stack([good, -np.eye(N), good, np.zeros((N, N))])
    A2 = A.copy()
    A2[N - 1, N // 2] = np.nan
    for kw in _keyword_sets(N):
        for fn in (la.eigen_sym_gen, la.eigenvals_sym_gen):
            with pytest.raises(_lib.Nd4HipError) as e:
                fn(A, -np.eye(N), **kw)
            assert e.value.code == -5 and MSG_B % 0 in str(e.value), (kw, str(e.value))
            with pytest.raises(_lib.Nd4HipError) as e:
                fn(As, Bs, **kw)
            assert e.value.code == -5 and MSG_B % 1 in str(e.value), (kw, str(e.value))
            with pytest.raises(_lib.Nd4HipError) as e:
                fn(A2, good, **kw)
            assert e.value.code == -3 and MSG_C in str(e.value), (kw, str(e.value))
        with pytest.raises(_lib.Nd4HipError) as e:
            dev.eigen_sym_gen(_up(As), _up(Bs), **kw)
        assert e.value.code == -5 and MSG_B % 1 in str(e.value)
        with pytest.raises(_lib.Nd4HipError) as e:
            la.eigen_sym_gen(np.stack([A, A2, A]), good, **kw)
        assert e.value.code == -3
        after = la.eigen_sym_gen(A, good, subset=(0, 2))
        assert G.same_bits(after[0], before[0]) and G.same_bits(after[1], before[1])
    for kw in ({"subset": (0, 1)}, {"interval": (0.0, 1.0)}, {"reduction": "tridiag"}):
        with pytest.raises(ValueError, match="not available with algo='jacobi'"):
            dev.eigen_sym_gen(_up(A), _up(good), algo="jacobi", **kw)


def test_gen_profile_and_empty():
    torch, dev = _dev()
    A, B = (_up(M) for M in G.inputs("gram_33"))
    h = _lib.handle(0)
    h.profile_enable(True)
    try:
        dev.eigen_sym_gen(A, B, subset=(0, 4))
        rec = h.profile_last()[0]
    finally:
        h.profile_enable(False)
    assert rec["op"] == "dsygvx_batched" and rec["valid"] and rec["kernel_ms"] > 0
    lam, X = la.eigen_sym_gen(np.zeros((0, 4, 4)), np.eye(4), subset=(1, 3))
    assert lam.shape == (0, 2) and X.shape == (0, 4, 2)
    lam, X = la.eigen_sym_gen(np.eye(4), np.eye(4), subset=(2, 2), reduction="tridiag")
    assert lam.shape == (0,) and X.shape == (4, 0)
    info = {}
    lam, X = dev.eigen_sym_gen(A, B, interval=(1e9, INF), info=info)
    assert tuple(lam.shape) == (0,) and tuple(X.shape) == (33, 0) and info["range"].cpu().tolist() == [0, 0]
