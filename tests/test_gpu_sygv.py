"""eigen_sym_gen / eigenvals_sym_gen on the device (csrc/sygv.hip) through la (host arrays) and dev (device tensors): the bounds of
tests/sygv_common.py against the committed LAPACK values on every catalogue case, and, for the fused small tier (N <= 64), the bits
of the numpy model of the same module composed with the solver's own model (Jacobi) or the device's own eigen_sym (default).

Largest shares of the bounds seen (values, residual, B-orthonormality, reduction): the model 4.9e-4, 8.2e-5, 1.3e-3, 3.1e-5
(test_sygv_host.py); the device, default route 4.5e-4 (gram_65_lead64), 1.8e-4 (gram_2), 1.5e-3 (gram_300), reduction 3.1e-5 in the
small tier (the model's bits) and 5.8e-6 in the large one (gram_65); with algo='jacobi' 4.8e-4, 1.1e-4, 1.1e-3. Every test prints
its shares.

Mutants of the kernels and the test that catches each:
  FMA contraction, another summation order        test_small_tier_sygst_is_the_model_bit_for_bit
  C taken from W instead of W^T                   test_small_tier_sygst_is_the_model_bit_for_bit, test_catalogue_through_la_and_dev
  upper triangle of A or B read                   test_catalogue_through_la_and_dev (NaN and 1e300 above the diagonals)
  last pivot not checked / only NaN checked       test_b_not_positive_definite (zero matrix, exact zero in the last pivot)
  B factorised per chunk position                 test_shared_b_equals_the_stacked_call
  member index in gridDim.y                       test_batch_of_70000_members"""
import ctypes
import functools

import numpy as np
import pytest

import eigsym_jacobi_common as J
import sygv_common as G
from nd4js_amd import _lib, la

pytestmark = pytest.mark.gpu

MSG_B = "eigen_sym_gen(A,B): B is not positive definite. (matrix %d)"
MSG_C = "eigen_sym_gen(A,B): L^-1 A L^-T is not finite (NaN or Infinity in the lower triangle of A, or overflow)."


def _dev():
    import torch
    from nd4js_amd import dev
    return torch, dev


@functools.lru_cache(maxsize=None)
def _run(name, algo=None):
    """(lambda, X, sweeps) of a catalogue case through la; read-only, shared by the tests"""
    A, B = G.inputs(name)
    info = {}
    lam, X = la.eigen_sym_gen(A, B, algo=algo, info=info)
    out = G.ec._freeze(lam, X)
    return out + (info.get("sweeps"),)


@functools.lru_cache(maxsize=None)
def _model_reduce(name):
    """(L, C) of the model for every member of a small-tier case, stacked like A"""
    A, B = G.inputs(name)
    N = A.shape[-1]
    L, C = np.empty(A.shape), np.empty(A.shape)
    for m, (a, b) in enumerate(G.members(A, B)):
        l, c, bad = G.reduce_model(a, b)
        assert not bad
        L.reshape(-1, N, N)[m], C.reshape(-1, N, N)[m] = l, c
    return G.ec._freeze(L, C)


@pytest.mark.parametrize("name", G.NAMES)
def test_catalogue_through_la_and_dev(name):
    torch, dev = _dev()
    A, B = G.inputs(name)
    lam, X, _ = _run(name)
    sh = G.check(A, B, lam, X, G.golden(name), name)
    print("%s shares of the bounds (values, residual, B-orthonormality): %.3g %.3g %.3g" % ((name,) + sh))
    assert G.same_bits(la.eigenvals_sym_gen(A, B), lam)
    ta, tb = torch.from_numpy(np.array(A)).cuda(), torch.from_numpy(np.array(B)).cuda()
    ka, kb = ta.clone(), tb.clone()
    ld, xd = dev.eigen_sym_gen(ta, tb)
    assert torch.equal(ta, ka) and torch.equal(tb, kb)
    assert G.same_bits(ld.cpu().numpy(), lam) and G.same_bits(xd.cpu().numpy(), X)
    assert G.same_bits(dev.eigenvals_sym_gen(ta, tb).cpu().numpy(), lam) and torch.equal(ta, ka) and torch.equal(tb, kb)
    if A.shape[-1] > 1:
        for fill in (np.nan, 1e300):
            A2, B2 = G.with_upper(A, fill), G.with_upper(B, fill)
            a0, b0 = A2.copy(), B2.copy()
            l2, x2 = la.eigen_sym_gen(A2, B2)
            assert np.array_equal(A2, a0, equal_nan=True) and np.array_equal(B2, b0, equal_nan=True)
            assert G.same_bits(l2, lam) and G.same_bits(x2, X), "%s: upper triangles %r changed the result" % (name, fill)


@pytest.mark.parametrize("name", [n for n in G.NAMES if G.SIZES[n] <= J.MAXN])
def test_catalogue_jacobi(name):
    torch, dev = _dev()
    A, B = G.inputs(name)
    lam, X, sweeps = _run(name, "jacobi")
    assert sweeps.dtype == np.int32 and sweeps.shape == A.shape[:-2] and np.all(sweeps >= 1)
    sh = G.check(A, B, lam, X, G.golden(name), name)
    print("%s (jacobi) shares of the bounds: %.3g %.3g %.3g" % ((name,) + sh))
    info = {}
    assert G.same_bits(la.eigenvals_sym_gen(A, B, algo="jacobi", info=info), lam) and np.array_equal(info["sweeps"], sweeps)
    info2 = {}
    ld, xd = dev.eigen_sym_gen(torch.from_numpy(np.array(A)).cuda(), torch.from_numpy(np.array(B)).cuda(), algo="jacobi", info=info2)
    assert G.same_bits(ld.cpu().numpy(), lam) and G.same_bits(xd.cpu().numpy(), X)
    assert info2["sweeps"].dtype == torch.int32 and np.array_equal(info2["sweeps"].cpu().numpy(), sweeps)


# ---- the small tier, bit for bit -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", G.SMALL_NAMES)
def test_small_tier_sygst_is_the_model_bit_for_bit(name):
    torch, dev = _dev()
    A, _ = G.inputs(name)
    L, C = _model_reduce(name)
    got = la._sygst(A, L)
    assert G.same_bits(got, C), "%s: C differs from the model by %.3g" % (name, np.abs(got - C).max())
    assert G.same_bits(dev._sygst(torch.from_numpy(np.array(A)).cuda(), torch.from_numpy(np.array(L)).cuda()).cpu().numpy(), C)
    print("%s reduction share: %.3g" % (name, G.reduction_share(A, L, got)))
    assert G.reduction_share(A, L, got) <= 1.0


@pytest.mark.parametrize("name", G.SMALL_NAMES)
def test_small_tier_jacobi_is_the_composed_model_bit_for_bit(name):
    A, B = G.inputs(name)
    N = A.shape[-1]
    L, C = _model_reduce(name)
    lam, X, sweeps = _run(name, "jacobi")
    for m in range(len(G.members(A, B))):
        l, y, sw, done = J.model(C.reshape(-1, N, N)[m])
        assert done
        x = G.back_model(L.reshape(-1, N, N)[m], y)
        assert G.same_bits(lam.reshape(-1, N)[m], l) and sweeps.reshape(-1)[m] == sw, "%s member %d" % (name, m)
        assert G.same_bits(X.reshape(-1, N, N)[m], x), "%s member %d: X differs from the model by %.3g" % (name, m, np.abs(X.reshape(-1, N, N)[m] - x).max())


@pytest.mark.parametrize("name", G.SMALL_NAMES)
def test_small_tier_default_route_is_model_reduce_eigen_sym_model_back(name):
    A, B = G.inputs(name)
    N = A.shape[-1]
    L, C = _model_reduce(name)
    lam, X, _ = _run(name)
    l, Y = la.eigen_sym(C)
    assert G.same_bits(lam, l)
    for m in range(len(G.members(A, B))):
        assert G.same_bits(X.reshape(-1, N, N)[m], G.back_model(L.reshape(-1, N, N)[m], Y.reshape(-1, N, N)[m])), "%s member %d" % (name, m)


@pytest.mark.parametrize("name", G.SMALL_NAMES)
@pytest.mark.parametrize("algo", [None, "jacobi"])
def test_identity_b_gives_the_bits_of_eigen_sym(name, algo):
    A = G.inputs(name)[0]
    lam, V = la.eigen_sym(A, algo=algo)
    l2, x2 = la.eigen_sym_gen(A, np.eye(A.shape[-1]), algo=algo)
    assert G.same_bits(l2, lam) and G.same_bits(x2, V)


# ---- the large tier and the tier edge --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["gram_65", "graded_65", "gram_130", "graded_130", "gram_300", "graded_300", "batch_2x130"])
def test_large_tier_sygst_meets_the_reduction_bound(name):
    A, B = G.inputs(name)
    L = np.linalg.cholesky(B)
    C = la._sygst(A, L)
    assert np.all(np.triu(C, 1) == 0.0)
    share = G.reduction_share(A, L, C)
    print("%s reduction share: %.3g" % (name, share))
    assert share <= 1.0
    assert G.same_bits(la._sygst(G.with_upper(A, np.nan), L), C)


def test_tier_edge_64_and_65_on_the_same_leading_data():
    A65, B65 = G.inputs("gram_65")
    A64, B64 = G.inputs("gram_65_lead64")
    assert np.array_equal(A64, A65[:64, :64]) and np.array_equal(B64, B65[:64, :64])
    for name in ("gram_65_lead64", "gram_65"):
        lam, X, _ = _run(name)
        G.check(*G.inputs(name), lam, X, G.golden(name), name)
    # interlacing of the leading principal pencil
    l64, l65 = _run("gram_65_lead64")[0], _run("gram_65")[0]
    tol = 1e-12 * np.abs(l65).max()
    assert np.all(l65[:-1] + tol >= l64) and np.all(l64 + tol >= l65[1:])


# ---- exact scalings --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [40, 130])
@pytest.mark.parametrize("k", [-500, -3, 1, 500])
def test_scaling_a_by_a_power_of_two_is_exact(N, k):
    A, B = G.inputs("gram_300")
    A, B = np.array(A[:N, :N]), np.array(B[:N, :N])
    lam, X = la.eigen_sym_gen(A, B)
    l2, x2 = la.eigen_sym_gen(np.ldexp(A, k), B)
    assert G.same_bits(l2, np.ldexp(lam, k)) and G.same_bits(x2, X)


@pytest.mark.parametrize("j", [-200, 3, 200])
def test_scaling_b_by_a_power_of_four_is_exact(j):
    A, B = G.inputs("gram_300")
    A, B = np.array(A[:40, :40]), np.array(B[:40, :40])
    lam, X = la.eigen_sym_gen(A, B)
    l2, x2 = la.eigen_sym_gen(A, np.ldexp(B, 2 * j))
    assert G.same_bits(l2, np.ldexp(lam, -2 * j)) and G.same_bits(x2, np.ldexp(X, -j))


# ---- batches ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name, algo", [("batch_5x40", None), ("batch_5x40", "jacobi"), ("batch_2x130", None), ("shared_3x40", None),
                                        ("shared_3x40", "jacobi")])
def test_batch_members_equal_their_single_runs(name, algo):
    A, B = G.inputs(name)
    lam, X, sweeps = _run(name, algo)
    for m, (a, b) in enumerate(G.members(A, B)):
        info = {}
        l1, x1 = la.eigen_sym_gen(np.array(a), np.array(b), algo=algo, info=info)
        assert G.same_bits(l1, lam[m]) and G.same_bits(x1, X[m]), "%s member %d" % (name, m)
        assert algo is None or info["sweeps"] == sweeps[m]


@pytest.mark.parametrize("algo", [None, "jacobi"])
def test_shared_b_equals_the_stacked_call(algo):
    A, B = G.inputs("shared_3x40")
    lam, X, _ = _run("shared_3x40", algo)
    l2, x2 = la.eigen_sym_gen(A, np.stack([B, B, B]), algo=algo)
    assert G.same_bits(l2, lam) and G.same_bits(x2, X)
    assert G.same_bits(la.eigenvals_sym_gen(A, B, algo=algo), lam)
    # the large tier's broadcast
    A2 = G.inputs("batch_2x130")[0]
    B2 = G.inputs("gram_130")[1]
    l3, x3 = la.eigen_sym_gen(A2, B2)
    l4, x4 = la.eigen_sym_gen(A2, np.stack([B2, B2]))
    assert G.same_bits(l3, l4) and G.same_bits(x3, x4)


def test_batch_of_70000_members():
    """more members than one grid dimension or one pass takes; the bounds of sygv_common, vectorised. The reference values here are
    not the committed scipy ones (70 000 members are not kept as a fixture): they come from numpy's LAPACK along the same route
    (cholesky, two solves, eigvalsh), which shares no code with the device."""
    nb = 70000
    g = G.rng.matrix(8400, nb, 4).reshape(nb, 2, 2)
    A = np.tril(g) + np.swapaxes(np.tril(g, -1), -1, -2)
    x = G.rng.matrix(8401, nb, 4).reshape(nb, 2, 2)
    B = x @ np.swapaxes(x, -1, -2) / 2 + np.eye(2)
    B = np.tril(B) + np.swapaxes(np.tril(B, -1), -1, -2)
    lam, X = la.eigen_sym_gen(A, B)
    Lc = np.linalg.cholesky(B)
    W = np.linalg.solve(Lc, A)
    Cm = np.linalg.solve(Lc, np.swapaxes(W, -1, -2))
    ref = np.linalg.eigvalsh(Cm)[:, ::-1]
    sv = np.linalg.svd(B, compute_uv=False)
    kappa = sv[:, 0] / sv[:, 1]
    na, nbn = np.linalg.norm(A, axis=(-2, -1)), np.linalg.norm(B, axis=(-2, -1))
    assert np.all(np.diff(lam, axis=-1) <= 0)
    share = np.abs(lam - ref) / (G.TOL * ((na / sv[:, 1])[:, None] + kappa[:, None] * np.abs(ref)))
    print("70000 x 2^2: largest share of the values bound %.3g" % share.max())
    assert np.all(share <= 1.0)
    res = np.linalg.norm(A @ X - (B @ X) * lam[:, None, :], axis=(-2, -1))
    assert np.all(res <= G.TOL * (na + nbn * np.abs(lam).max(-1)) * np.linalg.norm(X, axis=(-2, -1)))
    orth = np.linalg.norm(np.swapaxes(X, -1, -2) @ B @ X - np.eye(2), axis=(-2, -1))
    assert np.all(orth <= G.TOL * kappa * np.sqrt(2.0))
    # members on both sides of every pass boundary equal their single runs
    for m in (0, 32767, 32768, 65535, 65536, nb - 1):
        l1, x1 = la.eigen_sym_gen(A[m], B[m])
        assert G.same_bits(l1, lam[m]) and G.same_bits(x1, X[m]), "member %d" % m


# ---- errors ----------------------------------------------------------------------------------------------------------------------
def _exact_zero_last_pivot(N):
    """B = L0 L0^T exactly: L0 the identity with small integers in its last row and L0[N-1, N-1] = 0. Every product and sum of the
    factorisation is exact in any order, every pivot but the last is 1, the last radicand is an exact zero and no NaN appears"""
    L0 = np.eye(N)
    L0[N - 1, :] = np.round(G.rng.fill_uniform(8410 + N, N) * 2.0)
    L0[N - 1, N - 1] = 0.0
    return L0 @ L0.T


def _lowered_gram(N):
    """a gram B whose last diagonal entry is lowered until only the last pivot is <= 0"""
    B = np.array(G.gram(8420 + N, N))
    L, bad = G.chol_model(B)
    assert not bad
    B[N - 1, N - 1] -= 2.0 * L[N - 1, N - 1] ** 2
    L2, bad2 = G.chol_model(B)
    assert bad2 and np.all(np.isfinite(L2[:N - 1])) and np.all(np.diag(L2)[:N - 1] > 0)
    return B


def _bad_bs(N):
    out = {"minus_identity": -np.eye(N), "zero": np.zeros((N, N)), "lowered_gram": _lowered_gram(N), "exact_zero_last_pivot": _exact_zero_last_pivot(N)}
    if N > 1:
        out["ones"] = np.ones((N, N))
    return out


@pytest.mark.parametrize("N", [1, 3, 40, 130])
def test_b_not_positive_definite(N):
    torch, dev = _dev()
    A = np.array(G.inputs("gram_300")[0][:N, :N])
    good = np.array(G.inputs("gram_300")[1][:N, :N])
    before = la.eigen_sym_gen(A, good)
    for kind, Bb in _bad_bs(N).items():
        for fn in (la.eigen_sym_gen, la.eigenvals_sym_gen):
            for algo in (None, "jacobi") if N <= J.MAXN else (None,):
                with pytest.raises(_lib.Nd4HipError) as e:
                    fn(A, Bb, algo=algo)
                assert e.value.code == -5 and MSG_B % 0 in str(e.value), "%s N=%d: %s" % (kind, N, e.value)
        # in a batch the lowest bad member is named; one bad B that serves every member is member 0's
        As, Bs = np.stack([A, A, A, A]), np.stack([good, Bb, good, Bb])
        with pytest.raises(_lib.Nd4HipError) as e:
            la.eigen_sym_gen(As, Bs)
        assert e.value.code == -5 and MSG_B % 1 in str(e.value), "%s N=%d: %s" % (kind, N, e.value)
        with pytest.raises(_lib.Nd4HipError) as e:
            dev.eigen_sym_gen(torch.from_numpy(As).cuda(), torch.from_numpy(Bs).cuda())
        assert e.value.code == -5 and MSG_B % 1 in str(e.value)
        with pytest.raises(_lib.Nd4HipError) as e:
            la.eigen_sym_gen(As, Bb)
        assert e.value.code == -5 and MSG_B % 0 in str(e.value)
        after = la.eigen_sym_gen(A, good)
        assert G.same_bits(after[0], before[0]) and G.same_bits(after[1], before[1])


@pytest.mark.parametrize("N", [3, 40, 130])
def test_non_finite_a_is_noconv_and_the_handle_stays_usable(N):
    A = np.array(G.inputs("gram_300")[0][:N, :N])
    B = np.array(G.inputs("gram_300")[1][:N, :N])
    before = la.eigen_sym_gen(A, B)
    for bad in (np.nan, np.inf, -np.inf):
        A2 = A.copy()
        A2[N - 1, N // 2] = bad
        for fn in (la.eigen_sym_gen, la.eigenvals_sym_gen):
            with pytest.raises(_lib.Nd4HipError) as e:
                fn(A2, B)
            assert e.value.code == -3 and MSG_C in str(e.value)
        after = la.eigen_sym_gen(A, B)
        assert G.same_bits(after[0], before[0]) and G.same_bits(after[1], before[1])
    As = np.stack([A, A, A])
    As[2, 0, 0] = np.nan
    with pytest.raises(_lib.Nd4HipError) as e:
        la.eigen_sym_gen(As, B)
    assert e.value.code == -3


@pytest.mark.parametrize("N, algo", [(2049, 0), (129, 1)])
@pytest.mark.parametrize("vectors", [True, False])
def test_size_limits_are_argument_errors_and_nothing_is_written(N, algo, vectors):
    torch, dev = _dev()
    A = torch.zeros((1, N, N), dtype=torch.float64, device="cuda")
    B = torch.eye(N, dtype=torch.float64, device="cuda")
    lam = torch.full((1, N), 7.0, dtype=torch.float64, device="cuda")
    X = torch.full((1, N, N), 7.0, dtype=torch.float64, device="cuda")
    sw = torch.full((1,), 7, dtype=torch.int32, device="cuda")
    h = _lib.handle(0)
    p = lambda x: ctypes.c_void_p(x.data_ptr())
    rc = h.lib.nd4hip_dsygvd_batched_dev(h.ptr, algo, 1, N, p(A), p(B), 0, p(lam), p(X) if vectors else None, p(sw))
    assert rc == -1 and (b"N <= 128" if algo else b"N <= 2048") in h.lib.nd4hip_last_error()
    torch.cuda.synchronize()
    assert bool((lam == 7.0).all()) and bool((X == 7.0).all()) and bool((sw == 7).all())
    with pytest.raises(_lib.Nd4HipError) as e:
        (dev.eigen_sym_gen if vectors else dev.eigenvals_sym_gen)(A, B, algo="jacobi" if algo else None)
    assert e.value.code == -1
    if N == 129:
        with pytest.raises(_lib.Nd4HipError) as e:
            (la.eigen_sym_gen if vectors else la.eigenvals_sym_gen)(np.zeros((N, N)), np.eye(N), algo="jacobi")
        assert e.value.code == -1 and "N <= 128" in str(e.value)


def test_dev_argument_errors_on_device_tensors():
    torch, dev = _dev()
    z = lambda *shape: torch.zeros(shape, dtype=torch.float64, device="cuda")
    for fn, name in ((dev.eigen_sym_gen, "eigen_sym_gen"), (dev.eigenvals_sym_gen, "eigenvals_sym_gen")):
        for a, b, text in ((z(3), z(3, 3), "A.ndim must be at least 2."), (z(3, 3), z(3), "B.ndim must be at least 2."),
                           (z(2, 3, 4), z(3, 3), "A must be quadratic."), (z(3, 3), z(3, 4), "B must be quadratic."),
                           (z(3, 3), z(4, 4), "B.shape must be A.shape or A.shape[-2:]"),
                           (z(2, 3, 3), z(3, 3, 3), "B.shape must be A.shape or A.shape[-2:]"),
                           (z(3, 3), z(2, 3, 3), "B.shape must be A.shape or A.shape[-2:]")):
            with pytest.raises(ValueError) as e:
                fn(a, b)
            assert "%s(A,B): %s" % (name, text) in str(e.value)
        with pytest.raises(TypeError):
            fn(z(4, 4)[:3, :3], z(3, 3))                             # not contiguous
        with pytest.raises(TypeError):
            fn(z(3, 3), torch.eye(3, dtype=torch.float64))           # B on the host
    if torch.cuda.device_count() > 1:
        with pytest.raises(ValueError, match="same device"):
            dev.eigen_sym_gen(z(3, 3), torch.eye(3, dtype=torch.float64, device="cuda:1"))
    with pytest.raises(ValueError) as e:
        dev._sygst(z(3, 3), z(4, 4))
    assert "_sygst(A,L): L.shape must be A.shape or A.shape[-2:]" in str(e.value)


def test_empty_inputs():
    for algo in (None, "jacobi"):
        lam, X = la.eigen_sym_gen(np.zeros((3, 0, 0)), np.zeros((3, 0, 0)), algo=algo)
        assert lam.shape == (3, 0) and X.shape == (3, 0, 0)
        lam, X = la.eigen_sym_gen(np.zeros((0, 4, 4)), np.eye(4), algo=algo)
        assert lam.shape == (0, 4) and X.shape == (0, 4, 4)
        assert la.eigenvals_sym_gen(np.zeros((0, 4, 4)), np.zeros((0, 4, 4)), algo=algo).shape == (0, 4)


def test_profile_record():
    torch, dev = _dev()
    A, B = (torch.from_numpy(np.array(m)).cuda() for m in G.inputs("batch_5x40"))
    h = _lib.handle(0)
    h.profile_enable(True)
    try:
        recs = []
        for fn, algo in ((dev.eigen_sym_gen, None), (dev.eigenvals_sym_gen, None), (dev.eigen_sym_gen, "jacobi"), (dev.eigenvals_sym_gen, "jacobi")):
            fn(A, B, algo=algo)
            recs.append(h.profile_last()[0])
    finally:
        h.profile_enable(False)
    n3 = 40.0 ** 3
    reduce_ = 1.0 / 3.0 + 2.0
    want = [10.0 / 3.0 + 2.0 + 2.0 + reduce_ + 1.0, 10.0 / 3.0 + 2.0 + reduce_, 64.0 + reduce_ + 1.0, 32.0 + reduce_]
    for rec, w in zip(recs, want):
        assert rec["op"] == "dsygvd_batched" and rec["valid"] and rec["kernel_ms"] > 0
        assert rec["flops"] == pytest.approx(5 * w * n3, rel=1e-12)
