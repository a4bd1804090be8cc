"""eigen_sym / eigenvals_sym on the device (csrc/syev.hip) through la (host arrays) and dev (device tensors): every input of
tests/eigsym_common.py against LAPACK and, where committed, against the reference's own nd.la.eigen values, inside the bounds of
that module. Largest shares of those bounds: the numpy model 3.9e-3 (values), 1.3e-2 (residual), 2.6e-3 (orthogonality); the
device 9.0e-4, 3.5e-3 and 4.7e-3 (printed per input)."""
import ctypes

import numpy as np
import pytest

import eigsym_common as C
from nd4js_amd import _lib, la

pytestmark = pytest.mark.gpu


def _dev():
    import torch
    from nd4js_amd import dev
    return torch, dev


@pytest.mark.parametrize("name", C.NAMES)
def test_catalogue_through_la_and_dev(name):
    torch, dev = _dev()
    S, lam_ref, V_ref = C.reference(name)
    lam, V = la.eigen_sym(S)
    sh = C.check(S, lam, V, lam_ref, name)
    print("%s shares of the bounds (values, residual, orthogonality): %.3g %.3g %.3g" % ((name,) + sh))
    C.check_vectors(S, V, lam_ref, V_ref, name)
    assert np.array_equal(la.eigenvals_sym(S), lam), "eigenvals_sym must have eigen_sym's bits"
    # the device form: the same bits, and the input tensor is not written
    t = torch.from_numpy(np.array(S)).cuda()
    keep = t.clone()
    ld, vd = dev.eigen_sym(t)
    assert torch.equal(t, keep)
    assert np.array_equal(ld.cpu().numpy(), lam) and np.array_equal(vd.cpu().numpy(), V)
    assert np.array_equal(dev.eigenvals_sym(t).cpu().numpy(), lam) and torch.equal(t, keep)
    # the upper triangle is ignored: NaN and garbage there change no bit; S itself is never written
    for fill in (np.nan, 1e300):
        X = C.with_upper(S, fill)
        before = X.copy()
        l2, v2 = la.eigen_sym(X)
        assert np.array_equal(X, before, equal_nan=True)
        assert np.array_equal(l2, lam) and np.array_equal(v2, V), "%s: upper triangle %r changed the result" % (name, fill)


@pytest.mark.parametrize("name", sorted(C.golden_manifest()["cases"]))
def test_committed_reference_values(name):
    meta = C.golden_manifest()["cases"][name]
    S = C.golden_input(name, meta)
    want = C.golden_values(name, meta)
    lam, V = la.eigen_sym(S)
    lapack = np.linalg.eigvalsh(S)[::-1]
    C.check(S, lam, V, lapack, name)
    if want is not None:
        nrm = np.linalg.norm(S)
        assert np.abs(lam - np.sort(want.real)[::-1]).max() <= C.TOL * nrm


@pytest.mark.parametrize("name", ["batch_5x40", "batch_2x130"])
def test_batch_members_equal_their_single_runs(name):
    S, _, _ = C.reference(name)
    lam, V = la.eigen_sym(S)
    for b in range(S.shape[0]):
        l1, v1 = la.eigen_sym(S[b])
        assert np.array_equal(l1, lam[b]) and np.array_equal(v1, V[b]), "%s member %d" % (name, b)


@pytest.mark.parametrize("k", [-500, -3, 1, 500])
def test_power_of_two_scaling_is_exact(k):
    S, _, _ = C.reference("batch_5x40")
    S = S[0]
    lam, V = la.eigen_sym(S)
    l2, v2 = la.eigen_sym(np.ldexp(S, k))
    assert np.array_equal(l2, np.ldexp(lam, k)) and np.array_equal(v2, V)


def test_identity_and_zero_are_exact():
    for N in (2, 8, 130):
        lam, V = la.eigen_sym(np.eye(N))
        assert np.array_equal(lam, np.ones(N))
        assert np.linalg.norm(V.T @ V - np.eye(N)) <= C.TOL * np.sqrt(N)
        lam, V = la.eigen_sym(np.zeros((N, N)))
        assert np.array_equal(lam, np.zeros(N)) and not np.signbit(lam).any()
        assert np.linalg.norm(V.T @ V - np.eye(N)) <= C.TOL * np.sqrt(N)
    assert la.eigen_sym(np.zeros((3, 0, 0)))[0].shape == (3, 0) and la.eigenvals_sym(np.zeros((0, 4, 4))).shape == (0, 4)
    lam, V = la.eigen_sym(np.array([[[-2.5]], [[0.0]]]))
    assert np.array_equal(lam, [[-2.5], [0.0]]) and np.array_equal(V, np.ones((2, 1, 1)))


def test_n_above_the_solver_limit_is_an_argument_error():
    torch, dev = _dev()
    S = torch.zeros((2049, 2049), dtype=torch.float64, device="cuda")
    lam = torch.full((2049,), 7.0, dtype=torch.float64, device="cuda")
    V = torch.full((2049, 2049), 7.0, dtype=torch.float64, device="cuda")
    h = _lib.handle(0)
    rc = h.lib.nd4hip_dsyevd_batched_dev(h.ptr, 1, 2049, ctypes.c_void_p(S.data_ptr()), ctypes.c_void_p(lam.data_ptr()), ctypes.c_void_p(V.data_ptr()))
    assert rc == -1 and b"N <= 2048" in h.lib.nd4hip_last_error()
    torch.cuda.synchronize()
    assert bool((lam == 7.0).all()) and bool((V == 7.0).all())
    with pytest.raises(_lib.Nd4HipError) as e:
        la.eigenvals_sym(np.zeros((2049, 2049)))
    assert e.value.code == -1


@pytest.mark.parametrize("N", [3, 40, 130])
def test_nan_or_inf_in_the_lower_triangle_is_noconv_and_the_handle_stays_usable(N):
    S, _, _ = C.reference("batch_2x130" if N == 130 else "batch_5x40")
    S = np.array(S[0][:N, :N])
    before = la.eigen_sym(S)
    for bad in (np.nan, np.inf, -np.inf):
        X = S.copy()
        X[N - 1, N // 2] = bad
        for fn in (la.eigen_sym, la.eigenvals_sym):
            with pytest.raises(_lib.Nd4HipError) as e:
                fn(X)
            assert e.value.code == -3 and "NaN or Infinity in its lower triangle" in str(e.value)
        after = la.eigen_sym(S)
        assert np.array_equal(after[0], before[0]) and np.array_equal(after[1], before[1])
    # one bad member fails the call; the others are not looked at
    B = np.stack([S, S])
    B[1, 0, 0] = np.nan
    with pytest.raises(_lib.Nd4HipError):
        la.eigen_sym(B)


def test_profile_record():
    torch, dev = _dev()
    S = torch.from_numpy(np.array(C.reference("dense_70")[0])).cuda()
    h = _lib.handle(0)
    h.profile_enable(True)
    try:
        dev.eigen_sym(S)
        rec = h.profile_last()[0]
        stages = h.eigsym_last_stages()
        dev.eigenvals_sym(S)
        rec2 = h.profile_last()[0]
    finally:
        h.profile_enable(False)
    assert rec["op"] == "dsyevd_batched" and rec["flops"] == pytest.approx((10.0 / 3.0 + 4.0) * 70.0 ** 3, rel=1e-12)
    assert rec2["op"] == "dsyevd_batched" and rec2["flops"] == pytest.approx((10.0 / 3.0 + 2.0) * 70.0 ** 3, rel=1e-12)
    assert rec["valid"] and rec["kernel_ms"] > 0 and set(stages) == set(h.EIGSYM_STAGES) and all(v > 0 for v in stages.values())
