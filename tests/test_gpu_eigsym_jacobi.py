"""eigen_sym / eigenvals_sym with algo='jacobi' on the device (csrc/syevj.hip) through la (host arrays) and dev (device tensors).
The kernel has no reductions and is compiled without FMA contraction, so lambda, V and the sweep count of every member must be
the bits of the numpy model in tests/eigsym_jacobi_common.py; what the model itself is worth is test_eigsym_jacobi_host.py's
business (the bounds of eigsym_common against LAPACK, the relative bound against 60-digit values). The relative bound is asserted
here on the device's own output all the same.

Arithmetic mutants of the kernel (loop bounds untouched) and the test that catches each:
  absolute criterion                          test_relative_accuracy_on_graded_positive_definite_input (and every bitwise test)
  plain c / s rotation without tau            test_catalogue_bitwise_through_la_and_dev (every dense input)
  descending pair order (q < p)               test_catalogue_bitwise_through_la_and_dev (the sign pattern of V and the bits change)
  s_pq not zeroed                             test_catalogue_bitwise_through_la_and_dev (eqdiag_2: the sweep count; dense: the bits)
  sort ties by descending index               test_catalogue_bitwise_through_la_and_dev (diag_ties_6, identity_8, mixed_7x8: V)
  member 0's sweep count for the workgroup    test_catalogue_bitwise_through_la_and_dev (mixed_7x8: sweeps 1, 1, 6, 1, 6, 6, 7) and
                                              test_batch_members_equal_their_single_runs"""
import ctypes

import numpy as np
import pytest

import eigsym_common as C
import eigsym_jacobi_common as J
from nd4js_amd import _lib, la

pytestmark = pytest.mark.gpu


def _dev():
    import torch
    from nd4js_amd import dev
    return torch, dev


@pytest.mark.parametrize("name", J.names())
def test_catalogue_bitwise_through_la_and_dev(name):
    torch, dev = _dev()
    S, lam_m, V_m, sw_m = J.case(name)
    info = {}
    lam, V = la.eigen_sym(S, algo="jacobi", info=info)
    assert info["sweeps"].dtype == np.int32 and np.array_equal(info["sweeps"], sw_m), "%s: sweeps %s, model %s" % (name, info["sweeps"], sw_m)
    assert J.same_bits(lam, lam_m), "%s: lambda differs from the model by %.3g" % (name, np.abs(lam - lam_m).max())
    assert J.same_bits(V, V_m), "%s: V differs from the model by %.3g" % (name, np.abs(V - V_m).max())
    sh = C.check(S, lam, V, J.lapack(name)[0], name)
    print("%s shares of the bounds (values, residual, orthogonality): %.3g %.3g %.3g" % ((name,) + sh))
    # values only: the same bits and the same sweeps
    info2 = {}
    assert J.same_bits(la.eigenvals_sym(S, algo="jacobi", info=info2), lam) and np.array_equal(info2["sweeps"], sw_m)
    # the device form: the same bits, and the input tensor is not written
    t = torch.from_numpy(np.array(S)).cuda()
    keep = t.clone()
    info3 = {}
    ld, vd = dev.eigen_sym(t, algo="jacobi", info=info3)
    assert torch.equal(t, keep)
    assert J.same_bits(ld.cpu().numpy(), lam) and J.same_bits(vd.cpu().numpy(), V)
    assert info3["sweeps"].dtype == torch.int32 and np.array_equal(info3["sweeps"].cpu().numpy(), sw_m)
    assert J.same_bits(dev.eigenvals_sym(t, algo="jacobi").cpu().numpy(), lam) and torch.equal(t, keep)
    # the upper triangle is ignored: NaN and garbage there change no bit; S itself is never written
    if S.shape[-1] > 1:
        for fill in (np.nan, 1e300):
            X = C.with_upper(S, fill)
            before = X.copy()
            l2, v2 = la.eigen_sym(X, algo="jacobi")
            assert np.array_equal(X, before, equal_nan=True)
            assert J.same_bits(l2, lam) and J.same_bits(v2, V), "%s: upper triangle %r changed the result" % (name, fill)


@pytest.mark.parametrize("name", sorted(J.GRADED))
def test_relative_accuracy_on_graded_positive_definite_input(name):
    S = J.case(name)[0]
    N = S.shape[-1]
    ref = J.graded_reference(name)
    bound = N * J.EPS * J.scaled_kappa(S)
    lam, V = la.eigen_sym(S, algo="jacobi")
    err = (np.abs(lam - ref) / ref).max()
    err_default = (np.abs(la.eigenvals_sym(S) - ref) / ref).max()
    print("%s: relative error %.3g = %.3g of N eps kappa_2(A) = %.3g; the default route: %.3g" % (name, err, err / bound, bound, err_default))
    assert err <= bound


@pytest.mark.parametrize("name", ["mixed_7x8", "batch_3x40", "batch_5x40"])
def test_batch_members_equal_their_single_runs(name):
    S = J.case(name)[0]
    info = {}
    lam, V = la.eigen_sym(S, algo="jacobi", info=info)
    for b in range(S.shape[0]):
        one = {}
        l1, v1 = la.eigen_sym(S[b], algo="jacobi", info=one)
        assert J.same_bits(l1, lam[b]) and J.same_bits(v1, V[b]) and one["sweeps"] == info["sweeps"][b], "%s member %d" % (name, b)
    # another position, other neighbours, another batch size
    R = np.ascontiguousarray(S[::-1])
    info2 = {}
    l2, v2 = la.eigen_sym(np.concatenate([R, R[:2]]), algo="jacobi", info=info2)
    n = S.shape[0]
    assert J.same_bits(l2[:n], lam[::-1]) and J.same_bits(v2[:n], V[::-1]) and np.array_equal(info2["sweeps"][:n], info["sweeps"][::-1])
    assert J.same_bits(l2[n:], lam[::-1][:2]) and J.same_bits(v2[n:], V[::-1][:2])


@pytest.mark.parametrize("k", [-500, 500])
@pytest.mark.parametrize("N", [8, 40, 100])
def test_power_of_two_scaling_is_exact(N, k):
    S = np.array(J.case("dense_128")[0][:N, :N])
    info, info2 = {}, {}
    lam, V = la.eigen_sym(S, algo="jacobi", info=info)
    l2, v2 = la.eigen_sym(np.ldexp(S, k), algo="jacobi", info=info2)
    assert J.same_bits(l2, np.ldexp(lam, k)) and J.same_bits(v2, V) and info["sweeps"] == info2["sweeps"]


@pytest.mark.parametrize("vectors", [True, False])
def test_n_above_128_is_an_argument_error_and_nothing_is_written(vectors):
    torch, dev = _dev()
    S = torch.zeros((2, 129, 129), dtype=torch.float64, device="cuda")
    lam = torch.full((2, 129), 7.0, dtype=torch.float64, device="cuda")
    V = torch.full((2, 129, 129), 7.0, dtype=torch.float64, device="cuda")
    sw = torch.full((2,), 7, dtype=torch.int32, device="cuda")
    h = _lib.handle(0)
    p = lambda x: ctypes.c_void_p(x.data_ptr())
    rc = h.lib.nd4hip_dsyevj_batched_dev(h.ptr, 2, 129, p(S), p(lam), p(V) if vectors else None, p(sw))
    assert rc == -1 and b"N <= 128" in h.lib.nd4hip_last_error()
    torch.cuda.synchronize()
    assert bool((lam == 7.0).all()) and bool((V == 7.0).all()) and bool((sw == 7).all())
    with pytest.raises(_lib.Nd4HipError) as e:
        (la.eigen_sym if vectors else la.eigenvals_sym)(np.zeros((129, 129)), algo="jacobi")
    assert e.value.code == -1 and "N <= 128" in str(e.value)
    with pytest.raises(_lib.Nd4HipError):
        (dev.eigen_sym if vectors else dev.eigenvals_sym)(S, algo="jacobi")
    # empty input needs no launch
    assert la.eigen_sym(np.zeros((3, 0, 0)), algo="jacobi")[0].shape == (3, 0)
    assert la.eigenvals_sym(np.zeros((0, 4, 4)), algo="jacobi").shape == (0, 4)


@pytest.mark.parametrize("N", [3, 40, 100])
def test_nan_or_inf_in_the_lower_triangle_is_noconv_and_the_handle_stays_usable(N):
    S = np.array(J.case("dense_128")[0][:N, :N])
    before = la.eigen_sym(S, algo="jacobi")
    for bad in (np.nan, np.inf, -np.inf):
        X = S.copy()
        X[N - 1, N // 2] = bad
        for fn in (la.eigen_sym, la.eigenvals_sym):
            with pytest.raises(_lib.Nd4HipError) as e:
                fn(X, algo="jacobi")
            assert e.value.code == -3 and "eigen_sym(S): S contains NaN or Infinity in its lower triangle." in str(e.value)
        after = la.eigen_sym(S, algo="jacobi")
        assert J.same_bits(after[0], before[0]) and J.same_bits(after[1], before[1])
    # one bad member fails the call
    B = np.stack([S, S, S])
    B[1, 0, 0] = np.nan
    with pytest.raises(_lib.Nd4HipError):
        la.eigen_sym(B, algo="jacobi")
    assert J.same_bits(la.eigen_sym(S, algo="jacobi")[1], before[1])


@pytest.mark.parametrize("name", ["dense_33", "batch_5x40", "graded_60", "identity_8"])
def test_the_default_route_is_unchanged(name):
    torch, dev = _dev()
    S = C.reference(name)[0]
    lam, V = la.eigen_sym(S)
    for algo in (None, "dc"):
        info = {}
        l2, v2 = la.eigen_sym(S, algo=algo, info=info)
        assert J.same_bits(l2, lam) and J.same_bits(v2, V) and info == {}
        assert J.same_bits(la.eigenvals_sym(S, algo=algo), lam)
        t = torch.from_numpy(np.array(S)).cuda()
        ld, vd = dev.eigen_sym(t, algo=algo)
        assert J.same_bits(ld.cpu().numpy(), lam) and J.same_bits(vd.cpu().numpy(), V)
        assert J.same_bits(dev.eigenvals_sym(t, algo=algo).cpu().numpy(), lam)
    with pytest.raises(ValueError, match="algo must be None, 'dc' or 'jacobi'"):
        dev.eigen_sym(torch.from_numpy(np.array(S)).cuda(), algo="qr")


def test_profile_record():
    torch, dev = _dev()
    S = torch.from_numpy(np.array(J.case("batch_3x40")[0])).cuda()
    h = _lib.handle(0)
    h.profile_enable(True)
    try:
        dev.eigen_sym(S, algo="jacobi")
        rec = h.profile_last()[0]
        dev.eigenvals_sym(S, algo="jacobi")
        rec2 = h.profile_last()[0]
    finally:
        h.profile_enable(False)
    assert rec["op"] == "syevj" and rec["flops"] == pytest.approx(3 * 64.0 * 40.0 ** 3, rel=1e-12)
    assert rec2["op"] == "syevj" and rec2["flops"] == pytest.approx(3 * 32.0 * 40.0 ** 3, rel=1e-12)
    assert rec["valid"] and rec["kernel_ms"] > 0 and rec2["kernel_ms"] > 0
