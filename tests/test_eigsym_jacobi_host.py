"""CPU checks of the Jacobi route of the symmetric eigenproblem, eigen_sym(S, algo='jacobi') (csrc/syevj.hip): the numpy model of
tests/eigsym_jacobi_common.py, which the device has to equal bit for bit (test_gpu_eigsym_jacobi.py), is itself held to
  - the bounds of tests/eigsym_common.py against LAPACK on the whole catalogue, in at most 20 sweeps (the cap is 60);
  - the relative bound |lambda^ - lambda| <= N eps kappa_2(A) lambda for EVERY eigenvalue of the four graded positive definite
    inputs, against 60-digit reference values (tests/golden/eigsym_jacobi); LAPACK's eigh misses that bound from cond 1e20 on, and
    so does the same iteration with an absolute rotation threshold: that is why the route and its relative rule exist;
and the host-side argument errors of the new keyword.
Measured on the model: at most 13 sweeps; 7.4e-4, 2.7e-3 and 2.3e-3 of the three bounds; at most 0.076 of the relative bound."""
import numpy as np
import pytest

import eigsym_common as C
import eigsym_jacobi_common as J
from nd4js_amd import la

PLAIN = tuple(n for n in J.names() if n not in J.GRADED)


def test_the_catalogue_covers_what_the_kernel_can_get_wrong():
    have = {n: J.case(n)[0].shape for n in J.names()}
    for name in C.NAMES:
        assert (name in have) == (C.CATALOGUE[name]().shape[-1] <= J.MAXN), name
    for N in (1, 2, 3, 4, 5, 31, 32, 33, 63, 64, 65, 127, 128):             # around every tier's edge, odd sizes (a bye) included
        assert have["dense_%d" % N] == (N, N)
    assert have["mixed_7x8"] == (7, 8, 8) and have["batch_3x40"] == (3, 40, 40)
    sw = J.case("mixed_7x8")[3]
    assert sw[0] == 1 and sw[1] == 1 and len(set(sw.tolist())) >= 3, "the mixed batch needs members with different sweep counts"


@pytest.mark.parametrize("name", PLAIN)
def test_model_meets_the_bounds_of_eigsym_common(name):
    S, lam, V, sweeps = J.case(name)
    lam_ref, V_ref = J.lapack(name)
    sh = C.check(S, lam, V, lam_ref, name)
    print("%s: sweeps %s, shares of the bounds (values, residual, orthogonality): %.3g %.3g %.3g" % ((name, sweeps.tolist()) + sh))
    C.check_vectors(S, V, lam_ref, V_ref, name)
    assert sweeps.min() >= 1 and sweeps.max() <= 20


def test_model_special_cases():
    # identity, zero and diagonal input: one sweep, nothing rotated, exact values; ties keep their order of position
    S, lam, V, sweeps = J.case("diag_ties_6")
    assert sweeps == 1 and lam.tolist() == [3.0, 3.0, 1.0, 1.0, 0.0, -2.0]
    assert np.array_equal(V, np.eye(6)[:, [0, 2, 1, 4, 5, 3]])
    S, lam, V, sweeps = J.case("mixed_7x8")
    assert np.array_equal(lam[0], np.ones(8)) and np.array_equal(V[0], np.eye(8))
    assert np.array_equal(lam[1], np.zeros(8)) and not np.signbit(lam[1]).any() and np.array_equal(V[1], np.eye(8))
    # theta = 0: t = 1, a rotation by 45 degrees, then a sweep that finds s_pq = 0 exactly
    S, lam, V, sweeps = J.case("eqdiag_2")
    assert sweeps == 2 and lam.tolist() == [1.5, 0.5] and np.allclose(np.abs(V), np.sqrt(0.5), rtol=0, atol=2e-16)
    # theta^2 overflows: t = 1 / (2 theta), finite results
    S, lam, V, sweeps = J.case("theta_overflow_2")
    assert sweeps == 2 and lam[0] == 1.0 and np.all(np.isfinite(V))
    # denormal off-diagonals beside a diagonal of order one are below the rule; a matrix that is denormal throughout is scaled
    # up exactly and solved like any other
    assert J.case("denormal_offdiag_4")[3] == 1
    S, lam, V, sweeps = J.case("denormal_all_5")
    l2, v2, s2, _ = J.model(S / 5e-324)
    assert J.same_bits(v2, V) and sweeps == s2 and np.array_equal(lam, l2 * 5e-324)


@pytest.mark.parametrize("k", [-500, -3, 1, 500])
def test_model_power_of_two_scaling_is_exact(k):
    S, lam, V, sweeps = J.case("batch_3x40")
    l2, v2, s2, _ = J.model(np.ldexp(S[0], k))
    assert J.same_bits(l2, np.ldexp(lam[0], k)) and J.same_bits(v2, V[0]) and s2 == sweeps[0]


@pytest.mark.parametrize("name", sorted(J.GRADED))
def test_model_relative_accuracy_on_graded_positive_definite_input(name):
    S, lam, V, sweeps = J.case(name)
    N = S.shape[-1]
    ref = J.graded_reference(name)
    assert ref.shape == (N,) and ref[-1] > 0 and np.all(np.diff(ref) < 0)
    bound = N * J.EPS * J.scaled_kappa(S)
    err = (np.abs(lam - ref) / ref).max()
    err_lapack = (np.abs(J.lapack(name)[0] - ref) / ref).max()
    err_abs = (np.abs(J.model(S, criterion="absolute", vectors=False)[0] - ref) / ref).max()
    print("%s: cond %.1e, bound %.3g; relative error: model %.3g (%.3g of the bound), eigh %.3g, absolute criterion %.3g; sweeps %d"
          % (name, ref[0] / ref[-1], bound, err, err / bound, err_lapack, err_abs, sweeps))
    assert err <= bound
    assert sweeps <= 20
    # the norm-wise bounds hold as well
    C.check(S, lam, V, J.lapack(name)[0], name)
    # why the route exists: a tridiagonalising solver has lost the small eigenvalues from cond 1e20 on, and an absolute rotation
    # threshold loses them whatever the condition
    if ref[0] / ref[-1] >= 1e20:
        assert err_lapack > bound
    assert err_abs > bound


def test_values_only_model_has_the_same_bits():
    for name in ("dense_33", "graded_pd_24", "mixed_7x8"):
        S, lam, V, sweeps = J.case(name)
        for b, s in enumerate(S.reshape(-1, S.shape[-1], S.shape[-1])):
            l2, _, s2, _ = J.model(s, vectors=False)
            assert J.same_bits(l2, lam.reshape(-1, S.shape[-1])[b]) and s2 == sweeps.reshape(-1)[b]


def test_host_side_argument_errors():
    for fn, name in ((la.eigen_sym, "eigen_sym"), (la.eigenvals_sym, "eigenvals_sym")):
        for algo in ("qr", "Jacobi", "", 0):
            with pytest.raises(ValueError, match=r"%s\(S, algo\): algo must be None, 'dc' or 'jacobi'\." % name):
                fn(np.eye(3), algo=algo)
        for algo in ("jacobi", "dc", None):
            with pytest.raises(ValueError, match="S.ndim must be at least 2"):
                fn(np.ones(3), algo=algo)
            with pytest.raises(ValueError, match="S must be quadratic"):
                fn(np.ones((2, 3)), algo=algo)
            with pytest.raises(TypeError, match="must be float"):
                fn(np.ones((2, 2), dtype=np.complex128), algo=algo)
