"""CPU checks of what the GPU gate of test_gpu_trsm_paths.py rests on: the oracle's substitution is componentwise backward stable
on every family (so `16 * omega_oracle` is a tight bound, not a loose one), the one-launch ALGORITHM (explicitly inverted 8 x 8
diagonal sub-blocks coupled by substitution inside a 32-row block, a product for the other rows) stays within that factor in a
plain numpy model, and `omega` itself is right.

Measured at M = 256, J = 16 (omega of the oracle / ratio of the model's omega over it):
  well_lower 4.4e-16 / 0.39   well_upper 3.2e-16 / 0.54   qr_r_1e6 2.1e-16 / 0.69          qr_r_1e13 1.7e-16 / 1.01
  lu_u 2.7e-16 / 0.65         lu_l 1.4e-16 / 0.94         unit_dense_upper 1.4e-16 / 2.11  unit_dense_lower 1.2e-16 / 1.61
  row_graded 3.7e-16 / 0.37   col_graded 3.7e-16 / 0.42   kahan_1.2 1.5e-16 / 2.80
The cap (4 eps = 8.9e-16) holds on every family. Over seven right-hand sides kahan_1.2 stays at 2.6 to 3.3 (M = 1056, J = 32: 2.8
to 3.5). With the whole 32 x 32 block inverted explicitly, as the kernel did before, the same model gave 16.6 here and 5 to 240 over
those right-hand sides: the inverse of a 32 x 32 Kahan block has entries up to (1 + cos 1.2)^31 = 1.4e4, and X_b = inv B_b carries
eps |inv||B_b| where substitution carries eps |T||X|. With 16 x 16 sub-blocks it gave up to 18; an 8 x 8 inverse has entries below 10.
"""
import numpy as np
import pytest

import oracle
from nd4js_amd import rng
from trsm_common import FAMILIES, LD, effective, family, model_one_launch, omega, omega_cholesky, omega_ldl, subst

EPS = 2.0 ** -52
M, J = 256, 16


@pytest.fixture(scope="module")
def cases():
    out = {}
    for k, name in enumerate(FAMILIES):
        T, upper = family(name, 21000 + 10 * k, M)
        Y = rng.matrix(21500 + k, M, J)
        out[name] = (T, upper, Y, (oracle.triu_solve if upper else oracle.tril_solve)(T, Y))
    return out


@pytest.mark.parametrize("name", list(FAMILIES))
def test_oracle_backward_error_cap(cases, name):
    """the condition that keeps `omega_gpu <= 16 omega_oracle` meaningful: the reference's substitution reaches 4 eps on every family"""
    T, upper, Y, X = cases[name]
    w = omega(T, X, Y, upper)
    print(name, "omega_oracle %.3g" % w)
    assert w <= 4 * EPS


@pytest.mark.parametrize("name", list(FAMILIES))
def test_model_of_the_one_launch_algorithm_ratio(cases, name):
    """the gate's factor 16 is reachable by the algorithm itself: its numpy model is within 16 x the oracle on every family"""
    T, upper, Y, X = cases[name]
    wm, wo = omega(T, model_one_launch(T, Y, upper), Y, upper), omega(T, X, Y, upper)
    print(name, "omega_model %.3g ratio %.2f" % (wm, wm / wo))
    assert wm <= 16 * wo


def test_numpy_substitution_matches_the_oracle():
    """`subst` in fp64 is the reference's recurrence up to the order of the sums: same backward error class, results within
    cond x eps of each other; in np.longdouble it is the truth the extreme-scale cases are measured against"""
    for name in ("well_lower", "well_upper"):
        T, upper = family(name, 21900, 97)
        Y = rng.matrix(21901, 97, 5)
        ref = (oracle.triu_solve if upper else oracle.tril_solve)(T, Y)
        assert np.abs(subst(T, Y, upper) - ref).max() <= 64 * EPS * np.abs(ref).max()
        truth = subst(T.astype(LD), Y.astype(LD), upper)
        assert float(np.abs(ref - truth).max()) <= 64 * EPS * np.abs(ref).max()
        assert omega(T, truth.astype(np.float64), Y, upper) <= 2 * EPS      # the rounded truth: one rounding per entry


def test_omega_against_mpmath():
    """omega on a 40 x 40 case (an oracle solution with one entry pushed off by 1e-9) against the same quotient at 100 digits"""
    import mpmath
    n, j = 40, 3
    T, upper = family("lu_u", 21950, n)
    Y = rng.matrix(21951, n, j)
    X = oracle.triu_solve(T, Y)
    for bump in (0.0, 1e-9):
        Xb = X.copy()
        Xb[17, 1] *= 1.0 + bump
        with mpmath.workdps(100):
            Tm, Xm, Ym = (mpmath.matrix(a.tolist()) for a in (T, Xb, Y))
            R = Tm * Xm - Ym
            D = Tm.apply(abs) * Xm.apply(abs) + Ym.apply(abs)
            want = max(abs(R[i, k]) / D[i, k] for i in range(n) for k in range(j))
        got = omega(T, Xb, Y, upper)
        assert abs(got - float(want)) <= 1e-3 * float(want)        # the longdouble residual carries 11 bits beyond fp64
        assert (got > 1e-11) == (bump > 0)


def test_two_stage_omegas():
    """omega_cholesky / omega_ldl: small on the oracle's solves, above 1e-3 when one operand entry is dropped"""
    from families import spd, sym_indefinite
    n = 64
    Y = rng.matrix(21960, n, 4)
    L = np.linalg.cholesky(spd(21961, (n, n)))
    X = oracle.cholesky_solve(L, Y)
    assert omega_cholesky(L, X, Y) <= 8 * EPS
    L2 = L.copy()
    L2[40, 3] = 0.0
    assert omega_cholesky(L2, X, Y) > 1e-3
    LDm = oracle.ldl_decomp(sym_indefinite(21962, (n, n)))
    X = oracle.ldl_solve(LDm, Y)
    assert omega_ldl(LDm, X, Y) <= 8 * EPS
    Xd = X.copy()
    Xd[5] = 0.0
    assert omega_ldl(LDm, Xd, Y) > 1e-3


def test_effective_triangle():
    T = rng.matrix(21970, 5, 5)
    E = effective(T, True, unit=True)
    assert np.array_equal(np.tril(E, -1), np.zeros((5, 5))) and np.array_equal(np.diag(E), np.ones(5))
    assert np.array_equal(np.triu(E, 1), np.triu(T, 1))
