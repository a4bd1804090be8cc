"""schur_eigenvals, schur_eigen, eigen_balance_pre and eigen_balance_post on the device against the reference's recorded results
(tests/golden/eigvec, tools/gen_golden_eigvec.js). Up to N = 64 (the small tier) the device runs the reference's own
back-substitution, one lane per column, and with Q = I the eigenvectors are compared bit for bit. N = 65 (the blocked tier's
smallest size: row blocks [0, 64), [64, 65)) and N = 131 = 2 nb + 3 run the blocked tier (nb = 64), with variants whose 2x2 block
sits on rows nb-1, nb, where the boundary moves by one row, and a restart whose row (10) and column (100) lie in different row
blocks. The blocked tier and every dense Q sum in another order than the reference, so they are held to the residual, elementwise
and column-norm criteria below; the restart fixtures stay in the elementwise check (restarted columns are cleared in the diagonal
kernel, nothing is recomputed sequentially)."""
import functools

import numpy as np
import pytest

import eigvec_common as ec
from nd4js_amd import la

pytestmark = pytest.mark.gpu
EPS = ec.EPS
SMALL_MAX = 64          # the small tier's largest N; the blocked tier (nb = 64) beyond


def bits(a):
    return np.ascontiguousarray(a).view(np.float64)


@functools.lru_cache(maxsize=None)
def device_eigen(name, dense):
    T = ec.load(name, "T")
    N = T.shape[-1]
    Q = ec.load(name, "Q") if dense else np.broadcast_to(np.eye(N), T.shape)
    return la.schur_eigen(Q, T)


@pytest.mark.parametrize("name", ec.SCHUR)
def test_schur_eigenvals_bit_identical(name):
    assert np.array_equal(bits(la.schur_eigenvals(ec.load(name, "T"))), bits(ec.load(name, "Lam")))


@pytest.mark.parametrize("name", ec.SCHUR)
def test_schur_eigen_identity_q_bit_identical(name):
    """small tier (N <= 64): Lam and V bit for bit. Blocked tier: Lam bit for bit, then the criteria (b) and (c) of the dense test
    with Q = I. Unit columns to 4 eps in both (no product with Q follows the normalisation)."""
    case = ec.CASES[name]
    N = case["N"]
    L, V = device_eigen(name, False)
    assert np.array_equal(bits(L), bits(ec.load(name, "Lam")))
    ref = ec.load(name, "VI")
    print(name, "max |V - V_ref| =", np.abs(V - ref).max())
    if N <= SMALL_MAX:
        assert np.array_equal(bits(V), bits(ref))
    else:
        T, I = ec.load(name, "T"), np.eye(N)
        for t, l, v, r in zip(ec.mats(T, N), L.reshape(-1, N), ec.mats(V, N), ec.mats(ref, N)):
            res, e_ref, err = ec.residual(I, t, l, v), ec.e_ref(t, I, r), float(np.abs(v - r).max())
            print(name, "Q=I residual", res, "reference", case["ref_residual_identity_q"], "| max|V - V_ref|", err, "e_ref", e_ref)
            assert res <= 4 * case["ref_residual_identity_q"] + N * EPS
            assert err <= 4 * e_ref + N * EPS
    assert max(ec.col_norm_error(v) for v in ec.mats(V, N)) <= 4 * EPS


@pytest.mark.parametrize("name", ec.SCHUR_DENSE)
def test_schur_eigen_dense_q(name):
    """(a) eigenvalues bit-identical; (b) residual within 4x the reference's recorded one + N eps; (c) elementwise within
    4 e_ref + N eps of the reference, e_ref the reference's own distance from the longdouble back-substitution (restart cases
    included). Unit columns: to 4 eps, or where the reference's own columns miss that after its product with Q (5.5 eps at N = 131,
    recorded per case as ref_colnorm_err), to 4 times the reference's own error."""
    case = ec.CASES[name]
    N = case["N"]
    L, V = device_eigen(name, True)
    assert np.array_equal(bits(L), bits(ec.load(name, "Lam")))
    T, Q, VQ = ec.load(name, "T"), ec.load(name, "Q"), ec.load(name, "VQ")
    for t, q, l, v, ref in zip(ec.mats(T, N), ec.mats(Q, N), L.reshape(-1, N), ec.mats(V, N), ec.mats(VQ, N)):
        res, e_ref, err = ec.residual(q, t, l, v), ec.e_ref(t, q, ref), float(np.abs(v - ref).max())
        print(name, "residual", res, "reference", case["ref_residual"], "| max|V - V_ref|", err, "e_ref", e_ref)
        assert res <= 4 * case["ref_residual"] + N * EPS
        assert err <= 4 * e_ref + N * EPS
        print(name, "column norm error", ec.col_norm_error(v), "reference", case["ref_colnorm_err"])
        assert ec.col_norm_error(v) <= max(4 * EPS, 4 * case["ref_colnorm_err"])


@pytest.mark.parametrize("name", ["batch_3x2x5", "batch_3x2x65"])
def test_batch_members_equal_their_single_results(name):
    T, Q = ec.load(name, "T"), ec.load(name, "Q")
    L, V = device_eigen(name, True)
    N = T.shape[-1]
    assert len({bits(t).tobytes() for t in ec.mats(T, N)}) == 6                      # members differ
    for idx in np.ndindex(T.shape[:-2]):
        l, v = la.schur_eigen(Q[idx], T[idx])
        assert np.array_equal(bits(l), bits(L[idx])) and np.array_equal(bits(v), bits(V[idx]))
        assert np.array_equal(bits(la.schur_eigenvals(T[idx])), bits(L[idx]))


def test_schur_throw_cases():
    T = ec.load("throw_real_block", "T")
    for f in (lambda: la.schur_eigenvals(T), lambda: la.schur_eigen(np.eye(3), T)):
        with pytest.raises(ValueError) as e:
            f()
        assert str(e.value) == ec.CASES["throw_real_block"]["eigenvals_error"] == ec.CASES["throw_real_block"]["eigen_error"]
    # one bad member fails the batch, as the reference's loop over the matrices does
    with pytest.raises(ValueError):
        la.schur_eigenvals(np.stack([ec.load("n3", "T"), T]))
    with pytest.raises(ValueError) as e:
        la.schur_eigen(np.eye(2), np.array([[1.0, np.nan], [0.0, 1.0]]))
    assert str(e.value) == "Assertion failed."


@pytest.mark.parametrize("name", ec.BAL)
def test_eigen_balance_pre(name):
    A, Dg, Bg = (ec.load(name, k) for k in ("A", "D", "B"))
    N, p = A.shape[-1], ec.p_of(name)
    D, B = la.eigen_balance_pre(A, p)
    assert np.array_equal(D, Dg)
    assert np.array_equal(bits(B), bits(Bg), equal_nan=True)
    assert np.all(np.frexp(D)[0] == 0.5)
    keep = ~np.isnan(A)
    assert np.array_equal((A * D[..., None, :] / D[..., :, None])[keep], B[keep])
    for b in ec.mats(B, N):
        assert ec.balance_sweep_changes(b, p) == []
    if name == "bal_balanced_7":
        assert np.all(D == 1.0)


@pytest.mark.parametrize("name", ["throw_bal_nan_entry_pinf", "throw_bal_inf_entry_p2"])
def test_eigen_balance_pre_nan(name):
    with pytest.raises(ValueError) as e:
        la.eigen_balance_pre(ec.load(name, "A"), ec.p_of(name))
    assert str(e.value) == ec.CASES[name]["error"] == "NaN encountered."


@pytest.mark.parametrize("name", ec.POST)
def test_eigen_balance_post(name):
    D, V, Wg = (ec.load(name, k) for k in ("D", "V", "W"))
    W = la.eigen_balance_post(D, V)
    err = float(np.abs(W - Wg).max())
    print(name, "max |W - W_ref| =", err)
    assert err <= 4 * EPS
    assert max(ec.col_norm_error(w) for w in ec.mats(W, W.shape[-1])) <= 4 * EPS


def test_device_array_forms_equal_the_host_forms():
    import torch
    from nd4js_amd import dev
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    T, Q = ec.load("n65", "T"), ec.load("n65", "Q")
    L, V = device_eigen("n65", True)
    assert np.array_equal(bits(dev.schur_eigenvals(cu(T)).cpu().numpy()), bits(L))
    l, v = dev.schur_eigen(cu(Q), cu(T))
    assert np.array_equal(bits(l.cpu().numpy()), bits(L)) and np.array_equal(bits(v.cpu().numpy()), bits(V))
    A = ec.load("bal_batch_2x3x7_p2", "A")
    d, b = dev.eigen_balance_pre(cu(A), 2)
    assert np.array_equal(d.cpu().numpy(), ec.load("bal_batch_2x3x7_p2", "D")) and np.array_equal(b.cpu().numpy(), ec.load("bal_batch_2x3x7_p2", "B"))
    D, Vp = ec.load("post_batch_2x3x7", "D"), ec.load("post_batch_2x3x7", "V")
    assert np.array_equal(bits(dev.eigen_balance_post(cu(D), cu(Vp)).cpu().numpy()), bits(la.eigen_balance_post(D, Vp)))
    with pytest.raises(ValueError, match="real eigenvalued 2x2 blocks"):
        dev.schur_eigenvals(cu(ec.load("throw_real_block", "T")))
