"""schur_decomp, eigen and eigenvals on the device (csrc/schur.hip) against the reference's recorded results (tests/golden/schur,
tools/gen_golden_schur.js).

The Francis step la.schur_qrfrancis(U, H) is compared with the reference's (Q, T) bit for bit, on every fixture and in both tiers
(a fixture that fits LDS also runs through the global tier by the `tier` argument). schur_decomp end to end starts from the
device's own Hessenberg reduction, which has not the reference's bits, so the iteration may take another path: T is held to the
exact structural conditions, and the residual, the orthogonality error and (eigen) the column residual and column-norm error to
four times the reference's own value of the same fixture (N 2^-52 in place of a zero), never above the gate of 1e-10: in the
reference's own cases neighbouring N differ by less than a factor of two, and another rotation path of the same length deserves
that much again."""
import functools

import numpy as np
import pytest
import torch

import schur_common as sc
from nd4js_amd import dev, la

pytestmark = pytest.mark.gpu
LDS_MAX = 65                                    # the LDS tier's largest N (csrc/schur.hip)


def tiers(name):
    return ["lds", "global"] if sc.CASES[name]["N"] <= LDS_MAX else ["global"]


FRANCIS = [(k, t) for k in sc.ALL for t in tiers(k)]


@pytest.mark.parametrize("name,tier", FRANCIS)
def test_francis_step_bit_for_bit(name, tier):
    """every fixture: recursion, nesting, exceptional shift, 2x2 cases, the batches (member by member; the NaN member equals the
    fixture where that is finite and is NaN where that is NaN, and its finite neighbours keep their bits)"""
    U, H = sc.hessenberg_pair(name)
    Q, T, sweeps = la.schur_qrfrancis(U, H, tier=tier, sweeps=True)
    assert sc.same_bits(T, sc.load(name, "T"))
    assert sc.same_bits(Q, sc.load(name, "Q"))
    assert sweeps == max(st.max_sweeps for st in sc.reference(name)[2])


def test_auto_tier_has_the_same_bits():
    for name in ("dense_33", "dense_64", "dense_65", "hess_48"):
        U, H = sc.hessenberg_pair(name)
        Q, T = la.schur_qrfrancis(U, H)
        assert sc.same_bits(T, sc.load(name, "T")) and sc.same_bits(Q, sc.load(name, "Q"))


@pytest.mark.parametrize("name", ["dense_5", "dense_47", "cyclic_64", "hess_48", "hess_160", "batch_3x2x16", "batch_nan_3x8"])
def test_francis_step_on_device_arrays(name):
    U, H = (torch.from_numpy(x).cuda() for x in sc.hessenberg_pair(name))
    Q, T = dev.schur_qrfrancis(U, H)
    assert sc.same_bits(T.cpu().numpy(), sc.load(name, "T")) and sc.same_bits(Q.cpu().numpy(), sc.load(name, "Q"))


def test_nan_member_is_isolated():
    U, H = sc.hessenberg_pair("batch_nan_3x8")
    Q, T = la.schur_qrfrancis(U, H)
    Tr = sc.load("batch_nan_3x8", "T")
    assert np.isfinite(T[0]).all() and np.isfinite(T[2]).all() and np.isnan(T[1]).any()
    assert np.array_equal(np.isnan(T), np.isnan(Tr))
    assert sc.same_bits(T, Tr) and sc.same_bits(Q, sc.load("batch_nan_3x8", "Q"))


def distance(lam, exact):
    """the largest distance of an eigenvalue from its partner in `exact`: both sorted, which for conjugate pairs (equal real
    parts up to rounding) is done by pairing each exact eigenvalue with the nearest one not yet taken"""
    left = list(lam)
    worst = 0.0
    for z in exact:
        j = int(np.argmin([abs(z - w) for w in left]))
        worst = max(worst, abs(z - left.pop(j)))
    return float(worst)


@functools.lru_cache(maxsize=None)
def device_schur(name):
    return la.schur_decomp(sc.input_matrix(name), sweeps=True)


@pytest.mark.parametrize("name", sc.FINITE)
def test_schur_decomp_end_to_end(name):
    case = sc.CASES[name]
    N = case["N"]
    A = sc.input_matrix(name)
    Q, T, _ = device_schur(name)
    assert np.all(np.tril(T, -2) == 0)                                           # zero below the first subdiagonal
    sub = np.diagonal(T, -1)
    assert not np.any((sub[:-1] != 0) & (sub[1:] != 0))                          # no two consecutive subdiagonal entries
    lam = la.schur_eigenvals(T)                                                   # raises on a real-eigenvalued 2x2 block
    res, orth = sc.schur_errors(A, Q, T)
    print(name, "residual", res, "reference", case["ref_residual"], "| orth", orth, "reference", case["ref_orth"])
    assert res <= sc.bound(case["ref_residual"], N)
    assert orth <= sc.bound(case["ref_orth"], N)
    if case["family"] in ("symmetric", "cyclic"):                                # perfectly conditioned eigenvalues
        exact = np.linalg.eigvals(A)
        ref_lam = la.schur_eigenvals(sc.load(name, "T"))
        d_ref, d_dev = distance(ref_lam, exact), distance(lam, exact)
        print(name, "eigenvalue distance", d_dev, "reference", d_ref)
        assert d_dev <= min(4.0 * (d_ref if d_ref > 0 else N * sc.EPS), sc.GATE)


@pytest.mark.parametrize("name", ["dense_8", "dense_47", "dense_96", "sym_64", "cyclic_8", "rotblocks_8", "batch_3x2x16"])
def test_eigenvals_has_the_bits_of_the_pipeline(name):
    """eigenvals(A) = schur_eigenvals(T) of the pipeline's own T: balance, then schur_decomp"""
    A = sc.input_matrix(name)
    _, B = la.eigen_balance_pre(A, 2)
    T = la.schur_decomp(B)[1]
    assert sc.same_bits(la.eigenvals(A).view(np.float64), la.schur_eigenvals(T).view(np.float64))
    At = torch.from_numpy(A).cuda()
    assert sc.same_bits(dev.eigenvals(At).cpu().numpy().view(np.float64), la.eigenvals(A).view(np.float64))


@pytest.mark.parametrize("name", sc.EIGEN)
def test_eigen(name):
    case = sc.CASES[name]
    N = case["N"]
    A = sc.input_matrix(name)
    lam, V = la.eigen(A)
    assert sc.same_bits(lam.view(np.float64), la.eigenvals(A).view(np.float64))
    res, cn = sc.eig_errors(A, lam, V)
    print(name, "column residual", res, "reference", case["ref_eig_residual"], "| column norm error", cn, "reference", case["ref_eig_colnorm_err"])
    assert res <= sc.bound(case["ref_eig_residual"], N)
    assert cn <= sc.bound(case["ref_eig_colnorm_err"], N)


def test_eigen_on_device_arrays_and_batches():
    A = sc.input_matrix("batch_3x2x16")
    lam, V = la.eigen(A)
    l2, V2 = dev.eigen(torch.from_numpy(A).cuda())
    assert sc.same_bits(l2.cpu().numpy().view(np.float64), lam.view(np.float64))
    assert sc.same_bits(V2.cpu().numpy().view(np.float64), V.view(np.float64))
    for a, l, v in zip(A.reshape(-1, 16, 16), lam.reshape(-1, 16), V.reshape(-1, 16, 16)):
        l1, v1 = la.eigen(a)
        assert sc.same_bits(l1.view(np.float64), l.view(np.float64)) and sc.same_bits(v1.view(np.float64), v.view(np.float64))
    Q, T = dev.schur_decomp(torch.from_numpy(A).cuda())
    Qh, Th = la.schur_decomp(A)
    assert sc.same_bits(Q.cpu().numpy(), Qh) and sc.same_bits(T.cpu().numpy(), Th)


@pytest.mark.parametrize("name", [k for k in sc.FINITE if sc.CASES[k]["family"] == "dense" and sc.CASES[k]["N"] >= 3])
def test_sweep_count_is_positive_and_within_the_budget(name):
    sweeps = device_schur(name)[2]
    assert 0 < sweeps <= sc.budget(sc.CASES[name]["N"])


def test_lds_tier_refuses_what_does_not_fit():
    U, H = sc.hessenberg_pair("dense_96")
    with pytest.raises(ValueError, match="nd4hip_dhseqr_batched: tier 1 is not available at N = 96"):
        la.schur_qrfrancis(U, H, tier="lds")
