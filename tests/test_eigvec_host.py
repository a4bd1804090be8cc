"""No GPU: the eigvec golden files are what the manifest says, the numpy restatements of tests/eigvec_common.py (the yardsticks
of the GPU tests) reproduce the reference, and the argument errors raised before any device call carry the reference's text."""
import os
import re

import numpy as np
import pytest

import eigvec_common as ec
from conftest import ROOT
from nd4js_amd import la


def test_golden_files_match_the_manifest():
    assert len(ec.CASES) >= 40
    for name, case in ec.CASES.items():
        for key, fn in case["files"].items():
            path = os.path.join(ec.DIR, fn)
            assert os.path.exists(path), fn
            assert os.path.getsize(path) <= ec.SIZE_LIMIT, fn
            a = np.load(path)
            assert list(a.shape) == case["shapes"][key], fn
            assert a.dtype == (np.complex128 if key in ("Lam", "VI", "VQ", "V", "W") else np.float64), fn


@pytest.mark.parametrize("name", ec.SCHUR)
def test_float64_restatement_is_the_reference_bit_for_bit(name):
    N = ec.CASES[name]["N"]
    T, L, VI = ec.load(name, "T"), ec.load(name, "Lam"), ec.load(name, "VI")
    for t, l, v in zip(ec.mats(T, N), L.reshape(-1, N), ec.mats(VI, N)):
        lam, X = ec.eigvecs_ref(t, exact=True)
        assert np.array_equal(lam.view(np.float64), l.view(np.float64))
        assert np.array_equal(X.view(np.float64), v.view(np.float64))


@pytest.mark.parametrize("name", ec.SCHUR_DENSE)
def test_longdouble_restatement_agrees_with_the_reference(name):
    """the dense-Q criteria of the GPU test, applied to the reference's own result: residual as recorded, and the reference
    near Q times the longdouble back-substitution. The second bound is only a sanity check on the helper (it would catch a wrong
    formula, not a lost digit): the first-order perturbation bound of an eigenvector, |dv| <= |dT| / gap, with the
    back-substitution's backward error |dT| <= N eps |T|_F. The GPU test compares the device with e_ref itself."""
    N = ec.CASES[name]["N"]
    T, Q, L, VQ = (ec.load(name, k) for k in ("T", "Q", "Lam", "VQ"))
    for t, q, l, v in zip(ec.mats(T, N), ec.mats(Q, N), L.reshape(-1, N), ec.mats(VQ, N)):
        assert ec.residual(q, t, l, v) <= 4 * ec.CASES[name]["ref_residual"] + N * ec.EPS
        if not ec.CASES[name].get("restart"):                      # a restart is a decision, not a rounding: longdouble may take the other branch
            assert ec.e_ref(t, q, v) <= N * ec.EPS / (ec.CASES[name]["min_gap_over_fro"] or 1.0)


@pytest.mark.parametrize("name", ec.BAL)
def test_balance_sweep_restatement_finds_the_golden_balanced(name):
    A, D, B = (ec.load(name, k) for k in ("A", "D", "B"))
    N, p = A.shape[-1], ec.p_of(name)
    for a, d, b in zip(ec.mats(A, N), D.reshape(-1, N), ec.mats(B, N)):
        assert ec.balance_sweep_changes(b, p) == []
        assert np.all(np.frexp(d)[0] == 0.5)                       # powers of two
        keep = ~np.isnan(a)
        assert np.array_equal((a * d[None, :] / d[:, None])[keep], b[keep])
    if name.startswith("bal_graded") and N > 2:
        assert ec.balance_sweep_changes(ec.mats(A, N)[0], p) != []  # ... and the restatement is not blind


def test_argument_errors_carry_the_reference_text():
    c = ec.CASES
    with pytest.raises(ValueError) as e:
        la.schur_eigenvals(np.ones((2, 3)))
    assert str(e.value) == c["throw_vals_nonsquare"]["error"] == "T is not square."
    with pytest.raises(ValueError) as e:
        la.schur_eigen(np.ones((2, 3)), np.ones((2, 3)))
    assert str(e.value) == c["throw_eigen_nonsquare"]["error"] == "Q is not square."
    with pytest.raises(ValueError) as e:
        la.schur_eigen(np.eye(2), np.eye(3))
    assert str(e.value) == c["throw_eigen_shape"]["error"] == "Q.shape != T.shape."
    with pytest.raises(ValueError) as e:
        la.schur_eigen(np.eye(2), np.eye(2)[None])
    assert str(e.value) == c["throw_eigen_ndim"]["error"] == "Q.ndim != T.ndim."
    for name, p in (("throw_bal_p_half", 0.5), ("throw_bal_p_nan", float("nan"))):
        with pytest.raises(ValueError) as e:
            la.eigen_balance_pre(ec.load(name, "A"), p)
        assert str(e.value) == c[name]["error"]
    with pytest.raises(ValueError) as e:
        la.eigen_balance_pre(np.ones((3, 4)))
    assert str(e.value) == c["throw_bal_nonsquare"]["error"] == "A is not square"
    with pytest.raises(ValueError) as e:
        la.eigen_balance_post(np.ones(3), np.ones(3))
    assert str(e.value) == c["throw_post_ndim"]["error"]
    with pytest.raises(ValueError) as e:
        la.eigen_balance_post(np.ones(2), np.ones((2, 3)))
    assert str(e.value) == c["throw_post_nonsquare"]["error"]
    with pytest.raises(TypeError):
        la.schur_eigenvals(np.eye(2, dtype=np.float32))


def test_header_declares_the_entry_points():
    src = open(os.path.join(ROOT, "include", "nd4hip.h")).read()
    for stem in ("dtreval", "dtrevc", "dgebal", "zgebak"):
        for form in ("", "_dev"):
            assert re.search(r"\bint nd4hip_%s_batched%s\s*\(" % (stem, form), src), stem + form
