"""Strong rank-revealing QR on the GPU (csrc/srrqr.hip through the C ABI): P and the rank against the reference's fixtures,
the factorisation's properties, the Gu-Eisenstat bound from the device's own R, and the options."""
import numpy as np
import pytest

from nd4js_amd import la
from srrqr_common import EPS, input_of, load, manifest, strong_F, y_of

pytestmark = pytest.mark.gpu

CASES = {k: v for k, v in manifest().items() if v["op"] == "srrqr_decomp_full" and not v.get("sampled")}


def _members(A, Q, R, P):
    return [x.reshape((-1,) + x.shape[-2:]) for x in (A, Q, R)] + [P.reshape(-1, P.shape[-1])]


@pytest.mark.parametrize("name", sorted(CASES))
def test_srrqr_matches_reference(name):
    meta = CASES[name]
    A = input_of(meta)
    Q, R, P, r = la.srrqr_decomp_full(A, meta["opt"])
    np.testing.assert_array_equal(r, load(meta, "r"))
    if meta["family"] == "dupcols":                                       # columns 2j and 2j+1 are equal: either may come first
        np.testing.assert_array_equal(P // 2, load(meta, "P") // 2)
    else:
        np.testing.assert_array_equal(P, load(meta, "P"))
    M, N = A.shape[-2:]
    opt = meta["opt"] or {}
    dtol = opt.get("dtol", 1.01)
    for b, (a, q, rr, p, rk) in enumerate(zip(*_members(A, Q, R, P), np.ravel(r))):
        nA = np.linalg.norm(a)
        assert np.abs(q.T @ q - np.eye(M)).max() <= 1e-13
        assert np.abs(q @ rr - a[:, p]).max() <= 1e-13 * max(nA, 1)
        assert np.all(np.tril(rr, -1) == 0)                                # R[:r] upper trapezoidal (all of R here)
        ztol = opt.get("ztol", np.sqrt(EPS) * max(M, N)) * (nA if nA > 0 else 1)
        assert np.linalg.norm(rr[rk:, rk:]) <= ztol * (1 + 1e-8)
        assert strong_F(rr, rk) <= dtol * (1 + 1e-10)
    if "Q" in meta["files"]:
        for q, rr, qg, rg, rk in zip(*(x.reshape((-1,) + x.shape[-2:]) for x in (Q, R, load(meta, "Q"), load(meta, "R"))), np.ravel(r)):
            if rk == 0:
                continue
            s = np.where(np.diag(rr)[:rk] * np.diag(rg)[:rk] < 0, -1.0, 1.0)   # each row of R (column of Q) up to its sign
            scale = max(np.abs(rg).max(), 1e-300)
            assert np.abs(s[:, None] * rr[:rk] - rg[:rk]).max() <= 1e-12 * scale
            assert np.abs(q[:, :rk] * s[None, :] - qg[:, :rk]).max() <= 1e-12


@pytest.mark.parametrize("name", ["kahan60", "kahan90"])
def test_kahan_strong_rank(name):
    meta = CASES[name]
    A = input_of(meta)
    _, R, _, r = la.srrqr_decomp_full(A)
    sv = np.linalg.svd(A, compute_uv=False)
    svd_rank = int(la.svd_rank(sv))
    assert int(r) == svd_rank == A.shape[0] - 1
    _, Rw, _ = la.rrqr_decomp(A)
    assert int(la.rrqr_rank(Rw)) == A.shape[0]                           # column pivoting alone misses it


def test_large1024_decisions():
    meta = manifest()["large1024"]
    A = input_of(meta)
    Q, R, P, r = la.srrqr_decomp_full(A)
    assert int(r) == int(load(meta, "r"))
    np.testing.assert_array_equal(P, load(meta, "P"))
    rk = int(r)
    dg = np.abs(np.diag(R))[:rk]
    np.testing.assert_allclose(dg, np.abs(load(meta, "Rdiag"))[:rk], rtol=1e-9, atol=1e-12 * np.abs(dg).max())
    assert strong_F(R, rk) <= 1.01 * (1 + 1e-10)
    idx, val = load(meta, "R_idx"), load(meta, "R_val")                  # sampled entries of rows < r, up to each row's sign
    row, col = idx // 1024, idx % 1024
    keep = row < rk
    sg = np.sign(np.diag(R))[row[keep]] * np.sign(load(meta, "Rdiag"))[row[keep]]
    np.testing.assert_allclose(sg * R[row[keep], col[keep]], val[keep], rtol=0, atol=1e-10 * np.abs(load(meta, "Rdiag")).max())


def test_second_call_bit_identical_and_batch_equals_members():
    meta = CASES["batch5x24"]
    A = input_of(meta)
    out1 = la.srrqr_decomp_full(A)
    out2 = la.srrqr_decomp_full(A)
    for x, y in zip(out1, out2):
        np.testing.assert_array_equal(x, y)
    for b in range(A.shape[0]):
        one = la.srrqr_decomp_full(A[b])
        for x, y in zip(out1, one):
            np.testing.assert_array_equal(x[b], y)


def test_options_honoured():
    _, _, _, r = la.srrqr_decomp_full(np.eye(3), {"ztol": 2})
    assert int(r) == 0
    _, _, _, r = la.srrqr_decomp_full(np.eye(3), ztol=0.5)
    assert int(r) == 3
    for name in ("dtol15_40x60", "dtol15_rankdef_60x40"):                # r < N: the bound is checked for real
        meta = CASES[name]
        A = input_of(meta)
        _, R, P15, r15 = la.srrqr_decomp_full(A, dtol=1.5)
        _, R101, _, r101 = la.srrqr_decomp_full(A)
        assert int(r15) < A.shape[1]
        F15 = strong_F(R, int(r15))
        assert F15 <= 1.5 * (1 + 1e-10)
        if name == "dtol15_40x60":
            assert F15 > 1.01                                              # a swap the default dtol would have made was skipped
        assert strong_F(R101, int(r101)) <= 1.01 * (1 + 1e-10)
        np.testing.assert_array_equal(P15, load(meta, "P"))
    with pytest.raises(ValueError, match="Must be >=1"):
        la.srrqr_decomp_full(A, dtol=0.99)


def test_empty_and_zero():
    Q, R, P, r = la.srrqr_decomp_full(np.zeros((0, 4)))
    assert Q.shape == (0, 0) and R.shape == (0, 4) and list(P) == [0, 1, 2, 3] and int(r) == 0
    Q, R, P, r = la.srrqr_decomp_full(np.zeros((5, 3)))
    assert int(r) == 0 and list(P) == [0, 1, 2]
    np.testing.assert_allclose(Q @ R, 0.0)


@pytest.mark.parametrize("name", ["ls_rankdef_48", "ls_lowrank_300x200"])
def test_rrqr_lstsq_of_srrqr(name):
    meta = manifest()[name]
    A = input_of(meta)
    y = y_of(meta)
    x = la.rrqr_lstsq(la.srrqr_decomp_full(A), y)
    xg = load(meta, "x")
    np.testing.assert_allclose(x, xg, rtol=0, atol=1e-10 * np.abs(xg).max())


def test_rrqr_rank_of_srrqr_R():
    for name in ("kahan90", "rankdef_48x48", "lowrank40_256"):
        meta = CASES[name]
        _, R, _, _ = la.srrqr_decomp_full(input_of(meta))
        assert list(np.ravel(la.rrqr_rank(R))) == meta["rrqr_rank_of_srrqr_R"]


def test_dev_form_matches_host_form():
    torch = pytest.importorskip("torch")
    from nd4js_amd import dev
    meta = CASES["batch5x24"]
    A = input_of(meta)
    Qh, Rh, Ph, rh = la.srrqr_decomp_full(A)
    Q, R, P, r = dev.srrqr_decomp_full(torch.from_numpy(A).cuda())
    torch.cuda.synchronize()
    np.testing.assert_array_equal(P.cpu().numpy(), Ph)
    np.testing.assert_array_equal(r.cpu().numpy(), rh)
    np.testing.assert_array_equal(R.cpu().numpy(), Rh)
    np.testing.assert_array_equal(Q.cpu().numpy(), Qh)
