"""Column-pivoted QR on the MI355X against the reference's own outputs (tests/golden/rrqr/, tools/gen_golden_rrqr.js) and,
beyond the fixtures, against scipy's pivoted QR and the factorisation's own properties. Everything through the C ABI."""
import numpy as np
import pytest

from nd4js_amd import la
from rrqr_common import EPS, check_properties, decided_prefix, load, make, manifest, permuted, qrcp_ref, separated_prefix, y_of

pytestmark = pytest.mark.gpu
CASES = manifest()
DECOMP = sorted(k for k, v in CASES.items() if v["op"] == "rrqr_decomp" and not v.get("sampled"))


@pytest.mark.parametrize("name", DECOMP)
def test_rrqr_decomp_matches_reference(name):
    meta = CASES[name]
    A = make(meta["seed"], meta["shape"], meta["family"])
    Q, R, P = la.rrqr_decomp(A)
    gQ, gR, gP, grank = load(meta, "Q"), load(meta, "R"), load(meta, "P"), load(meta, "rank")
    check_properties(A, Q, R, P)
    rank = la.rrqr_rank(R)
    assert np.array_equal(rank, grank)
    A3, Q3, R3, gQ3, gR3 = (x.reshape((-1,) + x.shape[-2:]) for x in (A, Q, R, gQ, gR))
    P3, gP3 = P.reshape(-1, P.shape[-1]), gP.reshape(-1, gP.shape[-1])
    for b in range(A3.shape[0]):
        rP, margins, _ = qrcp_ref(A3[b])
        s = decided_prefix(A3[b], rP, margins)                    # every step that the input decides, exact ties included
        if meta["family"] == "dense":
            assert s == min(A3.shape[-2:]), (b, s)                # every member of a dense fixture is decided throughout
        assert np.array_equal(P3[b][:s], gP3[b][:s]) and np.array_equal(P3[b][:s], rP[:s]), (b, s)
        if separated_prefix(gR3[b], int(np.ravel(grank)[b])) == min(A3.shape[-2:]):
            # Compared exactly (no sign freedom) except in two documented limits of the existing QR that Q and R come from
            # (include/nd4hip.h): for tall input its c >= 0 sign rule is read off the leading minors of Q's top
            # block, which vanish for a permuted diagonal / zero-row matrix (diag_60x40, zerorow_60x40); and it forced
            # R_jj >= 0 on a column of the permuted square diagonal matrix whose sub-column is exactly zero, where the
            # reference keeps the entry's sign (then det Q = +1 flips the last column: diag_48x48). There the signs are
            # taken from the golden. A triangular input's trailing |R_ii| fall to ~1e-17 ||A||, where a column of Q is
            # determined only to eps ||A|| / |R_ii|: the well-determined columns, |R_ii| >= 1e-6 max |R_ii|, are compared.
            D = np.ones(Q3.shape[-1])
            keep = np.ones(Q3.shape[-1], dtype=bool)
            if meta["family"] in ("diag", "zerorow"):
                D = np.where(np.sign(np.diag(R3[b])) == np.sign(np.diag(gR3[b])), 1.0, -1.0)
            if meta["family"] == "triu":
                gd = np.abs(np.diag(gR3[b]))
                keep = gd >= 1e-6 * gd.max()
            assert np.linalg.norm((Q3[b] * D - gQ3[b])[:, keep]) <= 1e-12 * np.sqrt(Q3.shape[-1])
            assert np.linalg.norm((D[:, None] * R3[b] - gR3[b])[keep]) <= 1e-12 * np.linalg.norm(gR3[b])
    if meta["family"] == "zero":
        assert np.array_equal(P, np.arange(A.shape[-1]))
    # a second call gives the same bits
    Q2, R2, P2 = la.rrqr_decomp(A)
    assert np.array_equal(P2, P) and np.array_equal(Q2, Q) and np.array_equal(R2, R)


@pytest.mark.parametrize("name", sorted(k for k, v in CASES.items() if "Qf" in v["files"]))
def test_rrqr_decomp_full_matches_reference(name):
    meta = CASES[name]
    A = make(meta["seed"], meta["shape"], meta["family"])
    Q, R, P = la.rrqr_decomp_full(A)
    M, N = A.shape
    assert Q.shape == (M, M) and R.shape == (M, N)
    assert np.array_equal(P, load(meta, "Pf"))
    assert np.linalg.norm(Q[:, :N] - load(meta, "Qf")[:, :N]) <= 1e-12 * np.sqrt(N)
    assert np.linalg.norm(R - load(meta, "Rf")) <= 1e-12 * np.linalg.norm(R)
    assert np.abs(Q @ Q.T - np.eye(M)).max() <= 1e-13
    assert np.linalg.norm(permuted(A, P) - Q @ R) <= 1e-13 * np.linalg.norm(A)


@pytest.mark.parametrize("name", ["large1024", "large2048"])
def test_rrqr_large_identical_pivots(name):
    meta = CASES[name]
    N = meta["shape"][0]
    A = make(meta["seed"], meta["shape"], "dense")
    Q, R, P = la.rrqr_decomp(A)
    assert np.array_equal(P, load(meta, "P"))                     # s = K on dense inputs: P identical throughout
    assert np.abs(np.diag(R) - load(meta, "Rdiag")).max() <= 1e-12 * np.abs(load(meta, "Rdiag")).max()
    assert np.abs(Q.reshape(-1)[load(meta, "Q_idx")] - load(meta, "Q_val")).max() <= 1e-12
    assert np.abs(R.reshape(-1)[load(meta, "R_idx")] - load(meta, "R_val")).max() <= 1e-12 * np.abs(load(meta, "Rdiag")).max()
    assert abs(np.linalg.norm(R) - meta["fro_R"]) <= 1e-12 * meta["fro_R"]
    assert np.array_equal(la.rrqr_rank(R), load(meta, "rank"))
    check_properties(A, Q, R, P)
    assert np.linalg.norm(Q.T @ Q - np.eye(N)) <= 1e-13 * N


@pytest.mark.parametrize("name", sorted(k for k, v in CASES.items() if v["op"] in ("rrqr_lstsq", "solve")))
def test_lstsq_and_solve_match_reference(name):
    meta = CASES[name]
    A = make(meta["seed"], meta["shape"], meta["family"])
    y = y_of(meta)
    gx = load(meta, "x")
    if meta["op"] == "rrqr_lstsq":
        x = la.rrqr_lstsq(la.rrqr_decomp(A), y)
        x4 = la.rrqr_lstsq(*la.rrqr_decomp(A), y)
        assert np.array_equal(x, x4)
    elif meta["singular"]:
        with pytest.raises(la.SingularMatrixSolveError) as e:
            la.solve(A, y)
        x = e.value.x
    else:
        x = la.solve(A, y)
        Q, R, P = la.rrqr_decomp(A)
        assert np.array_equal(la.rrqr_solve(Q, R, P, y), x)
    assert np.linalg.norm(x - gx) <= 1e-10 * max(np.linalg.norm(gx), 1.0)


def test_solve_rejects_non_square():
    Q, R, P = la.rrqr_decomp(make(5, (6, 4), "dense"))
    with pytest.raises(ValueError, match=r"^rrqr_solve\(Q,R,P, y\): Q @ R not square\.$"):
        la.rrqr_solve(Q, R, P, np.ones((6, 1)))
    with pytest.raises(ValueError, match=r"not square"):
        la.solve(make(5, (6, 4), "dense"), np.ones((6, 1)))


def test_lstsq_broadcasts_over_q_r_p_y():
    A = make(31, (3, 20, 12), "dense")
    Q, R, P = la.rrqr_decomp(A)
    y = make(32, (2, 1, 20, 3), "dense")
    x = la.rrqr_lstsq(Q, R, P, y)
    assert x.shape == (2, 3, 12, 3)
    for i in range(2):
        for b in range(3):
            want = np.linalg.lstsq(A[b], y[i, 0], rcond=None)[0]
            assert np.linalg.norm(x[i, b] - want) <= 1e-10 * np.linalg.norm(want)
    # one factorisation broadcast against a batch of right-hand sides
    x1 = la.rrqr_lstsq(Q[0], R[0], P[0], y[:, 0])
    assert np.array_equal(x1, x[:, 0])


def test_lstsq_rejects_invalid_permutation():
    Q, R, P = la.rrqr_decomp(make(7, (8, 8), "dense"))
    P = P.copy()
    P[0] = P[1]
    with pytest.raises(ValueError, match=r"Invalid indices in P"):
        la.rrqr_lstsq(Q, R, P, np.ones((8, 1)))


def test_nan_input_returns_and_rank_raises():
    A = make(9, (16, 16), "dense")
    A[3, 5] = np.nan
    Q, R, P = la.rrqr_decomp(A)
    with pytest.raises(ValueError, match=r"^Infinity or NaN encountered during rank estimation\.$"):
        la.rrqr_rank(R)
    with pytest.raises(ValueError, match=r"Infinity or NaN encountered during rank estimation\."):
        la.rrqr_lstsq(Q, R, P, np.ones((16, 1)))
    A[...] = np.inf
    la.rrqr_decomp_full(A)                                        # returns; the values are unspecified


def test_dev_forms_match_host_bits():
    import torch
    from nd4js_amd import dev
    for shape in ((48, 48), (60, 40), (40, 60), (5, 24, 24)):
        A = make(41, shape, "dense")
        t = torch.from_numpy(A).cuda()
        for host, devf in ((la.rrqr_decomp, dev.rrqr_decomp), (la.rrqr_decomp_full, dev.rrqr_decomp_full)):
            hQ, hR, hP = host(A)
            dQ, dR, dP = devf(t)
            torch.cuda.synchronize()
            assert np.array_equal(dQ.cpu().numpy(), hQ) and np.array_equal(dR.cpu().numpy(), hR) and np.array_equal(dP.cpu().numpy(), hP)
        hQ, hR, hP = la.rrqr_decomp(A)
        dQ, dR, dP = dev.rrqr_decomp(t)
        assert np.array_equal(dev.rrqr_rank(dR).cpu().numpy(), la.rrqr_rank(hR))
        y = make(42, shape[:-1] + (2,), "dense")
        rank = torch.empty(shape[:-2], dtype=torch.int32, device="cuda")
        dx = dev.rrqr_lstsq(dQ, dR, dP, torch.from_numpy(y).cuda(), rank=rank)
        assert np.array_equal(dx.cpu().numpy(), la.rrqr_lstsq(hQ, hR, hP, y))
        assert np.array_equal(rank.cpu().numpy(), la.rrqr_rank(hR))


def _scipy_prefix_check(A, P):
    import scipy.linalg
    _, Rs, Ps = scipy.linalg.qr(A, mode="economic", pivoting=True)
    rank = int(np.sum(np.abs(np.diag(Rs)) > 2 * EPS * max(A.shape) * np.linalg.norm(np.triu(Rs))))
    s = separated_prefix(Rs, rank)
    assert np.array_equal(P[:s], Ps[:s].astype(np.int32)), s


@pytest.mark.parametrize("shape", [(3000, 500), (500, 3000), (4096, 4096)])
def test_beyond_fixtures_against_scipy(shape):
    A = make(51, shape, "dense")
    Q, R, P = la.rrqr_decomp(A)
    check_properties(A, Q, R, P)
    _scipy_prefix_check(A, P)


def test_batch_256_of_64():
    A = make(52, (256, 64, 64), "rankdef")
    Q, R, P = la.rrqr_decomp(A)
    check_properties(A, Q, R, P)
    assert np.all(la.rrqr_rank(R) == 32)
    for b in (0, 17, 255):
        _scipy_prefix_check(A[b], P[b])
