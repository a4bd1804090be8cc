"""CPU proofs behind test_gpu_rrqr_paths.py and the decided_prefix of test_gpu_rrqr.py (rrqr_common.py): the plain longdouble
reference of the pivot pass agrees with the reference project's fixtures wherever the input decides the step; every input of
the GPU file is decided at every step and takes the qp3_update tier it is there for; every synthetic triangle of the rank and
least-squares cases meets its margin."""
import numpy as np
import pytest

import rrqr_common as rc

CASES = rc.manifest()
DECOMP = sorted(k for k, v in CASES.items() if v["op"] == "rrqr_decomp" and not v.get("sampled"))
# the decided prefix of each rank-deficient fixture: its rank, except zerorow_48x48 (rank 47), whose step 47 has one candidate
# left and so one possible P; zerocol_40x60 and zerorow_60x40 lose nothing of their rank of 40
RANK_DEFICIENT = {"dupcols20x12": 6, "rankdef_48x48": 24, "rankdef_60x40": 20, "rankdef_40x60": 20, "zerocol_48x48": 47,
                  "zerocol_60x40": 39, "zerocol_40x60": 40, "zerorow_48x48": 48, "zerorow_60x40": 40, "zerorow_40x60": 39}
PIVOT = rc.pivot_cases()
RANK = rc.rank_cases()


def test_longdouble_is_wider_than_double():
    assert np.finfo(np.longdouble).eps <= 2.0 ** -63


@pytest.mark.parametrize("name", DECOMP)
def test_qrcp_ref_matches_the_fixtures_over_the_decided_prefix(name):
    meta = CASES[name]
    A = rc.make(meta["seed"], meta["shape"], meta["family"])
    A3 = A.reshape((-1,) + A.shape[-2:])
    gP = rc.load(meta, "P").reshape(-1, A.shape[-1])
    gR = rc.load(meta, "R")
    gR = gR.reshape((-1,) + gR.shape[-2:])
    grank = np.ravel(rc.load(meta, "rank"))
    K = min(A3.shape[-2:])
    for b in range(A3.shape[0]):
        P, margins, stopped_at = rc.qrcp_ref(A3[b])
        d = rc.decided_prefix(A3[b], P, margins)
        assert np.array_equal(P[:d], gP[b][:d]), (b, d)
        assert d >= rc.separated_prefix(gR[b], int(grank[b])), (b, d)      # never fewer steps than the rule it replaces
        if meta["family"] in ("dense", "identity"):
            assert d == K, (b, d)
        if name in RANK_DEFICIENT:
            assert d == RANK_DEFICIENT[name] and d >= int(grank[b]), (b, d)
        if meta["family"] == "zero":
            assert stopped_at == 0 and np.array_equal(P, np.arange(A.shape[-1]))


def test_ties_of_the_fixtures_are_compared():
    for name, steps in (("dupcols20x12", 6), ("identity16", 16)):
        meta = CASES[name]
        A = rc.make(meta["seed"], meta["shape"], meta["family"])
        P, margins, _ = rc.qrcp_ref(A)
        assert rc.decided_prefix(A, P, margins) == steps
        assert margins[0] == 0                                             # an exact tie at the first step


@pytest.mark.parametrize("name", sorted(PIVOT))
def test_every_gpu_case_is_decided_at_every_step_and_takes_its_tier(name):
    A, tiers = PIVOT[name]
    M, N = A.shape
    P, margins, stopped_at = rc.qrcp_ref(A)
    assert rc.decided_prefix(A, P, margins) == stopped_at
    assert np.all(np.sort(P) == np.arange(N))
    assert rc.tiers_taken(M, N, stopped_at) == tiers
    m = margins[:stopped_at]
    kind = name.split("-")[0]
    if kind in ("generic", "up1000", "down1000", "subnormal", "graded"):
        assert stopped_at == min(M, N) and np.all(m >= rc.DECIDED)
    if name == "planted-70x600":
        assert np.all(m[:5] == 0) and tuple(P[:5]) == rc.PLANT_WINNERS_600 and np.all(m[5:] >= 6.2e-5)
    elif kind == "planted":                                                # the late pair: the tie comes at step 38, under the lower tier (the earlier POSITION wins)
        assert stopped_at == 40 and m[38] == 0 and {P[38], P[39]} == {7, 29} and np.all(np.delete(m, 38) >= rc.DECIDED)
    if kind == "nan":
        assert stopped_at == N - 1 and P[-1] == 11 and np.all(m >= rc.DECIDED)
    if kind == "inf":
        want = np.arange(N)
        want[[0, 9]] = 9, 0
        assert stopped_at == 1 and np.array_equal(P, want)
    if kind == "stop3":
        q = np.arange(N)                                                   # three exchanges and nothing after them
        for i in range(3):
            j = int(np.flatnonzero(q == P[i])[0])
            q[[i, j]] = q[[j, i]]
        assert stopped_at == 3 and np.array_equal(P, q)
    if kind == "zero":
        assert stopped_at == 0 and np.array_equal(P, np.arange(N))


def test_margins_of_the_generic_inputs():
    """the figures of the table in test_gpu_rrqr_paths.py"""
    want = {(74, 40): 2.5e-4, (266, 40): 3.7e-5, (1036, 40): 6.8e-5, (2060, 40): 4.8e-7, (2049, 7): 1.1e-3, (64, 64): 1.4e-6,
            (65, 65): 2.5e-5, (70, 600): 1.2e-5, (40, 1100): 4.2e-5, (257, 259): 3.7e-5, (600, 130): 2.0e-6}
    for (M, N), least in want.items():
        m = float(rc.qrcp_ref(PIVOT["generic-%dx%d" % (M, N)][0])[1].min())
        assert 0.95 * least <= m <= 1.06 * least, (M, N, m)                # the table is rounded to two digits


def test_scaled_inputs_keep_the_permutation():
    P = rc.qrcp_ref(PIVOT["generic-74x40"][0])[0]
    for name in ("up1000-74x40", "down1000-74x40"):
        assert np.array_equal(rc.qrcp_ref(PIVOT[name][0])[0], P)
    A = PIVOT["subnormal-74x40"][0]
    assert np.abs(A)[A != 0].min() < 2.0 ** -1022                          # subnormal entries
    assert np.sqrt(np.sum(A.astype(np.longdouble) ** 2, axis=0)).max() < 5.6e-309   # 1 / norm overflows
    from nd4js_amd import rng
    Pu, mu, _ = rc.qrcp_ref(rng.matrix(8300, 74, 40))
    Ps, ms, _ = rc.qrcp_ref(A)
    assert np.array_equal(Ps, Pu) and ms.min() >= 2.7e-4
    G = PIVOT["graded-74x40"][0]
    e = np.frexp(np.abs(G).max(axis=0))[1]
    assert e.min() <= -598 and e.max() >= 399


def test_update_tier_boundaries():
    assert [rc.update_tier(n) for n in (1, 64, 65, 256, 257, 1024, 1025, 2048, 2049, 5000)] == [1, 1, 4, 4, 16, 16, 32, 32, 0, 0]


@pytest.mark.parametrize("name", sorted(RANK))
def test_rank_cases_meet_their_margin(name):
    build, want = RANK[name]
    R = build()
    M, N = R.shape
    L = min(M, N)
    r, tmp = rc.rank_ref(R)
    assert r == want
    if want < 0:
        return
    T = 2 * np.longdouble(rc.EPS) * max(M, N) * tmp[0]
    if r == 0:
        assert np.all(tmp == 0)
        return
    assert tmp[r - 1] >= 16 * T
    assert r == L or tmp[r] <= T / 16
    if name.startswith("jump"):                                            # T / 18: above the T / 23 that a halved rescaling shift needs
        assert T / 20 <= tmp[r] <= T / 16


def test_rank_ref_matches_the_fixture_ranks():
    for name in DECOMP:
        meta = CASES[name]
        gR = rc.load(meta, "R")
        for R, r in zip(gR.reshape((-1,) + gR.shape[-2:]), np.ravel(rc.load(meta, "rank"))):
            assert rc.rank_ref(R)[0] == r, name


def _ls_margin(R, r):
    got, tmp = rc.rank_ref(R)
    M, I = R.shape
    T = 2 * np.longdouble(rc.EPS) * max(M, I) * tmp[0]
    assert got == r and tmp[r - 1] >= 16 * T and (r == min(M, I) or tmp[r] <= T / 16)
    assert np.linalg.cond(R[:r, :r]) <= 1e3


@pytest.mark.parametrize("name", sorted(rc.LS_CASES))
def test_lstsq_cases_meet_their_margin(name):
    seed, N, M, I, J, r = rc.LS_CASES[name]
    Q, R, P, Y = rc.ls_factors(seed, N, M, I, J, r)
    _ls_margin(R, r)
    assert np.abs(Q.T @ Q - np.eye(M)).max() <= 1e-13 and np.array_equal(np.sort(P), np.arange(I))
    x = rc.lstsq_ref(Q, R, P, Y, r)
    # the formula is a least-squares solution of Q R[:, argsort P] with the rows at and below the rank cut off
    Rr = np.zeros_like(R)
    Rr[:r] = R[:r]
    Rr[:r, r:] = 0.0
    A = np.empty((N, I))
    A[:, P] = Q @ Rr
    xn = np.linalg.lstsq(A, Y, rcond=1e-12)[0]
    assert np.linalg.norm(x.astype(np.float64) - xn) <= 1e-10 * np.linalg.norm(xn)


def test_lstsq_batch_members_meet_their_margin():
    for seed, r in rc.LS_BATCH:
        _ls_margin(rc.ls_factors(seed, 80, 64, 70, 2, r)[1], r)
