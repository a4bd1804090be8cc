"""Every loop of srrqr.hip that takes a second pass only beyond 1024 rows, columns or rank, and the batch, scale and URV paths,
through the device forms (dev.srrqr_decomp_full, dev.urv_decomp_full, dev.urv_lstsq). P and r are decisions: they are
compared with the reference's own, from fixtures that hold P and r only (tools/gen_golden_srrqr.js: the five inputs beyond
1024 and the two finite 60^2 members of the batch; the Kahan member is the existing kahan60 fixture).

Case -> path -> condition in the source (srrqr.hip: srrqr_decide runs one workgroup of NT = 1024 threads per matrix)

  dense 1100^2             rank 1099: the loops over k and k0 (ab_update, ab_downdate, ab_copy, retri,      k, k0 > 1024
                           swap_elim's exchange, the cycle of inv(A0)'s columns) and over N and M
                           (cm / P init, ab_cycle, retri's row update, block_norm) take a second pass
  low-rank 300 of 1100^2   N, M > 1024 with k <= 300: ztol ends the search; srrqr_gather's row loop          M > 1024 = gridDim.y
  dense 40x1100            N > 1024 with k <= 40: ab_cycle's `j += NT` pass, col_norms over 1100 columns    N - p > 1024
  low-rank 20 of 40x1100   the same with K found by ztol
  dense 1100x40            M > 1024: swap_elim's reflector over 1100 rows, srrqr_gather's row loop
  batch of six 60^2        generic, one NaN entry, low-rank 20, one Inf entry, zero, Kahan: ranks             the return before the first
                           [60, -3, 20, -1, 0, 59]; every finite member bit-equal to its own call             barrier for NaN / Inf
  A 2^+-500                P and r of the scaled input equal those of A: W / ||A||_F has the same bits       block_norm's scaled form
  URV 40x1100 low-rank 20  urv_pack's row loop over the 1100 rows of X' and urv_unpack's over the 1100 rows of V   N > 1024
  URV 1100x40 low-rank 20  urv_unpack's row loop over the 1100 rows of R: r = 20 < N, so R is rewritten and          M > 1024, r < N
                           rows 1024..1099 must come out exactly zero
  URV 1100x40 dense | 48^2 r = N: R is left as srrqr wrote it (no R loop) and V is the exact permutation           r == N
  URV zero 20x12           r = 0: R = 0, V = I
  urv_lstsq order 1100     urv_mask's row loop, rank 1060                                                    Lr > 1024

Gates: P and r equal to the fixture's; strong_F(R, r) <= dtol (1 + 1e-10) from the device's own R; the residual, orthogonality
and ||R[r:, r:]|| <= ztol gates of test_gpu_srrqr.py; for URV those of test_gpu_urv.py. urv_lstsq: err_dev <= G max(err_f64,
eps ||x||) against the longdouble formula, G and the measured ratio as in test_gpu_rrqr_paths.py.

Measured on the MI355X: the 15 cases of this file take 4 s, the two 1100^2 about 1 s each.

Mutation of srrqr.hip tried once against this file, stopped at its first failure, not committed:
  ab_cycle without its `j += NT` pass (columns from p + 1024 on not cycled)   first caught by test_beyond_1024_matches_the_reference_decisions[dense_1100x1100]
                                                                              (P differs at 971 of 1100 positions)
"""
import functools

import numpy as np
import pytest

from srrqr_common import EPS, input_of, kahan, load, lowrank, manifest, strong_F, urvls_factors, urvls_ref
from rrqr_common import LSTSQ_G as G

pytestmark = pytest.mark.gpu
CASES = manifest()
LARGE = ("dense_1100x1100", "lowrank300_1100", "dense_40x1100", "dense_1100x40", "lowrank20_40x1100")


def _dev():
    import torch
    from nd4js_amd import dev
    return torch, dev


def _run(fn, *args):
    torch, dev = _dev()
    out = getattr(dev, fn)(*(torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in args))
    torch.cuda.synchronize()
    return tuple(x.cpu().numpy() for x in out) if isinstance(out, tuple) else out.cpu().numpy()


def _bits(x):
    return np.ascontiguousarray(x).view(np.int64 if x.dtype == np.float64 else x.dtype)


def check_factors(a, q, rr, p, rk, dtol=1.01):
    """the gates of test_gpu_srrqr.test_srrqr_matches_reference on one matrix"""
    M, N = a.shape
    nA = np.linalg.norm(a)
    assert np.abs(q.T @ q - np.eye(M)).max() <= 1e-13
    assert np.abs(q @ rr - a[:, p]).max() <= 1e-13 * max(nA, 1)
    assert np.all(np.tril(rr, -1) == 0)
    ztol = np.sqrt(EPS) * max(M, N) * (nA if nA > 0 else 1)
    assert np.linalg.norm(rr[rk:, rk:]) <= ztol * (1 + 1e-8)
    assert strong_F(rr, rk) <= dtol * (1 + 1e-10)


@pytest.mark.parametrize("name", LARGE)
def test_beyond_1024_matches_the_reference_decisions(name):
    meta = CASES[name]
    A = input_of(meta)
    Q, R, P, r = _run("srrqr_decomp_full", A)
    assert int(r) == int(load(meta, "r"))
    np.testing.assert_array_equal(P, load(meta, "P"))
    check_factors(A, Q, R, P, int(r))


@functools.lru_cache(maxsize=None)
def _batch_members():
    from nd4js_amd import rng
    g = rng.matrix(8900, 60, 60)
    nan, inf = g.copy(), g.copy()
    nan[17, 33] = np.nan
    inf[41, 2] = np.inf
    return g, nan, lowrank(8901, 60, 60, 20), inf, np.zeros((60, 60)), kahan(60, 1.2)


def test_batch_members_decide_alone():
    members = _batch_members()
    Q, R, P, r = _run("srrqr_decomp_full", np.stack(members))
    assert list(r) == [60, -3, 20, -1, 0, 59]
    for b, name in ((0, "b6_dense_60"), (2, "b6_lowrank20_60"), (5, "kahan60")):
        assert int(r[b]) == int(load(CASES[name], "r"))
        np.testing.assert_array_equal(P[b], load(CASES[name], "P"))
    assert list(P[4]) == list(range(60))
    for b in (0, 2, 4, 5):
        one = _run("srrqr_decomp_full", members[b])
        for x, y in zip((Q[b], R[b], P[b], r[b]), one):
            assert np.array_equal(_bits(np.asarray(x)), _bits(np.asarray(y))), b
        check_factors(members[b], Q[b], R[b], P[b], int(r[b]))


@pytest.mark.parametrize("name", ["dense_60x40", "rankdef_48x48", "lowrank40_256"])
def test_power_of_two_scale_keeps_the_decisions(name):
    meta = CASES[name]
    A = input_of(meta)
    for k in (0, 500, -500):
        _, _, P, r = _run("srrqr_decomp_full", np.ldexp(A, k))
        assert int(r) == int(load(meta, "r")), k
        np.testing.assert_array_equal(P, load(meta, "P"))


def _urv_inputs():
    from nd4js_amd import rng
    return {"lowrank20_40x1100": input_of(CASES["lowrank20_40x1100"]), "dense_1100x40": input_of(CASES["dense_1100x40"]),
            "lowrank20_1100x40": lowrank(8930, 1100, 40, 20),
            "dense_48x48": rng.matrix(8910, 48, 48), "zero_20x12": np.zeros((20, 12))}


@pytest.mark.parametrize("name", ["lowrank20_40x1100", "lowrank20_1100x40", "dense_1100x40", "dense_48x48", "zero_20x12"])
def test_urv(name):
    A = _urv_inputs()[name]
    M, N = A.shape
    U, R, V, r = _run("urv_decomp_full", A)
    _, _, P, rs = _run("srrqr_decomp_full", A)
    rk = int(r)
    assert rk == int(rs) == {"lowrank20_40x1100": 20, "lowrank20_1100x40": 20, "dense_1100x40": 40, "dense_48x48": 48, "zero_20x12": 0}[name]
    out = R.copy()
    out[:rk, :rk] = 0
    assert np.all(out == 0) and np.all(np.tril(R[:rk, :rk], -1) == 0)      # exact zeros outside the triangle T
    nA = max(np.linalg.norm(A), 1)
    assert np.abs(U @ R @ V - A).max() <= 1e-13 * nA
    assert np.abs(U.T @ U - np.eye(M)).max() <= 1e-13
    assert np.abs(V @ V.T - np.eye(N)).max() <= 1e-13
    if rk == N:                                                            # the exact permutation V[i, P[i]] = 1
        want = np.zeros((N, N))
        want[np.arange(N), P] = 1.0
        assert np.array_equal(V, want)
    if rk == 0:
        assert np.all(R == 0)


def test_urv_lstsq_beyond_1024():
    n, r = 1100, 1060
    U, R, V, Y = urvls_factors(8920, n, r)
    torch, dev = _dev()
    x = dev.urv_lstsq(*(torch.from_numpy(a).cuda() for a in (U, R, V)), torch.tensor(r, dtype=torch.int32, device="cuda"),
                      torch.from_numpy(Y).cuda()).cpu().numpy()
    ref = urvls_ref(U, R, V, r, Y)
    e64 = float(np.linalg.norm(urvls_ref(U, R, V, r, Y, dtype=np.float64) - ref))
    edev = float(np.linalg.norm(x - ref))
    floor = EPS * float(np.linalg.norm(ref))
    print("urv_lstsq 1100 r1060 err_dev %.3e err_f64 %.3e eps||x|| %.3e ratio %.2f" % (edev, e64, floor, edev / max(e64, floor)))
    assert edev <= G * max(e64, floor)
