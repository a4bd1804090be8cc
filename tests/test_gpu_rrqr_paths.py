"""Every kernel path of rrqr.hip through the device forms (dev.rrqr_decomp, dev.rrqr_rank, dev.rrqr_lstsq), against the plain
longdouble references of rrqr_common.py: qrcp_ref for the pivot pass (P is a decision: a wrong one still gives a valid
factorisation), rank_ref for the rank, lstsq_ref for the least squares. test_rrqr_ref_host.py proves on the CPU that every
input below is decided at every step (no step is left out of a comparison), takes the tier it is there for and meets its margin.

Every pivot case asserts: P equal to qrcp_ref's over all steps and over the tail after a stop; rrqr_common.check_properties,
the gates of test_gpu_rrqr.py (where the factors are finite and representable, see below); a second call gives the same bits.

Case -> path -> condition in the source (rrqr.hip: launch_update picks qp3_update<E> by len = M - i, M for the initial norms)

  generic 74x40 | 266x40 | 1036x40 | 2060x40   qp3_update<4> -> <1> | <16> -> <4> | <32> -> <16> | loop -> <32>   len crosses 64 | 256 | 1024 | 2048
                                                within one run                                                   during the 40 steps
  64^2 | 65^2                                   <1> throughout | <4> then <1>; 65 columns: last workgroup 1/4     len <= 64 | 65
  256x40 | 257x40                               <4> | <16> then <4>: the last register slot holds 1 row at 257    len 256 | 257
  1024x40 | 1025x40                             <16> | <32> then <16>                                             len 1024 | 1025
  2048x7 | 2049x7                               <32> | loop then <32>; 7 columns: 3 of 4 waves, then 2, 1 ...     len 2048 | 2049
  70x600 | 40x1100 | 257x259                    qp3_pivot: a thread's second and third (1100: up to fifth) stride  N > 256, 512, 1024
                                                slot; 600x130: <16> throughout, 130 columns
  planted 70x600                                five exact ties, one per step 0..4 (rrqr_common.PLANT_600): one    ob == best && oi < idx in the
                                                wave; two waves; one thread's slots 0 and 1; a high thread's slot  butterfly, `best < v` in the
                                                0 against a low thread's slot 1 at a higher index, negated; two    scan, the four-wave merge
                                                waves and two slots. The earlier position must win each.
  planted 74x40 | 266x40 | 1036x40 | 2060x40    a twin pair at half scale, decided at step 38: bit-identical       every tier of qp3_update keeps
                                                norms after 38 reflectors of two tiers each                        twins' norms bit-identical
  nan 74x40 ... 2060x40                         one NaN entry in column 11: nan_max keeps its norm NaN, `best < v` a NaN never wins; the column
                                                skips it in every tier                                             ends last, R[:, :-1] finite
  inf 74x40                                     one Inf at (5, 9): column 9 wins step 0, its reflector is NaN,     idx == INT_MAX: stop
                                                every norm after it NaN: the pass stops at step 1
  stop3 74x40 | zero 74x40                      rows >= 3 exactly zero: stop at step 3, the tail keeps its order   best == 0.0
  batch of five 74x40                           generic, stop3, zero, nan, planted: members that stop at steps     stop[b] per member
                                                40, 3, 0, 39 and 40; each P equal to its single call
  up1000 | down1000 74x40                       A 2^+-1000: the same P as A (norm_exp / ldexp / norm_finish)       exact power-of-two scaling
  subnormal 74x40                               uniform 2^-1040: subnormal entries, pivot norms < 5.6e-309         xk / den, not xk * (1 / den)
  graded 74x40                                  columns scaled 2^-600 ... 2^+400 in shuffled order

check_properties is run on the input scaled back by the exact power of two for up1000 and down1000; for the NaN inputs its gates
on R alone over the leading N - 1 columns (Q takes in the NaN reflector); not at all for inf (every factor is NaN by then) and
subnormal (R's entries are subnormal: they carry 2^-34 of their norm, not 1e-13). Q and R are the unpivoted QR of A[:, P], which
test_gpu_qr_paths.py covers.

Rank (qp3_rownorm + qp3_rank; rrqr_common.rank_cases): L = 1024, 1025 and 2049 square, 40x1100 and 1100x40; the crossing at r = 1, L,
L - 1024 and either side of it (the ends of qp3_rank's chunks of 1024 rows, walked from the bottom), r = 0 (a zero triangle over junk);
rows graded 2^(-i/4), a sawtooth 2^(-(i % 64)/4), tiny rows above large ones (the branch where the new exponent is not larger), a block
of zero rows, an all-zero tail, rows at 2^-600 under rows at 2^+400, and `jump`: 2^19 entries at one exponent under a row ten
exponents up, so that the rescaling of the running sum decides the rank. NaN and Inf in the lowest chunk, the highest chunk and on the
diagonal give -1; below the diagonal they change nothing.

Least squares (qp3_mask, qp3_unperm; rrqr_common.LS_CASES): synthetic Q R P with a known rank. Gate: err_dev <= G max(err_f64, eps ||x||),
both errors against lstsq_ref in longdouble, err_f64 the same formula in float64 numpy.

Measured on the MI355X (one run, the 79 cases of this file in 5.3 s, the slowest 0.4 s after the first call's start-up): err_dev /
max(err_f64, eps ||x||) per case; the worst is 1.85, so G = 4, the power of two at or above twice that. Nothing failed on the
kernels as they were: no kernel was changed.

  case                 err_dev    err_f64    eps ||x||   ratio
  1100-full            2.93e-14   1.58e-14   5.28e-15    1.85
  1100-r700            1.93e-14   1.22e-14   4.13e-15    1.59
  J3-L300              8.15e-15   6.32e-15   2.36e-15    1.29
  J300-L40             1.34e-14   1.12e-14   9.21e-15    1.19
  wide-40x300          1.59e-15   1.21e-15   8.91e-16    1.31
  wide-40x300-r25      9.82e-16   7.42e-16   6.72e-16    1.32
  batch of three       2.18e-15 | 1.17e-15 | 6.72e-17 against 1.72e-15 | 1.16e-15 | 2.42e-16: 1.27 | 1.00 | 0.28
  urv_lstsq 1100 r1060 3.05e-14   2.05e-14   5.12e-15    1.49   (test_gpu_srrqr_paths.py)

Mutations of rrqr.hip tried one at a time against this file and test_gpu_srrqr_paths.py, each run stopped at its first failure, none
committed (the sixth, in srrqr.hip, is in that file's docstring):
  the later index wins a tie in qp3_pivot (scan, butterfly and merge)     first caught by test_pivot_pass[planted-1036x40] (P[38], P[39] exchanged)
  nfrom = 0 in qp3_update (row i counted into the norm)                   test_pivot_pass[down1000-74x40], the first case run (P differs from step 3)
  the <16> tier taken up to len 1100 (rows beyond 1024 dropped)           test_pivot_pass[generic-1025x40] (P differs at steps 26 and 27)
  2 * (EX - ei) -> (EX - ei) in qp3_rank                                  test_rank[jump-2049-r1025] (1026 for 1025)
  qp3_mask without its row loop (rows >= 1024 of Tm and Z left as found)  test_lstsq[1100-full] (NaN)
"""
import functools

import numpy as np
import pytest

import rrqr_common as rc
from rrqr_common import check_properties

pytestmark = pytest.mark.gpu
G = rc.LSTSQ_G       # 4: see "Measured" above
PIVOT = rc.pivot_cases()
RANK = rc.rank_cases()


def _dev():
    import torch
    from nd4js_amd import dev
    return torch, dev


def _bits(x):
    return np.ascontiguousarray(x).view(np.int64 if x.dtype == np.float64 else x.dtype)


def _decomp(A):
    torch, dev = _dev()
    out = dev.rrqr_decomp(torch.from_numpy(np.ascontiguousarray(A)).cuda())
    torch.cuda.synchronize()
    return tuple(x.cpu().numpy() for x in out)


@functools.lru_cache(maxsize=None)
def _ref(name):
    P, margins, stopped_at = rc.qrcp_ref(PIVOT[name][0])
    P.setflags(write=False)
    return P, stopped_at


@functools.lru_cache(maxsize=None)
def _single(name):
    out = _decomp(PIVOT[name][0])
    for x in out:
        x.setflags(write=False)
    return out


@pytest.mark.parametrize("name", sorted(PIVOT))
def test_pivot_pass(name):
    A = PIVOT[name][0]
    M, N = A.shape
    wantP, stopped_at = _ref(name)
    Q, R, P = _single(name)
    assert np.array_equal(P, wantP), (np.flatnonzero(P != wantP)[:4], stopped_at)
    kind = name.split("-")[0]
    if kind == "nan":
        # Q is accumulated from every reflector, the NaN one included, and is not finite; the leading columns of R are, and
        # they are the triangle of A[:, P[:-1]]: R'^T R' = A'^T A' to twice the 1e-13 ||A|| of check_properties' residual
        Rl, Al = R[:N - 1, :N - 1], A[:, P[:-1]]
        assert P[-1] == 11 and np.all(np.isfinite(R[:, :N - 1])) and np.all(R[N - 1:, :N - 1] == 0) and np.all(np.tril(Rl, -1) == 0)
        assert np.linalg.norm(Rl.T @ Rl - Al.T @ Al) <= 2.1e-13 * np.linalg.norm(Al) ** 2
        d = np.abs(np.diag(Rl))
        assert np.all(d[1:] <= d[:-1] + 1e-13 * np.linalg.norm(Al))
    elif kind in ("up1000", "down1000"):
        k = -1000 if kind == "up1000" else 1000
        check_properties(np.ldexp(A, k), Q, np.ldexp(R, k), P)
        assert np.array_equal(P, _ref("generic-74x40")[0])
    elif kind not in ("inf", "subnormal"):
        check_properties(A, Q, R, P)
    Q2, R2, P2 = _decomp(A)
    assert np.array_equal(P2, P) and np.array_equal(_bits(Q2), _bits(Q)) and np.array_equal(_bits(R2), _bits(R))


def test_batch_members_stop_at_their_own_step():
    A = np.stack([PIVOT[n][0] for n in rc.BATCH_MEMBERS])
    assert [_ref(n)[1] for n in rc.BATCH_MEMBERS] == [40, 3, 0, 39, 40]
    Q, R, P = _decomp(A)
    for b, n in enumerate(rc.BATCH_MEMBERS):
        assert np.array_equal(P[b], _single(n)[2]), n
        assert np.array_equal(P[b], _ref(n)[0]), n
        assert np.array_equal(_bits(R[b]), _bits(_single(n)[1])) and np.array_equal(_bits(Q[b]), _bits(_single(n)[0])), n


# ---- rank -----------------------------------------------------------------------------------------------------------------------
def _rank(R):
    torch, dev = _dev()
    r = dev.rrqr_rank(torch.from_numpy(np.ascontiguousarray(R)).cuda())
    torch.cuda.synchronize()
    return r.cpu().numpy()


@pytest.mark.parametrize("name", sorted(RANK))
def test_rank(name):
    build, want = RANK[name]
    assert int(_rank(build())) == want


def test_rank_batch_members_are_independent():
    names = ("nan-lowest-chunk", "sawtooth-2049-r1025", "zero-2049", "jump-2049-r1025", "inf-below-diagonal")
    R = np.stack([RANK[n][0]() for n in names])
    assert list(_rank(R)) == [RANK[n][1] for n in names] == [-1, 1025, 0, 1025, 2049]


# ---- least squares ------------------------------------------------------------------------------------------------------------
def _lstsq(Q, R, P, Y):
    torch, dev = _dev()
    c = [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (Q, R, P, Y)]
    rank = torch.full(tuple(Y.shape[:-2]), -7, dtype=torch.int32, device="cuda")
    x = dev.rrqr_lstsq(*c, rank=rank)
    torch.cuda.synchronize()
    return x.cpu().numpy(), rank.cpu().numpy()


def _gate(name, x, Q, R, P, Y, r):
    ref = rc.lstsq_ref(Q, R, P, Y, r)
    e64 = float(np.linalg.norm(rc.lstsq_ref(Q, R, P, Y, r, dtype=np.float64) - ref))
    edev = float(np.linalg.norm(x - ref))
    floor = rc.EPS * float(np.linalg.norm(ref))
    print("lstsq %-18s err_dev %.3e err_f64 %.3e eps||x|| %.3e ratio %.2f" % (name, edev, e64, floor, edev / max(e64, floor)))
    assert edev <= G * max(e64, floor)
    assert np.all(x[P[r:]] == 0.0)                                         # past the rank (and past L): exact zeros


@pytest.mark.parametrize("name", sorted(rc.LS_CASES))
def test_lstsq(name):
    seed, N, M, I, J, r = rc.LS_CASES[name]
    Q, R, P, Y = rc.ls_factors(seed, N, M, I, J, r)
    x, rank = _lstsq(Q, R, P, Y)
    assert int(rank) == r == rc.rank_ref(R)[0]
    _gate(name, x, Q, R, P, Y, r)


def test_lstsq_batch_of_three_ranks():
    members = [rc.ls_factors(seed, 80, 64, 70, 2, r) for seed, r in rc.LS_BATCH]
    Q, R, P, Y = (np.stack(x) for x in zip(*members))
    x, rank = _lstsq(Q, R, P, Y)
    assert list(rank) == [rc.rank_ref(m[1])[0] for m in members] == [r for _, r in rc.LS_BATCH]
    for b, (m, (_, r)) in enumerate(zip(members, rc.LS_BATCH)):
        _gate("batch[%d]" % b, x[b], *m, r)
        assert np.array_equal(x[b], _lstsq(*m)[0])                         # and bit-equal to the member's own call
