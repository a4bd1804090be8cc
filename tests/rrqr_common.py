"""Shared helpers of the column-pivoted QR tests: the golden fixtures of tests/golden/rrqr/ (tools/gen_golden_rrqr.js) and
their inputs, regenerated from the seed with the repo's generator and the families of tests/families.py; and plain longdouble
references of the pivot pass, the rank and the least squares with the inputs of test_gpu_rrqr_paths.py (second half)."""
import json
import os

import numpy as np

from families import apply_family
from nd4js_amd.rng import fill_uniform

GOLDEN_RRQR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rrqr")
EPS = 2.0 ** -52


def manifest():
    with open(os.path.join(GOLDEN_RRQR, "manifest.json")) as f:
        return json.load(f)["cases"]


def load(meta, key):
    return np.load(os.path.join(GOLDEN_RRQR, meta["files"][key]))


def _special(fam, a):
    M, N = a.shape
    if fam == "identity":
        a[...] = np.eye(M, N)
    elif fam == "zero":
        a[...] = 0.0
    elif fam == "dupcols":
        a[:, 1::2] = a[:, 0:N - 1:2][:, :a[:, 1::2].shape[1]]
    else:
        apply_family(fam, a, 0)
    return a


def make(seed, shape, fam):
    """the generator's input(): nd4_uniform(seed, i) then the family on each batch member with seed + b"""
    shape = tuple(shape)
    a = fill_uniform(seed, int(np.prod(shape))).reshape((-1,) + shape[-2:])
    for b in range(a.shape[0]):
        if fam in ("identity", "zero", "dupcols"):
            _special(fam, a[b])
        else:
            apply_family(fam, a[b], seed + b)
    return a.reshape(shape)


def y_of(meta):
    N = meta["shape"][-2]
    return fill_uniform(meta["y_seed"], N * meta["J"]).reshape(N, meta["J"])


def permuted(A, P):
    return np.take_along_axis(A, np.broadcast_to(P[..., None, :].astype(np.int64), A.shape), axis=-1)


def check_properties(A, Q, R, P, full=False):
    M, N = A.shape[-2:]
    nA = max(np.linalg.norm(A), 1e-300)
    assert np.all(np.sort(P, axis=-1) == np.arange(N))
    assert np.linalg.norm(permuted(A, P) - Q @ R) <= 1e-13 * nA
    k = Q.shape[-1]
    QtQ = np.swapaxes(Q, -1, -2) @ Q
    assert np.abs(QtQ - np.eye(k)).max() <= 1e-13
    assert np.all(np.tril(R, -1) == 0.0)
    d = np.abs(np.diagonal(R, axis1=-2, axis2=-1))
    assert np.all(d[..., 1:] <= d[..., :-1] + 1e-13 * nA)


def separated_prefix(R, rank):
    """first step i where the winning trailing norm c_i = ||R[i:, i]|| is within 1e-10 (relative) of a later candidate
    c_k = ||R[i:, k]||, or at / below the rank threshold; K if neither happens (the rows >= i of the reference's R are the
    trailing matrix at step i up to an orthogonal transformation)"""
    M, N = R.shape
    K = min(M, N)
    T = 2 * EPS * max(M, N) * np.linalg.norm(np.triu(R))
    for i in range(K):
        c = np.linalg.norm(R[i:, i:], axis=0)
        if i >= rank or c[0] <= T:
            return i
        if c.size > 1 and (c[0] - c[1:].max()) / c[0] < 1e-10:
            return i
    return K


# ---- a plain reference of the pivot pass, the rank estimate and the least squares (csrc/rrqr.hip), in np.longdouble -----------
LD = np.longdouble
DECIDED = 1e-8       # a step whose winner leads by this (relative) is decided: the device recomputes every norm from at most
#                      2060 entries, relative error <= 2060 * 2^-52 ~ 5e-13, four orders of magnitude below


def update_tier(length):
    """E of the qp3_update<E> that launch_update picks for len = M - i (M for the initial norms); 0 is the loop form"""
    return 1 if length <= 64 else 4 if length <= 256 else 16 if length <= 1024 else 32 if length <= 2048 else 0


# decided_prefix keeps the signature (A, P, margins) that its callers read naturally: "how much of this P does this input decide".
# Whether a step is decided also needs who was tied with the winner and how far the rest trailed, which P and the margins do not
# hold, so one run per input yields all four results and is kept here by the input's bytes; decided_prefix checks that the P and
# margins it is handed are that run's and reads the fourth from it. At most 64 inputs are kept.
_QRCP = {}


def _qrcp(A):
    A = np.ascontiguousarray(A, dtype=np.float64)
    key = (A.shape, A.tobytes())
    if key not in _QRCP:
        if len(_QRCP) >= 64:
            _QRCP.clear()
        _QRCP[key] = _qrcp_run(A)
    return _QRCP[key]


def _qrcp_run(A):
    M, N = A.shape
    K = min(M, N)
    W = A.astype(LD)
    pos = np.arange(N)                                   # pos[j]: the input column now at position j
    margins = np.full(K, np.nan, dtype=LD)
    decided = np.zeros(K, dtype=bool)
    stopped_at = K
    exact = True                                         # every winner so far had one nonzero entry: its reflector is a sign flip
    with np.errstate(all="ignore"):
        # what the device's rounding can move the trailing norm of column j by (Householder QR is stable column by column;
        # the second term is the spacing of the subnormals)
        noise = max(M, N) * (LD(EPS) * np.sqrt((W * W).sum(axis=0)) + np.sqrt(LD(M)) * LD(2.0) ** -1074)
        for i in range(K):
            S = W[i:, i:]
            c = np.sqrt((S * S).sum(axis=0))             # every remaining norm from scratch; an Inf stays Inf, a NaN stays NaN
            ok = ~np.isnan(c)
            if not ok.any():
                stopped_at = i                           # nothing comparable
                break
            best = c[ok].max()
            if best == 0:
                stopped_at = i
                break
            p = int(np.flatnonzero(ok & (c == best))[0])  # the first maximum under a strict <
            others = ok.copy()
            others[p] = False
            tied = others & (c == best)
            rest = others & ~tied
            if not others.any():
                margins[i] = 1.0
            elif np.isinf(best):
                margins[i] = 0.0 if tied.any() else 1.0
            else:
                margins[i] = (best - c[others].max()) / best
            nz = noise[pos[i:]]
            clear = True                                 # the candidates that are not tied are out of the device's reach
            if rest.any() and not np.isinf(best):
                clear = bool((best - c[rest].max()) / best >= DECIDED and np.all(best - c[rest] >= nz[rest] + nz[p]))
            if tied.any():
                w = A[:, pos[i + p]]
                twins = all(np.array_equal(A[:, pos[i + t]], w) or np.array_equal(A[:, pos[i + t]], -w) for t in np.flatnonzero(tied))
                single = exact and bool(np.all(np.count_nonzero(S[:, tied | ~others & ok], axis=0) == 1))
                decided[i] = clear and (twins or single)
            else:
                decided[i] = clear
            exact = exact and np.count_nonzero(S[:, p]) == 1
            if p:
                W[:, [i, i + p]] = W[:, [i + p, i]]
                pos[[i, i + p]] = pos[[i + p, i]]
            x = W[i:, i].copy()
            alpha = x[0]
            beta = -np.copysign(best, alpha)
            v = x / (alpha - beta)
            v[0] = 1.0
            tau = (beta - alpha) / beta
            if i + 1 < N:
                T = W[i:, i + 1:]
                w = tau * (v[:, None] * T).sum(axis=0)   # row by row: two identical columns stay identical
                W[i:, i + 1:] = T - v[:, None] * w[None, :]
            W[i, i] = beta
            W[i + 1:, i] = 0.0
    for a in (margins, decided):
        a.setflags(write=False)
    return pos.astype(np.int32), margins, stopped_at, decided


def qrcp_ref(A):
    """(P, margins, stopped_at) of Householder QR with column pivoting in longdouble, by the rule of csrc/rrqr.hip: before every
    step each remaining column's norm below row i is recomputed from scratch; the first maximum wins under a strict < (an
    earlier position on a tie, a NaN never); the pass ends at step stopped_at when the maximum is exactly zero or nothing is
    comparable (min(M, N) when it never does), and the remaining columns keep their order. margins[i] = (winner - best other)
    / winner over the comparable candidates (1 when there is no other; for an infinite winner 1, or 0 when another is
    infinite too); NaN from stopped_at on."""
    P, margins, stopped_at, _ = _qrcp(A)
    return P.copy(), margins, stopped_at


def decided_prefix(A, P, margins):
    """the number of leading steps of qrcp_ref(A) = (P, margins, .) on which the device has no freedom. A step is decided when
      * its margin is >= 1e-8 (DECIDED above), or
      * its margin is exactly 0 and every tied candidate's input column is bit-identical to the winner's up to sign (the
        same lanes then run the same operations in the same order on both, so the device's norms are bit-identical too), or
      * its margin is exactly 0 and the winner, every tied candidate and every earlier winner has a single nonzero entry in
        its trailing column: each reflector so far was an exact sign flip and each of these norms is one entry's magnitude,
        exact in any arithmetic (the identity, a permuted diagonal);
    and, in each case, every candidate that is not tied trails the winner by 1e-8 and by more than the rounding of a double
    Householder QR can move the two norms, max(M, N) (eps ||A[:, j]|| + sqrt(M) 2^-1074) each. The last condition ends the
    prefix where a rank-deficient input's trailing matrix is rounding noise; on every input of test_gpu_rrqr_paths.py it is
    weaker than the margin by orders of magnitude."""
    rP, rm, stopped_at, decided = _qrcp(A)
    assert np.array_equal(rP, P) and np.array_equal(rm, margins, equal_nan=True), "decided_prefix: not qrcp_ref's P and margins"
    bad = np.flatnonzero(~decided[:stopped_at])
    return int(bad[0]) if bad.size else stopped_at


def rank_ref(R):
    """(rank, tmp): _rrqr_rank (rrqr.js:57-85) in longdouble. tmp[i] = ||triu(R)[i:L, :]||_F, T = 2 eps max(M, N) tmp[0], the
    rank is 1 + the last i with tmp[i] > T; -1 when a tmp[i] is not finite."""
    M, N = R.shape
    L = min(M, N)
    U = np.triu(np.asarray(R)[:L]).astype(LD)               # whatever lies below the diagonal (a NaN too) is not read
    with np.errstate(all="ignore"):
        tmp = np.sqrt(np.cumsum((U * U).sum(axis=1)[::-1])[::-1])
    if not np.all(np.isfinite(tmp)):
        return -1, tmp
    T = 2 * LD(EPS) * max(M, N) * (tmp[0] if L else LD(0))
    r = L
    while r > 0 and tmp[r - 1] <= T:
        r -= 1
    return r, tmp


# the gate of the least-squares tests: err_dev <= LSTSQ_G max(err_f64, eps ||x||), both errors against the longdouble formula and
# err_f64 the same formula in float64 numpy. Twice the worst ratio measured on the MI355X (1.85, the table in
# test_gpu_rrqr_paths.py), rounded up to a power of two; never more than 16.
LSTSQ_G = 4.0


def lstsq_ref(Q, R, P, Y, r, dtype=LD):
    """rrqr_lstsq (rrqr.js:447-580) for a given rank: x[P[i]] = (R[:r, :r]^-1 (Q^T Y)[:r])[i] for i < r, 0 elsewhere; in
    `dtype` (longdouble: the reference; float64: the same formula at the device's precision)"""
    I, J = R.shape[1], Y.shape[1]
    Qr, T = np.asarray(Q)[:, :r].astype(dtype), np.asarray(R)[:r, :r].astype(dtype)
    z = Qr.T @ np.asarray(Y).astype(dtype)
    for i in range(r - 1, -1, -1):
        z[i] = (z[i] - T[i, i + 1:] @ z[i + 1:]) / T[i, i]
    x = np.zeros((I, J), dtype=dtype)
    x[np.asarray(P[:r], dtype=np.int64)] = z
    return x


# ---- the inputs of test_gpu_rrqr_paths.py, each proved fully decided in test_rrqr_ref_host.py ----------------------------------
def generic(M, N):
    from nd4js_amd import rng
    return rng.matrix(8100 + M + 3 * N, M, N)


def plant(A, pairs):
    """pairs of (a, b, k, sign): column a is scaled by 2^k and column b becomes sign * column a, an exact tie that the earlier
    position a must win; distinct k decide pair after pair"""
    A = A.copy()
    for a, b, k, sign in pairs:
        A[:, a] = np.ldexp(A[:, a], k)
        A[:, b] = sign * A[:, a]
    return A


# 70 x 600, the layout of qp3_pivot (thread t scans positions i + t, i + t + 256, i + t + 512). The pair of step i:
#   0: 3, 40 one wave | 1: 10, 200 waves 0 and 3 | 2: 5, 261 one thread's slots 0 and 1 | 3: 250, 300 thread 247's slot 0 against
#   thread 41's slot 1, negated | 4: 100, 515 waves 1 and 3, slots 0 and 1
PLANT_600 = ((3, 40, 10, 1), (10, 200, 8, 1), (5, 261, 6, 1), (250, 300, 4, -1), (100, 515, 2, 1))
PLANT_WINNERS_600 = (3, 10, 5, 250, 100)
# one pair per update tier, at half the scale of the rest: it is decided last, after 38 reflectors have gone over both twins
PLANT_LATE = ((7, 29, -1, -1),)
TIER_SHAPES = ((74, 40), (266, 40), (1036, 40), (2060, 40))     # E = 4 -> 1, 16 -> 4, 32 -> 16, loop -> 32 within one run


def _with(A, edits):
    A = A.copy()
    for idx, val in edits:
        A[idx] = val
    return A


def _graded_columns(A):
    from nd4js_amd import rng
    N = A.shape[1]
    order = np.argsort(rng.fill_uniform(8400, N))
    return np.ldexp(A, (np.round(-600 + 1000.0 * order / (N - 1)).astype(np.int64))[None, :])


def pivot_cases():
    """name -> (input, the set of qp3_update tiers the run must take)"""
    c = {}
    for M, N, tiers in ((74, 40, {4, 1}), (266, 40, {16, 4}), (1036, 40, {32, 16}), (2060, 40, {0, 32}),
                        (64, 64, {1}), (65, 65, {4, 1}), (256, 40, {4}), (257, 40, {16, 4}), (1024, 40, {16}), (1025, 40, {32, 16}),
                        (2048, 7, {32}), (2049, 7, {0, 32}), (70, 600, {4, 1}), (40, 1100, {1}), (257, 259, {16, 4, 1}),
                        (600, 130, {16})):
        c["generic-%dx%d" % (M, N)] = (generic(M, N), tiers)
    from nd4js_amd import rng
    c["planted-70x600"] = (plant(rng.matrix(8200, 70, 600), PLANT_600), {4, 1})
    for M, N in TIER_SHAPES:
        g = generic(M, N)
        tiers = c["generic-%dx%d" % (M, N)][1]
        c["planted-%dx%d" % (M, N)] = (plant(g, PLANT_LATE), tiers)
        c["nan-%dx%d" % (M, N)] = (_with(g, [((M - 2, 11), np.nan)]), tiers)
    g = generic(74, 40)
    c["inf-74x40"] = (_with(g, [((5, 9), np.inf)]), {4})
    c["stop3-74x40"] = (_with(g, [((slice(3, None), slice(None)), 0.0)]), {4})
    c["zero-74x40"] = (np.zeros((74, 40)), {4})
    c["up1000-74x40"] = (np.ldexp(g, 1000), {4, 1})
    c["down1000-74x40"] = (np.ldexp(g, -1000), {4, 1})
    c["subnormal-74x40"] = (np.ldexp(rng.matrix(8300, 74, 40), -1040), {4, 1})
    c["graded-74x40"] = (_graded_columns(g), {4, 1})
    return c


BATCH_MEMBERS = ("generic-74x40", "stop3-74x40", "zero-74x40", "nan-74x40", "planted-74x40")


def tiers_taken(M, N, stopped_at):
    """the tiers of the launches whose result the pass reads: the initial norms, then the update of step i < stopped_at"""
    t = {update_tier(M)}
    for i in range(min(M, N) - 1):                       # the launch after step i runs when i + 1 < K; a stopped matrix returns at once
        if i < stopped_at:
            t.add(update_tier(M - i))
    return t


# ---- synthetic triangular factors for the rank and least-squares kernels -----------------------------------------------------
DROP = 2.0 ** -70    # rows at and below the rank: far under T / 16 whatever the shape here


def tri_rows(seed, M, N, r, top=None, bottom=DROP):
    """upper-trapezoidal R [M, N]: row i < r is a uniform row times top(i) (1 by default), row i >= r times `bottom`; what
    lies below the diagonal is junk the kernels must not read"""
    from nd4js_amd import rng
    R = np.triu(rng.matrix(seed, M, N))
    s = np.full(M, bottom)
    s[:r] = 1.0 if top is None else [top(i) for i in range(r)]
    R *= s[:, None]
    R[np.tril_indices(M, -1, N)] = 7.0
    return R


def _jump(seed, n, r):
    """rows above r: uniform, scaled by f. Row r: one diagonal entry 2^(e+10). Rows below r: every entry +-1.5 * 2^e, about
    2^19 of them. Walking up, qp3_rank meets row r with a sum S ~ 2^20 at exponent e and must rescale it by 2^-20; the true
    tmp[r] is T / 18, and a rescaling by 2^-10 would put it at 1.3 T and the rank at r + 1."""
    from nd4js_amd import rng
    e = -45
    R = np.triu(rng.matrix(seed, n, n))
    R[r + 1:] = np.triu(np.where(rng.matrix(seed + 1, n, n) < 0, -1.5, 1.5) * 2.0 ** e)[r + 1:]
    R[r] = 0.0
    R[r, r] = 2.0 ** (e + 10)
    below = np.sqrt(np.sum(R[r:].astype(LD) ** 2))
    top = np.sqrt(np.sum(R[:r].astype(LD) ** 2))
    R[:r] *= float(18 * below / (2 * LD(EPS) * n * top))
    return R


def rank_cases():
    """name -> (builder of R, the rank it is built for); test_rrqr_ref_host.py proves tmp[r-1] >= 16 T and tmp[r] <= T / 16 in
    longdouble. qp3_rank walks the rows from the bottom in chunks of 1024: for L = 2049 rows 1025.., rows 1..1024, row 0."""
    from functools import partial as f
    c = {}
    for L, ranks in ((1024, (1, 1024)), (1025, (1, 2, 1025)), (2049, (1, 1024, 1025, 1026, 2049))):
        for r in ranks:                                  # L - 1024 and either side of it, 1 and L
            c["step-%d-r%d" % (L, r)] = (f(tri_rows, 8500 + L, L, L, r), r)
        c["zero-%d" % L] = (f(tri_rows, 8500 + L, L, L, 0, bottom=0.0), 0)   # r = 0 exists only as an all-zero triangle
    for M, N in ((40, 1100), (1100, 40)):
        for r in (1, 17, 40):
            c["step-%dx%d-r%d" % (M, N, r)] = (f(tri_rows, 8600 + M, M, N, r), r)
        c["zero-%dx%d" % (M, N)] = (f(tri_rows, 8600 + M, M, N, 0, bottom=0.0), 0)
        c["graded-%dx%d-r30" % (M, N)] = (f(tri_rows, 8600 + M, M, N, 30, top=lambda i: 2.0 ** (-i / 4)), 30)
    c["graded-1025-r120"] = (f(tri_rows, 8701, 1025, 1025, 120, top=lambda i: 2.0 ** (-i / 4)), 120)
    c["sawtooth-2049-r1025"] = (f(tri_rows, 8702, 2049, 2049, 1025, top=lambda i: 2.0 ** (-(i % 64) / 4)), 1025)
    c["tinyrows-2049-r1025"] = (f(tri_rows, 8703, 2049, 2049, 1025, top=lambda i: 2.0 ** -30 if i % 7 == 3 else 1.0), 1025)
    c["zeroblock-2049-r1025"] = (f(tri_rows, 8704, 2049, 2049, 1025, top=lambda i: 0.0 if 300 <= i < 700 else 1.0), 1025)
    c["zerotail-2049-r1025"] = (f(tri_rows, 8705, 2049, 2049, 1025, bottom=0.0), 1025)
    c["extreme-2049-r1025"] = (f(tri_rows, 8706, 2049, 2049, 1025, top=lambda i: 2.0 ** 400, bottom=2.0 ** -600), 1025)
    c["jump-2049-r1025"] = (f(_jump, 8707, 2049, 1025), 1025)

    def full_with(edits):
        return _with(tri_rows(8500 + 2049, 2049, 2049, 2049), edits)
    for what, val in (("nan", np.nan), ("inf", np.inf)):
        c["%s-lowest-chunk" % what] = (f(full_with, [((2040, 2045), val)]), -1)
        c["%s-highest-chunk" % what] = (f(full_with, [((0, 5), val)]), -1)
        c["%s-diagonal" % what] = (f(full_with, [((1024, 1024), val)]), -1)
        c["%s-below-diagonal" % what] = (f(full_with, [((2040, 3), val), ((5, 2), val), ((1025, 1024), val)]), 2049)
    return c


def ls_factors(seed, N, M, I, J, r):
    """synthetic factors for rrqr_lstsq: Q [N, M] orthonormal (numpy's QR of a uniform matrix), R [M, I] whose leading r x r
    triangle is D + E (|D_ii| in [1, 2], ||E|| ~ 0.35: cond <= ~5) and whose rows from r on are DROP times uniform, P a
    random permutation of I, Y [N, J] uniform"""
    from nd4js_amd import rng
    Q = np.linalg.qr(rng.matrix(seed, N, M))[0]
    R = np.triu(rng.matrix(seed + 1, M, I))
    L = min(M, I)
    R[:r, :r] = np.triu(R[:r, :r], 1) * (0.3 / np.sqrt(max(r, 1)))
    d = rng.fill_uniform(seed + 2, L)
    R[np.arange(r), np.arange(r)] = np.where(d[:r] < 0, -1.0, 1.0) * (1.5 + 0.5 * d[:r])
    R[:r, r:] /= np.sqrt(I)
    R[r:] *= DROP
    P = np.argsort(rng.fill_uniform(seed + 3, I)).astype(np.int32)
    Y = rng.matrix(seed + 4, N, J)
    return Q, R, P, Y


# name -> (seed, N, M, I, J, rank)
LS_CASES = {
    "1100-full": (8800, 1100, 1100, 1100, 3, 1100),      # L and I beyond 1024: the row loops of qp3_mask and qp3_unperm
    "1100-r700": (8810, 1100, 1100, 1100, 3, 700),
    "wide-40x300": (8820, 60, 40, 300, 2, 40),           # I > L: rows P[L:] of x are 0
    "wide-40x300-r25": (8830, 60, 40, 300, 2, 25),
    "J300-L40": (8840, 60, 40, 40, 300, 33),             # J > L: the second column block of qp3_mask zeroes Z
    "J3-L300": (8850, 320, 300, 300, 3, 211),
}
LS_BATCH = ((8860, 64), (8870, 30), (8880, 1))           # three members of N, M, I, J = 80, 64, 70, 2 with three ranks
