"""Shared by the tests of the Jacobi route of the symmetric eigenproblem, eigen_sym(S, algo='jacobi') (test_eigsym_jacobi_host.py,
test_gpu_eigsym_jacobi.py, test_node_eigsym_jacobi.py): the catalogue of inputs and `model`, a numpy float64 restatement of exactly
the arithmetic of csrc/syevj.hip. The kernel is compiled without FMA contraction and has no reductions, so the device has to
return the model's lambda, V and sweep counts bit for bit.

What the model restates (each line is one decision of the kernel):
  scaling    the lower triangle is mirrored and scaled by 2^(512 - e), max|s_ij| = m 2^e with m in [0.5, 1); lambda is scaled
             back with ldexp
  pair order round r of a sweep holds the pairs nd4_rr_pair(n2, r, slot), slot = 0 .. n2/2 - 1, p < q; n2 = N rounded up to
             even, the pair with q = N is the bye
  criterion  rotate iff s_pq != 0 and |s_pq| > (eps sqrt|s_pp|) sqrt|s_qq|, eps = 2^-52, read from the lower triangle
  rotation   theta = (s_qq - s_pp) / (2 s_pq); t = copysign(1 / (|theta| + sqrt(1 + theta^2)), theta), or 0.5 / |theta| when
             theta^2 overflows; c = 1 / sqrt(1 + t^2); s = t c; tau = s / (1 + c)
  update     s_pp -= t s_pq, s_qq += t s_pq, s_pq = 0; then every 2 x 2 block (k, l) of the round's pairs with slot k > slot l gets
             the row rotation of pair k first, then the column rotation of pair l, and is mirrored (symmetry is exploited: S stays
             exactly symmetric); x_p' = x_p - s (x_q + tau x_p), x_q' = x_q + s (x_p - tau x_q), also for the rows of V^T.
             A pair with s = 0 moves nothing off its own block.
  end        after a sweep without a rotation (the count includes that sweep); the cap is 60
  sort       descending, ties by ascending position; V follows"""
import functools
import os

import numpy as np

import eigsym_common as ec
from nd4js_amd import rng

EPS = 2.0 ** -52
MAX_SWEEPS = 60
MAXN = 128
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "eigsym_jacobi")


def rr_pair(n2, s, i):
    """svd_internal.h nd4_rr_pair"""
    m = n2 - 1
    p, q = (m, s) if i == 0 else ((s + i) % m, (s - i + m) % m)
    return (q, p) if p > q else (p, q)


@functools.lru_cache(maxsize=None)
def rounds(N):
    """per round: (P, Q) of its pairs in slot order. Odd N: the pair with q = N is the bye; it never rotates (s_pN = 0), but its
    row and column p are rotated by the round's other pairs like any block"""
    n2 = (N + 1) & ~1
    out = []
    for s in range(n2 - 1):
        pq = [rr_pair(n2, s, i) for i in range(n2 // 2)]
        out.append((np.array([p for p, _ in pq], dtype=np.intp), np.array([q for _, q in pq], dtype=np.intp)))
    return out


def _rot(x, y, s, tau, on):
    return np.where(on, x - s * (y + tau * x), x), np.where(on, y + s * (x - tau * y), y)


def model(S, criterion="relative", vectors=True):
    """(lambda [N] descending, V [N, N], sweeps) of one symmetric matrix, by the kernel's arithmetic. `criterion='absolute'`
    replaces the rotation rule by |s_pq| > eps max|s_ij| (the rule the route exists to avoid; for the tests that show why)."""
    S = np.asarray(S, dtype=np.float64)
    N = S.shape[0]
    A = np.tril(S) + np.tril(S, -1).T
    mx = np.abs(A).max()
    assert np.isfinite(mx)
    sc = 512 - int(np.frexp(mx)[1]) if mx > 0 else 0
    n2 = (N + 1) & ~1
    A = np.pad(np.ldexp(A, sc), (0, n2 - N))                             # odd N: a zero row and column for the bye
    Vt = np.eye(n2)[:, :N]
    sweeps, done = 0, False
    with np.errstate(all="ignore"):
        while not done and sweeps < MAX_SWEEPS:
            rotated = False
            for P, Q in rounds(N):
                app, aqq, apq = A[P, P], A[Q, Q], A[Q, P]
                if criterion == "relative":
                    rot = (apq != 0.0) & (np.abs(apq) > (EPS * np.sqrt(np.abs(app))) * np.sqrt(np.abs(aqq)))
                else:
                    rot = (apq != 0.0) & (np.abs(apq) > EPS * np.ldexp(1.0, 512))
                if not rot.any():
                    continue
                rotated = True
                theta = (aqq - app) / (2.0 * apq)
                at = np.abs(theta)
                t2 = at * at
                t = np.where(t2 <= np.finfo(np.float64).max, 1.0 / (at + np.sqrt(1.0 + t2)), 0.5 / at)
                t = np.copysign(t, theta)
                c = 1.0 / np.sqrt(1.0 + t * t)
                sn = np.where(rot, t * c, 0.0)
                tau = np.where(rot, sn / (1.0 + c), 0.0)
                h = t * apq
                A[P, P] = np.where(rot, app - h, app)
                A[Q, Q] = np.where(rot, aqq + h, aqq)
                A[Q, P] = np.where(rot, 0.0, apq)
                A[P, Q] = A[Q, P]
                on = sn != 0.0
                K, L = np.tril_indices(P.size, -1)                        # blocks with slot k > slot l
                pk, qk, pl, ql = P[K], Q[K], P[L], Q[L]
                x00, x01, x10, x11 = A[pk, pl], A[pk, ql], A[qk, pl], A[qk, ql]
                sk, tk, ok = sn[K], tau[K], on[K]
                x00, x10 = _rot(x00, x10, sk, tk, ok)                     # rows pk, qk
                x01, x11 = _rot(x01, x11, sk, tk, ok)
                sl, tl, ol = sn[L], tau[L], on[L]
                x00, x01 = _rot(x00, x01, sl, tl, ol)                     # columns pl, ql
                x10, x11 = _rot(x10, x11, sl, tl, ol)
                A[pk, pl] = x00; A[pk, ql] = x01; A[qk, pl] = x10; A[qk, ql] = x11
                A[pl, pk] = x00; A[ql, pk] = x01; A[pl, qk] = x10; A[ql, qk] = x11
                if vectors:
                    x, y = Vt[P], Vt[Q]
                    Vt[P], Vt[Q] = _rot(x, y, sn[:, None], tau[:, None], on[:, None])
            sweeps += 1
            done = not rotated
    d = np.diag(A)[:N].copy()
    order = np.argsort(-d, kind="stable")
    return np.ldexp(d[order], -sc), np.ascontiguousarray(Vt[:N][order].T), sweeps, done


# ---- the catalogue ---------------------------------------------------------------------------------------------------------------
GRADED = {"graded_pd_24": (7400, 24, 8), "graded_pd_48": (7401, 48, 10), "graded_pd_64": (7402, 64, 20), "graded_pd_100": (7403, 100, 12)}


def graded_pd(seed, N, span):
    """S = D A D: A = x x^T / N + I scaled to unit diagonal (kappa_2(A) ~ 2.2), D_i = 10^(-span i / (N - 1)); cond(S) ~ 10^(2 span)"""
    x = rng.matrix(seed, N, N)
    A = x @ x.T / N + np.eye(N)
    r = 1.0 / np.sqrt(np.diag(A))
    A = A * r[:, None] * r[None, :]
    D = 10.0 ** (-span * np.arange(N) / (N - 1.0))
    return ec._sym(A * D[:, None] * D[None, :])


def graded_reference(name):
    """the fixture: eigenvalues descending, float64 rounded from mpmath.eigsy at 60 digits (tools/gen_golden_eigsym_jacobi.py)"""
    return np.load(os.path.join(GOLDEN, name + ".Lam.npy"))


def scaled_kappa(S):
    """kappa_2(A) of A = D^-1 S D^-1, D = diag(sqrt s_ii)"""
    r = 1.0 / np.sqrt(np.diag(S))
    return np.linalg.cond(S * r[:, None] * r[None, :])


def _theta_overflow():
    # s_pq passes the relative rule (2^-540 > eps 2^-520) and theta ~ -2^539: theta^2 overflows
    return np.array([[1.0, 0.0], [2.0 ** -540, 2.0 ** -1040]]) + np.array([[0.0, 2.0 ** -540], [0.0, 0.0]])


def _denormal_offdiag():
    S = np.diag([1.0, 2.0, 3.0, 4.0])
    for i in range(4):
        for j in range(i):
            S[i, j] = S[j, i] = 5e-324 * (1 + i + j)
    return S


def _denormal_all():
    g = np.round(rng.matrix(7410, 5, 5) * 1000.0)
    return ec._sym(g) * 5e-324                                          # every entry an integer multiple of the smallest denormal


def _mixed():
    m = [np.eye(8), np.zeros((8, 8)), ec.sym_uniform(7411, 8), np.diag([3.0, 1.0, 3.0, -2.0, 1.0, 0.0, 7.0, 7.0]),
         np.ldexp(ec.sym_uniform(7412, 8), -300), ec.tridiag(np.arange(8.0), np.ones(7)),
         ec._sym(np.outer(rng.fill_uniform(7413, 8), rng.fill_uniform(7413, 8)))]
    return np.stack(m)


@functools.lru_cache(maxsize=None)
def catalogue():
    """name -> builder; every eigsym_common.CATALOGUE entry with N <= 128 and the Jacobi route's own cases"""
    cat = {}
    for name, build in ec.CATALOGUE.items():
        if build().shape[-1] <= MAXN:
            cat[name] = build
    for N in (1, 2, 3, 4, 5, 31, 32, 33, 63, 64, 65, 127, 128):
        cat.setdefault("dense_%d" % N, functools.partial(ec.sym_uniform, ec.DENSE_SEED + N, N))
    cat.update({
        "eqdiag_2": lambda: np.array([[1.0, 0.5], [0.5, 1.0]]),           # theta = 0: t = 1
        "eqdiag_neg_2": lambda: np.array([[1.0, -0.5], [-0.5, 1.0]]),     # theta = -0: t = -1
        "theta_overflow_2": _theta_overflow,
        "diag_ties_6": lambda: np.diag([3.0, 1.0, 3.0, -2.0, 1.0, 0.0]),
        "denormal_offdiag_4": _denormal_offdiag,
        "denormal_all_5": _denormal_all,
        "mixed_7x8": _mixed,                                              # a partial workgroup; members need different sweep counts
        "batch_3x40": lambda: np.stack([ec.sym_uniform(7420 + b, 40) for b in range(3)]),
    })
    for name, (seed, N, span) in GRADED.items():
        cat[name] = functools.partial(graded_pd, seed, N, span)
    return cat


def names():
    return tuple(catalogue())


@functools.lru_cache(maxsize=None)
def case(name):
    """(S, lambda, V, sweeps int32) of the model, members stacked like S; read-only, shared by every test"""
    S = np.ascontiguousarray(catalogue()[name](), dtype=np.float64)
    assert np.array_equal(S, np.swapaxes(S, -1, -2))
    N = S.shape[-1]
    lam, V, sw = np.empty(S.shape[:-1]), np.empty(S.shape), np.empty(S.shape[:-2], dtype=np.int32)
    for b, s in enumerate(S.reshape(-1, N, N)):
        l, v, n, done = model(s)
        assert done, "%s[%d]: the model did not converge" % (name, b)
        lam.reshape(-1, N)[b], V.reshape(-1, N, N)[b], sw.reshape(-1)[b] = l, v, n
    return ec._freeze(S, lam, V, sw)


@functools.lru_cache(maxsize=None)
def lapack(name):
    """(lambda descending, V) of numpy.linalg.eigh on the same input"""
    w, v = np.linalg.eigh(case(name)[0])
    return ec._freeze(np.ascontiguousarray(w[..., ::-1]), np.ascontiguousarray(v[..., ::-1]))


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()
