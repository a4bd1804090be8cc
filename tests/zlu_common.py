"""The numpy model, inputs and bounds of tests/test_zlu_host.py and tests/test_gpu_zlu.py for zlu_decomp / zlu_solve / zsolve: the contract
of DESIGN.md 4.26 on a stack [B, N, N], right-looking, one operation at a time, each rounded on its own. The random inputs are seeded
(SEEDS) so that every pivot of the model's run beats its runner-up by a relative MARGIN, which keeps P equal on the matrix cores."""
import functools

import numpy as np

TOL = 1e-12                       # the project's tolerance
EPS = np.finfo(np.float64).eps
MARGIN = 1e-6
LMAX = np.sqrt(2.0) * (1.0 + 4.0 * EPS)      # |l_ij| <= sqrt 2 is what the pivot rule guarantees; the division's rounding on top
DBL_MAX = np.finfo(np.float64).max
HP_MAX_N = 300                    # bound 1 on every row up to here; above (520, 1030, 2048: once each) on 32 rows, see shares

SIZES = [1, 2, 3, 8, 16, 17, 31, 32, 33, 63, 64, 65, 80, 129, 193, 300]
PANEL_SIZES = [520, 1030]         # the heights at which the register panel changes its rows per thread
BATCHES = [(5, 40, 40), (2, 130, 130), (70000, 4, 4)]
SEEDS = {name: 1 for name in [str(n) for n in SIZES + PANEL_SIZES + [40, 130]] + ["5x40x40", "2x130x130", "70000x4x4"]}


def div(xr, xi, dr, di):
    with np.errstate(all="ignore"):
        r1 = di / dr
        den1 = dr + di * r1
        a = ((xr + xi * r1) / den1, (xi - xr * r1) / den1)
        r2 = dr / di
        den2 = dr * r2 + di
        b = ((xr * r2 + xi) / den2, (xi * r2 - xr) / den2)
        c = (xr / dr, xi / dr)
    big, real = np.abs(dr) >= np.abs(di), di == 0.0
    return tuple(np.where(real, c[k], np.where(big, a[k], b[k])) for k in (0, 1))


def nms(sr, si, ar, ai, br, bi):
    with np.errstate(all="ignore"):
        return (sr - ar * br) + ai * bi, (si - ar * bi) - ai * br


def lu_model(A):
    """(LU, P int32, info int32, margins [N]) of A [B, N, N] or [N, N]; margins[j]: the smallest relative lead of column j's pivot"""
    A = np.asarray(A, dtype=np.complex128)
    single = A.ndim == 2
    A = A.reshape((-1,) + A.shape[-2:])
    B, N = A.shape[0], A.shape[-1]
    re, im = np.array(A.real), np.array(A.imag)
    P = np.tile(np.arange(N, dtype=np.int32), (B, 1))
    info = np.zeros(B, dtype=np.int32)
    idx, margins = np.arange(B), np.full(N, np.inf)
    for j in range(N):
        with np.errstate(all="ignore"):
            key = np.abs(re[:, j:, j]) + np.abs(im[:, j:, j])
        nan = np.isnan(key)
        key[nan] = -1.0
        key[nan[:, 0], 0] = np.inf
        k = np.argmax(key, axis=1)                                          # the first maximum
        if key.shape[1] > 1:
            two = np.sort(key, axis=1)[:, -2:]
            with np.errstate(all="ignore"):
                rel = (two[:, 1] - two[:, 0]) / two[:, 1]
            margins[j] = np.min(rel[np.isfinite(rel)], initial=np.inf)
        piv = j + k
        for M in (re, im, P):
            tmp = np.array(M[idx, j])
            M[idx, j] = M[idx, piv]
            M[idx, piv] = tmp
        pr, pi = re[:, j, j], im[:, j, j]
        with np.errstate(all="ignore"):
            mag = np.abs(pr) + np.abs(pi)
        bad = ~((mag > 0.0) & (mag <= DBL_MAX))
        info = np.where((info == 0) & bad, j + 1, info).astype(np.int32)
        if j + 1 < N:
            lr, li = div(re[:, j + 1:, j], im[:, j + 1:, j], pr[:, None], pi[:, None])
            lr, li = np.where(bad[:, None], re[:, j + 1:, j], lr), np.where(bad[:, None], im[:, j + 1:, j], li)
            re[:, j + 1:, j], im[:, j + 1:, j] = lr, li
            re[:, j + 1:, j + 1:], im[:, j + 1:, j + 1:] = nms(re[:, j + 1:, j + 1:], im[:, j + 1:, j + 1:], lr[:, :, None], li[:, :, None],
                                                              re[:, j, None, j + 1:], im[:, j, None, j + 1:])
    LU = re + 1j * im
    return (LU[0], P[0], info[0], margins) if single else (LU, P, info, margins)


def solve_model(LU, P, Y):
    """X with A X = Y from LU [B, N, N], P [B, N], Y [B, N, K] (or one member each): Y[P], the unit lower sweep, the upper sweep"""
    LU, Y = np.asarray(LU, dtype=np.complex128), np.asarray(Y, dtype=np.complex128)
    single = LU.ndim == 2
    LU, P, Y = LU.reshape((-1,) + LU.shape[-2:]), np.asarray(P).reshape(-1, LU.shape[-1]), Y.reshape((-1,) + Y.shape[-2:])
    N = LU.shape[-1]
    X = np.take_along_axis(Y, P[:, :, None].astype(np.int64), axis=1)
    xr, xi, lr, li = np.array(X.real), np.array(X.imag), LU.real, LU.imag
    for i in range(N - 1):
        xr[:, i + 1:], xi[:, i + 1:] = nms(xr[:, i + 1:], xi[:, i + 1:], lr[:, i + 1:, i, None], li[:, i + 1:, i, None], xr[:, i, None], xi[:, i, None])
    for i in range(N - 1, -1, -1):
        xr[:, i], xi[:, i] = div(xr[:, i], xi[:, i], lr[:, i, i, None], li[:, i, i, None])
        xr[:, :i], xi[:, :i] = nms(xr[:, :i], xi[:, :i], lr[:, :i, i, None], li[:, :i, i, None], xr[:, i, None], xi[:, i, None])
    X = xr + 1j * xi
    return X[0] if single else X


def shares(A, LU, P, X=None, Y=None):
    """the largest share over the members of (bound 1, bound 3, bound 2 or None) in clongdouble; above N = 300 bound 1 on 32 rows"""
    A, LU, P = np.asarray(A), np.asarray(LU), np.asarray(P)
    N, hp = A.shape[-1], np.clongdouble
    norm = lambda M: np.sqrt(np.sum(np.abs(M.astype(hp)) ** 2, axis=(-2, -1)))   # noqa: E731
    L, U = np.tril(LU, -1) + np.eye(N), np.triu(LU)
    PA = np.take_along_axis(A, P[..., None].astype(np.int64), axis=-2)
    R = np.arange(N) if N <= HP_MAX_N else np.sort(np.random.default_rng(N).choice(N, 32, replace=False))
    s1 = np.max(norm(PA[..., R, :].astype(hp) - L[..., R, :].astype(hp) @ U.astype(hp)) / (TOL * norm(L[..., R, :]) * norm(U)))
    s3 = np.max(np.abs(np.tril(LU, -1))) / LMAX if N > 1 else 0.0
    if X is None:
        return float(s1), float(s3), None
    Y = np.asarray(Y, dtype=np.complex128)
    return float(s1), float(s3), float(np.max(norm(A.astype(hp) @ X.astype(hp) - Y.astype(hp)) / (TOL * (norm(A) * norm(X) + norm(Y)))))


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def cmatrix(seed, *shape):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


def name_of(shape):
    return "x".join(str(s) for s in shape)


@functools.lru_cache(maxsize=None)
def catalogue(name):
    """(A, LU, P, margin) of a catalogue input with the model's factorisation, computed once; read-only. name: '17' or '5x40x40'"""
    shape = tuple(int(s) for s in name.split("x"))
    shape = shape * 2 if len(shape) == 1 else shape
    A = cmatrix(SEEDS[name], *shape)
    LU, P, info, margins = lu_model(A)
    assert not np.any(info)
    out = (A, LU.reshape(shape), P.reshape(shape[:-1]), float(margins.min()))
    for M in out[:3]:
        M.setflags(write=False)
    return out


def exact_input(N, seed):
    """(A, LU, P) with small Gaussian (half-)integer factors: exact in every order of summation, every pivot twice its runner-up"""
    rng = np.random.default_rng(seed)
    units = np.array([1, 1j, -1, -1j])
    L = np.tril(rng.choice(np.array([0, 0.5, -0.5, 0.5j, -0.5j]), size=(N, N)), -1) + np.eye(N)
    U = np.triu(rng.integers(-2, 3, (N, N)) + 1j * rng.integers(-2, 3, (N, N)), 1) + np.diag(rng.choice(units, N) * rng.choice([1.0, 2.0], N))
    perm = rng.permutation(N)
    A = np.empty((N, N), dtype=np.complex128)
    A[perm] = L @ U                                                         # (L U)[i] = A[perm[i]]
    return A, np.tril(L, -1) + U, perm.astype(np.int32)


def tie_input(N, rows, seed):
    """column 0 holds 1, i, -1 and -i in `rows` and entries below 1/2 elsewhere: the first of the four must win"""
    A = 0.1 * cmatrix(seed, N, N)
    A[:, 0] *= 0.1
    A[list(rows), 0] = [1, 1j, -1, -1j]
    return A


def singular_members(N, seed):
    """[healthy, a zero column (N // 2), a zero last pivot, a NaN, an Inf, healthy] and the flags the first three and the last must get"""
    M = cmatrix(seed, 6, N, N)
    M[1][:, N // 2] = 0.0
    A, LU, P = exact_input(N, seed)
    LU = np.array(LU)
    LU[N - 1, N - 1] = 0.0
    M[2][P] = (np.tril(LU, -1) + np.eye(N)) @ np.triu(LU)
    M[3][N // 2, N // 3] = np.nan
    M[4][N - 1, 0] = np.inf
    return M, {0: 0, 1: N // 2 + 1, 2: N, 5: 0}


# ---- the argument rows of the C ABI: (operation, what, arguments after the handle, the error text or None for an empty call) ----
_B = 16          # any non-NULL pointer value
ROWS = [
    ("zgetrf_batched", "extent", (-1, 4, _B, _B, _B, None), "nd4hip_zgetrf_batched: negative extent"),
    ("zgetrf_batched", "limit", (1, 2049, _B, _B, _B, None), "nd4hip_zgetrf_batched: N <= 2048"),
    ("zgetrf_batched", "empty", (0, 4, None, None, None, None), None),
    ("zgetrf_batched", "null", (1, 4, _B, None, _B, None), "nd4hip_zgetrf_batched: NULL pointer"),
    ("zgetrs_batched", "extent", (1, 4, -1, _B, 16, _B, 4, _B, 4, _B), "nd4hip_zgetrs_batched: negative extent"),
    ("zgetrs_batched", "limit", (1, 2049, 1, _B, 0, _B, 0, _B, 0, _B), "nd4hip_zgetrs_batched: N <= 2048"),
    ("zgetrs_batched", "stride", (2, 4, 2, _B, 15, _B, 4, _B, 8, _B), "nd4hip_zgetrs_batched: a stride must be 0 or at least the size of one operand"),
    ("zgetrs_batched", "empty", (2, 4, 0, None, 16, None, 4, None, 0, None), None),
    ("zgetrs_batched", "null", (2, 4, 2, _B, 16, None, 4, _B, 8, _B), "nd4hip_zgetrs_batched: NULL pointer"),
    ("zgesv_batched", "extent", (1, -4, 1, _B, _B, _B), "nd4hip_zgesv_batched: negative extent"),
    ("zgesv_batched", "limit", (1, 2049, 1, _B, _B, _B), "nd4hip_zgesv_batched: N <= 2048"),
    ("zgesv_batched", "limit", (1, 4, 65535 * 64 + 1, _B, _B, _B), "nd4hip_zgesv_batched: K exceeds 4 194 240 right-hand sides"),
    ("zgetrs_batched", "limit", (1, 4, 65535 * 64 + 1, _B, 0, _B, 0, _B, 0, _B), "nd4hip_zgetrs_batched: K exceeds 4 194 240 right-hand sides"),
    ("zgesv_batched", "empty", (1, 4, 0, None, None, None), None),
    ("zgesv_batched", "null", (1, 4, 1, _B, None, _B), "nd4hip_zgesv_batched: NULL pointer"),
] + [(op, "handle", args, "nd4hip_%s: NULL handle" % op)               # a valid call without a handle
     for op, args in (("zgetrf_batched", (1, 4, _B, _B, _B, None)), ("zgetrs_batched", (1, 4, 2, _B, 16, _B, 4, _B, 8, _B)), ("zgesv_batched", (1, 4, 2, _B, _B, _B)))]
