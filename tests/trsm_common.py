"""Helpers of the triangular-solve tests (test_trsm_ref_host.py, test_gpu_trsm_paths.py); nothing here needs a GPU to import.

  families     triangles users actually pass: (T, upper) from the project's seeded generator
  omega        componentwise backward error max |T X - Y| / (|T||X| + |Y|), residual in np.longdouble; needs no reference solution
               and does not grow with the condition number
  subst        plain substitution, in the dtype of its operands (np.longdouble: the truth of the extreme-scale cases)
  model_one_launch   numpy model of trsm.hip's one-launch ALGORITHM (per 32-row block: 8 x 8 diagonal sub-blocks inverted column by
               column and coupled by substitution, the other rows by a product): what accuracy that algorithm can reach, not what
               the kernel does
  call_dtrsm_dev     nd4hip_dtrsm_batched_dev on operands embedded in sentinel-filled buffers
"""
import ctypes

import numpy as np

from families import triangle
from nd4js_amd import rng

LD = np.longdouble
TB = 32
SUB = 8                                                # the diagonal sub-blocks the one-launch path inverts explicitly
GUARD = 4096                                           # doubles before and after every operand and between batch members
SENTINEL = np.int64(0x7FF8C0DEC0DEC0DE)                # a quiet NaN with a payload no kernel produces


# ------------------------------------------------------------------------------------------------------------------- families
def _orth(seed, M):
    return np.linalg.qr(rng.matrix(seed, M, M))[0]


def _qr_r(seed, M, cond):
    a = (_orth(seed, M) * np.logspace(0, -np.log10(cond), M)) @ _orth(seed + 1, M).T
    return np.triu(np.linalg.qr(a)[1]), True


def _lu(seed, M, which):
    import scipy.linalg
    _, l, u = scipy.linalg.lu(rng.matrix(seed, M, M))
    return (np.tril(l), False) if which == "l" else (np.triu(u), True)


def _unit_dense(seed, M, upper):
    r = rng.matrix(seed, M, M)
    return (np.triu(r, 1) if upper else np.tril(r, -1)) + np.eye(M), upper


def _kahan(M, theta):
    s, c = np.sin(theta), np.cos(theta)
    return (s ** np.arange(M))[:, None] * (np.eye(M) - c * np.triu(np.ones((M, M)), 1)), True


FAMILIES = {
    "well_lower": lambda seed, M: (triangle(seed, (M, M), False), False),
    "well_upper": lambda seed, M: (triangle(seed, (M, M), True), True),
    "qr_r_1e6": lambda seed, M: _qr_r(seed, M, 1e6),
    "qr_r_1e13": lambda seed, M: _qr_r(seed, M, 1e13),
    "lu_u": lambda seed, M: _lu(seed, M, "u"),
    "lu_l": lambda seed, M: _lu(seed, M, "l"),
    "unit_dense_upper": lambda seed, M: _unit_dense(seed, M, True),
    "unit_dense_lower": lambda seed, M: _unit_dense(seed, M, False),
    "row_graded": lambda seed, M: (triangle(seed, (M, M), True) * np.logspace(0, -12, M)[:, None], True),
    "col_graded": lambda seed, M: (triangle(seed, (M, M), False) * np.logspace(0, -12, M)[None, :], False),
    "kahan_1.2": lambda seed, M: _kahan(M, 1.2),
}


def family(name, seed, M):
    """(T, upper): T holds exact zeros outside its triangle"""
    return FAMILIES[name](seed, M)


def effective(T, upper, unit=False):
    """the triangle a solve reads: the other half and (unit) the diagonal are ignored"""
    E = np.triu(T) if upper else np.tril(T)
    if unit:
        E = E.copy()
        E[..., np.arange(T.shape[-1]), np.arange(T.shape[-1])] = 1.0
    return E


# --------------------------------------------------------------------------------------------------- backward error, substitution
def _tri_matmul(F, Z, kind):
    """F @ Z for a triangular ('lower' / 'upper'), diagonal ('diag': F is the vector) or dense F, skipping the zero half"""
    if kind == "diag":
        return F[:, None] * Z
    if kind == "dense":
        return F @ Z
    M = F.shape[0]
    out = np.empty((M, Z.shape[1]), dtype=np.result_type(F, Z))
    for r0 in range(0, M, 256):
        r1 = min(r0 + 256, M)
        out[r0:r1] = F[r0:r1, :r1] @ Z[:r1] if kind == "lower" else F[r0:r1, r0:] @ Z[r0:]
    return out


def omega_factored(factors, X, Y):
    """max_ij |F1 (F2 (... X)) - Y|_ij / (|F1||F2|...|X| + |Y|)_ij; factors = [(F, kind), ...]. The residual is formed in np.longdouble,
    the denominator (no cancellation) in fp64. Y: the right-hand side, or (Y in np.longdouble, its magnitude bound) where the
    right-hand side is itself a product (qr_lstsq: Q^T y and |Q^T||y|)."""
    Yl, Ya = Y if isinstance(Y, tuple) else (Y.astype(LD), np.abs(Y))
    with np.errstate(all="ignore"):
        Z, A = X.astype(LD), np.abs(X)
        for F, kind in reversed(factors):
            Z, A = _tri_matmul(F.astype(LD), Z, kind), _tri_matmul(np.abs(F), A, kind)
        num, den = np.abs(Z - Yl), (A + Ya).astype(LD)
        q = np.where(den > 0, num / np.where(den > 0, den, 1), np.where(num == 0, 0, np.inf))
        return float(q.max())             # NaN (a non-finite X) fails every `<=` gate


def omega(T, X, Y, upper):
    """componentwise backward error of T X = Y; T already holds zeros outside its triangle (`effective`)"""
    return omega_factored([(T, "upper" if upper else "lower")], X, Y)


def omega_cholesky(L, X, Y):
    L = np.tril(L)
    return omega_factored([(L, "lower"), (np.ascontiguousarray(L.T), "upper")], X, Y)


def omega_ldl(LD_, X, Y):
    L = effective(LD_, False, unit=True)
    return omega_factored([(L, "lower"), (np.diag(LD_).copy(), "diag"), (np.ascontiguousarray(L.T), "upper")], X, Y)


def subst(T, Y, upper):
    """row-by-row substitution with true divisions, in the common dtype of T and Y (np.longdouble operands: 64-bit significands and
    no denormals anywhere near 2^-1074)"""
    M = T.shape[0]
    X = np.array(Y, dtype=np.result_type(T, Y))
    with np.errstate(all="ignore"):
        for i in (range(M - 1, -1, -1) if upper else range(M)):
            if upper and i + 1 < M:
                X[i] -= T[i, i + 1:] @ X[i + 1:]
            if not upper and i > 0:
                X[i] -= T[i, :i] @ X[:i]
            X[i] /= T[i, i]
    return X


def model_one_launch(T, Y, upper):
    """the one-launch algorithm in numpy fp64: per 32-row block b the matrix G of tri_inv_blocks, by substitution column by column
    (the explicit inverses D_k of the four 8 x 8 diagonal sub-blocks, and -D_k E_km beside them), the sub-blocks in the order of the
    substitution, x_k = D_k B_k - sum_m (D_k E_km) x_m over the sub-blocks m already solved; then every row still to be solved
    loses T[rows, b] X_b"""
    M = T.shape[0]
    X = np.array(Y, dtype=np.float64)
    nblk = (M + TB - 1) // TB
    for b in (range(nblk - 1, -1, -1) if upper else range(nblk)):
        r0, r1 = b * TB, min(b * TB + TB, M)
        E, n = T[r0:r1, r0:r1], r1 - r0
        subs = [(s, min(s + SUB, n)) for s in range(0, n, SUB)]
        B, Xb = X[r0:r1].copy(), np.zeros((n, X.shape[1]))
        for s0, s1 in (subs[::-1] if upper else subs):
            rhs = -E[s0:s1].copy()
            rhs[:, s0:s1] = np.eye(s1 - s0)
            G = subst(E[s0:s1, s0:s1], rhs, upper)
            done = slice(s1, n) if upper else slice(0, s0)
            Xb[s0:s1] = G[:, s0:s1] @ B[s0:s1] + G[:, done] @ Xb[done]
        X[r0:r1] = Xb
        if upper and r0 > 0:
            X[:r0] -= T[:r0, r0:r1] @ X[r0:r1]
        if not upper and r1 < M:
            X[r1:] -= T[r1:, r0:r1] @ X[r0:r1]
    return X


def colerr(X, truth):
    """max over the columns in which `truth` is finite of max_i |X - truth| / max_i |truth|, in np.longdouble"""
    with np.errstate(all="ignore"):
        ok = np.isfinite(truth).all(axis=0)
        d = np.abs(X.astype(LD)[:, ok] - truth[:, ok]).max(axis=0)
        return float((d / np.abs(truth[:, ok]).max(axis=0)).max())


def grid20(seed, *shape):
    """uniform [-1, 1) rounded to multiples of 2^-20: a power-of-two scaling stays exact down to 2^-1054"""
    return np.round(rng.matrix(seed, *shape) * 2.0 ** 20) * 2.0 ** -20


def triangle20(seed, M, upper):
    """families.triangle on the 2^-20 grid: off-diagonal / 4, |diag| in [2, 3]"""
    r = grid20(seed, M, M)
    d = np.diag(r) + np.where(np.diag(r) >= 0, 2.0, -2.0)
    t = np.round((np.triu(r, 1) if upper else np.tril(r, -1)) * 2.0 ** 18) * 2.0 ** -20
    return t + np.diag(d)


# ----------------------------------------------------------------------------------------------------------------- guarded call
def _guarded(members, stride, lead):
    """a sentinel-filled host buffer holding `members` (equal shapes) `stride` doubles apart after `lead` doubles; returns
    (buffer, element offset of member 0)"""
    size = members[0].size
    buf = np.full(lead + stride * (len(members) - 1) + size + GUARD, SENTINEL, dtype=np.int64).view(np.float64)
    for m, a in enumerate(members):
        buf[lead + m * stride: lead + m * stride + size] = a.ravel()
    return buf, lead


def call_dtrsm_dev(upper, unit, T, Y, shared_T=False, t_offset=0, stride_t=None):
    """X = op(T)^-1 Y through nd4hip_dtrsm_batched_dev. T [batch or 1, M, M], Y [batch, M, J]; every operand sits in a larger device
    buffer pre-filled with SENTINEL: GUARD doubles before and after it and between batch members (T and Y through a stride larger
    than the operand; X is dense by the ABI). t_offset shifts T by that many doubles (1: no longer 16-byte aligned), stride_t
    overrides T's batch stride (default M*M + GUARD, even for even M). Returns (X [batch, M, J], intact): intact is True when every
    guard region is bit-unchanged and T and Y themselves were not written."""
    import torch
    from nd4js_amd import _lib
    batch, M, J = Y.shape
    T = T.reshape(-1, M, M)
    assert T.shape[0] == (1 if shared_T else batch)
    sT = 0 if shared_T else (M * M + GUARD if stride_t is None else stride_t)
    sY = M * J + GUARD
    tb, t0 = _guarded(list(T), max(sT, 1), GUARD + t_offset)
    yb, y0 = _guarded(list(Y), sY, GUARD)
    n, x0 = batch * M * J, GUARD
    xb = np.full(GUARD + n + GUARD, SENTINEL, dtype=np.int64).view(np.float64)                  # X starts as sentinels too
    Td, Yd, Xd = (torch.from_numpy(b.copy()).cuda() for b in (tb, yb, xb))
    h = _lib.handle(0)
    h.set_stream(torch.cuda.current_stream().cuda_stream)
    _lib.check(h.lib.nd4hip_dtrsm_batched_dev(h.ptr, int(upper), int(unit), batch, M, J, ctypes.c_void_p(Td.data_ptr() + 8 * t0), sT,
                                              ctypes.c_void_p(Yd.data_ptr() + 8 * y0), sY, ctypes.c_void_p(Xd.data_ptr() + 8 * x0)))
    torch.cuda.synchronize()
    ta, ya, xa = (d.cpu().numpy() for d in (Td, Yd, Xd))
    bits = lambda a: a.view(np.int64)
    intact = (np.array_equal(bits(ta), bits(tb)) and np.array_equal(bits(ya), bits(yb))
              and np.array_equal(bits(xa[:x0]), bits(xb[:x0])) and np.array_equal(bits(xa[x0 + n:]), bits(xb[x0 + n:])))
    return xa[x0:x0 + n].reshape(batch, M, J).copy(), bool(intact)
