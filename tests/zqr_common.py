"""The numpy model, inputs and bounds of tests/test_zqr_host.py and tests/test_gpu_zqr.py for zqr_factor / zqr_apply_q / zqr_decomp / zqr_lstsq:
the operation order of the LDS tier of csrc/zgeqrf.hip on a stack [B, M, N], one operation at a time, each rounded on
its own. The model covers members of the LDS tier only (M <= 152: one row of a column's tail per thread)."""
import functools

import numpy as np

import zlu_common as Z

TOL = Z.TOL
HP = np.clongdouble
TINY, LIFT = 2.0 ** -900, 2.0 ** 450
LDS_SHAPES = [(1, 1), (2, 1), (2, 2), (3, 3), (8, 8), (17, 16), (33, 5), (64, 64), (96, 96)]      # 96 x 96: the largest square member in LDS
BLOCKED_SHAPES = [(97, 97), (153, 15), (153, 16), (153, 17), (153, 33), (512, 40), (513, 40), (1024, 20), (1025, 20), (130, 100), (300, 300),
                  (1030, 520)]
BATCHES = [(5, 40, 24), (2, 700, 130), (70000, 4, 4)]


def cmul(ar, ai, br, bi):
    with np.errstate(all="ignore"):
        return ar * br - ai * bi, ar * bi + ai * br


def cmulc(ar, ai, br, bi):                                                  # a conj(b)
    with np.errstate(all="ignore"):
        return ar * br + ai * bi, ai * br - ar * bi


def cdiv_re(ar, ai, br, bi):
    with np.errstate(all="ignore"):
        r = bi / br
        den = br + bi * r
        return (ar + ai * r) / den, (ai - ar * r) / den


def block_sum(x):
    """het_block_sum of x [B, 256]: the xor tree of each wave of 64, then the four waves in order"""
    x, idx = x.reshape(-1, 4, 64), np.arange(64)
    with np.errstate(all="ignore"):
        for off in (32, 16, 8, 4, 2, 1):
            x = x + x[..., idx ^ off]
        w = x[..., 0]
        return ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]


def factor_model(A):
    """(F, tau) of A [B, M, N] or [M, N] in the order of zgeqr2_small"""
    A = np.asarray(A, dtype=np.complex128)
    shape = A.shape
    A = A.reshape((-1,) + shape[-2:])
    B, M, N = A.shape
    assert M <= 152
    re, im = np.array(A.real), np.array(A.imag)
    with np.errstate(all="ignore"):
        mx = np.max(np.maximum(np.abs(re), np.abs(im)).reshape(B, -1), axis=1)
    ok = (mx > 0) & (mx <= Z.DBL_MAX)
    e1 = np.where(ok, np.frexp(np.where(ok, mx, 1.0))[1], 0)              # (np.max passes a NaN on, as the bit pattern does)
    re, im = np.ldexp(re, -e1[:, None, None]), np.ldexp(im, -e1[:, None, None])
    tr_, ti_ = np.zeros((B, N)), np.zeros((B, N))
    CW = 64 if N > 32 else 32 if N > 16 else 16 if N > 8 else 8
    RG = 256 // CW
    for k in range(N):
        n = M - k - 1
        xr, xi, ar, ai = re[:, k + 1:, k], im[:, k + 1:, k], np.array(re[:, k, k]), np.array(im[:, k, k])
        sq, cnt = np.zeros((B, 256)), np.zeros((B, 256))
        with np.errstate(all="ignore"):
            sq[:, :n], cnt[:, :n] = xr * xr + xi * xi, ((xr != 0) | (xi != 0)).astype(float)
            sigma, nz, c = block_sum(sq), block_sum(cnt), np.ones(B)
            for _ in range(2):
                car, cai = c * ar, c * ai
                tiny = ((car * car + cai * cai) + sigma < TINY) & ((nz > 0) | (ar != 0) | (ai != 0))
                c = np.where(tiny, c * LIFT, c)
                cx, cy = c[:, None] * xr, c[:, None] * xi
                sq[:, :n] = cx * cx + cy * cy
                sigma = np.where(tiny, block_sum(sq), sigma)
            on = (sigma > 0) | (ai != 0)
            s, car, cai = np.where(sigma > 0, sigma, 0.0), c * ar, c * ai
            nrm = np.sqrt((car * car + cai * cai) + s) / c
            beta = np.where(ar >= 0, -nrm, nrm)
            tr, ti = np.where(on, (beta - ar) / beta, 0.0), np.where(on, -ai / beta, 0.0)
            beta = np.where(on, beta, ar)
            vr, vi = np.ones((B, n + 1)), np.zeros((B, n + 1))
            vr[:, 1:], vi[:, 1:] = cdiv_re(xr, xi, (ar - beta)[:, None], ai[:, None])
            nc = N - k - 1
            accr, acci = np.zeros((B, RG, nc)), np.zeros((B, RG, nc))
            for r0 in range(0, n + 1, RG):                                  # group q takes the rows k + q, k + q + RG, ..
                g = min(RG, n + 1 - r0)
                pr, pi = cmulc(re[:, k + r0:k + r0 + g, k + 1:], im[:, k + r0:k + r0 + g, k + 1:], vr[:, r0:r0 + g, None], vi[:, r0:r0 + g, None])
                accr[:, :g], acci[:, :g] = accr[:, :g] + pr, acci[:, :g] + pi
            sr, si = accr[:, 0], acci[:, 0]
            for q in range(1, RG):
                sr, si = sr + accr[:, q], si + acci[:, q]
            wr, wi = cmul(tr[:, None], -ti[:, None], sr, si)
            ur, ui = cmul(vr[:, :, None], vi[:, :, None], wr[:, None, :], wi[:, None, :])
            o3 = on[:, None, None]
            re[:, k:, k + 1:], im[:, k:, k + 1:] = np.where(o3, re[:, k:, k + 1:] - ur, re[:, k:, k + 1:]), np.where(o3, im[:, k:, k + 1:] - ui, im[:, k:, k + 1:])
        re[:, k + 1:, k], im[:, k + 1:, k] = np.where(on[:, None], vr[:, 1:], xr), np.where(on[:, None], vi[:, 1:], xi)
        re[:, k, k], im[:, k, k] = beta, 0.0
        tr_[:, k], ti_[:, k] = tr, ti
    up = np.triu(np.ones((M, N), bool))
    re, im = np.where(up, np.ldexp(re, e1[:, None, None]), re), np.where(up, np.ldexp(im, e1[:, None, None]), im)
    return (re + 1j * im).reshape(shape), (tr_ + 1j * ti_).reshape(shape[:-2] + (N,))


def apply_model(F, tau, Zm, adjoint=False):
    """Q Z (adjoint: Q^H Z) in the order of zunmqr_small; F [B, M, N] or one member [M, N] for every member of Z [B, M, K]"""
    Zm = np.asarray(Zm, dtype=np.complex128)
    shape = Zm.shape
    Zm = Zm.reshape((-1,) + shape[-2:])
    F, tau = np.broadcast_to(F, Zm.shape[:1] + F.shape[-2:]), np.broadcast_to(tau, Zm.shape[:1] + tau.shape[-1:])
    M, N = F.shape[-2:]
    zr, zi = np.array(Zm.real), np.array(Zm.imag)
    for k in (range(N) if adjoint else range(N - 1, -1, -1)):
        vr, vi = np.array(F[:, k:, k].real), np.array(F[:, k:, k].imag)
        vr[:, 0], vi[:, 0] = 1.0, 0.0
        tr, ti = tau[:, k].real[:, None], (-tau[:, k].imag if adjoint else tau[:, k].imag)[:, None]
        dr, di = np.zeros(zr[:, 0].shape), np.zeros(zr[:, 0].shape)
        with np.errstate(all="ignore"):
            for i in range(M - k):
                pr, pi = cmulc(zr[:, k + i], zi[:, k + i], vr[:, i, None], vi[:, i, None])
                dr, di = dr + pr, di + pi
            dr, di = cmul(tr, ti, dr, di)
            ur, ui = cmul(vr[:, :, None], vi[:, :, None], dr[:, None, :], di[:, None, :])
            zr[:, k:], zi[:, k:] = zr[:, k:] - ur, zi[:, k:] - ui
    return (zr + 1j * zi).reshape(shape)


def lstsq_model(F, tau, Y):
    """X = R^-1 (Q^H Y)[:N]: apply_model, then the upper half of zlu_common.solve_model"""
    N = F.shape[-1]
    X = apply_model(F, tau, Y, adjoint=True)[..., :N, :]
    shape = X.shape
    X, R = X.reshape((-1,) + shape[-2:]), np.broadcast_to(F[..., :N, :], shape[:-2] + (N, N)).reshape(-1, N, N)
    xr, xi, lr, li = np.array(X.real), np.array(X.imag), R.real, R.imag
    for i in range(N - 1, -1, -1):
        xr[:, i], xi[:, i] = Z.div(xr[:, i], xi[:, i], lr[:, i, i, None], li[:, i, i, None])
        xr[:, :i], xi[:, :i] = Z.nms(xr[:, :i], xi[:, :i], lr[:, :i, i, None], li[:, :i, i, None], xr[:, i, None], xi[:, i, None])
    return (xr + 1j * xi).reshape(shape)


def norm(M):
    return np.sqrt(np.sum(np.abs(np.asarray(M).astype(HP)) ** 2, axis=(-2, -1)))


def ct(M):
    return np.conj(np.swapaxes(M, -1, -2))


def shares_qr(A, Q, R, rows=None, cols=None):
    """the largest shares over the members of the bounds 1 and 2 in clongdouble, and whether bound 3 holds; rows, cols: the 32 of 2048"""
    A, Q, R = np.asarray(A), np.asarray(Q), np.asarray(R)
    N = A.shape[-1]
    rows, cols = (slice(None), slice(None)) if rows is None else (rows, cols)
    Qh, Rh = Q.astype(HP), R.astype(HP)
    s1 = np.max(norm(A[..., rows, :][..., cols].astype(HP) - Qh[..., rows, :] @ Rh[..., cols]) / (TOL * norm(A[..., rows, :][..., cols])))
    Qc = Qh[..., cols]
    s2 = np.max(norm(ct(Qc) @ Qc - np.eye(Qc.shape[-1])) / (TOL * np.sqrt(Qc.shape[-1])))
    d = np.ascontiguousarray(np.diagonal(R, axis1=-2, axis2=-1).imag)
    b3 = not d.view(np.uint64).any() and not np.tril(R, -1).any()
    return float(s1), float(s2), b3 and N == R.shape[-1]


def share_apply(Zm, back):
    """bound 4: Q^H (Q Z) against Z"""
    return float(np.max(norm(np.asarray(back).astype(HP) - np.asarray(Zm).astype(HP)) / (TOL * norm(Zm))))


def share_lstsq(A, X, Y):
    """bound 5: the normal equations; on square members also the residual itself"""
    A, X, Y = (np.asarray(m, dtype=np.complex128).astype(HP) for m in (A, X, Y))
    res = A @ X - Y
    s = np.max(norm(ct(A) @ res) / (TOL * norm(A) * (norm(A) * norm(X) + norm(Y))))
    if A.shape[-1] == A.shape[-2]:
        s = max(s, np.max(norm(res) / (TOL * (norm(A) * norm(X) + norm(Y)))))
    return float(s)


same_bits, cmatrix, name_of = Z.same_bits, Z.cmatrix, Z.name_of


@functools.lru_cache(maxsize=None)
def catalogue(*shape):
    """a seeded input [..., M, N]: Gaussian entries on 4 sqrt(N) times the identity, cond_2 < 10; read-only"""
    A = cmatrix(sum(shape), *shape) + 4.0 * np.sqrt(shape[-1]) * np.eye(*shape[-2:])
    A.setflags(write=False)
    return A


def rhs(A, K, seed=99):
    return cmatrix(seed, *(A.shape[:-1] + (K,)))


def degenerate(M, N):
    """a stack [4, M, N]: healthy; column N // 2 zero; column 1's tail zero with a real alpha; the same with Im alpha != 0 (columns 0 and 1
    are then e_0 and alpha e_1, which the first reflector leaves alone up to the sign of row 0)"""
    S = np.array(np.broadcast_to(catalogue(M, N), (4, M, N)))
    S[1][:, N // 2] = 0.0
    for m, alpha in ((2, 3.0), (3, 3.0 - 2.0j)):
        S[m][:, 0], S[m][:, 1] = 0.0, 0.0
        S[m][0, 0], S[m][1, 1] = 1.0, alpha
    return S
