"""Shared by the eigvec tests: the golden manifest of tests/golden/eigvec, and restatements in plain Python / numpy of the
reference's schur_eigenvals, of schur_eigen's back-substitution (schur.js:170-363) and of one eigen_balance_pre sweep
(eigen.js:113-162, :189-219). `exact=True` runs float64 in the reference's operation order; `exact=False` runs numpy.longdouble
(with vectorised sums) and is the yardstick `e_ref` of how far the reference itself is from the exact back-substitution."""
import json
import math
import os

import numpy as np

from conftest import GOLDEN

DIR = os.path.join(GOLDEN, "eigvec")
EPS = 2.0 ** -52
SIZE_LIMIT = 1 << 20


def manifest():
    with open(os.path.join(DIR, "manifest.json")) as f:
        return json.load(f)


_M = manifest()
CASES = _M["cases"]


def load(name, key):
    return np.load(os.path.join(DIR, CASES[name]["files"][key]))


def names(pred):
    return sorted(k for k, v in CASES.items() if pred(k, v))


SCHUR = names(lambda k, v: "VI" in v["files"])                       # schur_eigen cases with outputs (all have T, Lam, VI)
SCHUR_DENSE = [k for k in SCHUR if "VQ" in CASES[k]["files"]]
BAL = names(lambda k, v: "B" in v["files"])
POST = names(lambda k, v: "W" in v["files"])


def mats(a, n):
    """[..., n, n] -> list of the batch members"""
    return list(a.reshape((-1, n, n)))


# ------------------------------------------------------------------------------------------------ schur_eigenvals
def eigenvals_ref(T):
    """schur.js:52-83 on one matrix: (Lam complex128 [N], block type per row: 0 = 1x1, 1 / 2 = first / second row of a 2x2 block)"""
    N = T.shape[0]
    lam, blk = np.zeros(N, dtype=np.complex128), [0] * N
    j = N - 1
    while j >= 0:
        i = j - 1
        if j == 0 or T[j, i] == 0:
            lam[j] = T[j, j]
        else:
            Tii, Tij, Tji, Tjj = (float(x) for x in (T[i, i], T[i, j], T[j, i], T[j, j]))
            diag, tr = Tii - Tjj, Tii + Tjj
            sqr = diag * diag + (4 * Tij) * Tji
            if sqr >= 0:
                raise ValueError("schur_eigenvals(T): T must not contain real eigenvalued 2x2 blocks.")
            s, half = 0.5 * math.sqrt((abs(sqr) - sqr) * 0.5), 0.5 * tr
            lam[i], lam[j] = complex(half, s), complex(half, 0.0 - s)
            blk[i], blk[j] = 1, 2
            j -= 1
        j -= 1
    return lam, blk


# ------------------------------------------------------------------------------------------------ schur_eigen without Q
def _cdiv(xr, xi, re, im):
    if im == 0:
        return xr / re, xi / re
    if abs(re) >= abs(im):
        R = im / re
        return (xr + xi * R) / (re + im * R), (xi - xr * R) / (re + im * R)
    R = re / im
    return (xr * R + xi) / (re * R + im), (xi * R - xr) / (re * R + im)


def eigvecs_ref(T, exact=True):
    """(Lam, X): X [N, N] the unit-norm eigenvectors of the quasi-triangular T as schur_eigen computes them before Q is applied.
    exact: float64 (Python floats) in the reference's order, complex128 result with the reference's bits. Otherwise longdouble:
    (Lam, Xre, Xim) with longdouble arrays."""
    N = T.shape[0]
    lam, blk = eigenvals_ref(T)
    if exact:
        F, hyp, sqrt = float, math.hypot, math.sqrt
        t = T.tolist()
    else:
        F, hyp, sqrt = np.longdouble, np.hypot, np.sqrt
        t = T.astype(np.longdouble)
    zero, one = F(0.0), F(1.0)
    # TOL (schur.js:254-269)
    s, mx = zero, zero
    for row in t:
        for x in row:
            e = abs(x)
            if e != 0:
                if e > mx:
                    s *= (mx / e) * (mx / e)
                    mx = e
                s += (e / mx) * (e / mx)
    TOL = F(math.sqrt(EPS)) * (sqrt(s) * mx)
    assert TOL >= 0
    Xr = [[zero] * N for _ in range(N)] if exact else np.zeros((N, N), dtype=np.longdouble)
    Xi = [[zero] * N for _ in range(N)] if exact else np.zeros((N, N), dtype=np.longdouble)

    def acc(vr, vi, row, j, K):
        if exact:
            tr_, re, im = t[row], vr[row], vi[row]
            for k in range(K - 1, j, -1):
                re0, im0, re1, im1 = vr[k], vi[k], tr_[k], 0.0
                re -= re0 * re1 - im0 * im1
                im -= re0 * im1 + im0 * re1
            vr[row], vi[row] = re, im
        else:
            vr[row] -= np.dot(t[row, j + 1:K], vr[j + 1:K])
            vi[row] -= np.dot(t[row, j + 1:K], vi[j + 1:K])

    def compute(lr, li, vr, vi, J, K):
        j = J - 1
        while j >= 0:
            acc(vr, vi, j, j, K)
            if j == 0 or t[j][j - 1] == 0:
                dre, dim = t[j][j] - lr, zero - li
                if hyp(dre, dim) <= TOL:
                    if hyp(vr[j], vi[j]) <= TOL:
                        vr[j], vi[j] = zero, zero
                    else:
                        vr[j], vi[j] = one, zero
                        for k in range(j + 1, K):
                            vr[k], vi[k] = zero, zero
                else:
                    vr[j], vi[j] = _cdiv(vr[j], vi[j], dre, dim)
            else:
                i = j - 1
                acc(vr, vi, i, j, K)
                ar, ai = t[i][i] - lr, zero - li              # T_ii - lambda
                br, bi = t[j][j] - lr, zero - li              # T_jj - lambda
                ij, ji = t[i][j], t[j][i]
                dr, di = ar * br - ai * bi, ar * bi + ai * br
                dr -= ij * ji - zero * zero
                di -= ij * zero + zero * ji
                assert not (dr == 0 and di == 0)
                xjr, xji, xir, xii = vr[j], vi[j], vr[i], vi[i]
                njr, nji = ar * xjr - ai * xji, ar * xji + ai * xjr
                njr -= ji * xir - zero * xii
                nji -= ji * xii + zero * xir
                njr, nji = _cdiv(njr, nji, dr, di)
                nir, nii = br * xir - bi * xii, br * xii + bi * xir
                nir -= ij * xjr - zero * xji
                nii -= ij * xji + zero * xjr
                nir, nii = _cdiv(nir, nii, dr, di)
                vr[i], vi[i], vr[j], vi[j] = nir, nii, njr, nji
                j -= 1
            j -= 1

    for c in range(N):
        vr = [zero] * N if exact else np.zeros(N, dtype=np.longdouble)
        vi = [zero] * N if exact else np.zeros(N, dtype=np.longdouble)
        lr, li = F(lam[c].real), F(lam[c].imag)
        if blk[c] == 0:
            vr[c] = one
            compute(lr, li, vr, vi, c, c + 1)
        else:
            i = c if blk[c] == 1 else c - 1
            j = i + 1
            if abs(t[i][j]) >= abs(t[j][i]):
                vr[i], vr[j], vi[j] = t[i][j], lr - t[i][i], li
            else:
                vr[j], vr[i], vi[i] = t[j][i], lr - t[j][j], li
            compute(lr, li, vr, vi, i, j + 1)
        # column norm (schur.js:338-363) and normalisation
        s, mx = zero, zero
        for r in range(N):
            for a in (abs(vr[r]), abs(vi[r])):
                if a > 0:
                    if a > mx:
                        scale = mx / a
                        mx = a
                        s *= scale * scale
                    ratio = a / mx
                    s += ratio * ratio
        nrm = sqrt(s) * mx
        for r in range(N):
            Xr[r][c], Xi[r][c] = vr[r] / nrm, vi[r] / nrm
    if exact:
        return lam, np.array(Xr) + 1j * np.array(Xi)
    return lam, Xr, Xi


def e_ref(T, Q, V_ref):
    """the reference's own distance max|V_ref - Q X| from the longdouble back-substitution X of the same T"""
    _, Xr, Xi = eigvecs_ref(T, exact=False)
    Ql = Q.astype(np.longdouble)
    return float(max(np.abs(V_ref.real - Ql @ Xr).max(), np.abs(V_ref.imag - Ql @ Xi).max()))


def residual(Q, T, lam, V):
    """max over the columns of ||(Q T Q^T) v - lambda v||_2 / (||T||_F ||v||_2)"""
    R = Q @ (T @ (Q.T @ V)) - V * lam[None, :]
    return float((np.linalg.norm(R, axis=0) / (np.linalg.norm(T) * np.linalg.norm(V, axis=0))).max())


def col_norm_error(V):
    """max over the columns of | scaled 2-norm - 1 |"""
    P = np.abs(np.concatenate([V.real, V.imag], axis=0))
    m = P.max(axis=0)
    return float(np.abs(np.sqrt(((P / m) ** 2).sum(axis=0)) * m - 1.0).max())


# ------------------------------------------------------------------------------------------------ eigen_balance_pre
def balance_sweep_changes(B, p):
    """one more sweep of the reference (eigen.js:113-162, :189-219 for p = inf) over B: the rows it would still rescale"""
    N = B.shape[0]
    A = [list(map(float, r)) for r in B]
    inf = p == float("inf")
    TOL = 1.0 if inf else 0.95 ** (1.0 / p)
    out = []
    for i in range(N):
        r = c = r_max = c_max = 0.0
        for j in range(N):
            if i == j:
                continue
            a, b = abs(A[i][j]), abs(A[j][i])
            if inf:
                r, c = max(r, a), max(c, b)
                continue
            if a > 0:
                if a > r_max:
                    r *= (r_max / a) ** p
                    r_max = a
                r += (a / r_max) ** p
            if b > 0:
                if b > c_max:
                    c *= (c_max / b) ** p
                    c_max = b
                c += (b / c_max) ** p
        if not inf:
            r, c = r ** (1.0 / p) * r_max, c ** (1.0 / p) * c_max
        if r * c == 0.0:
            continue
        norm = (lambda r, c: max(r, c)) if inf else (lambda r, c: (1 + (r / c) ** p) ** (1.0 / p) * c if c >= r else (1 + (c / r) ** p) ** (1.0 / p) * r)
        old, scale = norm(r, c), 1.0
        while r >= c * 2:
            c *= 2; r /= 2; scale *= 2
        while c >= r * 2:
            c /= 2; r *= 2; scale /= 2
        if norm(r, c) >= TOL * old:
            continue
        out.append(i)
        for j in range(N):
            A[i][j] /= scale
            A[j][i] *= scale
    return out


def p_of(case):
    p = CASES[case]["p"]
    return float("inf") if p == "Infinity" else float("nan") if p == "NaN" else float(p)
