"""Shared by the tests of the symmetric tridiagonal reduction (test_tridiag_host.py, test_gpu_tridiag.py): a plain numpy model of
the recurrence of csrc/sytrd.hip with its sign rule, the inputs, the three bounds, and the argument rows of the four new C
operations.

The model is not bit-exact: the device's sums are wave reductions whose order the tests do not pin. It fixes the convention
(LAPACK's dsytrd, lower, on row-major members):
  S = Q tridiag(d, e) Q^T, Q = H_0 H_1 ... H_{N-3}, H_k = I - tau_k v_k v_k^T, v_k zero in rows 0..k, 1 in row k+1, tail in F[k+2:, k];
  e_k = -sign(alpha) |x| for the column x = [alpha; tail], sign(0) = +1; a zero tail gives tau_k = 0, e_k = alpha; tau[N-2] = 0.

Bounds (the project's 1e-12 norm-wise gates, as in eigsym_common.py), nrm = ||S||_F of the symmetrised input:
  ||S - Q T Q^T||_F <= 1e-12 nrm,   ||Q^T Q - I||_F <= 1e-12 sqrt(N),   max |lambda(T) - lambda_LAPACK(S)| <= 1e-12 nrm."""
import ctypes
import functools

import numpy as np

import eigsym_common as C
from nd4js_amd import _lib, rng

TOL = 1e-12
SEED = 7700


def sym(S):
    """the lower triangle of S mirrored: what the device reads"""
    S = np.asarray(S, dtype=np.float64)
    return np.tril(S) + np.swapaxes(np.tril(S, -1), -1, -2)


def tridiag(d, e):
    return np.diag(d) + np.diag(e, 1) + np.diag(e, -1)


def exponent(S):
    """e1: the frexp exponent of max|s_ij| over the lower triangle, 0 for the zero matrix"""
    mx = np.abs(np.tril(S)).max() if S.size else 0.0
    return int(np.frexp(mx)[1]) if mx > 0.0 and np.isfinite(mx) else 0


def model(S):
    """(F, tau, d, e) of one symmetric S [N, N] by the recurrence of the module's docstring on 2^-e1 S; d and e get 2^e1 back"""
    S = np.asarray(S, dtype=np.float64)
    N = S.shape[0]
    e1 = exponent(S)
    A = np.ldexp(sym(S), -e1)
    F, tau, e = np.zeros((N, N)), np.zeros(max(N - 1, 0)), np.zeros(max(N - 1, 0))
    for k in range(N - 2):
        alpha, tail = A[k + 1, k], A[k + 2:, k].copy()
        sigma = float(tail @ tail)
        if sigma == 0.0:
            tau[k], e[k] = 0.0, alpha
            continue
        nrm = np.sqrt(alpha * alpha + sigma)
        beta = -nrm if alpha >= 0.0 else nrm
        tau[k], e[k] = (beta - alpha) / beta, beta
        v = np.concatenate(([1.0], tail / (alpha - beta)))
        sub = A[k + 1:, k + 1:]
        p = tau[k] * (sub @ v)
        w = p - (0.5 * tau[k] * (p @ v)) * v
        sub -= np.outer(v, w) + np.outer(w, v)
        F[k + 2:, k] = v[1:]
    if N >= 2:
        e[N - 2] = A[N - 1, N - 2]
    d = np.ldexp(np.diag(A).copy(), e1)
    e = np.ldexp(e, e1)
    F[np.arange(N), np.arange(N)] = d
    F[np.arange(1, N), np.arange(N - 1)] = e
    return F, tau, d, e


def apply_q(F, tau, Z, transpose=False):
    """Q Z or Q^T Z from the stored reflectors, one after the other"""
    N = F.shape[0]
    Z = np.array(Z, dtype=np.float64)
    ks = range(N - 2) if transpose else range(N - 3, -1, -1)
    for k in ks:
        v = np.zeros(N)
        v[k + 1] = 1.0
        v[k + 2:] = F[k + 2:, k]
        Z -= tau[k] * np.outer(v, v @ Z)
    return Z


def form_q(F, tau):
    return apply_q(F, tau, np.eye(F.shape[0]))


def shares(S, Q, d, e, lam_ref=None):
    """(reconstruction, orthogonality, eigenvalues) as fractions of the three bounds for one member; a missing part is 0"""
    N = S.shape[0]
    S = sym(S)
    nrm = max(np.linalg.norm(S), 1e-300)
    sc = np.ldexp(1.0, -np.frexp(nrm)[1])                       # keeps the products of a 2^+-500 member in range
    out = [0.0, 0.0, 0.0]
    if Q is not None:
        T = tridiag(d * sc, e * sc)
        out[0] = np.linalg.norm(S * sc - Q @ T @ Q.T) / (TOL * nrm * sc)
        out[1] = np.linalg.norm(Q.T @ Q - np.eye(N)) / (TOL * np.sqrt(N))
    if lam_ref is not None:
        from scipy.linalg import eigvalsh_tridiagonal
        lam = eigvalsh_tridiagonal(d * sc, e * sc) if N > 1 else d * sc
        out[2] = np.abs(np.sort(lam) - np.sort(lam_ref) * sc).max() / (TOL * nrm * sc)
    return tuple(out)


def check(S, Q, d, e, lam_ref=None, what=""):
    sh = shares(S, Q, d, e, lam_ref)
    assert sh[0] <= 1.0, "%s: ||S - Q T Q^T||_F is %.3g of its bound" % (what, sh[0])
    assert sh[1] <= 1.0, "%s: ||Q^T Q - I||_F is %.3g of its bound" % (what, sh[1])
    assert sh[2] <= 1.0, "%s: max|lambda(T) - lambda(S)| is %.3g of its bound" % (what, sh[2])
    return sh


def check_layout(F, tau, d, e, what=""):
    """F carries d and e on its diagonals and zeros above; tau[N-2] = 0"""
    N = F.shape[-1]
    assert np.array_equal(np.diagonal(F, 0, -2, -1), d), what
    if N > 1:
        assert np.array_equal(np.diagonal(F, -1, -2, -1), e) and not tau[..., N - 2].any(), what
    assert not np.triu(F, 1).any(), what


same_bits = C.same_bits


# ---- inputs -----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def dense(N):
    """(S, eigenvalues of LAPACK ascending); read-only, shared"""
    S = C.sym_uniform(SEED + N, N)
    lam = np.linalg.eigvalsh(S)
    S.setflags(write=False)
    lam.setflags(write=False)
    return S, lam


def block_diagonal(N, cut):
    """two dense blocks, the second starting at row `cut`: column cut-1 has a zero tail in the middle of the run"""
    S = np.zeros((N, N))
    S[:cut, :cut] = C.sym_uniform(SEED + 1000 + N, cut)
    S[cut:, cut:] = C.sym_uniform(SEED + 2000 + N, N - cut)
    return S


def mixed_batch(N, k):
    """five members: dense, diagonal, zero, tridiagonal and 2^k times the dense one"""
    D = np.array(dense(N)[0])
    return np.stack([D, np.diag(C.half_steps(SEED + 3000 + N, N)), np.zeros((N, N)),
                     tridiag(rng.fill_uniform(SEED + 3001 + N, N), rng.fill_uniform(SEED + 3002 + N, N - 1)), np.ldexp(D, k)])


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------
_buf = (ctypes.c_double * 64)()
P = ctypes.cast(_buf, ctypes.c_void_p)
Z = None
SUBSET = ": subset must satisfy 0 <= i0 <= i1 <= N"
# (operation, kind, arguments after the handle, return code, nd4hip_last_error()): every row ends inside the validation, which
# stands before the handle is looked at, so the rows hold with a NULL handle and the buffers are never read
ROWS = [
    ("dsytrd_batched", "extent", (-1, 1, P, P, P, P, P), -1, "nd4hip_dsytrd_batched: negative extent"),
    ("dsytrd_batched", "extent", (1, -1, P, P, P, P, P), -1, "nd4hip_dsytrd_batched: negative extent"),
    ("dsytrd_batched", "extent", (1, 2049, P, P, P, P, P), -1, "nd4hip_dsytrd_batched: N <= 2048"),
    ("dsytrd_batched", "empty", (0, 1, Z, Z, Z, Z, Z), 0, None),
    ("dsytrd_batched", "empty", (1, 0, Z, Z, Z, Z, Z), 0, None),
    ("dsytrd_batched", "null", (1, 1, Z, Z, Z, Z, Z), -1, "nd4hip_dsytrd_batched: NULL pointer"),
    ("dsytrd_batched", "null", (1, 2, P, P, Z, P, P), -1, "nd4hip_dsytrd_batched: NULL pointer"),
    ("dsytrd_batched", "null", (1, 2, P, P, P, P, Z), -1, "nd4hip_dsytrd_batched: NULL pointer"),
    ("dormtr_batched", "extent", (-1, 1, 1, 0, P, P, P), -1, "nd4hip_dormtr_batched: negative extent"),
    ("dormtr_batched", "extent", (1, 1, -1, 0, P, P, P), -1, "nd4hip_dormtr_batched: negative extent"),
    ("dormtr_batched", "extent", (1, 2049, 1, 0, P, P, P), -1, "nd4hip_dormtr_batched: N <= 2048"),
    ("dormtr_batched", "selector", (1, 4, 1, 2, P, P, P), -1, "nd4hip_dormtr_batched: transpose must be 0 or 1"),
    ("dormtr_batched", "selector", (1, 4, 1, -1, P, P, P), -1, "nd4hip_dormtr_batched: transpose must be 0 or 1"),
    ("dormtr_batched", "empty", (0, 1, 1, 0, Z, Z, Z), 0, None),
    ("dormtr_batched", "empty", (1, 3, 0, 1, Z, Z, Z), 0, None),
    ("dormtr_batched", "null", (1, 1, 1, 0, Z, Z, Z), -1, "nd4hip_dormtr_batched: NULL pointer"),
    ("dormtr_batched", "null", (1, 3, 1, 0, P, Z, P), -1, "nd4hip_dormtr_batched: NULL pointer"),
    ("dsyevd_tr_batched", "extent", (-1, 1, P, P, P), -1, "nd4hip_dsyevd_tr_batched: negative extent"),
    ("dsyevd_tr_batched", "extent", (1, -1, P, P, P), -1, "nd4hip_dsyevd_tr_batched: negative extent"),
    ("dsyevd_tr_batched", "extent", (1, 2049, P, P, P), -1, "nd4hip_dsyevd_tr_batched: N <= 2048"),
    ("dsyevd_tr_batched", "empty", (0, 1, Z, Z, Z), 0, None),
    ("dsyevd_tr_batched", "empty", (1, 0, Z, Z, Z), 0, None),
    ("dsyevd_tr_batched", "null", (1, 1, Z, Z, Z), -1, "nd4hip_dsyevd_tr_batched: NULL pointer"),
    ("dsyevd_tr_batched", "null", (1, 1, P, Z, P), -1, "nd4hip_dsyevd_tr_batched: NULL pointer"),
    ("dsyevx_tr_batched", "extent", (-1, 1, 0, 1, P, P, P), -1, "nd4hip_dsyevx_tr_batched: negative extent"),
    ("dsyevx_tr_batched", "extent", (1, -1, 0, 0, P, P, P), -1, "nd4hip_dsyevx_tr_batched: negative extent"),
    ("dsyevx_tr_batched", "selector", (1, 4, 3, 2, P, P, P), -1, "nd4hip_dsyevx_tr_batched" + SUBSET),
    ("dsyevx_tr_batched", "selector", (1, 4, 0, 5, P, P, P), -1, "nd4hip_dsyevx_tr_batched" + SUBSET),
    ("dsyevx_tr_batched", "extent", (1, 2049, 0, 1, P, P, P), -1, "nd4hip_dsyevx_tr_batched: N <= 2048"),
    ("dsyevx_tr_batched", "empty", (0, 1, 0, 1, Z, Z, Z), 0, None),
    ("dsyevx_tr_batched", "empty", (1, 0, 0, 0, Z, Z, Z), 0, None),
    ("dsyevx_tr_batched", "empty", (1, 4, 4, 4, Z, Z, Z), 0, None),
    ("dsyevx_tr_batched", "null", (1, 1, 0, 1, Z, Z, Z), -1, "nd4hip_dsyevx_tr_batched: NULL pointer"),
    ("dsyevx_tr_batched", "null", (1, 1, 0, 1, P, Z, P), -1, "nd4hip_dsyevx_tr_batched: NULL pointer"),
]
NEW = ("nd4hip_dsytrd_batched", "nd4hip_dormtr_batched", "nd4hip_dsyevd_tr_batched", "nd4hip_dsyevx_tr_batched")
# a valid call of each operation (arguments after the handle): refused only for the NULL handle
VALID = {"dsytrd_batched": (1, 1, P, P, Z, P, Z), "dormtr_batched": (1, 1, 1, 0, P, Z, P), "dsyevd_tr_batched": (1, 1, P, P, Z),
         "dsyevx_tr_batched": (1, 1, 0, 1, P, P, Z)}


def mismatches(handle):
    """the rows that a form answers differently, for test_gpu_tridiag.py too"""
    lib, bad = _lib.load(), []
    for op, kind, args, rc, text in ROWS:
        for form in ("_host", "_dev"):
            got = getattr(lib, "nd4hip_" + op + form)(handle, *args)
            err = lib.nd4hip_last_error().decode() if got != 0 else None
            if (got, err) != (rc, text):
                bad.append("nd4hip_%s%s%r [%s]: expected %r, got %r" % (op, form, args, kind, (rc, text), (got, err)))
    return bad
