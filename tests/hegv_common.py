"""Shared by the tests of the Hermitian Cholesky factorisation, the complex triangular solves and the generalised Hermitian-definite
eigenproblem eigen_herm_gen(A, B) (test_hegv_host.py, test_gpu_hegv.py, test_node_hegv.py): the catalogue of inputs, the committed
LAPACK eigenvalues (tools/gen_golden_hegv.py: scipy.linalg.eigh(A, B)), the six bounds, the rows of the C ABI, and the numpy model
of csrc/hegv.hip. That file is compiled without FMA contraction and has no reductions, and every entry sees its operations in the
same order whatever the tier and the block size, so the device returns the model's bits at every N.

What the model restates, on separate real and imaginary float64 arrays (numpy's complex multiply does not enter it). Every entry is a
chain that starts from the matrix entry and subtracts its products one at a time, every multiplication, subtraction, division and
square root rounded on its own, in the order in which the unknowns become known:
  L = chol(H)      l_jj = sqrt(Re h_jj - sum_{k<j} |l_jk|^2),  l_ij = (h_ij - sum_{k<j} l_ik conj(l_jk)) / l_jj         k ascending
  L X = Y          x_ic = (y_ic - sum_{k<i} l_ik x_kc) / l_ii                                                             k ascending
  L^H X = Y        x_ic = (y_ic - sum_{k>i} conj(l_ki) x_kc) / conj(l_ii)                                                 k DESCENDING
  C = L^-1 A L^-H  W = L^-1 A (A the Hermitian mirror of its lower triangle, Im a_ii dropped), C = L^-1 W^H; the lower triangle is kept,
                   Im c_ii = 0
with one order of the four real products, `nmsc` (s - a conj(b): Re (s_re - a_re b_re) - a_im b_im, Im (s_im - a_im b_re) + a_re b_im;
s - a b and s - conj(a) b negate an imaginary part first, which is exact), and one division, `div` (by the real part alone where the
imaginary part of the divisor is zero, else Smith's form). |l_jk|^2 is the same product with a = b. The model is right-looking, as
the kernels are: a finished column or row is subtracted from everything that waits for it, which gives every entry exactly that order.

Bounds, per member, TOL = 1e-12, sigma the singular values of B (numpy) and kappa = sigma_max / sigma_min:
  1 values         |lambda^_i - lambda_i| <= TOL (||A||_F / sigma_min + kappa |lambda_i|)   against the committed LAPACK values
  2 residual       ||A X - B X diag(lambda)||_F <= TOL (||A||_F + ||B||_F max|lambda|) ||X||_F
  3 B-orthonormal  ||X^H B X - I||_F <= TOL kappa sqrt(N)
  4 reduction      ||L C L^H - A||_F <= TOL ||L||_F^2 ||C||_F
  5 factorisation  ||L L^H - H||_F <= TOL ||H||_F
  6 solve          ||H X - Y||_F <= TOL (||H||_F ||X||_F + ||Y||_F)"""
import ctypes
import functools
import os

import numpy as np

import herm_common as hc
from herm_common import TOL, herm, herm_uniform, same_bits  # noqa: F401
from nd4js_amd import _lib, rng

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hegv")
SMALL_MAX = 64                                     # the LDS tier of csrc/hegv.hip
FUSED_MAX = 32                                     # eigen_herm_gen factorises a member's own B inside the reduction kernel up to here
SEED = 9400


# ---- the model -------------------------------------------------------------------------------------------------------------------
def nmsc(sr, si, ar, ai, br, bi):
    """s - a conj(b)"""
    return (sr - ar * br) - ai * bi, (si - ai * br) + ar * bi


def div(xr, xi, dr, di):
    """x / d for a scalar d"""
    if di == 0.0:
        return xr / dr, xi / dr
    if abs(dr) >= abs(di):
        r = di / dr
        den = dr + di * r
        return (xr + xi * r) / den, (xi - xr * r) / den
    r = dr / di
    den = dr * r + di
    return (xr * r + xi) / den, (xi * r - xr) / den


def _parts(M):
    M = np.asarray(M, dtype=np.complex128)
    return np.array(M.real, dtype=np.float64), np.array(M.imag, dtype=np.float64)


def _join(re, im):
    out = np.empty(re.shape, dtype=np.complex128)
    out.real, out.imag = re, im
    return out


def chol_model(H):
    """(L, bad) of one matrix, from its lower triangle; bad: some radicand was not a finite number > 0"""
    Lr, Li = _parts(H)
    N = Lr.shape[0]
    d = np.empty(N)
    bad = False
    with np.errstate(all="ignore"):
        for j in range(N):
            s = Lr[j, j]
            bad = bad or not (np.isfinite(s) and s > 0.0)
            d[j] = np.sqrt(s)
            Lr[j + 1:, j] = Lr[j + 1:, j] / d[j]
            Li[j + 1:, j] = Li[j + 1:, j] / d[j]
            cr, ci = Lr[j + 1:, j], Li[j + 1:, j]
            Lr[j + 1:, j + 1:], Li[j + 1:, j + 1:] = nmsc(Lr[j + 1:, j + 1:], Li[j + 1:, j + 1:], cr[:, None], ci[:, None], cr[None, :], ci[None, :])
    Lr, Li = np.tril(Lr), np.tril(Li, -1)
    Lr[np.arange(N), np.arange(N)] = d
    return _join(Lr, Li), bad


def solve_model(L, Y, adjoint=False):
    """X with L X = Y, or L^H X = Y; L [N, N] lower (only i >= j is read), Y [N, K]"""
    Lr, Li = _parts(L)
    Xr, Xi = _parts(Y)
    N = Lr.shape[0]
    with np.errstate(all="ignore"):
        if not adjoint:
            for i in range(N):
                Xr[i], Xi[i] = div(Xr[i], Xi[i], Lr[i, i], Li[i, i])
                Xr[i + 1:], Xi[i + 1:] = nmsc(Xr[i + 1:], Xi[i + 1:], Lr[i + 1:, i, None], Li[i + 1:, i, None], Xr[i][None, :], -Xi[i][None, :])
        else:
            for i in range(N - 1, -1, -1):
                Xr[i], Xi[i] = div(Xr[i], Xi[i], Lr[i, i], -Li[i, i])
                Xr[:i], Xi[:i] = nmsc(Xr[:i], Xi[:i], Lr[i, :i, None], -Li[i, :i, None], Xr[i][None, :], -Xi[i][None, :])
    return _join(Xr, Xi)


def potrs_model(L, Y):
    return solve_model(L, solve_model(L, Y), True)


def mirror(A):
    """the Hermitian matrix that the lower triangle of A stands for: Im a_ii dropped"""
    A = np.asarray(A, dtype=np.complex128)
    N = A.shape[-1]
    lo = np.tril(A, -1)
    out = lo + np.conj(np.swapaxes(lo, -1, -2))
    out[..., np.arange(N), np.arange(N)] = A[..., np.arange(N), np.arange(N)].real
    return out


def hegst_model(A, L):
    """C = L^-1 A L^-H: lower triangle, zeros above, real diagonal"""
    W = solve_model(L, mirror(A))
    G = solve_model(L, np.conj(W.T))
    C = np.tril(G)
    N = C.shape[0]
    C[np.arange(N), np.arange(N)] = C[np.arange(N), np.arange(N)].real
    return C


def reduce_model(A, B):
    L, bad = chol_model(B)
    return L, hegst_model(A, L), bad


def model(A, B, solver=None):
    """(lambda, X) of one member: reduce_model, `solver` (C -> lambda descending, Y; numpy.linalg.eigh by default), X = L^-H Y. N = 1:
    lambda = Re a / Re b, X = 1 / sqrt(Re b)"""
    if A.shape[-1] == 1:
        return np.array([A[0, 0].real / B[0, 0].real]), np.array([[1.0 / np.sqrt(B[0, 0].real)]], dtype=np.complex128)
    L, C, bad = reduce_model(A, B)
    assert not bad
    if solver is None:
        w, v = np.linalg.eigh(C, UPLO="L")
        lam, Y = w[::-1].copy(), np.ascontiguousarray(v[:, ::-1])
    else:
        lam, Y = solver(C)
    return lam, solve_model(L, Y, True)


# ---- the catalogue ---------------------------------------------------------------------------------------------------------------
def cmatrix(seed, n, k):
    return rng.matrix(seed, n, k) + 1j * rng.matrix(seed + 50000, n, k)


def gram(seed, N):
    """a complex Gram matrix plus the identity"""
    x = cmatrix(seed, N, N)
    return herm(x @ np.conj(x.T) / N + np.eye(N))


def graded(seed, N):
    """U diag(logspace(0, -6, N)) U^H with a unitary reflector U: kappa_2 = 1e6 (N > 1)"""
    v = cmatrix(seed, N, 1)
    U = np.eye(N) - 2.0 * (v @ np.conj(v.T)) / np.vdot(v, v).real
    return herm((U * np.logspace(0.0, -6.0, N)) @ np.conj(U.T))


def diag2(N):
    return np.diag(np.ldexp(1.0, (np.arange(N) * 5) % 13 - 6)).astype(np.complex128)


CAT_N = (1, 2, 3, 17, 33, 64, 65, 97, 130, 193, 300)


def _single(kind, N):
    return lambda: (herm_uniform(SEED + N, N), kind(SEED + (1000 if kind is gram else 2000) + N, N))


CATALOGUE, SIZES = {}, {}
for _N in CAT_N:
    CATALOGUE["gram_%d" % _N], CATALOGUE["graded_%d" % _N] = _single(gram, _N), _single(graded, _N)
    SIZES["gram_%d" % _N] = SIZES["graded_%d" % _N] = _N
CATALOGUE.update({
    "batch_5x40": lambda: (np.stack([herm_uniform(SEED + 3000 + b, 40) for b in range(5)]), np.stack([gram(SEED + 3010 + b, 40) for b in range(5)])),
    "batch_2x130": lambda: (np.stack([herm_uniform(SEED + 3020 + b, 130) for b in range(2)]),
                            np.stack([gram(SEED + 3030, 130), graded(SEED + 3031, 130)])),
    "shared_3x40": lambda: (np.stack([herm_uniform(SEED + 3040 + b, 40) for b in range(3)]), gram(SEED + 3050, 40)),
    "shared_4x17": lambda: (np.stack([herm_uniform(SEED + 3080 + b, 17) for b in range(4)]), graded(SEED + 3090, 17)),
    "shared_2x130": lambda: (np.stack([herm_uniform(SEED + 3060 + b, 130) for b in range(2)]), gram(SEED + 3070, 130)),
})
SIZES.update({"batch_5x40": 40, "batch_2x130": 130, "shared_3x40": 40, "shared_4x17": 17, "shared_2x130": 130})
NAMES = tuple(CATALOGUE)
SINGLES = tuple(n for n in NAMES if n.startswith(("gram_", "graded_")))


def _freeze(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def inputs(name):
    """(A, B) of a catalogue case, Hermitian, read-only, shared by every test"""
    A, B = CATALOGUE[name]()
    A, B = np.ascontiguousarray(A, dtype=np.complex128), np.ascontiguousarray(B, dtype=np.complex128)
    assert np.array_equal(A, np.conj(np.swapaxes(A, -1, -2))) and np.array_equal(B, np.conj(np.swapaxes(B, -1, -2))) and A.shape[-1] == SIZES[name]
    return _freeze(A, B)


def members(A, B):
    """the members as (a [N, N], b [N, N]) pairs; one B serves every member when it is 2-D"""
    N = A.shape[-1]
    return list(zip(A.reshape(-1, N, N), np.broadcast_to(B, A.shape).reshape(-1, N, N)))


@functools.lru_cache(maxsize=None)
def golden(name):
    """the committed LAPACK eigenvalues of a catalogue case, descending, shaped like A.shape[:-1]; read-only"""
    return _freeze(np.load(os.path.join(GOLDEN, name + ".Lam.npy")))[0]


def rhs(name, K):
    """a seeded complex right-hand side [..., N, K] for a catalogue case"""
    A, _ = inputs(name)
    N = A.shape[-1]
    return cmatrix(SEED + 4000 + N + K, int(np.prod(A.shape[:-2], dtype=np.int64)) * N, K).reshape(A.shape[:-1] + (K,))


def with_unread(M, fill=np.nan):
    return hc.with_unread(M, fill)


# ---- the bounds ------------------------------------------------------------------------------------------------------------------
def shares(A, B, lam, X, lam_ref, subset=None):
    """(values, residual, B-orthonormality) as fractions of bounds 1-3, the largest over the members; X may be None. subset=(i0, i1):
    lam and X hold that slice of the descending spectrum"""
    N = A.shape[-1]
    i0, i1 = subset if subset is not None else (0, N)
    k = i1 - i0
    out = [0.0, 0.0, 0.0]
    l2, r2 = lam.reshape(-1, k), lam_ref.reshape(-1, N)[:, i0:i1]
    X3 = None if X is None else X.reshape(-1, N, k)
    for m, (a, b) in enumerate(members(A, B)):
        a, b = mirror(a), mirror(b)
        sv = np.linalg.svd(b, compute_uv=False)
        kappa, na, nb = sv[0] / sv[-1], np.linalg.norm(a), np.linalg.norm(b)
        if k:
            out[0] = max(out[0], (np.abs(l2[m] - r2[m]) / (TOL * (na / sv[-1] + kappa * np.abs(r2[m])))).max())
        if X3 is not None and k:
            x = X3[m]
            out[1] = max(out[1], np.linalg.norm(a @ x - (b @ x) * l2[m]) / (TOL * (na + nb * np.abs(l2[m]).max()) * np.linalg.norm(x)))
            out[2] = max(out[2], np.linalg.norm(np.conj(x.T) @ b @ x - np.eye(k)) / (TOL * kappa * np.sqrt(N)))
    return tuple(out)


def check(A, B, lam, X, lam_ref, what="", subset=None):
    """bounds 1-3; returns the shares"""
    N = A.shape[-1]
    k = N if subset is None else subset[1] - subset[0]
    assert lam.shape == A.shape[:-2] + (k,) and lam.dtype == np.float64, what
    assert np.all(np.isfinite(lam)), what
    assert np.all(np.diff(lam, axis=-1) <= 0), what + ": eigenvalues must be descending"
    if X is not None:
        assert X.shape == A.shape[:-1] + (k,) and X.dtype == np.complex128 and np.all(np.isfinite(X)), what
    sh = shares(A, B, lam, X, lam_ref, subset)
    print("%s: shares of bounds 1-3: %.3g %.3g %.3g" % (what, sh[0], sh[1], sh[2]))
    assert sh[0] <= 1.0, "%s: max|dlambda| is %.3g of its bound" % (what, sh[0])
    assert sh[1] <= 1.0, "%s: ||A X - B X L||_F is %.3g of its bound" % (what, sh[1])
    assert sh[2] <= 1.0, "%s: ||X^H B X - I||_F is %.3g of its bound" % (what, sh[2])
    return sh


def reduction_share(A, L, C):
    """bound 4: ||L C L^H - A||_F / (TOL ||L||_F^2 ||C||_F), the largest over the members; C's lower triangle is mirrored"""
    out = 0.0
    N = A.shape[-1]
    for (a, l), c in zip(members(A, L), C.reshape(-1, N, N)):
        cs = mirror(c)
        out = max(out, np.linalg.norm(l @ cs @ np.conj(l.T) - mirror(a)) / (TOL * np.linalg.norm(l) ** 2 * np.linalg.norm(cs)))
    return out


def chol_share(H, L):
    """bound 5, the largest over the members; L must be lower triangular with a real positive diagonal whose imaginary part is +0"""
    N = H.shape[-1]
    out = 0.0
    for h, l in zip(H.reshape(-1, N, N), L.reshape(-1, N, N)):
        assert not np.triu(l, 1).any() and not np.signbit(np.triu(l, 1).real).any() and not np.signbit(np.triu(l, 1).imag).any()
        dg = np.diagonal(l)
        assert np.all(dg.real > 0.0) and not dg.imag.any() and not np.signbit(dg.imag).any()
        hm = mirror(h)
        out = max(out, np.linalg.norm(l @ np.conj(l.T) - hm) / (TOL * np.linalg.norm(hm)))
    return out


def solve_share(H, X, Y):
    """bound 6, the largest over the members"""
    N, K = H.shape[-1], Y.shape[-1]
    out = 0.0
    Hb = np.broadcast_to(H, Y.shape[:-2] + (N, N)).reshape(-1, N, N)
    for h, x, y in zip(Hb, X.reshape(-1, N, K), Y.reshape(-1, N, K)):
        hm = mirror(h)
        out = max(out, np.linalg.norm(hm @ x - y) / (TOL * (np.linalg.norm(hm) * np.linalg.norm(x) + np.linalg.norm(y))))
    return out


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------
_buf = (ctypes.c_double * 64)()
P = ctypes.cast(_buf, ctypes.c_void_p)
Z = None
SUBSET = ": subset must satisfy 0 <= i0 <= i1 <= N"
# (operation, kind, arguments after the handle, return code, nd4hip_last_error()): every row ends inside the validation, which
# stands before the handle is looked at, so the rows hold with a NULL handle and the buffers are never read. The checks run in the
# family's order: negative extent, subset / selector, N <= 2048, stride, empty call, NULL pointer
ROWS = [
    ("zpotrf_batched", "extent", (-1, 1, P, P), -1, "nd4hip_zpotrf_batched: negative extent"),
    ("zpotrf_batched", "extent", (1, -1, P, P), -1, "nd4hip_zpotrf_batched: negative extent"),
    ("zpotrf_batched", "extent", (1, 2049, P, P), -1, "nd4hip_zpotrf_batched: N <= 2048"),
    ("zpotrf_batched", "extent", (0, 2049, Z, Z), -1, "nd4hip_zpotrf_batched: N <= 2048"),
    ("zpotrf_batched", "empty", (0, 1, Z, Z), 0, None),
    ("zpotrf_batched", "empty", (1, 0, Z, Z), 0, None),
    ("zpotrf_batched", "null", (1, 1, Z, P), -1, "nd4hip_zpotrf_batched: NULL pointer"),
    ("zpotrf_batched", "null", (1, 1, P, Z), -1, "nd4hip_zpotrf_batched: NULL pointer"),
    ("zpotrs_batched", "extent", (-1, 1, 1, P, 1, P, P), -1, "nd4hip_zpotrs_batched: negative extent"),
    ("zpotrs_batched", "extent", (1, 1, -1, P, 1, P, P), -1, "nd4hip_zpotrs_batched: negative extent"),
    ("zpotrs_batched", "extent", (1, 2049, 1, P, 0, P, P), -1, "nd4hip_zpotrs_batched: N <= 2048"),
    ("zpotrs_batched", "stride", (2, 3, 1, P, 8, P, P), -1, "nd4hip_zpotrs_batched: strideL must be N*N or 0"),
    ("zpotrs_batched", "empty", (0, 1, 1, Z, 1, Z, Z), 0, None),
    ("zpotrs_batched", "empty", (1, 3, 0, Z, 0, Z, Z), 0, None),
    ("zpotrs_batched", "null", (1, 1, 1, Z, 1, P, P), -1, "nd4hip_zpotrs_batched: NULL pointer"),
    ("zpotrs_batched", "null", (1, 1, 1, P, 0, P, Z), -1, "nd4hip_zpotrs_batched: NULL pointer"),
    ("zpotrs_batched", "null", (1, 1, 1, P, 0, Z, P), -1, "nd4hip_zpotrs_batched: NULL pointer"),
    ("ztrsm_batched", "extent", (-1, 1, 1, 0, P, 1, P), -1, "nd4hip_ztrsm_batched: negative extent"),
    ("ztrsm_batched", "extent", (1, -1, 1, 0, P, 1, P), -1, "nd4hip_ztrsm_batched: negative extent"),
    ("ztrsm_batched", "extent", (1, 2049, 1, 0, P, 0, P), -1, "nd4hip_ztrsm_batched: N <= 2048"),
    ("ztrsm_batched", "selector", (1, 4, 1, 2, P, 16, P), -1, "nd4hip_ztrsm_batched: adjoint must be 0 or 1"),
    ("ztrsm_batched", "selector", (1, 4, 1, -1, P, 16, P), -1, "nd4hip_ztrsm_batched: adjoint must be 0 or 1"),
    ("ztrsm_batched", "stride", (2, 3, 1, 1, P, 10, P), -1, "nd4hip_ztrsm_batched: strideL must be N*N or 0"),
    ("ztrsm_batched", "empty", (0, 1, 1, 0, Z, 1, Z), 0, None),
    ("ztrsm_batched", "empty", (1, 3, 0, 1, Z, 9, Z), 0, None),
    ("ztrsm_batched", "null", (1, 1, 1, 0, Z, 1, P), -1, "nd4hip_ztrsm_batched: NULL pointer"),
    ("ztrsm_batched", "null", (1, 1, 1, 1, P, 1, Z), -1, "nd4hip_ztrsm_batched: NULL pointer"),
    ("zhegst_batched", "extent", (-1, 1, P, P, 1, P), -1, "nd4hip_zhegst_batched: negative extent"),
    ("zhegst_batched", "extent", (1, 2049, P, P, 0, P), -1, "nd4hip_zhegst_batched: N <= 2048"),
    ("zhegst_batched", "stride", (2, 3, P, P, 3, P), -1, "nd4hip_zhegst_batched: strideL must be N*N or 0"),
    ("zhegst_batched", "empty", (0, 1, Z, Z, 1, Z), 0, None),
    ("zhegst_batched", "empty", (1, 0, Z, Z, 0, Z), 0, None),
    ("zhegst_batched", "null", (1, 1, P, Z, 1, P), -1, "nd4hip_zhegst_batched: NULL pointer"),
    ("zhegst_batched", "null", (1, 1, P, P, 1, Z), -1, "nd4hip_zhegst_batched: NULL pointer"),
    ("zhegvd_batched", "extent", (-1, 1, P, P, 1, P, P), -1, "nd4hip_zhegvd_batched: negative extent"),
    ("zhegvd_batched", "extent", (1, -1, P, P, 1, P, P), -1, "nd4hip_zhegvd_batched: negative extent"),
    ("zhegvd_batched", "extent", (1, 2049, P, P, 0, P, P), -1, "nd4hip_zhegvd_batched: N <= 2048"),
    ("zhegvd_batched", "stride", (2, 3, P, P, 4, P, P), -1, "nd4hip_zhegvd_batched: strideB must be N*N or 0"),
    ("zhegvd_batched", "empty", (0, 1, Z, Z, 1, Z, Z), 0, None),
    ("zhegvd_batched", "empty", (1, 0, Z, Z, 0, Z, Z), 0, None),
    ("zhegvd_batched", "null", (1, 1, Z, P, 1, P, P), -1, "nd4hip_zhegvd_batched: NULL pointer"),
    ("zhegvd_batched", "null", (1, 1, P, Z, 1, P, P), -1, "nd4hip_zhegvd_batched: NULL pointer"),
    ("zhegvd_batched", "null", (1, 1, P, P, 0, Z, P), -1, "nd4hip_zhegvd_batched: NULL pointer"),
    ("zhegvx_batched", "extent", (-1, 1, 0, 1, P, P, 1, P, P), -1, "nd4hip_zhegvx_batched: negative extent"),
    ("zhegvx_batched", "selector", (1, 4, 3, 2, P, P, 16, P, P), -1, "nd4hip_zhegvx_batched" + SUBSET),
    ("zhegvx_batched", "selector", (1, 4, 0, 5, P, P, 16, P, P), -1, "nd4hip_zhegvx_batched" + SUBSET),
    ("zhegvx_batched", "selector", (1, 2049, 0, 2050, P, P, 0, P, P), -1, "nd4hip_zhegvx_batched" + SUBSET),
    ("zhegvx_batched", "extent", (1, 2049, 0, 1, P, P, 0, P, P), -1, "nd4hip_zhegvx_batched: N <= 2048"),
    ("zhegvx_batched", "stride", (2, 3, 0, 1, P, P, 5, P, P), -1, "nd4hip_zhegvx_batched: strideB must be N*N or 0"),
    ("zhegvx_batched", "empty", (0, 1, 0, 1, Z, Z, 1, Z, Z), 0, None),
    ("zhegvx_batched", "empty", (1, 4, 4, 4, Z, Z, 16, Z, Z), 0, None),
    ("zhegvx_batched", "null", (1, 1, 0, 1, Z, P, 1, P, P), -1, "nd4hip_zhegvx_batched: NULL pointer"),
    ("zhegvx_batched", "null", (1, 1, 0, 1, P, P, 1, Z, P), -1, "nd4hip_zhegvx_batched: NULL pointer"),
]
NEW = ("nd4hip_zpotrf_batched", "nd4hip_zpotrs_batched", "nd4hip_ztrsm_batched", "nd4hip_zhegst_batched", "nd4hip_zhegvd_batched",
       "nd4hip_zhegvx_batched")
# a valid call of each operation (arguments after the handle): refused only for the NULL handle
VALID = {"zpotrf_batched": (1, 1, P, P), "zpotrs_batched": (1, 1, 1, P, 1, P, P), "ztrsm_batched": (1, 1, 1, 0, P, 1, P),
         "zhegst_batched": (1, 1, P, P, 1, P), "zhegvd_batched": (1, 1, P, P, 1, P, Z), "zhegvx_batched": (1, 1, 0, 1, P, P, 1, P, Z)}


def mismatches(handle):
    """the rows that a form answers differently, for test_gpu_hegv.py too"""
    lib, bad = _lib.load(), []
    for op, kind, args, rc, text in ROWS:
        for form in ("_host", "_dev"):
            got = getattr(lib, "nd4hip_" + op + form)(handle, *args)
            err = lib.nd4hip_last_error().decode() if got != 0 else None
            if (got, err) != (rc, text):
                bad.append("nd4hip_%s%s%r [%s]: expected %r, got %r" % (op, form, args, kind, (rc, text), (got, err)))
    return bad
