"""Shared by the tests of the generalised symmetric-definite eigenproblem, eigen_sym_gen(A, B) (test_sygv_host.py, test_gpu_sygv.py,
test_node_sygv.py): the catalogue of inputs, the committed LAPACK eigenvalues (tools/gen_golden_sygv.py: scipy.linalg.eigh(A, B)),
the bounds, and `reduce_model` / `back_model`, a numpy float64 restatement of exactly the arithmetic of the small tier (N <= 64) of
csrc/sygv.hip. That file is compiled without FMA contraction and has no reductions, so the device returns the model's bits.

What the model restates. Every sum starts from the matrix entry and subtracts its products in ascending index k, each
multiplication, subtraction, division and square root rounded on its own; only the lower triangles of A and B are read:
  L = chol(B)      for j = 0 .. N-1:  r = b_jj - sum_{k<j} L_jk L_jk  (the radicand; bad unless finite and > 0),  L_jj = sqrt(r),
                                      L_ij = (b_ij - sum_{k<j} L_ik L_jk) / L_jj   for i > j
  W = L^-1 A       for i = 0 .. N-1:  W_ic = (a_ic - sum_{k<i} L_ik W_kc) / L_ii   (A mirrored from its lower triangle)
  C = L^-1 W^T     for i = 0 .. N-1:  C_ic = (W_ci - sum_{k<i} L_ik C_kc) / L_ii   (every column in full; the lower triangle is kept)
  X = L^-T Y       for i = N-1 .. 0:  X_ic = (Y_ic - sum_{k>i} L_ki X_kc) / L_ii

Bounds, per member, TOL = 1e-12, sigma the singular values of B (numpy) and kappa = sigma_max / sigma_min:
  values         |lambda^_i - lambda_i| <= TOL (||A||_F / sigma_min + kappa |lambda_i|)   against the committed LAPACK values
  residual       ||A X - B X diag(lambda)||_F <= TOL (||A||_F + ||B||_F max|lambda|) ||X||_F
  B-orthonormal  ||X^T B X - I||_F <= TOL kappa sqrt(N)
  reduction      ||L C L^T - A||_F <= TOL ||L||_F^2 ||C||_F
They are the first-order perturbation bounds of the route: chol(B) and the two solves perturb C by eps kappa ||C||, with
||C|| <= ||A|| / sigma_min, and X = L^-T Y inherits kappa from L."""
import functools
import json
import os

import numpy as np

import eigsym_common as ec
from eigsym_common import TOL, reflector, sym_uniform, with_upper  # noqa: F401 (with_upper: for the tests)
from nd4js_amd import rng

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sygv")
SMALL_MAX = 64                                     # the fused tier of csrc/sygv.hip


# ---- the model -------------------------------------------------------------------------------------------------------------------
def chol_model(B):
    """(L, bad) of one matrix; bad: some radicand was not a finite number > 0"""
    B = np.asarray(B, dtype=np.float64)
    N = B.shape[0]
    L = np.zeros((N, N))
    bad = False
    with np.errstate(all="ignore"):
        for j in range(N):
            t = B[j:, j].copy()
            for k in range(j):
                t = t - L[j:, k] * L[j, k]
            bad = bad or not (np.isfinite(t[0]) and t[0] > 0.0)
            d = np.sqrt(t[0])
            L[j, j] = d
            L[j + 1:, j] = t[1:] / d
    return L, bad


def sygst_model(A, L):
    """C = L^-1 A L^-T, lower triangle and zeros above, from the lower triangle of A"""
    A = np.asarray(A, dtype=np.float64)
    N = A.shape[0]
    Am = np.tril(A) + np.tril(A, -1).T
    W, G = np.empty((N, N)), np.empty((N, N))
    with np.errstate(all="ignore"):
        for i in range(N):
            t = Am[i, :].copy()
            for k in range(i):
                t = t - L[i, k] * W[k, :]
            W[i, :] = t / L[i, i]
        for i in range(N):
            t = W[:, i].copy()
            for k in range(i):
                t = t - L[i, k] * G[k, :]
            G[i, :] = t / L[i, i]
    return np.tril(G)


def reduce_model(A, B):
    """(L, C, bad): the kernel sygv_reduce_small"""
    L, bad = chol_model(B)
    return L, sygst_model(A, L), bad


def back_model(L, Y):
    """X = L^-T Y: the kernel sygv_back_small"""
    N = L.shape[0]
    X = np.empty((N, N))
    with np.errstate(all="ignore"):
        for i in range(N - 1, -1, -1):
            t = Y[i, :].copy()
            for k in range(i + 1, N):
                t = t - L[k, i] * X[k, :]
            X[i, :] = t / L[i, i]
    return X


def model(A, B, solver=None):
    """(lambda, X) of one member: reduce_model, `solver` (C -> lambda descending, Y; numpy.linalg.eigh by default), back_model"""
    L, C, bad = reduce_model(A, B)
    assert not bad
    if solver is None:
        w, v = np.linalg.eigh(C, UPLO="L")
        lam, Y = w[::-1].copy(), np.ascontiguousarray(v[:, ::-1])
    else:
        lam, Y = solver(C)
    return lam, back_model(L, Y)


# ---- the catalogue ---------------------------------------------------------------------------------------------------------------
def gram(seed, N):
    x = rng.matrix(seed, N, N)
    return ec._sym(x @ x.T / N + np.eye(N))


def graded(seed, N):
    """Q diag(logspace(0, -6, N)) Q^T, kappa_2 = 1e6 (N > 1)"""
    q = reflector(seed, N)
    return ec._sym((q * np.logspace(0.0, -6.0, N)) @ q.T)


def diag2(N):
    return np.diag(np.ldexp(1.0, (np.arange(N) * 5) % 13 - 6))


SMALL_N = (1, 2, 3, 33, 64)
LARGE_N = (65, 130, 300)
def _single(kind, N):
    return lambda: (sym_uniform(8100 + N, N), kind(8500 + N if kind is gram else 8900 + N, N))


def _lead64():
    A, B = CATALOGUE["gram_65"]()
    return np.ascontiguousarray(A[:64, :64]), np.ascontiguousarray(B[:64, :64])


# name -> builder of (A [..., N, N], B [..., N, N] or [N, N]); SIZES: name -> N, known without building anything
CATALOGUE, SIZES = {}, {}
for _N in SMALL_N + LARGE_N:
    CATALOGUE["gram_%d" % _N], CATALOGUE["graded_%d" % _N] = _single(gram, _N), _single(graded, _N)
    SIZES["gram_%d" % _N] = SIZES["graded_%d" % _N] = _N
CATALOGUE.update({
    "gram_65_lead64": _lead64,                       # the tier edge: the leading 64 x 64 blocks of gram_65
    "diag2_33": lambda: (sym_uniform(8133, 33), diag2(33)),
    "eye_33": lambda: (sym_uniform(8133, 33), np.eye(33)),
    "diag2_130": lambda: (sym_uniform(8230, 130), diag2(130)),
    "batch_5x40": lambda: (np.stack([sym_uniform(8300 + b, 40) for b in range(5)]), np.stack([gram(8310 + b, 40) for b in range(5)])),
    "batch_2x130": lambda: (np.stack([sym_uniform(8320 + b, 130) for b in range(2)]),
                            np.stack([gram(8330, 130), graded(8331, 130)])),
    "shared_3x40": lambda: (np.stack([sym_uniform(8340 + b, 40) for b in range(3)]), gram(8350, 40)),
})
SIZES.update({"gram_65_lead64": 64, "diag2_33": 33, "eye_33": 33, "diag2_130": 130, "batch_5x40": 40, "batch_2x130": 130, "shared_3x40": 40})
NAMES = tuple(CATALOGUE)
SMALL_NAMES = tuple(n for n in NAMES if SIZES[n] <= SMALL_MAX)


@functools.lru_cache(maxsize=None)
def inputs(name):
    """(A, B) of a catalogue case, symmetric, read-only, shared by every test"""
    A, B = CATALOGUE[name]()
    A, B = np.ascontiguousarray(A, dtype=np.float64), np.ascontiguousarray(B, dtype=np.float64)
    assert np.array_equal(A, np.swapaxes(A, -1, -2)) and np.array_equal(B, np.swapaxes(B, -1, -2)) and A.shape[-1] == SIZES[name]
    return ec._freeze(A, B)


def members(A, B):
    """the members as (a [N, N], b [N, N]) pairs; one B serves every member when it is 2-D"""
    N = A.shape[-1]
    A3 = A.reshape(-1, N, N)
    B3 = np.broadcast_to(B, A.shape).reshape(-1, N, N)
    return list(zip(A3, B3))


@functools.lru_cache(maxsize=None)
def manifest():
    with open(os.path.join(GOLDEN, "manifest.json")) as f:
        return json.load(f)


@functools.lru_cache(maxsize=None)
def golden(name):
    """the committed LAPACK eigenvalues of a catalogue case, descending, shaped like A.shape[:-1]; read-only"""
    return ec._freeze(np.load(os.path.join(GOLDEN, name + ".Lam.npy")))[0]


# ---- the bounds ------------------------------------------------------------------------------------------------------------------
def shares(A, B, lam, X, lam_ref):
    """(values, residual, B-orthonormality) as fractions of their bounds, the largest over the members; X may be None"""
    N = A.shape[-1]
    out = [0.0, 0.0, 0.0]
    l2, r2 = lam.reshape(-1, N), lam_ref.reshape(-1, N)
    X3 = None if X is None else X.reshape(-1, N, N)
    for m, (a, b) in enumerate(members(A, B)):
        sv = np.linalg.svd(b, compute_uv=False)
        kappa, na, nb = sv[0] / sv[-1], np.linalg.norm(a), np.linalg.norm(b)
        if N:
            out[0] = max(out[0], (np.abs(l2[m] - r2[m]) / (TOL * (na / sv[-1] + kappa * np.abs(r2[m])))).max())
        if X3 is not None and N:
            x = X3[m]
            out[1] = max(out[1], np.linalg.norm(a @ x - (b @ x) * l2[m]) / (TOL * (na + nb * np.abs(l2[m]).max()) * np.linalg.norm(x)))
            out[2] = max(out[2], np.linalg.norm(x.T @ b @ x - np.eye(N)) / (TOL * kappa * np.sqrt(N)))
    return tuple(out)


def check(A, B, lam, X, lam_ref, what=""):
    """every bound of the module's docstring but the reduction's; returns the shares"""
    assert lam.shape == A.shape[:-1] and lam.dtype == np.float64, what
    assert np.all(np.isfinite(lam)), what
    assert np.all(np.diff(lam, axis=-1) <= 0), what + ": eigenvalues must be descending"
    if X is not None:
        assert X.shape == A.shape and X.dtype == np.float64 and np.all(np.isfinite(X)), what
    sh = shares(A, B, lam, X, lam_ref)
    assert sh[0] <= 1.0, "%s: max|dlambda| is %.3g of its bound" % (what, sh[0])
    assert sh[1] <= 1.0, "%s: ||A X - B X L||_F is %.3g of its bound" % (what, sh[1])
    assert sh[2] <= 1.0, "%s: ||X^T B X - I||_F is %.3g of its bound" % (what, sh[2])
    return sh


def reduction_share(A, L, C):
    """||L C L^T - A||_F / (TOL ||L||_F^2 ||C||_F), the largest over the members; C's lower triangle is mirrored"""
    N = A.shape[-1]
    out = 0.0
    for (a, l), c in zip(members(A, L), C.reshape(-1, N, N)):
        cs = np.tril(c) + np.tril(c, -1).T
        out = max(out, np.linalg.norm(l @ cs @ l.T - a) / (TOL * np.linalg.norm(l) ** 2 * np.linalg.norm(cs)))
    return out


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()
