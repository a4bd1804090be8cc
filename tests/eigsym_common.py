"""Shared by the symmetric-eigenproblem tests (test_eigsym_host.py, test_gpu_eigsym.py, test_node_eigsym.py): the catalogue of
inputs, LAPACK's results for them (computed once per input and never modified), the bounds, and a numpy model of the two steps
of csrc/syev.hip that are new arithmetic (the shift-and-Cholesky recurrence and the back-transformation of the values), with
numpy.linalg.svd standing in for the device's bidiagonal solver and a plain Householder tridiagonalisation for hess.hip.

Bounds, with nrm = ||S||_F of the symmetrised input (the project's norm-wise parity bound, README "within 1e-12 norm-wise"):
  max |lambda - lambda_ref|   <= 1e-12 nrm          (the model uses at most 3.9e-15 of nrm)
  ||S V - V diag(lambda)||_F  <= 1e-12 nrm          (model: 1.3e-14)
  ||V^T V - I||_F             <= 1e-12 sqrt(N)      (model: 2.6e-15)
  lambda descending; for eigenvalues isolated by more than 1e-6 nrm the vectors agree with LAPACK's up to sign within 1e-8
  (sensitivity eps nrm / gap <= 2.3e-10 at that gap).
The error of an eigenvalue is absolute, ~ eps nrm: the catalogue's graded case is held to nrm like every other."""
import functools
import json
import os

import numpy as np

from nd4js_amd import rng

EPS = 2.0 ** -52
TOL = 1e-12
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "eigsym")


def sym_uniform(seed, N):
    """the lower triangle of rng.matrix(seed, N, N), mirrored (tools/gen_golden_eigsym.js `symmetric`)"""
    g = rng.matrix(seed, N, N)
    return np.tril(g) + np.tril(g, -1).T


def tridiag(d, e):
    return np.diag(d) + np.diag(e, 1) + np.diag(e, -1)


def reflector(seed, N):
    """the orthogonal Q = I - 2 v v^T / v^T v of a seeded v"""
    v = rng.fill_uniform(seed, N)
    return np.eye(N) - 2.0 * np.outer(v, v) / (v @ v)


def _sym(a):
    return np.tril(a) + np.tril(a, -1).T


def _spectrum(seed, lam):
    q = reflector(seed, len(lam))
    return _sym((q * lam) @ q.T)


def _zdiag_tri(seed, N):
    return tridiag(np.zeros(N), rng.fill_uniform(seed, N - 1))


def _tri_zeros(seed, N):
    e = rng.fill_uniform(seed, N - 1)
    e[[3, 4, N // 2, N - 2]] = 0.0
    return tridiag(rng.fill_uniform(seed + 1, N), e)


def _rank5(seed, N):
    x = rng.matrix(seed, N, 5)
    return _sym(x @ x.T)


def _negdef(seed, N):
    x = rng.matrix(seed, N, N)
    return _sym(-(x @ x.T) - N * np.eye(N))


DENSE_SEED = 7100                                   # dense_N is sym_uniform(DENSE_SEED + N, N), as in tools/gen_golden_eigsym.js
# name -> builder of the input [..., N, N] (symmetric; the tests overwrite the upper triangle themselves)
CATALOGUE = {}
for _N in (1, 2, 3, 33, 70, 127, 128, 255, 256, 300, 1024):     # 1-3: leaves only; 33, 70: first merge levels; 127/128 and 255/256:
    CATALOGUE["dense_%d" % _N] = functools.partial(sym_uniform, DENSE_SEED + _N, _N)   # around the reduction's route changes
CATALOGUE.update({
    "batch_5x40": lambda: np.stack([sym_uniform(7300 + b, 40) for b in range(5)]),
    "batch_2x130": lambda: np.stack([sym_uniform(7310 + b, 130) for b in range(2)]),
    "zdiag_tri_3": lambda: _zdiag_tri(7320, 3),       # +- pairs: an SVD shortcut without the shift returns |lambda|
    "zdiag_tri_64": lambda: _zdiag_tri(7321, 64),
    "clusters_40": lambda: _spectrum(7330, np.repeat([1.0, 2.0], 20)),
    "rank5_50": lambda: _rank5(7340, 50),
    "negdef_33": lambda: _negdef(7350, 33),
    "identity_8": lambda: np.eye(8),
    "zero_8": lambda: np.zeros((8, 8)),
    "tri_zeros_40": lambda: _tri_zeros(7360, 40),
    "graded_60": lambda: _spectrum(7370, 10.0 ** (-np.arange(60) / 10.0)),
    "scaled_p500_40": lambda: np.ldexp(sym_uniform(7300, 40), 500),
    "scaled_m500_40": lambda: np.ldexp(sym_uniform(7300, 40), -500),
})
NAMES = tuple(CATALOGUE)
SMALL = tuple(n for n in NAMES if n != "dense_1024")


def _freeze(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def reference(name):
    """(S, lambda descending, V) of LAPACK (numpy.linalg.eigh); read-only, shared by every test"""
    S = np.ascontiguousarray(CATALOGUE[name](), dtype=np.float64)
    assert np.array_equal(S, np.swapaxes(S, -1, -2))
    w, v = np.linalg.eigh(S)
    return _freeze(S, np.ascontiguousarray(w[..., ::-1]), np.ascontiguousarray(v[..., ::-1]))


def with_upper(S, fill):
    """S with its strict upper triangle replaced by `fill` (a number, NaN included)"""
    out = np.array(S)
    iu = np.triu_indices(S.shape[-1], 1)
    out[..., iu[0], iu[1]] = fill
    return out


def shares(S, lam, V, lam_ref):
    """(values, residual, orthogonality) as fractions of their bounds, the largest over the members"""
    N = S.shape[-1]
    S3, l2, r2 = S.reshape(-1, N, N), lam.reshape(-1, N), lam_ref.reshape(-1, N)
    V3 = None if V is None else V.reshape(-1, N, N)
    out = [0.0, 0.0, 0.0]
    for b in range(S3.shape[0]):
        nrm = max(np.linalg.norm(S3[b]), 1e-300)
        out[0] = max(out[0], np.abs(l2[b] - r2[b]).max() / (TOL * nrm))
        if V3 is not None:
            # (scaled so that the products of a 2^+-500 member neither overflow nor underflow)
            sc = np.ldexp(1.0, -np.frexp(nrm)[1])
            out[1] = max(out[1], np.linalg.norm((S3[b] * sc) @ V3[b] - V3[b] * (l2[b] * sc)) / (TOL * nrm * sc))
            out[2] = max(out[2], np.linalg.norm(V3[b].T @ V3[b] - np.eye(N)) / (TOL * np.sqrt(N)))
    return tuple(out)


def check(S, lam, V, lam_ref, what=""):
    """every bound of the module's docstring but the vectors' agreement; returns the shares"""
    N = S.shape[-1]
    assert lam.shape == S.shape[:-1] and lam.dtype == np.float64, what
    assert np.all(np.isfinite(lam)), what
    assert np.all(np.diff(lam, axis=-1) <= 0), what + ": eigenvalues must be descending"
    if V is not None:
        assert V.shape == S.shape and V.dtype == np.float64 and np.all(np.isfinite(V)), what
    sh = shares(S, lam, V, lam_ref)
    assert sh[0] <= 1.0, "%s: max|dlambda| is %.3g of its bound" % (what, sh[0])
    assert sh[1] <= 1.0, "%s: ||S V - V L||_F is %.3g of its bound" % (what, sh[1])
    assert sh[2] <= 1.0, "%s: ||V^T V - I||_F is %.3g of its bound" % (what, sh[2])
    return sh


def check_vectors(S, V, lam_ref, V_ref, what=""):
    """columns of eigenvalues isolated by more than 1e-6 nrm agree with LAPACK's up to sign within 1e-8; returns how many were compared"""
    N = S.shape[-1]
    count = 0
    for s, v, l, vr in zip(S.reshape(-1, N, N), V.reshape(-1, N, N), lam_ref.reshape(-1, N), V_ref.reshape(-1, N, N)):
        nrm = np.linalg.norm(s)
        gap = np.full(N, np.inf)
        if N > 1:
            d = np.abs(np.diff(l))
            gap[:-1] = d
            gap[1:] = np.minimum(gap[1:], d)
        iso = gap > 1e-6 * nrm
        sign = np.sign(np.einsum("ik,ik->k", v, vr))
        sign[sign == 0] = 1.0
        err = np.abs(v * sign - vr)[:, iso]
        assert err.size == 0 or err.max() <= 1e-8, "%s: vectors differ from LAPACK's by %.3g" % (what, err.max())
        count += int(iso.sum())
    return count


# ---- the numpy model of csrc/syev.hip ---------------------------------------------------------------------------------------
def householder_tridiag(S):
    """(U, d, e) with S = U tridiag(d, e) U^T: plain Householder steps from the last row up, as hessenberg_decomp orders them"""
    A = np.array(S, dtype=np.float64)
    N = A.shape[0]
    U = np.eye(N)
    for i in range(N - 1, 1, -1):
        x = A[i, :i].copy()
        alpha = np.linalg.norm(x)
        if alpha == 0.0 or np.all(x[:-1] == 0.0):
            continue
        v = x
        v[-1] += np.copysign(alpha, x[-1])
        v /= np.linalg.norm(v)
        sub = A[:i, :i]
        p = sub @ v
        w = p - (v @ p) * v
        sub -= 2.0 * (np.outer(v, w) + np.outer(w, v))
        A[i, :i] -= 2.0 * (A[i, :i] @ v) * v
        A[:i, i] = A[i, :i]
        U[:, :i] -= 2.0 * np.outer(U[:, :i] @ v, v)
    return U, np.diag(A).copy(), np.diag(A, -1).copy()


def shift_chol(d, e):
    """step 3 of syev.hip on float64 scalars: (p, q, c, k, smallest radicand), or None for T = 0"""
    N = len(d)
    ea = np.abs(np.concatenate(([0.0], e, [0.0])))
    g = float((np.abs(d) + ea[:-1] + ea[1:]).max())
    if g == 0.0:
        return None
    k = int(np.clip(1 - np.frexp(g)[1], -1022, 1022))
    c = float(np.ldexp(g, k) * (1.0 + 2.0 ** -20))
    ds, es = np.ldexp(d, k), np.ldexp(e, k)
    p, q = np.empty(N), np.empty(max(N - 1, 0))
    rad = ds[0] + c
    low = rad
    for i in range(N):
        low = min(low, rad)
        assert rad > 0.0 and np.isfinite(rad)
        p[i] = np.sqrt(rad)
        if i + 1 < N:
            q[i] = es[i] / p[i]
            rad = (ds[i + 1] + c) - q[i] * q[i]
    return p, q, c, k, low


def model_tridiag(d, e):
    """(lambda descending, rows = eigenvectors of T, smallest radicand): steps 3-5 with numpy.linalg.svd as the solver"""
    N = len(d)
    f = shift_chol(d, e)
    if f is None:
        return np.zeros(N), np.eye(N), 1.0
    p, q, c, k, low = f
    if not np.any(e):                                   # a diagonal T: its d, sorted (the kernel's marked members)
        order = np.argsort(-d, kind="stable")
        return d[order], np.eye(N)[order], low
    _, sv, vt = np.linalg.svd(np.diag(p) + np.diag(q, 1))
    return np.ldexp(sv * sv - c, -k), vt, low


def model(S):
    """the whole route on one symmetric matrix: (lambda, V, smallest radicand)"""
    N = S.shape[0]
    if N == 1:
        return S[0].copy(), np.ones((1, 1)), 1.0
    mx = np.abs(S).max()
    e1 = int(np.frexp(mx)[1]) if mx > 0 and np.isfinite(mx) else 0
    U, d, e = householder_tridiag(np.ldexp(S, -e1))
    lam, vt, low = model_tridiag(d, e)
    return np.ldexp(lam, e1), U @ vt.T, low


# ---- the committed reference values (tools/gen_golden_eigsym.js) ------------------------------------------------------------------
def golden_manifest():
    with open(os.path.join(GOLDEN, "eigsym_manifest.json")) as f:
        return json.load(f)


def golden_input(name, meta):
    """the input of a fixture: regenerated from its seed, or the stored matrix"""
    kind = meta["input"]["kind"]
    if kind == "uniform":
        return sym_uniform(meta["input"]["seed"], meta["N"])
    assert kind == "file"
    return np.load(os.path.join(GOLDEN, meta["files"]["S"]))


def golden_values(name, meta):
    """the reference's eigen(S) eigenvalues as stored (complex128 [N]), or None where the manifest says they were not kept"""
    if "Lam" not in meta["files"]:
        return None
    return np.load(os.path.join(GOLDEN, meta["files"]["Lam"]))
