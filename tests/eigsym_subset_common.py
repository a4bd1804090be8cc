"""Shared by the tests of the selected-eigenpair route (test_eigsym_subset_host.py, test_gpu_eigsym_subset.py,
test_node_eigsym_subset.py): a numpy model of csrc/syevx.hip, operation by operation, and the inputs.

prepare, count, bisect and clusters use + - * / and comparisons only, each rounded once, in the kernels' order: the device
returns the model's bits for counts, eigenvalues, cluster heads and perturbed shifts. factor_solve and orth are the same
arithmetic with numpy's sums in place of the kernels' fixed-order tree reductions: those are held to bounds, not bits.

Bounds (eigsym_common: TOL = 1e-12), nrm = ||T||_F or ||S||_F, k the number of selected pairs:
  max |lambda - lambda_ref| <= TOL nrm;  ||T Z - Z diag(lambda)||_F <= TOL nrm;  ||Z^T Z - I||_F <= TOL sqrt(k)."""
import ctypes
import functools

import numpy as np

from eigsym_common import CATALOGUE, EPS, SMALL, TOL, check, householder_tridiag, shares, sym_uniform, tridiag  # noqa: F401
from nd4js_amd import _lib, rng

PIVMIN = 2.0 ** -1022
MAXIT = 128
SEED = 20480
CTOL = 1e-3                                                    # cluster: gap <= CTOL g
PERT = 10.0 * EPS                                              # shifts of a cluster at least PERT g apart


# ---- step 1 ------------------------------------------------------------------------------------------------------------------------
def prepare(d, e):
    """stx_prepare on one member: dict(ds, es, e2 [N] with es[N-1] = e2[N-1] = 0, g, lexp, diag)"""
    d, e = np.asarray(d, dtype=np.float64), np.asarray(e, dtype=np.float64)
    N = len(d)
    assert len(e) == N - 1 and np.all(np.isfinite(d)) and np.all(np.isfinite(e))
    mx = max(np.abs(d).max(), np.abs(e).max() if N > 1 else 0.0)
    mm = int(np.frexp(mx)[1]) if mx > 0.0 else 0
    ds = np.ldexp(d, -mm)
    es = np.concatenate((np.ldexp(e, -mm), [0.0]))
    ep = np.concatenate(([0.0], es[:-1]))
    g = float(((np.abs(ds) + np.abs(ep)) + np.abs(es)).max())
    return {"ds": ds, "es": es, "e2": es * es, "g": g, "lexp": mm, "diag": not np.any(es), "N": N}


# ---- step 2 ------------------------------------------------------------------------------------------------------------------------
def negatives(p, xs):
    """#{i: q_i < 0} for every scaled probe of xs"""
    xs = np.asarray(xs, dtype=np.float64)
    ds, e2 = p["ds"], p["e2"]
    with np.errstate(all="ignore"):
        q = ds[0] - xs
        q = np.where(np.abs(q) < PIVMIN, -PIVMIN, q)
        c = (q < 0.0).astype(np.int32)
        for i in range(1, p["N"]):
            q = (ds[i] - xs) - e2[i - 1] / q
            q = np.where(np.abs(q) < PIVMIN, -PIVMIN, q)
            c += q < 0.0
    return c


def count(d, e, x):
    """tridiag_count on one member: int32, #{lambda > x}"""
    p = prepare(d, e)
    with np.errstate(all="ignore"):
        xs = np.ldexp(np.asarray(x, dtype=np.float64), -p["lexp"])
    return (p["N"] - negatives(p, xs)).astype(np.int32)


# ---- step 3 ------------------------------------------------------------------------------------------------------------------------
def bisect(p, i0, i1):
    """(scaled values, values, most halvings of any lane) for the indices i0 .. i1 - 1 of the descending spectrum"""
    N, g = p["N"], p["g"]
    if p["diag"]:
        order = np.argsort(-p["ds"], kind="stable")[i0:i1]
        return p["ds"][order], np.ldexp(p["ds"][order], p["lexp"]), 0
    j = np.arange(i0, i1)
    hi = np.full(len(j), g * (1.0 + 2.0 ** -20))
    lo = -hi
    active = np.ones(len(j), dtype=bool)
    halvings = np.zeros(len(j), dtype=np.int64)
    for _ in range(MAXIT):
        mid = 0.5 * (lo + hi)
        stop = (hi - lo <= (2.0 * EPS) * np.maximum(np.abs(lo), np.abs(hi)) + EPS * g) | (mid == lo) | (mid == hi)
        active &= ~stop
        if not active.any():
            break
        more = N - negatives(p, mid) > j
        lo = np.where(active & more, mid, lo)
        hi = np.where(active & ~more, mid, hi)
        halvings += active
    v = 0.5 * (lo + hi)
    return v, np.ldexp(v, p["lexp"]), int(halvings.max())


# ---- step 4 ------------------------------------------------------------------------------------------------------------------------
def clusters(lams, g):
    """(head int32 [k], shift [k]) of stx_clusters"""
    k = len(lams)
    head, shift = np.zeros(k, dtype=np.int32), np.array(lams, dtype=np.float64)
    ctol, pert = CTOL * g, PERT * g
    cur, prev = 0, shift[0]
    for j in range(1, k):
        s = lams[j]
        if lams[j - 1] - s > ctol:
            cur = j
        elif prev - s < pert:
            s = prev - pert
        head[j], shift[j], prev = cur, s, s
    return head, shift


# ---- steps 5 and 6 -----------------------------------------------------------------------------------------------------------------
def start_vectors(N, i0, i1):
    """[k, N]: row jj is u(SEED, (i0 + jj) N + i)"""
    return rng.fill_uniform(SEED, (i1 - i0) * N, offset=i0 * N).reshape(i1 - i0, N)


def _guard(p, tiny):
    return np.where(np.abs(p) < tiny, np.copysign(tiny, p), p)


def factor_solve(p, shift, Z):
    """stx_factor_solve for all k vectors at once: rows of Z [k, N] -> the solutions of (T - shift_j) x = scale_j z_j"""
    N, g, D, E = p["N"], p["g"], p["ds"], p["es"]
    tiny = EPS * g
    zmax = np.abs(Z).max(axis=1)
    ok = (zmax > 0.0) & np.isfinite(zmax)
    scale = np.where(ok, ((N * g) * EPS) / np.where(ok, zmax, 1.0), 1.0)
    src = Z * scale[:, None]
    k = len(shift)
    u0, u1, u2, y = (np.zeros((N, k)) for _ in range(4))
    pv, sup, yi = D[0] - shift, np.full(k, E[0] if N > 1 else 0.0), src[:, 0].copy()
    with np.errstate(all="ignore"):
        for i in range(N - 1):
            l, dd, ee, zn = E[i], D[i + 1] - shift, (E[i + 1] if i + 2 < N else 0.0), src[:, i + 1]
            keep = np.abs(pv) >= abs(l)
            piv = _guard(np.where(keep, pv, l), tiny)
            mult = np.where(keep, l, pv) / piv
            u0[i], u1[i], u2[i], y[i] = piv, np.where(keep, sup, dd), np.where(keep, 0.0, ee), np.where(keep, yi, zn)
            pv, sup, yi = (np.where(keep, dd - mult * sup, sup - mult * dd), np.where(keep, ee, -(mult * ee)),
                           np.where(keep, zn - mult * yi, yi - mult * zn))
        X = np.empty((k, N))
        x1, x2 = yi / _guard(pv, tiny), np.zeros(k)
        X[:, N - 1] = x1
        for i in range(N - 2, -1, -1):
            x = ((y[i] - u1[i] * x1) - u2[i] * x2) / u0[i]
            X[:, i], x2, x1 = x, x1, x
    return X


def orth(Z, head, last):
    """stx_orth in place on the rows of Z [k, N]"""
    k = len(head)
    for j in range(k):
        h = head[j]
        for _ in range(2 if j > h else 0):
            dots = Z[h:j] @ Z[j]
            Z[j] -= dots @ Z[h:j]
        nrm = np.sqrt(Z[j] @ Z[j])
        if nrm > 0.0 and np.isfinite(nrm):
            Z[j] /= nrm
        if last and Z[j, np.argmax(np.abs(Z[j]))] < 0.0:
            Z[j] = -Z[j]
    return Z


def tridiag_eigen_model(d, e, subset=None, vectors=True):
    """(lambda [k] descending, Z [N, k] columns or None, info) of the whole route on one member"""
    p = prepare(d, e)
    N = p["N"]
    i0, i1 = (0, N) if subset is None else subset
    lams, lam, halvings = bisect(p, i0, i1)
    info = {"halvings": halvings, "lams": lams, "prepared": p}
    if not vectors or i1 == i0:
        return lam, None, info
    if p["diag"]:
        order = np.argsort(-p["ds"], kind="stable")[i0:i1]
        return lam, np.eye(N)[:, order], info
    head, shift = clusters(lams, p["g"])
    info["head"], info["shift"] = head, shift
    Z = start_vectors(N, i0, i1)
    for r in range(3):
        Z = orth(factor_solve(p, shift, Z), head, r == 2)
    return lam, np.ascontiguousarray(Z.T), info


def eigen_sym_model(S, subset):
    """eigen_sym(S, subset) on one matrix with the plain Householder tridiagonalisation of eigsym_common: (lambda [k], V [N, k])"""
    N = S.shape[0]
    if N == 1:
        lam, Z, _ = tridiag_eigen_model(S[0], np.zeros(0), subset)
        return lam, Z
    mx = np.abs(np.tril(S)).max()
    e1 = int(np.frexp(mx)[1]) if mx > 0 else 0
    U, d, e = householder_tridiag(np.ldexp(np.tril(S) + np.tril(S, -1).T, -e1))
    lam, Z, _ = tridiag_eigen_model(d, e, subset)
    return np.ldexp(lam, e1), U @ Z


def subset_shares(A, lam, Z, lam_ref):
    """(values, residual, orthogonality) of k selected pairs of the symmetric A [N, N] as fractions of their bounds; lam_ref [k]"""
    mx = np.abs(A).max()
    m = int(np.frexp(mx)[1]) if mx > 0 else 0                 # everything times 2^-m, exactly: the squares of a 2^+-500 (or 2^-700)
    A, lam, lam_ref = np.ldexp(A, -m), np.ldexp(lam, -m), np.ldexp(lam_ref, -m)   # member neither overflow nor underflow
    nrm = max(np.linalg.norm(A), 1e-300)
    k = len(lam)
    out = [np.abs(lam - lam_ref).max() / (TOL * nrm) if k else 0.0, 0.0, 0.0]
    if Z is not None and k:
        out[1] = np.linalg.norm(A @ Z - Z * lam) / (TOL * nrm)
        out[2] = np.linalg.norm(Z.T @ Z - np.eye(k)) / (TOL * np.sqrt(k))
    return tuple(out)


def check_subset(A, lam, Z, lam_ref, what=""):
    """the three bounds, descending order and shapes; returns the shares"""
    N, k = A.shape[0], len(lam_ref)
    assert lam.shape == (k,) and lam.dtype == np.float64 and np.all(np.isfinite(lam)), what
    assert np.all(np.diff(lam) <= 0), what + ": eigenvalues must be descending"
    if Z is not None:
        assert Z.shape == (N, k) and Z.dtype == np.float64 and np.all(np.isfinite(Z)), what
    sh = subset_shares(A, lam, Z, lam_ref)
    for name, s in zip(("max|dlambda|", "||A Z - Z L||_F", "||Z^T Z - I||_F"), sh):
        assert s <= 1.0, "%s: %s is %.3g of its bound" % (what, name, s)
    return sh


def signs_ok(Z):
    """every column's first component of largest magnitude is positive"""
    return all(Z[np.argmax(np.abs(Z[:, j])), j] > 0.0 for j in range(Z.shape[1]))


# ---- the tridiagonal inputs ----------------------------------------------------------------------------------------------------------
def _dense(N):
    _, d, e = householder_tridiag(sym_uniform(7100 + N, N))
    return d, e


def _of(name):
    _, d, e = householder_tridiag(CATALOGUE[name]())
    return d, e


def wilkinson(n=21):
    m = (n - 1) // 2
    return np.abs(np.arange(-m, m + 1)).astype(np.float64), np.ones(n - 1)


def glued_wilkinson(copies=5, glue=1e-8):
    d, e = wilkinson()
    return np.tile(d, copies), np.concatenate([np.concatenate((e, [glue])) for _ in range(copies)])[:-1]


def _graded(N=48):
    return 10.0 ** (-12.0 * np.arange(N) / (N - 1)), 10.0 ** (-12.0 * (np.arange(N - 1) + 0.5) / (N - 1)) * 0.25


def _zeros_in_e(N=40):
    e = rng.fill_uniform(7360, N - 1)
    e[[3, 4, N // 2, N - 2]] = 0.0
    return rng.fill_uniform(7361, N), e


def _scaled(m):
    d, e = _dense(50)
    return np.ldexp(d, m), np.ldexp(e, m)


# name -> builder of (d, e); the small ones are shared by the CPU and the GPU tests
TRIDIAGS = {
    "dense_3": functools.partial(_dense, 3),
    "dense_50": functools.partial(_dense, 50),
    "dense_200": functools.partial(_dense, 200),
    "clusters_40": functools.partial(_of, "clusters_40"),
    "rank5_50": functools.partial(_of, "rank5_50"),
    "w21": wilkinson,
    "glued_w21": glued_wilkinson,
    "identity_8": lambda: (np.ones(8), np.zeros(7)),
    "diag_ties_zero": lambda: (np.array([2.0, -1.0, 0.0, 2.0, 0.5, -1.0, 0.5, 3.0]), np.zeros(7)),
    "zeros_in_e_40": _zeros_in_e,
    "graded_48": _graded,
    "scaled_p500": functools.partial(_scaled, 500),
    "scaled_m500": functools.partial(_scaled, -500),
}
LARGE_TRIDIAGS = {
    "dense_300": functools.partial(_dense, 300),
    "dense_1024": functools.partial(_dense, 1024),
    "toeplitz_1000": lambda: (np.full(1000, 2.0), np.full(999, -1.0)),
}


@functools.lru_cache(maxsize=None)
def tridiag_input(name):
    """(d, e) of TRIDIAGS or LARGE_TRIDIAGS, read-only, built once"""
    d, e = (TRIDIAGS[name] if name in TRIDIAGS else LARGE_TRIDIAGS[name])()
    d, e = np.ascontiguousarray(d, dtype=np.float64), np.ascontiguousarray(e, dtype=np.float64)
    d.setflags(write=False), e.setflags(write=False)
    return d, e


@functools.lru_cache(maxsize=None)
def tridiag_reference(name):
    """LAPACK's eigenvalues of the input, descending, read-only (computed on the member scaled into the normal range)"""
    from scipy.linalg import eigvalsh_tridiagonal
    d, e = tridiag_input(name)
    mx = max(np.abs(d).max(), np.abs(e).max() if len(e) else 0.0)
    m = int(np.frexp(mx)[1]) if mx > 0 else 0
    w = np.ldexp(eigvalsh_tridiagonal(np.ldexp(d, -m), np.ldexp(e, -m)) if len(d) > 1 else np.ldexp(d, -m), m)
    w = np.ascontiguousarray(w[::-1])
    w.setflags(write=False)
    return w


@functools.lru_cache(maxsize=None)
def tridiag_model(name, subset=None):
    """(lambda, Z, info) of the model for an input, read-only, computed once"""
    d, e = tridiag_input(name)
    lam, Z, info = tridiag_eigen_model(d, e, subset)
    lam.setflags(write=False)
    if Z is not None:
        Z.setflags(write=False)
    return lam, Z, info


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ---- the argument contract of the three operations in the C ABI ---------------------------------------------------------------------
_buf = (ctypes.c_double * 64)()
_ibuf = (ctypes.c_int32 * 16)()
P = ctypes.cast(_buf, ctypes.c_void_p)
Q = ctypes.cast(_ibuf, ctypes.c_void_p)
Z = None
SUBSET = ": subset must satisfy 0 <= i0 <= i1 <= N"
# (operation, kind, arguments after the handle, return code, nd4hip_last_error()): every row ends inside the validation, which
# stands before the handle is looked at, so the rows hold with a NULL handle and the buffers are never read
ROWS = [
    ("dstcnt_batched", "extent", (-1, 1, 1, P, P, P, Q), -1, "nd4hip_dstcnt_batched: negative extent"),
    ("dstcnt_batched", "extent", (1, 1, -1, P, P, P, Q), -1, "nd4hip_dstcnt_batched: negative extent"),
    ("dstcnt_batched", "extent", (1, 2049, 1, P, P, P, Q), -1, "nd4hip_dstcnt_batched: N <= 2048"),
    ("dstcnt_batched", "empty", (0, 1, 1, Z, Z, Z, Z), 0, None),
    ("dstcnt_batched", "empty", (1, 2, 0, Z, Z, Z, Z), 0, None),
    ("dstcnt_batched", "null", (1, 1, 1, Z, Z, Z, Z), -1, "nd4hip_dstcnt_batched: NULL pointer"),
    ("dstcnt_batched", "null", (1, 2, 1, P, Z, P, Q), -1, "nd4hip_dstcnt_batched: NULL pointer"),
    ("dstevx_batched", "extent", (-1, 1, 0, 1, P, P, P, P), -1, "nd4hip_dstevx_batched: negative extent"),
    ("dstevx_batched", "selector", (1, 4, 3, 2, P, P, P, P), -1, "nd4hip_dstevx_batched" + SUBSET),
    ("dstevx_batched", "selector", (1, 4, -1, 2, P, P, P, P), -1, "nd4hip_dstevx_batched" + SUBSET),
    ("dstevx_batched", "selector", (1, 4, 0, 5, P, P, P, P), -1, "nd4hip_dstevx_batched" + SUBSET),
    ("dstevx_batched", "extent", (1, 2049, 0, 1, P, P, P, P), -1, "nd4hip_dstevx_batched: N <= 2048"),
    ("dstevx_batched", "empty", (0, 1, 0, 1, Z, Z, Z, Z), 0, None),
    ("dstevx_batched", "empty", (1, 4, 2, 2, Z, Z, Z, Z), 0, None),
    ("dstevx_batched", "null", (1, 1, 0, 1, Z, Z, Z, Z), -1, "nd4hip_dstevx_batched: NULL pointer"),
    ("dstevx_batched", "null", (1, 2, 0, 1, P, Z, P, Z), -1, "nd4hip_dstevx_batched: NULL pointer"),
    ("dsyevx_batched", "extent", (-1, 1, 0, 1, P, P, P), -1, "nd4hip_dsyevx_batched: negative extent"),
    ("dsyevx_batched", "extent", (1, -1, 0, 0, P, P, P), -1, "nd4hip_dsyevx_batched: negative extent"),
    ("dsyevx_batched", "selector", (1, 4, 3, 2, P, P, P), -1, "nd4hip_dsyevx_batched" + SUBSET),
    ("dsyevx_batched", "selector", (1, 4, 0, 5, P, P, P), -1, "nd4hip_dsyevx_batched" + SUBSET),
    ("dsyevx_batched", "selector", (1, 2049, 0, 2050, P, P, P), -1, "nd4hip_dsyevx_batched" + SUBSET),
    ("dsyevx_batched", "extent", (1, 2049, 0, 1, P, P, P), -1, "nd4hip_dsyevx_batched: N <= 2048"),
    ("dsyevx_batched", "empty", (0, 1, 0, 1, Z, Z, Z), 0, None),
    ("dsyevx_batched", "empty", (1, 0, 0, 0, Z, Z, Z), 0, None),
    ("dsyevx_batched", "empty", (1, 4, 4, 4, Z, Z, Z), 0, None),
    ("dsyevx_batched", "null", (1, 1, 0, 1, Z, Z, Z), -1, "nd4hip_dsyevx_batched: NULL pointer"),
    ("dsyevx_batched", "null", (1, 1, 0, 1, P, Z, P), -1, "nd4hip_dsyevx_batched: NULL pointer"),
]
NEW = ("nd4hip_dstcnt_batched", "nd4hip_dstevx_batched", "nd4hip_dsyevx_batched")


def mismatches(handle):
    """the rows that a form answers differently, for test_gpu_eigsym_subset.py too"""
    lib, bad = _lib.load(), []
    for op, kind, args, rc, text in ROWS:
        for form in ("_host", "_dev"):
            got = getattr(lib, "nd4hip_" + op + form)(handle, *args)
            err = lib.nd4hip_last_error().decode() if got != 0 else None
            if (got, err) != (rc, text):
                bad.append("nd4hip_%s%s%r [%s]: expected %r, got %r" % (op, form, args, kind, (rc, text), (got, err)))
    return bad
