"""Shared by the tests of the selected-singular-triplet route (test_svd_subset_host.py, test_gpu_svd_subset.py,
test_node_svd_subset.py): a numpy model of csrc/bdsvdx.hip and the bounds.

A singular value of the upper bidiagonal B [K, J] (J = K or K + 1) is an eigenvalue of the Golub-Kahan matrix: the symmetric
tridiagonal of order K + J with a zero diagonal and the off-diagonals d0, e0, d1, e1, ...; its eigenvector for sigma is
(v0, u0, v1, u1, ...) / sqrt(2). The model is therefore the model of csrc/syevx.hip (eigsym_subset_common.py) applied to
(zeros, interleave(d, e)), then the split, then the rule that sends a member to the full solver:
  values    bisect() of the existing model, then max(value, +0): the device returns these bits;
  vectors   clusters(), three rounds of factor_solve() and orth(), then v = the even entries, u = the odd entries, each
            normalised on its own: held to bounds, not bits;
  fallback  a member is flagged when B = 0, when two or more of its selected scaled values lie below CTOL g / 2, or when
            min(|u|^2, |v|^2) < 1/8 for one of its vectors. A flagged member's U2 and V2 are those of the full solver, sliced.

Bounds, each TOL = 1e-12 norm-wise against LAPACK (numpy.linalg.svd), everything scaled as eigsym_subset_common.subset_shares
scales (by the exact power of two of max|B|), k the number of selected triplets:
  max|sv - ref| / ||B||_F;  ||B V2^T - U2 S||_F / ||B||_F;  ||B^T U2 - V2^T S||_F / ||B||_F;
  ||U2^T U2 - I||_F / sqrt(k);  ||V2 V2^T - I||_F / sqrt(k)."""
import ctypes
import functools

import numpy as np

import eigsym_subset_common as S
from eigsym_subset_common import CTOL, TOL, same_bits  # noqa: F401
from svd_dc_common import BIDIAG_CASES, PATH_CASES, bidiag_dense
from nd4js_amd import _lib

SPLIT_MIN = 0.125                                              # of |u|^2 and |v|^2; the ideal is 1/2
SWEEP_SKIP = ("max_2048",)                                     # the sweep's one exclusion: too slow for the numpy model's vectors


def interleave(d, e):
    """the off-diagonals d0, e0, d1, e1, ... of the Golub-Kahan matrix of order K + J: K + J - 1 entries"""
    d, e = np.asarray(d, dtype=np.float64), np.asarray(e, dtype=np.float64)
    K, J = len(d), len(e) + 1
    assert K >= 1 and J in (K, K + 1)
    b = np.empty(K + J - 1)
    b[0::2], b[1::2] = d, e
    return b


def prepare(d, e):
    """bdx_prepare on one member: stx_prepare of (zeros, interleave(d, e))"""
    b = interleave(d, e)
    return S.prepare(np.zeros(len(b) + 1), b)


def clamp(v):
    """max(value, +0): a bisected value of a singular B may come out as -0 or a rounding below 0"""
    return np.where(v > 0.0, v, 0.0)


def values(d, e, subset=None):
    """(sv [k], scaled unclamped values [k], prepared) for the indices of the descending singular values"""
    p = prepare(d, e)
    i0, i1 = (0, len(d)) if subset is None else subset
    if i0 == i1:
        return np.empty(0), np.empty(0), p
    lams, lam, _ = S.bisect(p, i0, i1)
    return clamp(lam), lams, p


def values_flag(lams, p):
    """the part of the fallback rule that needs the values alone"""
    return bool(p["diag"]) or int(np.sum(lams < 0.5 * (CTOL * p["g"]))) >= 2


def split(Z):
    """rows of Z [k, K + J] -> (U2 [K, k], V2 [k, J], min over the vectors of min(|u|^2, |v|^2))"""
    v, u = Z[:, 0::2], Z[:, 1::2]
    nu, nv = np.sum(u * u, axis=1), np.sum(v * v, axis=1)
    with np.errstate(all="ignore"):
        U2 = np.where((nu > 0)[:, None], u / np.sqrt(nu)[:, None], u).T
        V2 = np.where((nv > 0)[:, None], v / np.sqrt(nv)[:, None], v)
    return np.ascontiguousarray(U2), np.ascontiguousarray(V2), float(min(nu.min(), nv.min()))


def full_solver(d, e):
    """what stands in for bidiag_svd(d, e) in the model: LAPACK on the dense B; U2 [K, K], V2 [J, J] rows = right vectors"""
    B = bidiag_dense(np.asarray(d, dtype=np.float64), np.asarray(e, dtype=np.float64))
    u, _, vt = np.linalg.svd(B, full_matrices=True)
    return u, vt


def bidiag_svd_model(d, e, subset=None, vectors=True):
    """(U2 [K, k] or None, sv [k], V2 [k, J] or None, info) of the whole route on one member; info['fallback'] is the flag,
    info['split_min'] the smallest min(|u|^2, |v|^2) (None where no vector was iterated)"""
    K = len(d)
    i0, i1 = (0, K) if subset is None else subset
    sv, lams, p = values(d, e, (i0, i1))
    info = {"fallback": values_flag(lams, p) if i1 > i0 else bool(p["diag"]), "split_min": None, "lams": lams, "prepared": p}
    if not vectors:
        return None, sv, None, info
    J, k = len(e) + 1, i1 - i0
    if k == 0:
        return np.empty((K, 0)), sv, np.empty((0, J)), info
    U2 = V2 = None
    if not p["diag"]:
        head, shift = S.clusters(lams, p["g"])
        Z = S.start_vectors(K + J, i0, i1)
        for r in range(3):
            Z = S.orth(S.factor_solve(p, shift, Z), head, r == 2)
        U2, V2, info["split_min"] = split(Z)
        info["fallback"] = info["fallback"] or not info["split_min"] >= SPLIT_MIN
    if info["fallback"]:
        u, vt = full_solver(d, e)
        U2, V2 = np.ascontiguousarray(u[:, i0:i1]), np.ascontiguousarray(vt[i0:i1])
    return U2, sv, V2, info


NAMES = ("max|dsv|", "||B V2^T - U2 S||_F", "||B^T U2 - V2^T S||_F", "||U2^T U2 - I||_F", "||V2 V2^T - I||_F")


def shares(B, U2, sv, V2, ref):
    """the five bounds of k selected triplets of B [M, N] (bidiagonal or dense) as fractions; ref [k]; U2 [M, k], V2 [k, N] or None"""
    mx = np.abs(B).max() if B.size else 0.0
    m = int(np.frexp(mx)[1]) if mx > 0 else 0                  # everything times 2^-m, exactly
    B, sv, ref = np.ldexp(B, -m), np.ldexp(sv, -m), np.ldexp(ref, -m)
    nrm = max(np.linalg.norm(B), 1e-300)
    k = len(sv)
    out = [np.abs(sv - ref).max() / (TOL * nrm) if k else 0.0, 0.0, 0.0, 0.0, 0.0]
    if U2 is not None and k:
        out[1] = np.linalg.norm(B @ V2.T - U2 * sv) / (TOL * nrm)
        out[2] = np.linalg.norm(B.T @ U2 - V2.T * sv) / (TOL * nrm)
        out[3] = np.linalg.norm(U2.T @ U2 - np.eye(k)) / (TOL * np.sqrt(k))
        out[4] = np.linalg.norm(V2 @ V2.T - np.eye(k)) / (TOL * np.sqrt(k))
    return tuple(out)


def check_triplets(B, U2, sv, V2, ref, what=""):
    """the contract (shapes, sv >= 0 and descending, finite) and the five bounds; returns the shares"""
    M, N = B.shape
    k = len(ref)
    assert sv.shape == (k,) and sv.dtype == np.float64 and np.all(np.isfinite(sv)), what
    assert np.all(sv >= 0.0) and np.all(np.diff(sv) <= 0), what + ": sv must be non-negative and descending"
    if U2 is not None:
        assert U2.shape == (M, k) and V2.shape == (k, N) and np.all(np.isfinite(U2)) and np.all(np.isfinite(V2)), what
    sh = shares(B, U2, sv, V2, ref)
    for name, s in zip(NAMES, sh):
        assert s <= 1.0, "%s: %s is %.3g of its bound" % (what, name, s)
    return sh


# ---- the catalogue sweep ---------------------------------------------------------------------------------------------------------
def subsets_of(K):
    """top 8, all, bottom 8 and a middle three, clipped to K and without repeats"""
    out = []
    for s in ((0, min(8, K)), (0, K), (max(K - 8, 0), K), (K // 2 - 1 if K >= 3 else 0, min(K // 2 + 2, K) if K >= 3 else K)):
        if s not in out:
            out.append(s)
    return out


def catalogue():
    """name -> (d, e) of every entry of BIDIAG_CASES and PATH_CASES"""
    c = dict(BIDIAG_CASES)
    c.update(PATH_CASES)
    return c


def sweep_runs():
    """(name, subset) of the sweep: every catalogue entry but SWEEP_SKIP with each of its subsets"""
    return [(name, s) for name, (d, _) in catalogue().items() if name not in SWEEP_SKIP for s in subsets_of(len(d))]


@functools.lru_cache(maxsize=None)
def case_input(name):
    d, e = catalogue()[name]
    d, e = np.ascontiguousarray(d, dtype=np.float64), np.ascontiguousarray(e, dtype=np.float64)
    d.setflags(write=False), e.setflags(write=False)
    return d, e


@functools.lru_cache(maxsize=None)
def case_reference(name):
    """(B, LAPACK's singular values of it, descending), read-only"""
    d, e = case_input(name)
    B = bidiag_dense(d, e)
    sv = np.linalg.svd(B, compute_uv=False)
    B.setflags(write=False), sv.setflags(write=False)
    return B, sv


@functools.lru_cache(maxsize=None)
def case_model(name, subset, vectors=True):
    """the model's result for a catalogue entry, read-only, computed once"""
    d, e = case_input(name)
    U2, sv, V2, info = bidiag_svd_model(d, e, subset, vectors)
    for x in (U2, sv, V2):
        if x is not None:
            x.setflags(write=False)
    return U2, sv, V2, info


# ---- the argument contract of the two operations in the C ABI ---------------------------------------------------------------------
_buf = (ctypes.c_double * 64)()
_ibuf = (ctypes.c_int32 * 16)()
P = ctypes.cast(_buf, ctypes.c_void_p)
Q = ctypes.cast(_ibuf, ctypes.c_void_p)
Z = None
BSUB = "nd4hip_dbdsvdx_batched: subset must satisfy 0 <= i0 <= i1 <= K"
GSUB = "nd4hip_dgesvdx_batched: subset must satisfy 0 <= i0 <= i1 <= min(M, N)"
# (operation, kind, arguments after the handle, return code, nd4hip_last_error()): every row ends inside the validation, which
# stands before the handle is looked at, so the rows hold with a NULL handle and the buffers are never read.
# dbdsvdx_batched(batch, K, J, i0, i1, d, e, U2, sv, V2, fallback); dgesvdx_batched(batch, M, N, i0, i1, A, U, sv, V, fallback)
ROWS = [
    ("dbdsvdx_batched", "extent", (-1, 1, 1, 0, 1, P, P, P, P, P, Q), -1, "nd4hip_dbdsvdx_batched: negative extent"),
    ("dbdsvdx_batched", "extent", (1, -1, -1, 0, 0, P, P, P, P, P, Q), -1, "nd4hip_dbdsvdx_batched: negative extent"),
    ("dbdsvdx_batched", "shape", (1, 4, 6, 0, 1, P, P, P, P, P, Q), -1, "nd4hip_dbdsvdx_batched: B must be K x K or K x (K+1)"),
    ("dbdsvdx_batched", "shape", (1, 4, 3, 0, 1, P, P, P, P, P, Q), -1, "nd4hip_dbdsvdx_batched: B must be K x K or K x (K+1)"),
    ("dbdsvdx_batched", "selector", (1, 4, 4, 3, 2, P, P, P, P, P, Q), -1, BSUB),
    ("dbdsvdx_batched", "selector", (1, 4, 5, -1, 2, P, P, P, P, P, Q), -1, BSUB),
    ("dbdsvdx_batched", "selector", (1, 4, 5, 0, 5, P, P, P, P, P, Q), -1, BSUB),
    ("dbdsvdx_batched", "extent", (1, 2049, 2049, 0, 1, P, P, P, P, P, Q), -1, "nd4hip_dbdsvdx_batched: K <= 2048"),
    ("dbdsvdx_batched", "empty", (0, 1, 1, 0, 1, Z, Z, Z, Z, Z, Z), 0, None),
    ("dbdsvdx_batched", "empty", (1, 0, 0, 0, 0, Z, Z, Z, Z, Z, Z), 0, None),
    ("dbdsvdx_batched", "empty", (1, 4, 5, 2, 2, Z, Z, Z, Z, Z, Z), 0, None),
    ("dbdsvdx_batched", "null", (1, 1, 1, 0, 1, Z, Z, Z, Z, Z, Z), -1, "nd4hip_dbdsvdx_batched: NULL pointer"),
    ("dbdsvdx_batched", "null", (1, 2, 2, 0, 1, P, Z, P, P, P, Z), -1, "nd4hip_dbdsvdx_batched: NULL pointer"),
    ("dbdsvdx_batched", "null", (1, 2, 2, 0, 1, P, P, Z, Z, Z, Z), -1, "nd4hip_dbdsvdx_batched: NULL pointer"),
    ("dbdsvdx_batched", "null", (1, 2, 2, 0, 1, P, P, P, P, Z, Z), -1, "nd4hip_dbdsvdx_batched: U2 and V2 go together"),
    ("dgesvdx_batched", "extent", (-1, 1, 1, 0, 1, P, P, P, P, Q), -1, "nd4hip_dgesvdx_batched: negative extent"),
    ("dgesvdx_batched", "extent", (1, 2, -1, 0, 0, P, P, P, P, Q), -1, "nd4hip_dgesvdx_batched: negative extent"),
    ("dgesvdx_batched", "selector", (1, 4, 7, 3, 2, P, P, P, P, Q), -1, GSUB),
    ("dgesvdx_batched", "selector", (1, 7, 4, 0, 5, P, P, P, P, Q), -1, GSUB),
    ("dgesvdx_batched", "selector", (1, 4, 4, -1, 1, P, P, P, P, Q), -1, GSUB),
    ("dgesvdx_batched", "extent", (1, 2049, 4000, 0, 1, P, P, P, P, Q), -1, "nd4hip_dgesvdx_batched: min(M, N) <= 2048"),
    ("dgesvdx_batched", "empty", (0, 1, 1, 0, 1, Z, Z, Z, Z, Z), 0, None),
    ("dgesvdx_batched", "empty", (1, 0, 3, 0, 0, Z, Z, Z, Z, Z), 0, None),
    ("dgesvdx_batched", "empty", (1, 4, 5, 4, 4, Z, Z, Z, Z, Z), 0, None),
    ("dgesvdx_batched", "null", (1, 1, 1, 0, 1, Z, Z, Z, Z, Z), -1, "nd4hip_dgesvdx_batched: NULL pointer"),
    ("dgesvdx_batched", "null", (1, 2, 2, 0, 1, P, Z, Z, Z, Z), -1, "nd4hip_dgesvdx_batched: NULL pointer"),
    ("dgesvdx_batched", "null", (1, 2, 2, 0, 1, P, P, P, Z, Z), -1, "nd4hip_dgesvdx_batched: U and V go together"),
]
NEW = ("nd4hip_dbdsvdx_batched", "nd4hip_dgesvdx_batched", "nd4hip_dgesvdx_last_stages")


def mismatches(handle):
    """the rows that a form answers differently, for test_gpu_svd_subset.py too"""
    lib, bad = _lib.load(), []
    for op, kind, args, rc, text in ROWS:
        for form in ("_host", "_dev"):
            got = getattr(lib, "nd4hip_" + op + form)(handle, *args)
            err = lib.nd4hip_last_error().decode() if got != 0 else None
            if (got, err) != (rc, text):
                bad.append("nd4hip_%s%s%r [%s]: expected %r, got %r" % (op, form, args, kind, (rc, text), (got, err)))
    return bad
