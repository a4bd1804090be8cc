"""Shared by the tests of the interval forms (test_eigsym_interval_host.py, test_gpu_eigsym_interval.py): the numpy model of
interval=(lo, hi) on top of eigsym_subset_common's model of csrc/syevx.hip, boundaries whose expected count is unambiguous, and the
argument contract of the new entry points.

interval=(lo, hi) selects lo < lambda <= hi, which is defined as subset=(count(hi), count(lo)) with the Sturm count of stx_count on
the member's scaled tridiagonal form: the model is eigsym_subset_common.count followed by tridiag_eigen_model."""
import ctypes

import numpy as np

import eigsym_subset_common as X
from nd4js_amd import _lib

GAP = 1e-6                                                     # a boundary is placed only inside a reference gap of at least GAP g


def model_range(d, e, lo, hi):
    """(i0, i1) = (count(hi), count(lo)) of one member"""
    c = X.count(d, e, [hi, lo])
    return int(c[0]), int(c[1])


def model(d, e, lo, hi, vectors=True):
    """((i0, i1), lambda [k], Z [N, k] or None) of tridiag_eigen(d, e, interval=(lo, hi)) on one member"""
    i0, i1 = model_range(d, e, lo, hi)
    if i1 == i0:
        return (i0, i1), np.zeros(0), (np.zeros((len(d), 0)) if vectors else None)
    lam, Z, _ = X.tridiag_eigen_model(d, e, (i0, i1), vectors)
    return (i0, i1), lam, Z


def gershgorin(d, e):
    p = X.prepare(d, e)
    return float(np.ldexp(p["g"], p["lexp"]))


def cuts(ref, g):
    """{j: x_j}: x_j the midpoint of the gap between the descending reference values ref[j - 1] > ref[j], for every gap of at least
    GAP g, so that exactly j eigenvalues are greater than x_j whatever the last bits of the computed values are"""
    out = {}
    for j in range(1, len(ref)):
        if ref[j - 1] - ref[j] >= GAP * g:
            out[j] = 0.5 * (ref[j - 1] + ref[j])
    return out


def padded(lam, vec, ranges, axis=-1):
    """the ragged protocol on host arrays: lam [batch, kmax], vec [batch, N, kmax] or None, ranges [batch, 2]: NaN / zeros exactly in
    the entries k_b .. kmax - 1 of every member, finite values before them"""
    kb = ranges[:, 1] - ranges[:, 0]
    assert lam.shape[-1] == (kb.max() if len(kb) else 0)
    for b in range(len(lam)):
        if not (np.all(np.isfinite(lam[b, :kb[b]])) and np.all(np.isnan(lam[b, kb[b]:]))):
            return False
        if vec is not None and vec[b][:, kb[b]:].any():
            return False
    return True


# ---- the argument contract of the three operations in the C ABI ---------------------------------------------------------------------
P, Q, Z = X.P, X.Q, X.Z
_kmax = ctypes.c_int64(-7)
K = ctypes.pointer(_kmax)
# (operation, kind, arguments after the handle, return code, nd4hip_last_error()): every row ends inside the validation, which
# stands before the handle is looked at, so the rows hold with a NULL handle and the buffers are never read.
# dstevxv: (batch, N, kcap, bounds, d, e, lambda, Z, range, kmax); dsyevxv, dsyevxv_tr: (batch, N, kcap, bounds, S, lambda, V, range, kmax)
ROWS = [
    ("dstevxv_batched", "extent", (-1, 1, 1, P, P, P, P, P, Q, K), -1, "nd4hip_dstevxv_batched: negative extent"),
    ("dstevxv_batched", "extent", (1, -1, 1, P, P, P, P, P, Q, K), -1, "nd4hip_dstevxv_batched: negative extent"),
    ("dstevxv_batched", "kcap", (1, 1, -1, P, P, P, P, P, Q, K), -1, "nd4hip_dstevxv_batched: negative extent"),
    ("dstevxv_batched", "extent", (1, 2049, 1, P, P, P, P, P, Q, K), -1, "nd4hip_dstevxv_batched: N <= 2048"),
    ("dstevxv_batched", "empty", (0, 1, 1, Z, Z, Z, Z, Z, Z, None), 0, None),
    ("dstevxv_batched", "empty", (1, 0, 0, Z, Z, Z, Z, Z, Z, None), 0, None),
    ("dstevxv_batched", "null", (1, 1, 1, Z, Z, Z, Z, Z, Z, None), -1, "nd4hip_dstevxv_batched: NULL pointer"),
    ("dstevxv_batched", "null", (1, 2, 1, P, P, Z, P, P, Q, K), -1, "nd4hip_dstevxv_batched: NULL pointer"),
    ("dstevxv_batched", "null", (1, 1, 1, Z, P, Z, P, P, Q, K), -1, "nd4hip_dstevxv_batched: NULL pointer"),
    ("dstevxv_batched", "null", (1, 1, 1, P, P, Z, P, P, Z, K), -1, "nd4hip_dstevxv_batched: NULL pointer"),
    ("dstevxv_batched", "null", (1, 1, 1, P, P, Z, P, P, Q, None), -1, "nd4hip_dstevxv_batched: NULL pointer"),
    ("dstevxv_batched", "kcap", (1, 1, 1, P, P, Z, Z, Z, Q, K), -1, "nd4hip_dstevxv_batched: NULL pointer"),
]
for _op in ("dsyevxv_batched", "dsyevxv_tr_batched"):
    _t = "nd4hip_" + _op
    ROWS += [
        (_op, "extent", (-1, 1, 1, P, P, P, P, Q, K), -1, _t + ": negative extent"),
        (_op, "kcap", (1, 4, -1, P, P, P, P, Q, K), -1, _t + ": negative extent"),
        (_op, "extent", (1, 2049, 1, P, P, P, P, Q, K), -1, _t + ": N <= 2048"),
        (_op, "empty", (0, 1, 1, Z, Z, Z, Z, Z, None), 0, None),
        (_op, "empty", (1, 0, 0, Z, Z, Z, Z, Z, None), 0, None),
        (_op, "null", (1, 1, 1, Z, Z, Z, Z, Z, None), -1, _t + ": NULL pointer"),
        (_op, "null", (1, 4, 4, P, Z, P, P, Q, K), -1, _t + ": NULL pointer"),
        (_op, "null", (1, 4, 4, P, P, P, P, Z, K), -1, _t + ": NULL pointer"),
        (_op, "null", (1, 4, 4, P, P, P, P, Q, None), -1, _t + ": NULL pointer"),
        (_op, "kcap", (1, 4, 1, P, P, Z, Z, Q, K), -1, _t + ": NULL pointer"),
    ]
# dsygvx: (reduction, select, batch, N, i0, i1, kcap, bounds, A, B, strideB, lambda, X, range, kmax); the two forms end in _host and _dev
_g = "nd4hip_dsygvx_batched"
GEN_ROWS = [
    ("selector", (2, 0, 1, 4, 0, 0, 0, Z, P, P, 16, P, P, Z, None), -1, _g + ": reduction must be 0 (hessenberg) or 1 (tridiag)"),
    ("selector", (0, 3, 1, 4, 0, 0, 0, Z, P, P, 16, P, P, Z, None), -1, _g + ": select must be 0 (all), 1 (subset) or 2 (interval)"),
    ("selector", (0, -1, 1, 4, 0, 0, 0, Z, P, P, 16, P, P, Z, None), -1, _g + ": select must be 0 (all), 1 (subset) or 2 (interval)"),
    ("extent", (0, 0, -1, 4, 0, 0, 0, Z, P, P, 16, P, P, Z, None), -1, _g + ": negative extent"),
    ("kcap", (0, 2, 1, 4, 0, 0, -1, P, P, P, 16, P, P, Q, K), -1, _g + ": negative extent"),
    ("selector", (1, 1, 1, 4, 3, 2, 0, Z, P, P, 16, P, P, Z, None), -1, _g + ": subset must satisfy 0 <= i0 <= i1 <= N"),
    ("selector", (0, 1, 1, 4, 0, 5, 0, Z, P, P, 16, P, P, Z, None), -1, _g + ": subset must satisfy 0 <= i0 <= i1 <= N"),
    ("extent", (0, 0, 1, 2049, 0, 0, 0, Z, P, P, 0, P, P, Z, None), -1, _g + ": N <= 2048"),
    ("stride", (0, 0, 1, 4, 0, 0, 0, Z, P, P, 15, P, P, Z, None), -1, _g + ": strideB must be N*N or 0"),
    ("empty", (1, 0, 0, 4, 0, 0, 0, Z, Z, Z, 16, Z, Z, Z, None), 0, None),
    ("empty", (0, 1, 1, 4, 2, 2, 0, Z, Z, Z, 0, Z, Z, Z, None), 0, None),
    ("empty", (0, 2, 1, 0, 0, 0, 0, Z, Z, Z, 0, Z, Z, Z, None), 0, None),
    ("null", (0, 0, 1, 4, 0, 0, 0, Z, Z, P, 16, P, P, Z, None), -1, _g + ": NULL pointer"),
    ("null", (1, 1, 1, 4, 0, 2, 0, Z, P, P, 16, Z, P, Z, None), -1, _g + ": NULL pointer"),
    ("null", (0, 2, 1, 4, 0, 0, 4, Z, P, P, 16, P, P, Q, K), -1, _g + ": NULL pointer"),
    ("null", (0, 2, 1, 4, 0, 0, 4, P, P, P, 16, P, P, Z, K), -1, _g + ": NULL pointer"),
    ("null", (0, 2, 1, 4, 0, 0, 4, P, P, P, 16, P, P, Q, None), -1, _g + ": NULL pointer"),
    ("kcap", (0, 2, 1, 4, 0, 0, 1, P, P, P, 16, Z, Z, Q, K), -1, _g + ": NULL pointer"),
]
GEN_VALID = [(0, 0, 1, 4, 9, 9, 9, Z, P, P, 16, P, Z, Z, None), (1, 1, 2, 4, 1, 3, 0, Z, P, P, 0, P, P, Z, None),
             (1, 2, 1, 4, 0, 0, 4, P, P, P, 16, P, P, Q, K), (0, 2, 1, 4, 0, 0, 0, P, P, P, 16, Z, Z, Q, K)]


def gen_mismatches(handle):
    lib, bad = _lib.load(), []
    for kind, args, rc, text in GEN_ROWS:
        for form in ("_host", "_dev"):
            got = getattr(lib, _g + form)(handle, *args)
            err = lib.nd4hip_last_error().decode() if got != 0 else None
            if (got, err) != (rc, text) or _kmax.value != -7:
                bad.append("%s%s%r [%s]: expected %r, got %r" % (_g, form, args, kind, (rc, text), (got, err)))
    return bad


# valid argument lists (kcap = 0 needs no lambda; the vectors are optional): what is refused then is the NULL handle
VALID = {
    "dstevxv_batched": [(1, 1, 1, P, P, Z, P, Z, Q, K), (1, 2, 0, P, P, P, Z, Z, Q, K)],
    "dsyevxv_batched": [(1, 4, 4, P, P, P, Z, Q, K), (1, 4, 0, P, P, Z, Z, Q, K)],
    "dsyevxv_tr_batched": [(1, 4, 4, P, P, P, P, Q, K), (2, 1, 0, P, P, Z, Z, Q, K)],
}
NEW = ("nd4hip_dstevxv_batched", "nd4hip_dsyevxv_batched", "nd4hip_dsyevxv_tr_batched")


def mismatches(handle):
    """the rows that a form answers differently; an empty call must leave kmax alone"""
    lib, bad = _lib.load(), []
    for op, kind, args, rc, text in ROWS:
        for form in ("_host", "_dev"):
            got = getattr(lib, "nd4hip_" + op + form)(handle, *args)
            err = lib.nd4hip_last_error().decode() if got != 0 else None
            if (got, err) != (rc, text) or _kmax.value != -7:
                bad.append("nd4hip_%s%s%r [%s]: expected %r, got %r" % (op, form, args, kind, (rc, text), (got, err)))
    return bad
