"""Argument validation of the C ABI, pinned call by call: every operation of include/nd4hip.h that has a host-pointer form
(nd4hip_X) and a device-pointer form (nd4hip_X_dev) refuses the same bad call with the same code and the same text, and
returns 0 for the same empty call.

ROWS holds one bad or empty call per row: (operation, kind, arguments after the handle, return code, nd4hip_last_error()).
Every row ends inside the validation: a row whose pointers are NULL fails the NULL check or is empty, every other row fails
exactly one check that stands before the pointers are looked at, so the dummy buffers P, P2 and Q are never read, no kernel is
launched and nothing is staged (the one exception is named at its row).

  kind      what the row breaks
  extent    a negative extent, or one beyond the operation's limit
  stride    a stride rule
  selector  a tier, algo, tolerance or shape rule
  empty     nothing: batch (or an extent) is 0 and all pointers are NULL, the call returns 0
  null      the NULL-pointer rule, at the smallest non-empty extents

  forms     which forms the row is asserted for
  both      nd4hip_X and nd4hip_X_dev (the default)
  dev/host  one form alone: nd4hip_zgebak_batched_dev refuses V == W and words its NULL check accordingly, the host form
            stages V and W apart and allows in-place use
  early     the check stands in the _dev form alone where the two forms carry their checks separately, so that the host form
            only meets it inside its first chunk, after the staging is sized and allocated: such a row cannot be given to that
            host form (N = 32769 would need real buffers of that size). Where the checks are shared (csrc/nd4hip_args.h exists)
            the host form refuses the call itself and the row is asserted for both forms.
"""
import ctypes
import math
import os

import pytest

from conftest import ROOT
from nd4js_amd import _lib

_buf = (ctypes.c_double * 128)()
_ibuf = (ctypes.c_int32 * 16)()
P = ctypes.cast(_buf, ctypes.c_void_p)                       # a valid buffer that no row reads or writes
P2 = ctypes.c_void_p(ctypes.addressof(_buf) + 512)           # its second half: never overlaps the first 64 doubles
Q = ctypes.cast(_ibuf, ctypes.c_void_p)
Z = None                                                     # NULL
NAN, INF = math.nan, math.inf
I31 = 1 << 31

SHARED_CHECKS = os.path.exists(os.path.join(ROOT, "nd4js_amd", "csrc", "nd4hip_args.h"))
STRIDE = ": a stride must be 0 or at least the size of one operand"


def _family(op, lead, extents, ptrs, null_text=": NULL pointer", neg_text=": negative extent", tail=()):
    """The three rows every operation has: a negative extent, the empty call, NULL pointers at extents of 1. `lead`: the
    selector arguments before the extents; `extents`: how many; `ptrs`: the pointer arguments as a template in which P / P2 / Q
    mark a pointer and an int is a stride (given as it is); `tail`: the arguments after them."""
    name = "nd4hip_%s" % op.replace("_ex", "")
    one, valid, null = (1,) * extents, tuple(ptrs), tuple(Z if isinstance(a, ctypes.c_void_p) else a for a in ptrs)
    return [(op, "extent", lead + (-1,) + one[1:] + valid + tail, -1, name + neg_text),
            (op, "empty", lead + (0,) + one[1:] + null + tail, 0, None),
            (op, "null", lead + one + null + tail, -1, name + null_text)]


ROWS = []
# ---- matmul: (batch, I, K, J, A, strideA, B, strideB, C); zgemm has (a_complex, b_complex) in front
ROWS += _family("dgemm_batched", (), 4, (P, 0, P, 0, P2), null_text=": NULL matrix pointer")
ROWS += [("dgemm_batched", "extent", (1, 1, 1, -1, P, 0, P, 0, P2), -1, "nd4hip_dgemm_batched: negative extent"),
         ("dgemm_batched", "stride", (2, 2, 2, 2, P, 3, P, 0, P2), -1, "nd4hip_dgemm_batched: strideA must be 0 or >= I*K"),
         ("dgemm_batched", "stride", (2, 2, 2, 2, P, 0, P, 3, P2), -1, "nd4hip_dgemm_batched: strideB must be 0 or >= K*J"),
         ("dgemm_batched", "empty", (1, 0, 1, 1, Z, 0, Z, 0, Z), 0, None),
         ("dgemm_batched", "null", (1, 1, 0, 1, Z, 0, Z, 0, Z), -1, "nd4hip_dgemm_batched: NULL matrix pointer")]
ROWS += _family("zgemm_batched", (1, 1), 4, (P, 0, P, 0, P2), null_text=": NULL matrix pointer")
ROWS += [("zgemm_batched", "selector", (0, 0, 1, 1, 1, 1, P, 0, P, 0, P2), -1, "nd4hip_zgemm_batched: at least one operand must be complex"),
         ("zgemm_batched", "stride", (1, 0, 2, 2, 2, 2, P, 3, P, 0, P2), -1, "nd4hip_zgemm_batched: strideA must be 0 or >= I*K"),
         ("zgemm_batched", "stride", (0, 1, 2, 2, 2, 2, P, 0, P, 3, P2), -1, "nd4hip_zgemm_batched: strideB must be 0 or >= K*J")]
# ---- LU and the solves: (batch, N, A, LU, P), (batch, N, J, LU, strideLU, P, strideP, Y, strideY, X), (upper, unit, batch, M, J, T, strideT, Y, strideY, X)
ROWS += _family("dgetrf_batched", (), 2, (P, P2, Q))
ROWS += [("dgetrf_batched", "empty", (1, 0, Z, Z, Z), 0, None)]
ROWS += _family("dgetrs_batched", (), 3, (P, 0, Q, 0, P, 0, P2))
ROWS += [("dgetrs_batched", "stride", (2, 2, 1, P, 3, Q, 2, P, 2, P2), -1, "nd4hip_dgetrs_batched" + STRIDE),
         ("dgetrs_batched", "stride", (2, 2, 1, P, 4, Q, 1, P, 2, P2), -1, "nd4hip_dgetrs_batched" + STRIDE),
         ("dgetrs_batched", "stride", (2, 2, 1, P, 4, Q, 2, P, 1, P2), -1, "nd4hip_dgetrs_batched" + STRIDE)]
ROWS += _family("dtrsm_batched", (0, 0), 3, (P, 0, P, 0, P2))
ROWS += [("dtrsm_batched", "stride", (0, 0, 2, 2, 1, P, 3, P, 2, P2), -1, "nd4hip_dtrsm_batched" + STRIDE),
         ("dtrsm_batched", "stride", (1, 1, 2, 2, 1, P, 4, P, 1, P2), -1, "nd4hip_dtrsm_batched" + STRIDE)]
# ---- least squares from a factorisation: (batch, N, M, I, J, Q, strideQ, R, strideR, Y, strideY, X); dsvdls has (sv, strideSv, V, strideV) for R
ROWS += _family("dqrls_batched", (), 5, (P, 0, P, 0, P, 0, P2))
ROWS += [("dqrls_batched", "selector", (1, 1, 1, 2, 1, P, 0, P, 0, P, 0, P2), -1,
          "qr_lstsq(Q,R,y): Under-determined systems not supported. Use rrqr instead."),
         ("dqrls_batched", "stride", (2, 2, 2, 2, 1, P, 3, P, 4, P, 2, P2), -1, "nd4hip_dqrls_batched" + STRIDE),
         ("dqrls_batched", "stride", (2, 2, 2, 2, 1, P, 4, P, 4, P, 1, P2), -1, "nd4hip_dqrls_batched" + STRIDE)]
ROWS += _family("dsvdls_batched", (), 5, (P, 0, P, 0, P, 0, P, 0, P2))
ROWS += [("dsvdls_batched", "stride", (2, 2, 2, 2, 1, P, 4, P, 1, P, 4, P, 2, P2), -1, "nd4hip_dsvdls_batched" + STRIDE)]
# ---- Cholesky, LDL^T, pivoted LDL^T
for _op in ("dpotrf_batched", "dldltrf_batched"):                                   # (batch, N, S, L)
    ROWS += _family(_op, (), 2, (P, P2))
for _op in ("dpotrs_batched", "dldltrs_batched"):                                   # (batch, N, J, L, strideL, Y, strideY, X)
    ROWS += _family(_op, (), 3, (P, 0, P, 0, P2))
    ROWS += [(_op, "stride", (2, 2, 1, P, 3, P, 2, P2), -1, "nd4hip_" + _op + STRIDE),
             (_op, "stride", (2, 2, 1, P, 4, P, 1, P2), -1, "nd4hip_" + _op + STRIDE)]
ROWS += _family("dsytrf_bk_batched", (), 2, (P, P2, Q))                             # (batch, N, S, LD, P[, tier])
ROWS += _family("dsytrf_bk_batched_ex", (), 2, (P, P2, Q), tail=(0,))
ROWS += [("dsytrf_bk_batched_ex", "selector", (1, 2, P, P2, Q, 4), -1, "nd4hip_dsytrf_bk_batched: unknown tier 4"),
         ("dsytrf_bk_batched_ex", "selector", (1, 2, P, P2, Q, -1), -1, "nd4hip_dsytrf_bk_batched: unknown tier -1"),
         ("dsytrf_bk_batched_ex", "selector", (1, 2049, P, P2, Q, 2), -1, "nd4hip_dsytrf_bk_batched: tier 2 is not available at N = 2049")]
ROWS += _family("dsytrs_bk_batched", (), 3, (P, 0, Q, 0, P, 0, P2))                 # as dgetrs
ROWS += [("dsytrs_bk_batched", "stride", (2, 2, 1, P, 3, Q, 2, P, 2, P2), -1, "nd4hip_dsytrs_bk_batched" + STRIDE),
         ("dsytrs_bk_batched", "stride", (2, 2, 1, P, 4, Q, 1, P, 2, P2), -1, "nd4hip_dsytrs_bk_batched" + STRIDE)]
# ---- structure functions
ROWS += _family("dtranspose_batched", (), 3, (P, P2))                               # (batch, M, N, A, B)
ROWS += _family("dtri_batched", (1, 0), 3, (P, P2))                                 # (upper, k, batch, M, N, A, B)
ROWS += _family("ddiag_batched", (), 2, (1, 0, P, P2))                              # (batch, M, N, offset, A, d)
ROWS += [("ddiag_batched", "selector", (1, 2, 2, 2, P, P2), -1, "nd4hip_ddiag_batched: offset=2 out of the shape [2,2]"),
         ("ddiag_batched", "selector", (1, 2, 3, -2, P, P2), -1, "nd4hip_ddiag_batched: offset=-2 out of the shape [2,3]")]
ROWS += _family("ddiagmat_batched", (), 2, (P, P2))                                 # (batch, N, d, D)
ROWS += _family("dpermute_batched", (0, 0), 3, (P, 0, Q, 0, P2))                    # (cols, inverse, batch, M, N, A, strideA, P, strideP, B)
ROWS += [("dpermute_batched", "stride", (0, 0, 2, 2, 2, P, 3, Q, 2, P2), -1, "nd4hip_dpermute_batched" + STRIDE),
         ("dpermute_batched", "stride", (1, 0, 2, 3, 2, P, 6, Q, 1, P2), -1, "nd4hip_dpermute_batched" + STRIDE),
         ("dpermute_batched", "extent", (0, 0, 1, I31, 1, Z, 0, Z, 0, Z), -1, "nd4hip_dpermute_batched: M and N must fit int32 (P is int32)", "early")]
# ---- reductions to condensed form and QR
ROWS += _family("dgebrd_batched", (), 3, (P, P2, P2, P2))                           # (batch, M, N, A, U, B, V)
ROWS += _family("dgehrd_batched", (), 2, (P, P2, P2))                               # (batch, N, A, U, H)
for _op in ("dgeqrf_q_batched", "dgeqrf_full_batched"):                             # (batch, M, N, A, Q, R)
    ROWS += _family(_op, (), 3, (P, P2, P2))
ROWS += _family("dgeqrf_qty_batched", (), 4, (P, P2))                               # (batch, M, N, L, A, Y)
for _op in ("dgeqp3_batched", "dgeqp3_full_batched"):                               # (batch, M, N, A, Q, R, P)
    ROWS += _family(_op, (), 3, (P, P2, P2, Q))
# ---- strong rank-revealing QR and URV: (batch, M, N, A, dtol, ztol, Q, R, P, rank), (batch, M, N, A, U, R, V, rank)
ROWS += _family("dsrrqr_batched", (), 3, (P, 2.0, 0.0, P2, P2, Q, Q))
ROWS += [("dsrrqr_batched", "selector", (1, 1, 1, P, 0.5, 0.0, P2, P2, Q, Q), -1,
          "srrqr_decomp_full(A,opt): Invalid opt.dtol: a value below 1. Must be >=1."),
         ("dsrrqr_batched", "selector", (1, 1, 1, P, NAN, 0.0, P2, P2, Q, Q), -1, "srrqr_decomp_full(A,opt): Invalid opt.dtol: NaN. Must be >=1."),
         ("dsrrqr_batched", "selector", (1, 1, 1, P, INF, 0.0, P2, P2, Q, Q), -1, "Assertion failed. Invalid dtol: Infinity."),
         ("dsrrqr_batched", "selector", (1, 1, 1, P, 2.0, NAN, P2, P2, Q, Q), -1,
          "srrqr_decomp_full(A,opt): invalid opt.ztol: NaN. Must be non-negative number."),
         ("dsrrqr_batched", "selector", (1, 1, 1, P, 2.0, INF, P2, P2, Q, Q), -1, "Assertion failed. Invalid ztol: Infinity.")]
ROWS += _family("durv_batched", (), 3, (P, P2, P2, P2, Q))
# (batch, I, J, K, L, Jc, U, strideU, R, strideR, V, strideV, rank, strideRank, Y, strideY, X)
ROWS += _family("durvls_batched", (), 6, (P, 0, P, 0, P, 0, Q, 0, P, 0, P2))
ROWS += [("durvls_batched", "selector", (1, 1, 2, 1, 1, 1, P, 0, P, 0, P, 0, Q, 0, P, 0, P2), -1, "Assertion failed."),
         ("durvls_batched", "selector", (1, 1, 1, 2, 1, 1, P, 0, P, 0, P, 0, Q, 0, P, 0, P2), -1, "Assertion failed."),
         ("durvls_batched", "stride", (2, 1, 1, 1, 1, 1, P, 1, P, 1, P, 1, Q, 2, P, 1, P2), -1, "nd4hip_durvls_batched" + STRIDE),
         ("durvls_batched", "stride", (2, 2, 1, 1, 1, 1, P, 1, P, 1, P, 1, Q, 1, P, 2, P2), -1, "nd4hip_durvls_batched" + STRIDE)]
# ---- det, slogdet, det_tri, slogdet_tri, norm: (batch, M, N, A, det | sign, logdet), (batch, N, A, ...), (n, A, out)
ROWS += _family("ddet_batched", (), 3, (P, P2))
ROWS += [("ddet_batched", "selector", (1, 1, 2, P, P2), -1, "det_tri(a): a must be square matrices.")]
ROWS += _family("dslogdet_batched", (), 3, (P, P2, P2))
ROWS += [("dslogdet_batched", "selector", (1, 1, 2, P, P2, P2), -1, "det_tri(A): A must be square matrices.")]
ROWS += _family("ddettri_batched", (), 2, (P, P2))
ROWS += _family("dslogdettri_batched", (), 2, (P, P2, P2))
ROWS += [("dnrmfro", "extent", (-1, P, P2), -1, "nd4hip_dnrmfro: negative extent"),
         ("dnrmfro", "null", (1, Z, Z), -1, "nd4hip_dnrmfro: NULL pointer"),
         ("dnrmfro", "null", (0, Z, Z), -1, "nd4hip_dnrmfro: NULL pointer")]            # n = 0 still writes *out: there is no empty call
# ---- eigenpairs of a Schur form and balancing: N <= 32768 in all four
RANGE = ": extent out of range"
ROWS += _family("dtreval_batched", (), 2, (P, P2), neg_text=RANGE)                                      # (batch, N, T, Lam)
ROWS += [("dtreval_batched", "extent", (1, 32769, Z, Z), -1, "nd4hip_dtreval_batched" + RANGE, "early")]
ROWS += _family("dtrevc_batched", (), 2, (P, P, P2, P2), neg_text=RANGE)                                # (batch, N, Q, T, Lam, V)
ROWS += [("dtrevc_batched", "extent", (1, 32769, Z, Z, Z, Z), -1, "nd4hip_dtrevc_batched" + RANGE, "early")]
ROWS += [("dgebal_batched", "extent", (-1, 1, 2.0, P, P2, P2), -1, "nd4hip_dgebal_batched" + RANGE),     # (batch, N, p, A, D, B)
         ("dgebal_batched", "extent", (1, 32769, 2.0, Z, Z, Z), -1, "nd4hip_dgebal_batched" + RANGE, "early"),
         ("dgebal_batched", "selector", (1, 1, 0.5, P, P2, P2), -1, "nd4hip_dgebal_batched: p must be >= 1"),
         ("dgebal_batched", "selector", (1, 1, NAN, P, P2, P2), -1, "nd4hip_dgebal_batched: p must be >= 1"),
         ("dgebal_batched", "empty", (0, 1, 2.0, Z, Z, Z), 0, None),
         ("dgebal_batched", "null", (1, 1, 2.0, Z, Z, Z), -1, "nd4hip_dgebal_batched: NULL pointer")]
ROWS += [("zgebak_batched", "extent", (-1, 1, P, P, P2), -1, "nd4hip_zgebak_batched" + RANGE),           # (batch, N, D, V, W)
         ("zgebak_batched", "extent", (1, 32769, Z, Z, Z), -1, "nd4hip_zgebak_batched" + RANGE, "early"),
         ("zgebak_batched", "empty", (0, 1, Z, Z, Z), 0, None),
         ("zgebak_batched", "null", (1, 1, Z, Z, Z), -1, "nd4hip_zgebak_batched: NULL pointer", "host"),
         ("zgebak_batched", "null", (1, 1, Z, Z, Z), -1, "nd4hip_zgebak_batched: NULL or aliased pointer", "dev"),
         ("zgebak_batched", "alias", (1, 1, P, P2, P2), -1, "nd4hip_zgebak_batched: NULL or aliased pointer", "dev")]
# ---- Schur decomposition and the nonsymmetric eigenproblem
ROWS += _family("dhseqr_batched", (), 2, (P, P, P2, P2), neg_text=RANGE, tail=(Z,))                      # (batch, N, U, H, Q, T, sweeps_out[, tier])
ROWS += _family("dhseqr_batched_ex", (), 2, (P, P, P2, P2), neg_text=RANGE, tail=(Z, 0))
# the one row that a host form with checks of its own lets through to its first chunk (one matrix of one element is staged, the
# _dev form then refuses the tier with this text before anything is launched): the buffers are real and large enough
ROWS += [("dhseqr_batched_ex", "selector", (1, 1, P, P, P2, P2, Z, 3), -1, "nd4hip_dhseqr_batched: unknown tier 3"),
         ("dhseqr_batched_ex", "selector", (1, 1, P, P, P2, P2, Z, -1), -1, "nd4hip_dhseqr_batched: unknown tier -1")]
ROWS += _family("dgees_batched", (), 2, (P, P2, P2), neg_text=RANGE, tail=(Z,))                          # (batch, N, A, Q, T, sweeps_out)
ROWS += _family("dgeev_batched", (), 2, (P, P2, P2), neg_text=RANGE)                                     # (batch, N, A, Lam, V)
# ---- rank and least squares of a pivoted QR
ROWS += _family("dqp3rank_batched", (), 3, (P, Q))                                                       # (batch, M, N, R, rank)
# (batch, N, M, I, J, Q, strideQ, R, strideR, P, strideP, Y, strideY, X, rank)
ROWS += _family("dqp3ls_batched", (), 5, (P, 0, P, 0, Q, 0, P, 0, P2, Q))
ROWS += [("dqp3ls_batched", "stride", (2, 2, 2, 2, 1, P, 3, P, 4, Q, 2, P, 2, P2, Q), -1, "nd4hip_dqp3ls_batched" + STRIDE),
         ("dqp3ls_batched", "stride", (2, 2, 2, 2, 1, P, 4, P, 4, Q, 1, P, 2, P2, Q), -1, "nd4hip_dqp3ls_batched" + STRIDE)]
# ---- SVD
ROWS += _family("dgesvdj_batched", (), 3, (P, P2, P2, P2), tail=(Z, Z))                                  # (batch, M, N, A, U, sv, V, sweeps_out, offnorm_out)
ROWS += _family("dgesdd_batched", (), 3, (P, P2, P2, P2))
ROWS += _family("dbdsdc_batched", (), 2, (1, P, P, P2, P2, P2))                                          # (batch, K, J, d, e, U2, sv, V2)
ROWS += [("dbdsdc_batched", "selector", (1, 1, 3, P, P, P2, P2, P2), -1, "nd4hip_dbdsdc_batched: B must be K x K or K x (K+1)"),
         ("dbdsdc_batched", "selector", (1, 2, 1, P, P, P2, P2, P2), -1, "nd4hip_dbdsdc_batched: B must be K x K or K x (K+1)")]
# ---- symmetric eigenproblems
ROWS += _family("dsyevd_batched", (), 2, (P, P2, P2))                                                    # (batch, N, S, lambda, V)
ROWS += [("dsyevd_batched", "extent", (1, 2049, P, P2, P2), -1, "nd4hip_dsyevd_batched: the divide & conquer solver takes N <= 2048")]
ROWS += _family("dsyevj_batched", (), 2, (P, P2, P2, Q))                                                 # (batch, N, S, lambda, V, sweeps)
ROWS += [("dsyevj_batched", "extent", (1, 129, P, P2, P2, Q), -1, "nd4hip_dsyevj_batched: the Jacobi route takes N <= 128")]
for _algo in (0, 1):                                                                                     # (algo, batch, N, A, B, strideB, lambda, X, sweeps)
    ROWS += _family("dsygvd_batched", (_algo,), 2, (P, P, 0, P2, P2, Q))
ROWS += [("dsygvd_batched", "selector", (2, 1, 4, P, P, 0, P2, P2, Q), -1, "nd4hip_dsygvd_batched: algo must be 0 (dc) or 1 (jacobi)"),
         ("dsygvd_batched", "extent", (0, 1, 2049, P, P, 0, P2, P2, Q), -1, "nd4hip_dsygvd_batched: the divide & conquer solver takes N <= 2048"),
         ("dsygvd_batched", "extent", (1, 1, 129, P, P, 0, P2, P2, Q), -1, "nd4hip_dsygvd_batched: the Jacobi route takes N <= 128"),
         ("dsygvd_batched", "stride", (0, 1, 4, P, P, 5, P2, P2, Q), -1, "nd4hip_dsygvd_batched: strideB must be N*N or 0")]
ROWS += _family("dsygst_batched", (), 2, (P, P, 0, P2))                                                  # (batch, N, A, L, strideL, C)
ROWS += [("dsygst_batched", "extent", (1, 2049, P, P, 0, P2), -1, "nd4hip_dsygst_batched: N <= 2048"),
         ("dsygst_batched", "stride", (1, 4, P, P, 5, P2), -1, "nd4hip_dsygst_batched: strideL must be N*N or 0")]

# these refuse a bad extent, stride or selector before they look at the handle
ARGS_FIRST = ("zgemm_batched", "dsytrf_bk_batched", "dsytrf_bk_batched_ex", "dsytrs_bk_batched", "dsygvd_batched", "dsygst_batched")
# no stride, tier, algo or shape rule to break
PLAIN = ("dgetrf_batched", "dpotrf_batched", "dldltrf_batched", "dsytrf_bk_batched", "dtranspose_batched", "dtri_batched", "ddiagmat_batched",
         "dgebrd_batched", "dgehrd_batched", "dgeqrf_q_batched", "dgeqrf_full_batched", "dgeqrf_qty_batched", "dgeqp3_batched",
         "dgeqp3_full_batched", "durv_batched", "ddettri_batched", "dslogdettri_batched", "dnrmfro", "dtreval_batched", "dtrevc_batched",
         "zgebak_batched", "dhseqr_batched", "dgees_batched", "dgeev_batched", "dqp3rank_batched", "dgesvdj_batched", "dgesdd_batched", "dsyevd_batched", "dsyevj_batched")


def _forms(row):
    """the entry points the row is asserted for: (name, function) pairs"""
    lib, op, forms = _lib.load(), row[0], row[5] if len(row) > 5 else "both"
    if forms == "early" and not SHARED_CHECKS:
        forms = "dev"              # the one difference between the two layouts: see "early" in the module docstring
    names = {"both": ("nd4hip_%s", "nd4hip_%s_dev"), "early": ("nd4hip_%s", "nd4hip_%s_dev"), "dev": ("nd4hip_%s_dev",), "host": ("nd4hip_%s",)}[forms]
    return [(n % op, getattr(lib, n % op)) for n in names]


def _mismatches(rows, handle):
    lib, bad = _lib.load(), []
    for row in rows:
        op, kind, args, rc, text = row[:5]
        for name, fn in _forms(row):
            got = fn(handle, *args)
            err = lib.nd4hip_last_error().decode() if got != 0 else None
            if (got, err) != (rc, text):
                bad.append("%s%r [%s]: expected %r, got %r" % (name, args, kind, (rc, text), (got, err)))
    return bad


def test_every_two_form_operation_is_in_the_table():
    sigs = _lib.SIGNATURES
    two_form = sorted(n[len("nd4hip_"):] for n in sigs if n + "_dev" in sigs)
    assert len(two_form) >= 45
    kinds = {}
    for row in ROWS:
        kinds.setdefault(row[0], set()).add(row[1])
    assert sorted(kinds) == two_form
    for op in two_form:
        want = {"extent", "null"} | (set() if op == "dnrmfro" else {"empty"})
        assert want <= kinds[op], op
        assert (op in PLAIN) != bool(kinds[op] & {"stride", "selector"}), op
    # the rows are what they say: a NULL or empty row has no pointer, every other row has them all (the "early" rows aside)
    for row in ROWS:
        ptrs = [a for a in row[2] if a is None or isinstance(a, ctypes.c_void_p)]
        if row[1] in ("null", "empty") or (len(row) > 5 and row[5] == "early"):
            assert all(a is None for a in ptrs), row
        else:
            assert sum(a is None for a in ptrs) <= {"dhseqr_batched": 1, "dhseqr_batched_ex": 1, "dgees_batched": 1, "dgesvdj_batched": 2}.get(row[0], 0), row
    assert set(ARGS_FIRST) <= set(two_form)


def test_checks_before_the_handle_agree_in_both_forms():
    """without a device: the operations that validate first refuse a bad extent, stride or selector with a NULL handle, in both
    forms, with the row's code and text"""
    rows = [r for r in ROWS if r[0] in ARGS_FIRST and r[1] in ("extent", "stride", "selector")]
    assert len(rows) >= 20
    assert _mismatches(rows, None) == []


@pytest.mark.gpu
def test_both_forms_refuse_every_row_alike():
    """with a handle: every row, in both forms. Nothing is launched: the calls end in the validation"""
    h = _lib.handle()
    assert _mismatches(ROWS, h.ptr) == []
    h.synchronize()
