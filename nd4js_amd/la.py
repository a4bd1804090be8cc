"""Python host mirror of the reference's `nd.la` hot-path functions (same names, argument meaning and
error text) on top of the C ABI — used by the parity tests and bench.py. The production host is the
JS wrapper nd4js_amd/js/index.js over the N-API shim; both call the same libnd4hip.so entry points.

  matmul2(a, b)        src/la/matmul.js:91-147      -> nd4hip_dgemm_batched, complex128: nd4hip_zgemm_batched
  matmul(*ms)          src/la/matmul.js:150-236     (chain ordering stays on the host)
  qr_decomp(A)         src/la/qr.js:80-145          -> nd4hip_dgeqrf_q_batched
  lu_decomp(A)         src/la/lu.js:24-81           -> nd4hip_dgetrf_batched
  svd_decomp(A)        src/la/svd.js:25             -> nd4hip_dgesvdj_batched; algo='dc' (opt-in): nd4hip_dgesdd_batched
  bidiag_svd(d, e)     src/la/svd_dc.js:169-824     -> nd4hip_dbdsdc_batched
  svd_decomp(A, subset), svd_vals(A), bidiag_svd(d, e, subset), bidiag_svdvals(d, e)   not in the reference (opt-in): selected
                                   singular triplets -> nd4hip_dgesvdx_batched_host, nd4hip_dbdsvdx_batched_host
  eigen_sym(S), eigenvals_sym(S)   planned at src/la/eigen.js:28-30   -> nd4hip_dsyevd_batched; algo='jacobi' (opt-in): nd4hip_dsyevj_batched
                                   subset=(i0, i1) (opt-in): a slice of the descending spectrum -> nd4hip_dsyevx_batched_host
                                   reduction='tridiag' (opt-in): the symmetric reduction of csrc/sytrd.hip -> nd4hip_dsyevd_tr_batched_host, nd4hip_dsyevx_tr_batched_host
  tridiag_factor(S), tridiag_apply_q(F, tau, Z), tridiag_decomp(S)   not in the reference   -> nd4hip_dsytrd_batched_host, nd4hip_dormtr_batched_host
  herm_tridiag_factor(H), herm_tridiag_apply_q(F, tau, Z), herm_tridiag_decomp(H)   complex128 Hermitian H, not in the reference
                                   -> nd4hip_zhetrd_batched_host, nd4hip_zunmtr_batched_host (csrc/hetrd.hip)
  eigen_herm(H, subset), eigenvals_herm(H, subset)   not in the reference   -> nd4hip_zheevd_batched_host, nd4hip_zheevx_batched_host
  herm_cholesky_decomp(H), herm_cholesky_solve(L, Y), ztril_solve(L, Y, adjoint), herm_gen_reduce(A, L)   complex128, not in the reference
                                   -> nd4hip_zpotrf_batched_host, nd4hip_zpotrs_batched_host, nd4hip_ztrsm_batched_host, nd4hip_zhegst_batched_host
  eigen_herm_gen(A, B, subset), eigenvals_herm_gen(A, B, subset)   not in the reference   -> nd4hip_zhegvd_batched_host, nd4hip_zhegvx_batched_host
                                   (csrc/hegv.hip)
  tridiag_eigen(d, e), tridiag_eigenvals(d, e), tridiag_count(d, e, x)   not in the reference   -> nd4hip_dstevx_batched_host, nd4hip_dstcnt_batched_host
                                   interval=(lo, hi) (opt-in, here and in eigen_sym): the eigenvalues in (lo, hi] -> nd4hip_dstevxv_batched_host,
                                   nd4hip_dsyevxv_batched_host, nd4hip_dsyevxv_tr_batched_host
  eigen_sym_gen(A, B), eigenvals_sym_gen(A, B)   A x = lambda B x, not in the reference   -> nd4hip_dsygvd_batched
                                   subset, interval, reduction (opt-in, as eigen_sym's) -> nd4hip_dsygvx_batched_host

Inputs are numpy arrays / nested lists (NDArray analogue: dense, row-major, leading axes = batch).
Only float64 (and int32 promoted to float64 for QR/LU/SVD, as qr.js:31-37, lu.js:27, svd_dc.js:904
do) runs here, plus complex128 (paired with complex128, float64 or int32) in matmul2 / matmul; other
dtypes raise TypeError — there is NO CPU fallback in this package.
"""
import ctypes

import numpy as np

from . import _lib


def _asarray(a, what):
    a = np.asarray(a)
    if a.dtype == np.int32 or a.dtype == np.int64 or a.dtype == np.bool_:
        a = a.astype(np.float64)
    if a.dtype != np.float64:
        raise TypeError("%s: only float64 (or int32 promoted to float64) runs on the GPU path, got %s" % (what, a.dtype))
    return np.ascontiguousarray(a)


def _asarray_mm(a, what):
    """matmul operands: complex128 as it is (interleaved re, im: the reference's ComplexArray._array layout), else _asarray."""
    a = np.asarray(a)
    if a.dtype == np.complex128:
        return np.ascontiguousarray(a)
    if a.dtype.kind == "c":
        raise TypeError("%s: only complex128 runs on the GPU path, got %s" % (what, a.dtype))
    return _asarray(a, what)


def _ptr(a):
    return ctypes.c_void_p(a.ctypes.data)


def _bcast_groups(lead, la, lb, IK, KJ):
    """Flatten NumPy-style broadcasting of the leading axes into (count, offA, sA, offB, sB, offC)
    groups with batch strides in {0, dense} — the job of the odometer at matmul.js:44-70."""
    nb = len(lead)
    la = (1,) * (nb - len(la)) + tuple(la)
    lb = (1,) * (nb - len(lb)) + tuple(lb)
    total = int(np.prod(lead, dtype=np.int64)) if nb else 1
    offA = np.broadcast_to((np.arange(int(np.prod(la, dtype=np.int64)), dtype=np.int64) * IK).reshape(la), lead).reshape(-1)
    offB = np.broadcast_to((np.arange(int(np.prod(lb, dtype=np.int64)), dtype=np.int64) * KJ).reshape(lb), lead).reshape(-1)
    groups, b0 = [], 0
    while b0 < total:
        b1 = b0 + 1
        if b1 < total:
            sA, sB = int(offA[b1] - offA[b0]), int(offB[b1] - offB[b0])
            if sA in (0, IK) and sB in (0, KJ):
                while b1 < total and offA[b1] - offA[b1 - 1] == sA and offB[b1] - offB[b1 - 1] == sB:
                    b1 += 1
            else:
                sA = sB = 0
        else:
            sA = sB = 0
        groups.append((b1 - b0, int(offA[b0]), sA, int(offB[b0]), sB, b0))
        b0 = b1
    return groups


def matmul2(a, b, device=None, out=None):
    """`out`: optional preallocated C-contiguous float64 result (a fresh 128 MiB array costs 8-15 ms of page faults on its first
    write — the OS's price, tools/pcie_fresh.hip — which a caller that reuses buffers does not pay)."""
    a = _asarray_mm(a, "matmul2(a,b)")
    b = _asarray_mm(b, "matmul2(a,b)")
    if a.ndim < 2:
        raise ValueError("A must be at least 2D.")
    if b.ndim < 2:
        raise ValueError("B must be at least 2D.")
    I, K = a.shape[-2:]
    J = b.shape[-1]
    if b.shape[-2] != K:
        raise ValueError("The last dimension of A and the 2nd to last dimension of B do not match.")
    try:
        lead = np.broadcast_shapes(a.shape[:-2], b.shape[:-2])
    except ValueError:
        raise ValueError("Shapes are not broadcast-compatible.")
    ac, bc = a.dtype == np.complex128, b.dtype == np.complex128
    dt = np.complex128 if ac or bc else np.float64
    c = np.empty(tuple(lead) + (I, J), dtype=dt) if out is None else out
    if c.shape != tuple(lead) + (I, J) or c.dtype != dt or not c.flags.c_contiguous:
        raise ValueError("matmul2(a,b,out): out must be a C-contiguous %s array of shape %r" % (np.dtype(dt).name, tuple(lead) + (I, J)))
    h = _lib.handle(device)
    groups = _bcast_groups(tuple(lead), a.shape[:-2], b.shape[:-2], I * K, K * J)
    if ac or bc:
        # strides and offsets count elements of each operand: 16 bytes for a complex one, 8 for a real one
        for cnt, offA, sA, offB, sB, offC in groups:
            _lib.check(h.lib.nd4hip_zgemm_batched(
                h.ptr, int(ac), int(bc), cnt, I, K, J,
                ctypes.c_void_p(a.ctypes.data + a.itemsize * offA), sA,
                ctypes.c_void_p(b.ctypes.data + b.itemsize * offB), sB,
                ctypes.c_void_p(c.ctypes.data + 16 * offC * I * J)))
        return c
    for cnt, offA, sA, offB, sB, offC in groups:
        _lib.check(h.lib.nd4hip_dgemm_batched(
            h.ptr, cnt, I, K, J,
            ctypes.c_void_p(a.ctypes.data + 8 * offA), sA,
            ctypes.c_void_p(b.ctypes.data + 8 * offB), sB,
            ctypes.c_void_p(c.ctypes.data + 8 * offC * I * J)))
    return c


def _product_shape(sa, sb):
    """Shape of matmul2 of operands shaped `sa`, `sb` (leading axes NumPy-broadcast) and its inner extent K."""
    if sb[-2] != sa[-1]:
        raise ValueError("Shape mismatch.")
    la_, lb_ = tuple(sa[:-2]), tuple(sb[:-2])
    rank = max(len(la_), len(lb_))
    la_, lb_ = (1,) * (rank - len(la_)) + la_, (1,) * (rank - len(lb_)) + lb_
    if any(x != y and x != 1 and y != 1 for x, y in zip(la_, lb_)):
        raise ValueError("Shapes are not broadcast-compatible.")
    return tuple(y if x == 1 else x for x, y in zip(la_, lb_)) + (sa[-2], sb[-1]), sa[-1]


def chain_plan(shapes):
    """Matrix-chain ordering (CLRS 15.2) generalised to broadcast leading axes: the cost of one product is
    numel(result)·K multiply-adds, as matmul.js:150-236 counts it. Returns `cut` with cut[lo][hi] = last operand
    of the left factor of the cheapest split of operands lo..hi (the first one among equals, in double
    arithmetic like the reference's Number). The shape of a sub-chain does not depend on how it is split, so one
    shape per span is enough."""
    n = len(shapes)
    shape = [[None] * n for _ in range(n)]
    cost = [[0.0] * n for _ in range(n)]
    cut = [[-1] * n for _ in range(n)]
    for k in range(n):
        shape[k][k] = tuple(shapes[k])
    for width in range(1, n):
        for lo in range(n - width):
            hi = lo + width
            best = float("inf")
            for mid in range(lo, hi):
                shp, K = _product_shape(shape[lo][mid], shape[mid + 1][hi])
                numel = 1.0
                for e in shp:
                    numel *= e
                c = numel * K + (cost[lo][mid] + cost[mid + 1][hi])
                if c < best:
                    best, cut[lo][hi], shape[lo][hi] = c, mid, shp
            if cut[lo][hi] < 0:
                raise ValueError("Integer overflow (too many FLOPs).")
            cost[lo][hi] = best
    return cut


def matmul(*matrices, device=None, _matmul2=None):
    """Product of a chain of matrices in the FLOP-optimal order (contract of matmul.js:150-236): one operand
    is returned as is, two go straight to matmul2, longer chains are parenthesised by `chain_plan`."""
    ms = [_asarray_mm(m, "matmul(...)") for m in matrices]
    mm = _matmul2 or (lambda x, y: matmul2(x, y, device))
    if len(ms) == 1:
        return ms[0]
    if len(ms) == 2:
        return mm(ms[0], ms[1])
    cut = chain_plan([m.shape for m in ms])

    def evaluate(lo, hi):
        if lo == hi:
            return ms[lo]
        return mm(evaluate(lo, cut[lo][hi]), evaluate(cut[lo][hi] + 1, hi))
    return evaluate(0, len(ms) - 1)


def qr_decomp(A, device=None):
    A = _asarray(A, "qr_decomp(A)")
    if A.ndim < 2:
        raise ValueError("qr_decomp(A): A.ndim must be at least 2.")
    M, N = A.shape[-2:]
    L = min(M, N)
    batch = int(np.prod(A.shape[:-2], dtype=np.int64))
    Q = np.empty(A.shape[:-2] + (M, L))
    R = np.empty(A.shape[:-2] + (L, N))
    h = _lib.handle(device)
    _lib.check(h.lib.nd4hip_dgeqrf_q_batched(h.ptr, batch, M, N, _ptr(A), _ptr(Q), _ptr(R)))
    return Q, R


def qr_decomp_full(A, device=None):
    """qr.js:27-77: Q [..., M, M], R [..., M, N]."""
    A = _asarray(A, "qr_decomp_full(A)")
    if A.ndim < 2:
        raise ValueError("A must be at least 2D.")
    M, N = A.shape[-2:]
    batch = int(np.prod(A.shape[:-2], dtype=np.int64))
    Q = np.empty(A.shape[:-2] + (M, M))
    R = np.empty(A.shape[:-2] + (M, N))
    h = _lib.handle(device)
    _lib.check(h.lib.nd4hip_dgeqrf_full_batched(h.ptr, batch, M, N, _ptr(A), _ptr(Q), _ptr(R)))
    return Q, R


def qr_decomp_inplace(A, Y, device=None):
    """_qr_decomp_inplace (qr.js:146-183) on writable float64 arrays A [..., M, N] and Y [..., M, L] with equal leading
    dims: A <- R, Y <- Q^T Y, in place like the reference. Returns (A, Y)."""
    for a, n in ((A, "A"), (Y, "Y")):
        if not (isinstance(a, np.ndarray) and a.dtype == np.float64 and a.flags.c_contiguous and a.flags.writeable):
            raise TypeError("qr_decomp_inplace: %s must be a writable C-contiguous float64 ndarray" % n)
    if A.ndim < 2 or Y.ndim < 2 or A.shape[:-1] != Y.shape[:-1]:
        raise ValueError("Assertion failed.")                      # the reference's only message (qr.js:148-166)
    M, N = A.shape[-2:]
    L = Y.shape[-1]
    batch = int(np.prod(A.shape[:-2], dtype=np.int64))
    h = _lib.handle(device)
    _lib.check(h.lib.nd4hip_dgeqrf_qty_batched(h.ptr, batch, M, N, L, _ptr(A), _ptr(Y)))
    return A, Y


def lu_decomp(A, device=None):
    A = _asarray(A, "lu_decomp(A)")
    if A.ndim < 2 or A.shape[-1] != A.shape[-2]:
        raise ValueError("Last two dimensions must be quadratic.")
    N = A.shape[-1]
    batch = int(np.prod(A.shape[:-2], dtype=np.int64))
    LU = np.empty_like(A)
    P = np.empty(A.shape[:-1], dtype=np.int32)
    h = _lib.handle(device)
    _lib.check(h.lib.nd4hip_dgetrf_batched(h.ptr, batch, N, _ptr(A), _ptr(LU), _ptr(P)))
    return LU, P


def _svd_algo(algo):
    """None / 'jacobi': block one-sided Jacobi (the default route); 'dc': bidiagonalisation + divide & conquer, the
    reference's own algorithm (svd_dc.js), opt-in"""
    if algo is None or algo == "jacobi":
        return False
    if algo == "dc":
        return True
    raise ValueError("svd_decomp(A, algo): algo must be None, 'jacobi' or 'dc'.")


def _svd_subset(subset, L, what, jacobi):
    """(i0, i1) of subset=(i0, i1), the half-open slice sv[i0:i1] of the descending singular values, 0 <= i0 <= i1 <= L"""
    if jacobi:
        raise ValueError("%s: subset is not available with algo='jacobi'." % what)
    try:
        return _subset(subset, L, what)
    except ValueError:
        raise ValueError("%s: subset must be (i0, i1) with 0 <= i0 <= i1 <= min(M, N), got %r for min(M, N) = %d." % (what, subset, L)) from None


def _gesvdx(A, what, subset, vectors, device, info):
    """the selected-triplet route (csrc/bdsvdx.hip): bidiagonalisation, bisection and inverse iteration on the Golub-Kahan form"""
    A = np.asarray(A)
    if np.iscomplexobj(A):
        raise TypeError("%s: A.dtype must be float." % what)
    A = _asarray(A, what)
    if A.ndim < 2:
        raise ValueError("%s: A.ndim must be at least 2." % what)
    M, N = A.shape[-2:]
    L = min(M, N)
    if L > 2048:
        raise ValueError("%s: min(M, N) <= 2048." % what)
    lead = A.shape[:-2]
    i0, i1 = (0, L) if subset is None else _svd_subset(subset, L, what, False)
    k = i1 - i0
    sv = np.empty(lead + (k,))
    U = np.empty(lead + (M, k)) if vectors else None
    V = np.empty(lead + (k, N)) if vectors else None
    fb = np.zeros(lead, dtype=np.int32)
    if sv.size:
        h = _lib.handle(device)
        _lib.check(h.lib.nd4hip_dgesvdx_batched_host(h.ptr, int(np.prod(lead, dtype=np.int64)), M, N, i0, i1, _ptr(A), _ptr(U) if vectors else None,
                                                     _ptr(sv), _ptr(V) if vectors else None, _ptr(fb) if info is not None else None))
    if info is not None:
        info["fallback"] = fb
    return (U, sv, V) if vectors else sv


def svd_decomp(A, device=None, info=None, algo=None, subset=None):
    """subset=(i0, i1) (opt-in): the triplets sv[i0:i1] of the descending singular values alone, U [..., M, k], sv [..., k],
    V [..., k, N], by bidiagonalisation, bisection and inverse iteration (csrc/bdsvdx.hip); algo None or 'dc'."""
    dc = _svd_algo(algo)
    if subset is not None:
        if algo == "jacobi":
            _svd_subset(subset, 0, "svd_decomp(A, subset)", True)
        return _gesvdx(A, "svd_decomp(A, subset)", subset, True, device, info)
    A = np.asarray(A)
    if np.iscomplexobj(A):
        raise TypeError("svd_dc(A): A.dtype must be float.")
    A = _asarray(A, "svd_decomp(A)")
    if A.ndim < 2:
        raise ValueError("svd_decomp(A): A.ndim must be at least 2.")
    M, N = A.shape[-2:]
    L = min(M, N)
    batch = int(np.prod(A.shape[:-2], dtype=np.int64))
    U = np.empty(A.shape[:-2] + (M, L))
    sv = np.empty(A.shape[:-2] + (L,))
    V = np.empty(A.shape[:-2] + (L, N))
    sweeps, off = ctypes.c_int(0), ctypes.c_double(0.0)
    h = _lib.handle(device)
    if dc:
        _lib.check(h.lib.nd4hip_dgesdd_batched(h.ptr, batch, M, N, _ptr(A), _ptr(U), _ptr(sv), _ptr(V)))
        return U, sv, V
    _lib.check(h.lib.nd4hip_dgesvdj_batched(h.ptr, batch, M, N, _ptr(A), _ptr(U), _ptr(sv), _ptr(V),
                                            ctypes.byref(sweeps), ctypes.byref(off)))
    if info is not None:
        info["sweeps"], info["offnorm"] = sweeps.value, off.value
        info["rotations"] = h.svd_last_info()["rotations"]
    return U, sv, V


svd_dc = svd_decomp


def svd_vals(A, device=None, info=None, subset=None):
    """The singular values of A [..., M, N] alone, descending (subset=(i0, i1): sv[i0:i1]): no vectors are formed and no product
    runs. The bits of the sv of svd_decomp(A, subset). min(M, N) <= 2048."""
    return _gesvdx(A, "svd_vals(A)", subset, False, device, info)


def _bidiag_operands(d, e, what, asarray):
    d, e = asarray(d, what), asarray(e, what)
    if d.ndim < 1 or e.ndim < 1 or tuple(d.shape[:-1]) != tuple(e.shape[:-1]):
        raise ValueError("%s: d and e must have the same leading dimensions." % what)
    K, J = d.shape[-1], e.shape[-1] + 1
    if K < 1 or J not in (K, K + 1):
        raise ValueError("%s: e must have len(d) - 1 or len(d) entries." % what)
    return d, e, K, J


def _bdsvdx(d, e, what, subset, vectors, device, info):
    """the selected-triplet solver on a bidiagonal matrix (csrc/bdsvdx.hip)"""
    d, e, K, J = _bidiag_operands(d, e, what, _asarray)
    if K > 2048:
        raise ValueError("%s: K <= 2048." % what)
    i0, i1 = (0, K) if subset is None else _subset(subset, K, what)
    lead, k = d.shape[:-1], i1 - i0
    sv = np.empty(lead + (k,))
    U2 = np.empty(lead + (K, k)) if vectors else None
    V2 = np.empty(lead + (k, J)) if vectors else None
    fb = np.zeros(lead, dtype=np.int32)
    if sv.size:
        h = _lib.handle(device)
        _lib.check(h.lib.nd4hip_dbdsvdx_batched_host(h.ptr, int(np.prod(lead, dtype=np.int64)), K, J, i0, i1, _ptr(d), _ptr(e),
                                                     _ptr(U2) if vectors else None, _ptr(sv), _ptr(V2) if vectors else None,
                                                     _ptr(fb) if info is not None else None))
    if info is not None:
        info["fallback"] = fb
    return (U2, sv, V2) if vectors else sv


def bidiag_svd(d, e, device=None, subset=None, info=None):
    """SVD of the upper bidiagonal K x J matrix with diagonal d [..., K] and super-diagonal e [..., J-1], J = K or K + 1 (the
    shapes bidiag_decomp produces), by the reference's divide & conquer (svd_dc.js:169-824):
    (U2 [..., K, K], sv [..., K] >= 0 descending, V2 [..., J, J] with rows = right vectors), B = U2 diag(sv) V2[:K].
    subset=(i0, i1) (opt-in): the triplets sv[i0:i1] alone, (U2 [..., K, k], sv [..., k], V2 [..., k, J]), by bisection and inverse
    iteration on the Golub-Kahan form (csrc/bdsvdx.hip); info['fallback'] (int32 [...]) marks the members that went through the
    divide & conquer solver instead (their sv is still the bisection's). K <= 2048 there."""
    if subset is not None:
        return _bdsvdx(d, e, "bidiag_svd(d,e, subset)", subset, True, device, info)
    d, e, K, J = _bidiag_operands(d, e, "bidiag_svd(d,e)", _asarray)
    lead = d.shape[:-1]
    U2, sv, V2 = np.empty(lead + (K, K)), np.empty(lead + (K,)), np.empty(lead + (J, J))
    h = _lib.handle(device)
    _lib.check(h.lib.nd4hip_dbdsdc_batched(h.ptr, int(np.prod(lead, dtype=np.int64)), K, J, _ptr(d), _ptr(e), _ptr(U2), _ptr(sv), _ptr(V2)))
    return U2, sv, V2


def bidiag_svdvals(d, e, device=None, subset=None, info=None):
    """The singular values sv[i0:i1] (subset=None: all) of the bidiagonal matrix of bidiag_svd, descending, by bisection alone: the
    bits of the sv of bidiag_svd(d, e, subset). K <= 2048."""
    return _bdsvdx(d, e, "bidiag_svdvals(d,e)", subset, False, device, info)


# ---------------------------------------------------------------------------------------------------
# solve-side consumers of the path, device kernels in csrc/trsm.hip
# ---------------------------------------------------------------------------------------------------
def _bcast_groups_n(lead, shapes, units):
    """n-operand form of _bcast_groups: yields (count, [offset_k], [stride_k], out_index) with every stride in
    {0, units[k]} (what the odometers at lu.js:148-163 / tri.js:193-215 do one matrix at a time)."""
    nb = len(lead)
    total = int(np.prod(lead, dtype=np.int64)) if nb else 1
    offs = []
    for shp, unit in zip(shapes, units):
        shp = (1,) * (nb - len(shp)) + tuple(shp)
        offs.append(np.broadcast_to((np.arange(int(np.prod(shp, dtype=np.int64)), dtype=np.int64) * unit).reshape(shp), lead).reshape(-1))
    groups, b0 = [], 0
    while b0 < total:
        b1, strides = b0 + 1, [0] * len(offs)
        if b1 < total:
            cand = [int(o[b1] - o[b0]) for o in offs]
            if all(c in (0, u) for c, u in zip(cand, units)):
                strides = cand
                while b1 < total and all(int(o[b1] - o[b1 - 1]) == c for o, c in zip(offs, cand)):
                    b1 += 1
        groups.append((b1 - b0, [int(o[b0]) for o in offs], strides, b0))
        b0 = b1
    return groups


def _off(a, elems, itemsize=8):
    return ctypes.c_void_p(a.ctypes.data + itemsize * elems)


def _tri_solve(upper, T, Y, name, device=None):
    T = _asarray(T, name)
    Y = _asarray(Y, name)
    if T.ndim < 2:
        raise ValueError("%s: %s.ndim must be at least 2." % (name, "U" if upper else "L"))
    if Y.ndim < 2:
        raise ValueError("%s: Y.ndim must be at least 2." % name)
    M, J = Y.shape[-2:]
    if T.shape[-2] != M:
        raise ValueError("%s: %s and Y don't match." % (name, "U" if upper else "L"))
    if T.shape[-1] != M:
        raise ValueError("%s: Last two dimensions of %s must be quadratic." % (name, "U" if upper else "L"))
    try:
        lead = np.broadcast_shapes(T.shape[:-2], Y.shape[:-2])
    except ValueError:
        raise ValueError("%s: %s and Y not broadcast-compatible." % (name, "U" if upper else "L"))
    X = np.empty(tuple(lead) + (M, J))
    h = _lib.handle(device)
    for cnt, (oT, oY), (sT, sY), b0 in _bcast_groups_n(tuple(lead), [T.shape[:-2], Y.shape[:-2]], [M * M, M * J]):
        _lib.check(h.lib.nd4hip_dtrsm_batched(h.ptr, 1 if upper else 0, 0, cnt, M, J, _off(T, oT), sT, _off(Y, oY), sY, _off(X, b0 * M * J)))
    return X


def tril_solve(L, Y, device=None):
    """tri.js:155-221"""
    return _tri_solve(False, L, Y, "tril_solve(L,Y)", device)


def triu_solve(U, Y, device=None):
    """tri.js:224-290"""
    return _tri_solve(True, U, Y, "triu_solve(U,Y)", device)


def lu_solve(LU, P, y=None, device=None):
    """lu.js:84-177; accepts lu_solve((LU,P), y) like the reference (:86)."""
    if y is None:
        y = P
        LU, P = LU
    LU = _asarray(LU, "lu_solve")
    P = np.ascontiguousarray(np.asarray(P), dtype=np.int32)
    y = _asarray(y, "lu_solve")
    if LU.ndim < 2:
        raise ValueError("LU must be at least 2D.")
    if P.ndim < 1:
        raise ValueError("P must be at least 1D.")
    if y.ndim < 2:
        raise ValueError("y must be at least 2D.")
    N = LU.shape[-2]
    I, J = y.shape[-2:]
    if LU.shape[-1] != N:
        raise ValueError("Last two dimensions of LU must be quadratic.")
    if N != I:
        raise ValueError("LU and y don't match.")
    if P.shape[-1] != N:
        raise ValueError("LU and P don't match.")
    try:
        lead = np.broadcast_shapes(LU.shape[:-2], y.shape[:-2])
    except ValueError:
        raise ValueError("LU and y are not broadcast-compatible.")
    try:
        lead = np.broadcast_shapes(lead, P.shape[:-1])
    except ValueError:
        raise ValueError("P is not broadcast-compatible.")
    X = np.empty(tuple(lead) + (N, J))
    h = _lib.handle(device)
    for cnt, (oLU, oP, oY), (sLU, sP, sY), b0 in _bcast_groups_n(tuple(lead), [LU.shape[:-2], P.shape[:-1], y.shape[:-2]], [N * N, N, N * J]):
        _lib.check(h.lib.nd4hip_dgetrs_batched(h.ptr, cnt, N, J, _off(LU, oLU), sLU, _off(P, oP, 4), sP, _off(y, oY), sY, _off(X, b0 * N * J)))
    return X


def qr_lstsq(Q, R, y=None, device=None):
    """qr.js:186-273; accepts qr_lstsq((Q,R), y) like the reference (:188)."""
    if y is None:
        y = R
        Q, R = Q
    Q, R, y = np.asarray(Q), np.asarray(R), np.asarray(y)
    if Q.ndim < 2:
        raise ValueError("qr_lstsq(Q,R,y): Q.ndim must be at least 2.")
    if R.ndim < 2:
        raise ValueError("qr_lstsq(Q,R,y): R.ndim must be at least 2.")
    if y.ndim < 2:
        raise ValueError("qr_lstsq(Q,R,y): y.ndim must be at least 2.")
    Q, R, y = _asarray(Q, "qr_lstsq"), _asarray(R, "qr_lstsq"), _asarray(y, "qr_lstsq")
    N, M = Q.shape[-2:]
    I, J = R.shape[-1], y.shape[-1]
    if N != y.shape[-2]:
        raise ValueError("qr_lstsq(Q,R,y): Q and y don't match.")
    if M != R.shape[-2]:
        raise ValueError("qr_lstsq(Q,R,y): Q and R don't match.")
    if I > N:
        raise ValueError("qr_lstsq(Q,R,y): Under-determined systems not supported. Use rrqr instead.")
    try:
        lead = np.broadcast_shapes(Q.shape[:-2], R.shape[:-2], y.shape[:-2])
    except ValueError:
        raise ValueError("Q, R, y are not broadcast-compatible.")
    X = np.empty(tuple(lead) + (I, J))
    h = _lib.handle(device)
    for cnt, (oQ, oR, oY), (sQ, sR, sY), b0 in _bcast_groups_n(tuple(lead), [Q.shape[:-2], R.shape[:-2], y.shape[:-2]], [N * M, M * I, N * J]):
        _lib.check(h.lib.nd4hip_dqrls_batched(h.ptr, cnt, N, M, I, J, _off(Q, oQ), sQ, _off(R, oR), sR, _off(y, oY), sY, _off(X, b0 * I * J)))
    return X


def svd_rank(sv):
    """svd.js:31-63: per matrix, the first r with |sv_r| <= sqrt(eps) |sv_0| (host side: sv is tiny)."""
    sv = np.asarray(sv, dtype=np.float64)
    N = sv.shape[-1]
    with np.errstate(invalid="ignore"):
        small = np.abs(sv) <= np.sqrt(2.0 ** -52) * np.abs(sv[..., :1])
    rank = np.where(small.any(axis=-1), small.argmax(axis=-1), N).astype(np.int32)
    # the reference's loop only looks at the entries up to the cut (and at the cut itself): a NaN behind it does not raise
    seen = np.arange(N) <= rank[..., None]
    if not np.all(np.isfinite(sv[seen])):
        raise ValueError("svd_rank(): NaN or Infinity encountered.")
    return rank


def svd_lstsq(U, sv, V=None, y=None, device=None):
    """svd.js:100-228; accepts svd_lstsq((U,sv,V), y) like the reference (:102-108)."""
    if y is None:
        if V is not None:
            raise ValueError("svd_lstsq(Q,R,P, y): Either 2 ([Q,R,P], y) or 4 arguments (Q,R,P, y) expected.")
        y = sv
        U, sv, V = U
    U, sv, V, y = np.asarray(U), np.asarray(sv), np.asarray(V), np.asarray(y)
    if U.ndim < 2:
        raise ValueError("svd_lstsq(U,sv,V, y): U.ndim must be at least 2.")
    if sv.ndim < 1:
        raise ValueError("svd_lstsq(U,sv,V, y): sv.ndim must be at least 1.")
    if V.ndim < 2:
        raise ValueError("svd_lstsq(U,sv,V, y): V.ndim must be at least 2.")
    if y.ndim < 2:
        raise ValueError("svd_lstsq(U,sv,V, y): y.ndim must be at least 2.")
    U, sv, V, y = (_asarray(a, "svd_lstsq") for a in (U, sv, V, y))
    N, M = U.shape[-2:]
    I, J = V.shape[-1], y.shape[-1]
    if N != y.shape[-2]:
        raise ValueError("svd_lstsq(U,sv,V, y): U and y don't match.")
    if M != sv.shape[-1]:
        raise ValueError("svd_lstsq(U,sv,V, y): U and sv don't match.")
    if M != V.shape[-2]:
        raise ValueError("svd_lstsq(U,sv,V, y): V and sv don't match.")
    try:
        lead = np.broadcast_shapes(U.shape[:-2], V.shape[:-2], y.shape[:-2], sv.shape[:-1])
    except ValueError:
        raise ValueError("svd_lstsq(U,sv,V, y): U,sv,V,y not broadcast-compatible.")
    if not np.all(np.isfinite(sv)):
        raise ValueError("svd_solve(): NaN or Infinity encountered.")      # svd.js:171-172 (the reference's own wording)
    X = np.empty(tuple(lead) + (I, J))
    h = _lib.handle(device)
    for cnt, (oU, oS, oV, oY), (sU, sS, sV, sY), b0 in _bcast_groups_n(
            tuple(lead), [U.shape[:-2], sv.shape[:-1], V.shape[:-2], y.shape[:-2]], [N * M, M, M * I, N * J]):
        _lib.check(h.lib.nd4hip_dsvdls_batched(h.ptr, cnt, N, M, I, J, _off(U, oU), sU, _off(sv, oS), sS, _off(V, oV), sV,
                                               _off(y, oY), sY, _off(X, b0 * I * J)))
    return X


def svd_solve(U, sv, V=None, y=None, device=None):
    """svd.js:66-97. The reference's singularity loop (`for( let r; r < N; r++ )`, :85) never executes, so apart from
    the squareness check this IS svd_lstsq; mirrored as such."""
    if y is None:
        if V is not None:
            raise ValueError("svd_lstsq(Q,R,P, y): Either 2 ([Q,R,P], y) or 4 arguments (Q,R,P, y) expected.")
        y = sv
        U, sv, V = U
    if np.asarray(U).shape[-2] != np.asarray(V).shape[-1]:
        raise ValueError("rrqr_solve(Q,R,P, y): System not square.")
    return svd_lstsq(U, sv, V, y, device=device)


def cholesky_decomp(S, device=None):
    """cholesky.js:51-71: L with S = L L^T, strict upper part zero; only the lower triangle of S is read."""
    S = _asarray(S, "cholesky_decomp(S)")
    if S.ndim < 2 or S.shape[-1] != S.shape[-2]:
        raise ValueError("Last two dimensions must be quadratic.")
    N = S.shape[-1]
    L = np.empty_like(S)
    h = _lib.handle(device)
    try:
        _lib.check(h.lib.nd4hip_dpotrf_batched(h.ptr, int(np.prod(S.shape[:-2], dtype=np.int64)), N, _ptr(S), _ptr(L)))
    except _lib.Nd4HipError as e:
        if e.code == -5:
            # cholesky.js:43-44; a multi-device handle adds which of its devices reported it
            where = str(e)[str(e).find(" (device "):] if " (device " in str(e) else ""
            raise ValueError("Matrix contains NaNs or is (near) singular." + where)
        raise
    return L


def cholesky_solve(L, y, device=None):
    """cholesky.js:74-150"""
    L, y = np.asarray(L), np.asarray(y)
    if L.ndim < 2:
        raise ValueError("L must be at least 2D.")
    if y.ndim < 2:
        raise ValueError("y must be at least 2D.")
    L, y = _asarray(L, "cholesky_solve"), _asarray(y, "cholesky_solve")
    N, M = L.shape[-2:]
    I, J = y.shape[-2:]
    if N != M:
        raise ValueError("Last two dimensions of L must be quadratic.")
    if I != M:
        raise ValueError("L and y don't match.")
    try:
        lead = np.broadcast_shapes(L.shape[:-2], y.shape[:-2])
    except ValueError:
        raise ValueError("Shapes are not broadcast-compatible.")
    X = np.empty(tuple(lead) + (N, J))
    h = _lib.handle(device)
    for cnt, (oL, oY), (sL, sY), b0 in _bcast_groups_n(tuple(lead), [L.shape[:-2], y.shape[:-2]], [N * N, N * J]):
        _lib.check(h.lib.nd4hip_dpotrs_batched(h.ptr, cnt, N, J, _off(L, oL), sL, _off(y, oY), sY, _off(X, b0 * N * J)))
    return X


def ldl_decomp(S, device=None):
    """ldl.js:67-90: packed LD (unit-lower L below the diagonal, D on it, zeros above), S = L D L^T, no pivoting."""
    S = _asarray(S, "ldl_decomp(S)")
    if S.ndim < 2 or S.shape[-1] != S.shape[-2]:
        raise ValueError("Last two dimensions must be quadratic.")
    LD = np.empty_like(S)
    h = _lib.handle(device)
    _lib.check(h.lib.nd4hip_dldltrf_batched(h.ptr, int(np.prod(S.shape[:-2], dtype=np.int64)), S.shape[-1], _ptr(S), _ptr(LD)))
    return LD


def ldl_solve(LD, y, device=None):
    """ldl.js:133-201"""
    LD, y = np.asarray(LD), np.asarray(y)
    if LD.ndim < 2:
        raise ValueError("ldl_solve(LD,y): LD must be at least 2D.")
    if y.ndim < 2:
        raise ValueError("ldl_solve(LD,y): y must be at least 2D.")
    LD, y = _asarray(LD, "ldl_solve"), _asarray(y, "ldl_solve")
    N, M = LD.shape[-2:]
    I, J = y.shape[-2:]
    if N != M:
        raise ValueError("ldl_solve(LD,y): Last two dimensions of LD must be quadratic.")
    if I != M:
        raise ValueError("ldl_solve(LD,y): LD and y don't match.")
    try:
        lead = np.broadcast_shapes(LD.shape[:-2], y.shape[:-2])
    except ValueError:
        raise ValueError("Shapes are not broadcast-compatible.")
    X = np.empty(tuple(lead) + (N, J))
    h = _lib.handle(device)
    for cnt, (oL, oY), (sL, sY), b0 in _bcast_groups_n(tuple(lead), [LD.shape[:-2], y.shape[:-2]], [N * N, N * J]):
        _lib.check(h.lib.nd4hip_dldltrs_batched(h.ptr, cnt, N, J, _off(LD, oL), sL, _off(y, oY), sY, _off(X, b0 * N * J)))
    return X


def hessenberg_decomp(A, device=None):
    """hessenberg.js:89-115: (U, H) with A = U H U^T, H upper Hessenberg."""
    A = np.asarray(A)
    if A.ndim < 2:
        raise ValueError("hessenberg_decomp(A): A must at least be 2D.")
    A = _asarray(A, "hessenberg_decomp(A)")
    N = A.shape[-1]
    if A.shape[-2] != N:
        raise ValueError("hessenberg_decomp(A): A must be square.")
    U, H = np.empty_like(A), np.empty_like(A)
    h = _lib.handle(device)
    _lib.check(h.lib.nd4hip_dgehrd_batched(h.ptr, int(np.prod(A.shape[:-2], dtype=np.int64)), N, _ptr(A), _ptr(U), _ptr(H)))
    return U, H


def bidiag_decomp(A, device=None):
    """bidiag.js:245-319: (U [..., M, I], B [..., I, J], V [..., J, N]) with A = U B V, B upper bidiagonal."""
    A = np.asarray(A)
    if A.ndim < 2:
        raise ValueError("bidiag_decomp(A): A must be at least 2D.")
    if np.iscomplexobj(A):
        raise ValueError("bidiag_decomp(A): complex A not yet supported.")
    A = _asarray(A, "bidiag_decomp(A)")
    M, N = A.shape[-2:]
    I = min(M, N)
    J = I if M >= N else I + 1
    lead = A.shape[:-2]
    U, B, V = np.empty(lead + (M, I)), np.empty(lead + (I, J)), np.empty(lead + (J, N))
    h = _lib.handle(device)
    _lib.check(h.lib.nd4hip_dgebrd_batched(h.ptr, int(np.prod(lead, dtype=np.int64)), M, N, _ptr(A), _ptr(U), _ptr(B), _ptr(V)))
    return U, B, V


# ---------------------------------------------------------------------------------------------------
# Column-pivoted QR (src/la/rrqr.js) and the general solver built on it (src/la/solve.js), csrc/rrqr.hip
# ---------------------------------------------------------------------------------------------------
class SingularMatrixSolveError(ValueError):
    """singular_matrix_solve_error.js: raised by rrqr_solve / solve when a matrix is rank-deficient; `.x` holds the
    least-squares solution that was computed anyway."""

    def __init__(self, x, *args):
        super().__init__(*args)
        self.x = x


def _rrqr(A, full, name, device):
    A = np.asarray(A)
    if A.ndim < 2:
        raise ValueError("A must be at least 2D.")                   # rrqr.js:91 / :281
    A = _asarray(A, name)
    M, N = A.shape[-2:]
    L = M if full else min(M, N)
    lead = A.shape[:-2]
    Q, R = np.empty(lead + (M, L)), np.empty(lead + (L, N))
    P = np.empty(lead + (N,), dtype=np.int32)
    h = _lib.handle(device)
    fn = h.lib.nd4hip_dgeqp3_full_batched if full else h.lib.nd4hip_dgeqp3_batched
    _lib.check(fn(h.ptr, int(np.prod(lead, dtype=np.int64)), M, N, _ptr(A), _ptr(Q), _ptr(R), _ptr(P)))
    return Q, R, P


def rrqr_decomp(A, device=None):
    """rrqr.js:278-395: (Q, R, P) with A[..., :, P] = Q R; Q [..., M, L], R [..., L, N], L = min(M, N)."""
    return _rrqr(A, False, "rrqr_decomp(A)", device)


def rrqr_decomp_full(A, device=None):
    """rrqr.js:88-184: (Q [..., M, M], R [..., M, N], P [..., N])."""
    return _rrqr(A, True, "rrqr_decomp_full(A)", device)


def rrqr_rank(R, device=None):
    """rrqr.js:398-414: int32 ranks of the leading matrices of R (threshold 2 eps max(M,N) ||R||_upper)."""
    R = np.asarray(R)
    if R.ndim < 2:
        raise ValueError("rrqr_rank(R): R.ndim must be at least 2.")
    R = _asarray(R, "rrqr_rank(R)")
    M, N = R.shape[-2:]
    r = np.empty(R.shape[:-2], dtype=np.int32)
    h = _lib.handle(device)
    try:
        _lib.check(h.lib.nd4hip_dqp3rank_batched(h.ptr, int(np.prod(R.shape[:-2], dtype=np.int64)), M, N, _ptr(R), _ptr(r)))
    except _lib.Nd4HipError as e:
        if e.code == -1 and "Infinity or NaN" in str(e):
            raise ValueError("Infinity or NaN encountered during rank estimation.")
        raise
    return r


def _rrqr_args(Q, R, P, y):
    if y is None:
        if P is not None:
            raise ValueError("rrqr_lstsq(Q,R,P, y): Either 2 ([Q,R,P], y) or 4 arguments (Q,R,P, y) expected.")
        y = R
        Q, R, P = tuple(Q)[:3]                                        # srrqr_decomp_full's (Q, R, P, r) works too
    return Q, R, P, y


def _rrqr_lstsq(Q, R, P, y, device):
    """rrqr.js:447-580 -> (X, ranks of the broadcast members)"""
    Q, R, P, y = np.asarray(Q), np.asarray(R), np.asarray(P), np.asarray(y)
    if Q.ndim < 2:
        raise ValueError("rrqr_lstsq(Q,R,P, y): Q.ndim must be at least 2.")
    if R.ndim < 2:
        raise ValueError("rrqr_lstsq(Q,R,P, y): R.ndim must be at least 2.")
    if P.ndim < 1:
        raise ValueError("rrqr_lstsq(Q,R,P, y): P.ndim must be at least 1.")
    if y.ndim < 2:
        raise ValueError("rrqr_lstsq(Q,R,P, y): y.ndim must be at least 2.")
    if P.dtype != np.int32:
        raise ValueError('rrqr_lstsq(Q,R,P, y): P.dtype must be "int32".')
    Q, R, y = _asarray(Q, "rrqr_lstsq"), _asarray(R, "rrqr_lstsq"), _asarray(y, "rrqr_lstsq")
    P = np.ascontiguousarray(P)
    N, M = Q.shape[-2:]
    I, J = R.shape[-1], y.shape[-1]
    if N != y.shape[-2]:
        raise ValueError("rrqr_lstsq(Q,R,P,y): Q and y don't match.")
    if M != R.shape[-2]:
        raise ValueError("rrqr_lstsq(Q,R,P,y): Q and R don't match.")
    if I != P.shape[-1]:
        raise ValueError("rrqr_lstsq(Q,R,P,y): R and P don't match.")
    try:
        lead = np.broadcast_shapes(Q.shape[:-2], R.shape[:-2], y.shape[:-2], P.shape[:-1])
    except ValueError:
        raise ValueError("rrqr_lstsq(Q,R,P,y): Q,R,P,y not broadcast-compatible.")
    X = np.empty(tuple(lead) + (I, J))
    ranks = np.empty(tuple(lead), dtype=np.int32)
    h = _lib.handle(device)
    for cnt, (oQ, oR, oP, oY), (sQ, sR, sP, sY), b0 in _bcast_groups_n(
            tuple(lead), [Q.shape[:-2], R.shape[:-2], P.shape[:-1], y.shape[:-2]], [N * M, M * I, I, N * J]):
        try:
            _lib.check(h.lib.nd4hip_dqp3ls_batched(h.ptr, cnt, N, M, I, J, _off(Q, oQ), sQ, _off(R, oR), sR, _off(P, oP, 4), sP,
                                                   _off(y, oY), sY, _off(X, b0 * I * J), _off(ranks, b0, 4)))
        except _lib.Nd4HipError as e:
            msg = str(e)
            for text in ("Infinity or NaN encountered during rank estimation.", "rrqr_lstsq(Q,R,P,y): Invalid indices in P."):
                if e.code == -1 and text in msg:
                    raise ValueError(text)
            raise
    return X, ranks


def rrqr_lstsq(Q, R, P=None, y=None, device=None):
    """rrqr.js:447-580; accepts rrqr_lstsq((Q,R,P), y) like the reference (:449-454)."""
    Q, R, P, y = _rrqr_args(Q, R, P, y)
    return _rrqr_lstsq(Q, R, P, y, device)[0]


def rrqr_solve(Q, R, P=None, y=None, device=None):
    """rrqr.js:417-444: rrqr_lstsq of a square Q @ R; raises SingularMatrixSolveError (with .x) when a rank is < N."""
    Q, R, P, y = _rrqr_args(Q, R, P, y)
    Q, R = np.asarray(Q), np.asarray(R)
    N = Q.shape[-2]
    if N != R.shape[-1]:
        raise ValueError("rrqr_solve(Q,R,P, y): Q @ R not square.")
    x, ranks = _rrqr_lstsq(Q, R, P, y, device)
    if np.any(ranks < N):
        raise SingularMatrixSolveError(x)
    return x


def solve(A, y, device=None):
    """solve.js:23-27: rrqr_solve(rrqr_decomp(A), y)."""
    Q, R, P = rrqr_decomp(A, device=device)
    return rrqr_solve(Q, R, P, y, device=device)


# ---------------------------------------------------------------------------------------------------
# Strong rank-revealing QR (src/la/srrqr.js), csrc/srrqr.hip
# ---------------------------------------------------------------------------------------------------
def _js_num(x):
    """a number as the reference's template strings print it"""
    x = float(x)
    if x != x:
        return "NaN"
    if x in (float("inf"), float("-inf")):
        return "Infinity" if x > 0 else "-Infinity"
    return str(int(x)) if x == int(x) and abs(x) < 1e21 else repr(x)


def _srrqr_opts(opt, dtol, ztol):
    """srrqr.js:186-225: (dtol, ztol) for the C ABI; ztol -1 selects the reference's default"""
    opt = dict(opt or {})
    if dtol is not None:
        opt["dtol"] = dtol
    if ztol is not None:
        opt["ztol"] = ztol
    d = opt.get("dtol", 1.01)
    z = opt.get("ztol", None)
    if isinstance(d, np.ndarray):
        raise ValueError("srrqr_decomp_full(A,opt): NDArray as opt.dtol not yet supported.")
    d = float(d)
    if not d >= 1:
        raise ValueError("srrqr_decomp_full(A,opt): Invalid opt.dtol: %s. Must be >=1." % _js_num(d))
    if isinstance(z, np.ndarray):
        raise ValueError("srrqr_decomp_full(A,opt): NDArray as opt.ztol not yet supported.")
    if z is not None:
        z = float(z)
        if not z >= 0:
            raise ValueError("srrqr_decomp_full(A,opt): invalid opt.ztol: %s. Must be non-negative number." % _js_num(z))
    if d == float("inf"):                                             # srrqr.js:601-604, per matrix, after the option checks
        raise ValueError("Assertion failed. Invalid dtol: Infinity.")
    if z == float("inf"):
        raise ValueError("Assertion failed. Invalid ztol: Infinity.")
    return d, (-1.0 if z is None else z)


def _arg_error(e):
    """the reference's message of an ND4HIP_ERR_ARG raised by the library (the text after 'nd4hip error -1: ')"""
    return ValueError(str(e).split(": ", 1)[1]) if e.code == -1 else e


def srrqr_decomp_full(A, opt=None, dtol=None, ztol=None, device=None):
    """srrqr.js:58-802: (Q [..., M, M], R [..., M, N], P [..., N] int32, r [...] int32) with A[..., :, P] = Q R and r the
    rank found by the strong RRQR. `opt` is the reference's {dtol, ztol}; dtol / ztol may also be given as keywords."""
    A = np.asarray(A)
    if A.ndim < 2:
        raise ValueError("srrqr_decomp_full(A,opt): A must be at least 2D.")
    if np.iscomplexobj(A):
        raise ValueError("srrqr_decomp_full(A,opt): Complex A not (yet) supported.")
    d, z = _srrqr_opts(opt, dtol, ztol)
    A = _asarray(A, "srrqr_decomp_full(A,opt)")
    M, N = A.shape[-2:]
    lead = A.shape[:-2]
    Q, R = np.empty(lead + (M, M)), np.empty(lead + (M, N))
    P = np.empty(lead + (N,), dtype=np.int32)
    r = np.empty(lead, dtype=np.int32)
    h = _lib.handle(device)
    try:
        _lib.check(h.lib.nd4hip_dsrrqr_batched(h.ptr, int(np.prod(lead, dtype=np.int64)), M, N, _ptr(A), d, z, _ptr(Q), _ptr(R),
                                               _ptr(P), _ptr(r)))
    except _lib.Nd4HipError as e:
        raise _arg_error(e)
    return Q, R, P, r


# ---------------------------------------------------------------------------------------------------
# URV (src/la/urv.js), csrc/srrqr.hip
# ---------------------------------------------------------------------------------------------------
def urv_decomp_full(A, device=None):
    """urv.js:100-135: (U [..., M, M], R [..., M, N], V [..., N, N], ranks [...] int32) with A = U R V and
    R = [[T, 0], [0, 0]], T upper triangular of size rank."""
    A = np.asarray(A)
    if A.ndim < 2:
        raise ValueError("srrqr_decomp_full(A,opt): A must be at least 2D.")
    if np.iscomplexobj(A):
        raise ValueError("srrqr_decomp_full(A,opt): Complex A not (yet) supported.")
    A = _asarray(A, "urv_decomp_full(A)")
    M, N = A.shape[-2:]
    lead = A.shape[:-2]
    U, R, V = np.empty(lead + (M, M)), np.empty(lead + (M, N)), np.empty(lead + (N, N))
    r = np.empty(lead, dtype=np.int32)
    h = _lib.handle(device)
    try:
        _lib.check(h.lib.nd4hip_durv_batched(h.ptr, int(np.prod(lead, dtype=np.int64)), M, N, _ptr(A), _ptr(U), _ptr(R), _ptr(V), _ptr(r)))
    except _lib.Nd4HipError as e:
        raise _arg_error(e)
    return U, R, V, r


def urv_lstsq(U, R, V=None, ranks=None, Y=None, device=None):
    """urv.js:138-323: the minimum-norm least-squares X = V[:r]^T T^-1 (U^T Y)[:r] per (broadcast) matrix; accepts
    urv_lstsq((U, R, V, ranks), Y) like the reference (:200-206)."""
    if Y is None:
        if ranks is not None or V is not None:
            raise ValueError("urv_lstsq( U,R,V,ranks, Y ): Either 2 ([U,R,V,ranks], Y) or 5 arguments (U,R,V,ranks, Y) expected.")
        Y = R
        U, R, V, ranks = U
    U, R, V, Y = np.asarray(U), np.asarray(R), np.asarray(V), np.asarray(Y)
    for x, n in ((U, "U"), (R, "R"), (V, "V"), (Y, "Y")):
        if x.ndim < 2:
            raise ValueError("urv_lstsq(U,R,V, Y): %s.ndim must be at least 2." % n)
    ranks = np.asarray(ranks)
    U, R, V, Y = (_asarray(x, "urv_lstsq") for x in (U, R, V, Y))
    ranks = np.array(ranks, dtype=np.int32, order="C")                 # (keeps a 0-d rank 0-d)
    try:
        lead = np.broadcast_shapes(U.shape[:-2], R.shape[:-2], V.shape[:-2], Y.shape[:-2], ranks.shape)
    except ValueError:
        raise ValueError("urv_lstsq( U,R,V,ranks, Y ): U,R,V,ranks, Y not broadcast-compatible.")
    I, J = U.shape[-2:]
    K, L = V.shape[-2:]
    Jc = Y.shape[-1]
    if R.shape[-2] != J or R.shape[-1] != K or Y.shape[-2] != I:
        raise ValueError("urv_lstsq( U,R,V,ranks, Y ): Matrix dimensions incompatible.")
    if J != K and ((I < L and I != J) or (I >= L and K != L)):
        raise ValueError("Assertion failed.")
    if not (I >= J) or not (K <= L):
        raise ValueError("Assertion failed.")
    X = np.zeros(tuple(lead) + (L, Jc))
    h = _lib.handle(device)
    for cnt, (oU, oR, oV, oK, oY), (sU, sR, sV, sK, sY), b0 in _bcast_groups_n(
            tuple(lead), [U.shape[:-2], R.shape[:-2], V.shape[:-2], ranks.shape, Y.shape[:-2]], [I * J, J * K, K * L, 1, I * Jc]):
        try:
            _lib.check(h.lib.nd4hip_durvls_batched(h.ptr, cnt, I, J, K, L, Jc, _off(U, oU), sU, _off(R, oR), sR, _off(V, oV), sV,
                                                   _off(ranks, oK, 4), sK, _off(Y, oY), sY, _off(X, b0 * L * Jc)))
        except _lib.Nd4HipError as e:
            raise _arg_error(e)
    return X


# ---------------------------------------------------------------------------------------------------
# Determinants, rank, lstsq and norm (src/la/det.js, rank.js, lstsq.js, norm.js), csrc/det.hip
# ---------------------------------------------------------------------------------------------------
def _det_args(A, what):
    A = np.asarray(A)
    if A.ndim < 2:
        raise ValueError("qr_decomp(A): A.ndim must be at least 2.")        # det.js:97 / :104 go through qr_decomp first
    M, N = A.shape[-2:]
    if M < N:                                                            # qr_decomp succeeds, det_tri rejects its M x N R
        raise ValueError(what)
    return _asarray(A, "det(A)"), M, N


def det(A, device=None):
    """det.js:95-99: det_tri(qr_decomp(A)[1]) -> float64 [...] (0-d for one matrix). Square N <= 64 runs the reference's own
    Givens elimination (bit-identical); larger and tall inputs take qr_decomp's R without Q."""
    A, M, N = _det_args(A, "det_tri(a): a must be square matrices.")
    D = np.empty(A.shape[:-2])
    h = _lib.handle(device)
    try:
        _lib.check(h.lib.nd4hip_ddet_batched(h.ptr, int(np.prod(A.shape[:-2], dtype=np.int64)), M, N, _ptr(A), _ptr(D)))
    except _lib.Nd4HipError as e:
        raise _arg_error(e)
    return D


def slogdet(A, device=None):
    """det.js:102-106: [sign, logdet] of slogdet_tri(qr_decomp(A)[1])."""
    A, M, N = _det_args(A, "det_tri(A): A must be square matrices.")
    S, L = np.empty(A.shape[:-2]), np.empty(A.shape[:-2])
    h = _lib.handle(device)
    try:
        _lib.check(h.lib.nd4hip_dslogdet_batched(h.ptr, int(np.prod(A.shape[:-2], dtype=np.int64)), M, N, _ptr(A), _ptr(S), _ptr(L)))
    except _lib.Nd4HipError as e:
        raise _arg_error(e)
    return [S, L]


def _dettri_args(A, ndim_msg, square_msg):
    A = np.asarray(A)
    if A.ndim < 2:
        raise ValueError(ndim_msg)
    M, N = A.shape[-2:]
    if M != N:
        raise ValueError(square_msg)
    return _asarray(A, "det_tri(a)"), N


def det_tri(A, device=None):
    """det.js:24-50: the product of each matrix's diagonal in index order."""
    a = np.asarray(A)
    A, N = _dettri_args(a, "det_tri(a): a.shape=[%s]; a.ndim must be at least 2." % ",".join(str(s) for s in a.shape),
                        "det_tri(a): a must be square matrices.")
    D = np.empty(A.shape[:-2])
    h = _lib.handle(device)
    _lib.check(h.lib.nd4hip_ddettri_batched(h.ptr, int(np.prod(A.shape[:-2], dtype=np.int64)), N, _ptr(A), _ptr(D)))
    return D


def slogdet_tri(A, device=None):
    """det.js:53-92: [sign, logdet] with Math.sign's signed zeros and NaN, the log-sum in index order."""
    A, N = _dettri_args(A, "det_tri(A): A.ndim must be at least 2.", "det_tri(A): A must be square matrices.")
    S, L = np.empty(A.shape[:-2]), np.empty(A.shape[:-2])
    h = _lib.handle(device)
    _lib.check(h.lib.nd4hip_dslogdettri_batched(h.ptr, int(np.prod(A.shape[:-2], dtype=np.int64)), N, _ptr(A), _ptr(S), _ptr(L)))
    return [S, L]


def rank(A, device=None):
    """rank.js:23-27: svd_rank(svd_decomp(A)[1])."""
    return svd_rank(svd_decomp(A, device=device)[1])


def lstsq(A, y, device=None):
    """lstsq.js:22-26: svd_lstsq(...svd_decomp(A), y)."""
    U, sv, V = svd_decomp(A, device=device)
    return svd_lstsq(U, sv, V, y, device=device)


def norm(A, ord="fro", axis=None, device=None):
    """norm.js:74-85 (FrobeniusNorm :22-71): the Frobenius norm of the whole array as a Python float."""
    A = np.asarray(A)
    if not (isinstance(ord, str) and ord == "fro"):
        o = "null" if ord is None else ord if isinstance(ord, str) else _js_num(ord)
        raise ValueError("norm(A,ord,axis): Unsupported ord: %s." % o)
    if axis is not None:
        raise ValueError("norm(A,ord,axis): axis argument not yet supported.")
    A = _asarray(A, "norm(A)")
    out = ctypes.c_double(0.0)
    h = _lib.handle(device)
    _lib.check(h.lib.nd4hip_dnrmfro(h.ptr, A.size, _ptr(A), ctypes.byref(out)))
    return out.value


# ---------------------------------------------------------------------------------------------------
# Eigenpairs of a real Schur form and balancing (src/la/schur.js:31-370, eigen.js:91-270), csrc/eigvec.hip
# ---------------------------------------------------------------------------------------------------
def _ev_call(fn, *args):
    try:
        _lib.check(fn(*args))
    except _lib.Nd4HipError as e:
        raise _arg_error(e)


def schur_eigenvals(T, device=None):
    """schur.js:31-87: the eigenvalues of a quasi-triangular T [..., N, N] -> complex128 [..., N], the reference's bits."""
    T = np.asarray(T)
    if T.ndim < 2 or T.shape[-2] != T.shape[-1]:
        raise ValueError("T is not square.")
    T = _asarray(T, "schur_eigenvals(T)")
    N = T.shape[-1]
    L = np.empty(T.shape[:-1], dtype=np.complex128)
    h = _lib.handle(device)
    _ev_call(h.lib.nd4hip_dtreval_batched, h.ptr, int(np.prod(T.shape[:-2], dtype=np.int64)), N, _ptr(T), _ptr(L))
    return L


def schur_eigen(Q, T, device=None):
    """schur.js:90-370: [eigenvalues complex128 [..., N], Q V complex128 [..., N, N]] with V the unit-norm eigenvectors of the
    quasi-triangular T by the reference's back-substitution."""
    Q, T = np.asarray(Q), np.asarray(T)
    if Q.ndim != T.ndim:
        raise ValueError("Q.ndim != T.ndim.")
    if Q.shape != T.shape:
        raise ValueError("Q.shape != T.shape.")
    if T.ndim < 2 or T.shape[-2] != T.shape[-1]:
        raise ValueError("Q is not square.")                               # the reference's text for a non-square T (schur.js:150)
    Q, T = _asarray(Q, "schur_eigen(Q,T)"), _asarray(T, "schur_eigen(Q,T)")
    N = T.shape[-1]
    L = np.empty(T.shape[:-1], dtype=np.complex128)
    V = np.empty(T.shape, dtype=np.complex128)
    h = _lib.handle(device)
    _ev_call(h.lib.nd4hip_dtrevc_batched, h.ptr, int(np.prod(T.shape[:-2], dtype=np.int64)), N, _ptr(Q), _ptr(T), _ptr(L), _ptr(V))
    return [L, V]


def eigen_balance_pre(A, p=2, device=None):
    """eigen.js:91-226: [D [..., N], B [..., N, N]] with B = diag(D)^-1 A diag(D), D powers of two that balance the p-norms of
    every off-diagonal row and column (p >= 1, or Infinity for the max-norm variant)."""
    if p is None:
        p = 2
    p = float(p)
    if not p >= 1:
        raise ValueError("Invalid norm p=%s;" % _js_num(p))
    A = np.asarray(A)
    if A.ndim < 2 or A.shape[-2] != A.shape[-1]:
        raise ValueError("A is not square")
    A = _asarray(A, "eigen_balance_pre(A,p)")
    N = A.shape[-1]
    D, B = np.empty(A.shape[:-1]), np.empty(A.shape)
    h = _lib.handle(device)
    _ev_call(h.lib.nd4hip_dgebal_batched, h.ptr, int(np.prod(A.shape[:-2], dtype=np.int64)), N, p, _ptr(A), _ptr(D), _ptr(B))
    return [D, B]


def eigen_balance_post(D, V, device=None):
    """eigen.js:229-270: diag(D) V with columns of unit 2-norm, complex128 [..., N, N]; D [..., N] real, V complex128 or real."""
    D, V = np.asarray(D), np.asarray(V)
    if V.ndim < 2:
        raise ValueError("eigen_balance_post(D,V): V.ndim must be at least 2.")
    if V.shape[-2] != V.shape[-1]:
        raise ValueError("eigen_balance_post(D,V): V must be square.")
    V = _asarray_mm(V, "eigen_balance_post(D,V)")
    D = _asarray(D, "eigen_balance_post(D,V)")
    lead = np.broadcast_shapes(D.shape[:-1], V.shape[:-2])
    N = V.shape[-1]
    if D.shape[-1] != N:
        raise ValueError("Shapes are not broadcast-compatible.")
    D = np.ascontiguousarray(np.broadcast_to(D, tuple(lead) + (N,)))
    V = np.ascontiguousarray(np.broadcast_to(V, tuple(lead) + (N, N)).astype(np.complex128))
    W = np.empty(V.shape, dtype=np.complex128)
    h = _lib.handle(device)
    _ev_call(h.lib.nd4hip_zgebak_batched, h.ptr, int(np.prod(lead, dtype=np.int64)), N, _ptr(D), _ptr(V), _ptr(W))
    return W


# ---------------------------------------------------------------------------------------------------
# schur_decomp (src/la/schur.js:372-683), eigen and eigenvals (src/la/eigen.js:33-88), csrc/schur.hip
# ---------------------------------------------------------------------------------------------------
SCHUR_TIERS = {None: 0, "auto": 0, "lds": 1, "global": 2}


def _schur_tier(tier):
    if tier not in SCHUR_TIERS:
        raise ValueError("schur_qrfrancis(U,H): unknown tier %r (auto, lds or global)." % (tier,))
    return SCHUR_TIERS[tier]


def schur_qrfrancis(U, H, tier=None, device=None, sweeps=False):
    """schur.js:388-683 (the reference's private schur_qrfrancis_inplace, returning new arrays): the real Schur decomposition
    [Q, T] of U H U^T from a Hessenberg decomposition (U, H) [..., N, N] by the reference's Francis iteration, its bits. `tier`
    picks where the kernel keeps the matrices ('lds': N <= 65, 'global': any N <= 2048; the same bits); sweeps=True appends the
    most sweeps one francis_qr call took."""
    U, H = np.asarray(U), np.asarray(H)
    if U.ndim < 2 or U.shape[-2] != U.shape[-1]:
        raise ValueError("Q is not square.")
    if U.ndim != H.ndim:
        raise ValueError("Q.ndim != H.ndim.")
    if U.shape != H.shape:
        raise ValueError("Q.shape != H.shape.")
    t = _schur_tier(tier)
    U, H = _asarray(U, "schur_qrfrancis(U,H)"), _asarray(H, "schur_qrfrancis(U,H)")
    N = U.shape[-1]
    Q, T = np.empty_like(U), np.empty_like(H)
    sw = ctypes.c_int(0)
    h = _lib.handle(device)
    _ev_call(h.lib.nd4hip_dhseqr_batched_ex, h.ptr, int(np.prod(U.shape[:-2], dtype=np.int64)), N, _ptr(U), _ptr(H), _ptr(Q), _ptr(T),
             ctypes.byref(sw), t)
    return [Q, T, sw.value] if sweeps else [Q, T]


def schur_decomp(A, device=None, sweeps=False):
    """schur.js:372-381: [Q, T] with A = Q T Q^T, Q orthogonal and T quasi-triangular with complex-eigenvalued 2x2 blocks only:
    hessenberg_decomp, then the Francis iteration, on the device without a round trip."""
    A = np.asarray(A)
    if A.ndim < 2:
        raise ValueError("hessenberg_decomp(A): A must at least be 2D.")
    A = _asarray(A, "schur_decomp(A)")
    N = A.shape[-1]
    if A.shape[-2] != N:
        raise ValueError("hessenberg_decomp(A): A must be square.")
    Q, T = np.empty_like(A), np.empty_like(A)
    sw = ctypes.c_int(0)
    h = _lib.handle(device)
    _ev_call(h.lib.nd4hip_dgees_batched, h.ptr, int(np.prod(A.shape[:-2], dtype=np.int64)), N, _ptr(A), _ptr(Q), _ptr(T), ctypes.byref(sw))
    return [Q, T, sw.value] if sweeps else [Q, T]


def _geev(A, what, vectors, device):
    A = np.asarray(A)
    if A.ndim < 2 or A.shape[-2] != A.shape[-1]:
        raise ValueError("A is not square")                                # eigen_balance_pre's text (eigen.js:91-100)
    A = _asarray(A, what)
    N = A.shape[-1]
    L = np.empty(A.shape[:-1], dtype=np.complex128)
    V = np.empty(A.shape, dtype=np.complex128) if vectors else None
    h = _lib.handle(device)
    _ev_call(h.lib.nd4hip_dgeev_batched, h.ptr, int(np.prod(A.shape[:-2], dtype=np.int64)), N, _ptr(A), _ptr(L), _ptr(V) if vectors else None)
    return [L, V] if vectors else L


def eigen(A, device=None):
    """eigen.js:33-80: [eigenvalues complex128 [..., N], eigenvectors complex128 [..., N, N] with unit columns]: balancing with
    p = 2, schur_decomp, schur_eigen, then the balancing undone, all on the device."""
    return _geev(A, "eigen(A)", True, device)


def eigenvals(A, device=None):
    """eigen.js:83-88: schur_eigenvals of the Schur form of the balanced matrix, complex128 [..., N]."""
    return _geev(A, "eigenvals(A)", False, device)


def _eigsym_algo(algo, what):
    """True for the Jacobi route (csrc/syevj.hip, N <= 128, opt-in); None / 'dc' is the default route (csrc/syev.hip)"""
    if algo is None or algo == "dc":
        return False
    if algo == "jacobi":
        return True
    raise ValueError("%s: algo must be None, 'dc' or 'jacobi'." % what.replace("(S)", "(S, algo)"))


def _subset(subset, N, what, jacobi=False):
    """(i0, i1) of subset=(i0, i1), the half-open slice lambda[i0:i1] of the descending spectrum, 0 <= i0 <= i1 <= N"""
    if jacobi:
        raise ValueError("%s: subset is not available with algo='jacobi'." % what)
    try:
        i0, i1 = subset
        i0, i1 = int(i0), int(i1)
        ok = (i0, i1) == tuple(subset)
    except (TypeError, ValueError):
        ok = False
    if not ok or not 0 <= i0 <= i1 <= N:
        raise ValueError("%s: subset must be (i0, i1) with 0 <= i0 <= i1 <= N, got %r for N = %d." % (what, subset, N))
    return i0, i1


def _interval_what(what, jacobi, subset):
    """the text that names a call with interval=(lo, hi), after the two refusals that need no operand"""
    what = what.replace("(S)", "(S, interval)").replace("(d,e)", "(d,e, interval)")
    if jacobi:
        raise ValueError("%s: interval is not available with algo='jacobi'." % what)
    if subset is not None:
        raise ValueError("%s: interval and subset exclude each other." % what)
    return what


def _interval(interval, lead, what):
    """bounds float64 [..., 2] = (lo, hi) of interval=(lo, hi), which selects the eigenvalues lo < lambda <= hi: lo and hi are scalars
    or arrays that broadcast to the leading dimensions `lead`; lo <= hi; NaN is refused, +-inf is a bound like any other"""
    try:
        lo, hi = interval
        lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("%s: interval must be (lo, hi), got %r." % (what, interval)) from None
    if np.isnan(lo).any() or np.isnan(hi).any():
        raise ValueError("%s: interval contains NaN." % what)
    try:
        lo, hi = np.broadcast_to(lo, lead), np.broadcast_to(hi, lead)
    except ValueError:
        raise ValueError("%s: interval must broadcast to the leading dimensions %r." % (what, tuple(lead))) from None
    if (lo > hi).any():
        raise ValueError("%s: interval must satisfy lo <= hi." % what)
    return np.ascontiguousarray(np.stack((lo, hi), axis=-1))


def _interval_call(name, device, N, bounds, operands, vshape, info):
    """the interval entry point `name` with kcap = N: (L [..., N], vectors of shape vshape or None (vshape None), kmax): the first
    kmax entries along the selected axis are the results; info['range'] = int32 [..., 2]"""
    lead = bounds.shape[:-1]
    L = np.empty(lead + (N,))
    Zs = np.empty(vshape) if vshape is not None else None
    ranges = np.zeros(lead + (2,), dtype=np.int32)
    kmax = ctypes.c_int64(0)
    if L.size:
        h = _lib.handle(device)
        _lib.check(getattr(h.lib, name)(h.ptr, int(np.prod(lead, dtype=np.int64)), N, N, _ptr(bounds), *[_ptr(a) for a in operands], _ptr(L),
                                        _ptr(Zs) if Zs is not None else None, _ptr(ranges), ctypes.byref(kmax)))
    if info is not None:
        info["range"] = ranges
    return L, Zs, kmax.value


def _reduction(reduction, what, jacobi):
    """True for reduction='tridiag' (csrc/sytrd.hip, opt-in); None / 'hessenberg' is the default reduction (csrc/hess.hip)"""
    what = what.replace("(S)", "(S, reduction)")
    if reduction is None or reduction == "hessenberg":
        return False
    if reduction != "tridiag":
        raise ValueError("%s: reduction must be None, 'hessenberg' or 'tridiag'." % what)
    if jacobi:
        raise ValueError("%s: reduction is not available with algo='jacobi'." % what)
    return True


def _syevd(S, what, vectors, device, algo=None, info=None, subset=None, reduction=None, interval=None):
    jacobi = _eigsym_algo(algo, what)
    tr = _reduction(reduction, what, jacobi)
    if interval is not None:
        what = _interval_what(what, jacobi, subset)
    elif subset is not None:
        what = what.replace("(S)", "(S, subset)")
        if jacobi:
            _subset(subset, 0, what, True)
    S = np.asarray(S)
    if np.iscomplexobj(S):
        raise TypeError("%s: S.dtype must be float." % what)
    if S.ndim < 2:
        raise ValueError("%s: S.ndim must be at least 2." % what)
    if S.shape[-2] != S.shape[-1]:
        raise ValueError("%s: S must be quadratic." % what)
    S = _asarray(S, what)
    N = S.shape[-1]
    batch = int(np.prod(S.shape[:-2], dtype=np.int64))
    if interval is not None:                                                # the same, the subset of each member chosen by value
        bounds = _interval(interval, S.shape[:-2], what)
        L, V, k = _interval_call("nd4hip_dsyevxv_tr_batched_host" if tr else "nd4hip_dsyevxv_batched_host", device, N, bounds, (S,),
                                 S.shape if vectors else None, info)
        L = np.ascontiguousarray(L[..., :k])
        return (L, np.ascontiguousarray(V[..., :k])) if vectors else L
    if subset is not None:                                                  # bisection and inverse iteration (csrc/syevx.hip)
        i0, i1 = _subset(subset, N, what)
        L = np.empty(S.shape[:-2] + (i1 - i0,))
        V = np.empty(S.shape[:-1] + (i1 - i0,)) if vectors else None
        if L.size:
            h = _lib.handle(device)
            fn = h.lib.nd4hip_dsyevx_tr_batched_host if tr else h.lib.nd4hip_dsyevx_batched_host
            _lib.check(fn(h.ptr, batch, N, i0, i1, _ptr(S), _ptr(L), _ptr(V) if vectors else None))
        return (L, V) if vectors else L
    L = np.empty(S.shape[:-1])
    V = np.empty(S.shape) if vectors else None
    h = _lib.handle(device)
    if tr:                                                                  # the symmetric reduction (csrc/sytrd.hip)
        _lib.check(h.lib.nd4hip_dsyevd_tr_batched_host(h.ptr, batch, N, _ptr(S), _ptr(L), _ptr(V) if vectors else None))
    elif jacobi:
        sweeps = np.zeros(S.shape[:-2], dtype=np.int32)
        _lib.check(h.lib.nd4hip_dsyevj_batched(h.ptr, batch, N, _ptr(S), _ptr(L), _ptr(V) if vectors else None, sweeps.ctypes.data))
        if info is not None:
            info["sweeps"] = sweeps
    else:
        _lib.check(h.lib.nd4hip_dsyevd_batched(h.ptr, batch, N, _ptr(S), _ptr(L), _ptr(V) if vectors else None))
    return (L, V) if vectors else L


def eigen_sym(S, device=None, algo=None, info=None, subset=None, reduction=None, interval=None):
    """the function the reference plans at eigen.js:28-30: (eigenvalues float64 [..., N] descending, eigenvectors float64
    [..., N, N] as columns) of the symmetric S, S V = V diag(L) and V^T V = I. Only the lower triangle of S is read. NaN or
    Infinity there raises Nd4HipError with code -3. N <= 2048.
    algo None / 'dc': tridiagonalisation + divide & conquer (the default route). algo 'jacobi' (opt-in, N <= 128): every member by
    cyclic two-sided Jacobi inside one launch; for positive definite S every eigenvalue, however small, is accurate to
    N eps kappa_2(D^-1 S D^-1) relative to itself, D = diag(sqrt s_ii). `info` (a dict) then receives 'sweeps', int32 [...].
    subset=(i0, i1) (opt-in, not with 'jacobi'): only L[i0:i1] of the descending spectrum and the matching columns of V, k = i1 - i0
    of them: (L [..., k], V [..., N, k]), by bisection and inverse iteration on the tridiagonal form (tridiag_eigen below).
    reduction='tridiag' (opt-in, not with 'jacobi'; None / 'hessenberg': the default): the tridiagonal form by tridiag_factor below,
    straight from the lower triangle, and the eigenvectors by tridiag_apply_q, 2 N^2 k flops for k of them.
    interval=(lo, hi) (opt-in, not with subset or 'jacobi'; combines with reduction): the eigenvalues lo < lambda <= hi of every member,
    lo and hi scalars or arrays that broadcast to the leading dimensions of S, lo <= hi, +-inf allowed, NaN refused. Member b gets
    subset=(i0_b, i1_b) = (count(hi), count(lo)) with tridiag_count's count on its tridiagonal form, and the bits of that subset call.
    The results are ragged: (L [..., kmax], V [..., N, kmax]) with kmax the largest k_b = i1_b - i0_b; a member's k_b pairs stand
    first, then NaN in L and zero columns in V. `info` receives 'range', int32 [..., 2], the (i0_b, i1_b)."""
    return _syevd(S, "eigen_sym(S)", True, device, algo, info, subset, reduction, interval)


def eigenvals_sym(S, device=None, algo=None, info=None, subset=None, reduction=None, interval=None):
    """the eigenvalues of eigen_sym alone (the same bits); no eigenvector product is computed or stored. With algo='jacobi' no
    eigenvector is accumulated at all; with subset or interval no inverse iteration is made; with reduction='tridiag' no Q is applied."""
    return _syevd(S, "eigenvals_sym(S)", False, device, algo, info, subset, reduction, interval)


def _tridiag_s(S_ndim, S_shape, what):
    """the shape checks of tridiag_factor / tridiag_decomp, shared with dev.py; returns N"""
    if S_ndim < 2:
        raise ValueError("%s: S.ndim must be at least 2." % what)
    if S_shape[-2] != S_shape[-1]:
        raise ValueError("%s: S must be quadratic." % what)
    if S_shape[-1] > 2048:
        raise ValueError("%s: N <= 2048." % what)
    return int(S_shape[-1])


def _tridiag_fz(F_shape, tau_shape, Z_shape, what):
    """the shape checks of tridiag_apply_q, shared with dev.py; returns (N, K)"""
    if len(F_shape) < 2 or F_shape[-2] != F_shape[-1]:
        raise ValueError("%s: F must be quadratic." % what)
    N = int(F_shape[-1])
    if N > 2048:
        raise ValueError("%s: N <= 2048." % what)
    lead = tuple(F_shape[:-2])
    if len(tau_shape) < 1 or tuple(tau_shape) != lead + (max(N - 1, 0),):
        raise ValueError("%s: tau must be [..., N - 1] with the leading dimensions of F." % what)
    if len(Z_shape) < 2 or tuple(Z_shape[:-1]) != lead + (N,):
        raise ValueError("%s: Z must be [..., N, K] with the leading dimensions of F." % what)
    return N, int(Z_shape[-1])


def tridiag_factor(S, device=None):
    """(F [..., N, N], tau [..., max(N-1, 0)], d [..., N], e [..., max(N-1, 0)]) with S = Q tridiag(d, e) Q^T for the symmetric float64 S,
    read only in its lower triangle: Q = H_0 H_1 ... H_{N-3}, H_k = I - tau_k v_k v_k^T, v_k zero in rows 0..k, 1 in row k+1, its tail in
    F[k+2:, k] (LAPACK's dsytrd, lower). F carries d on its diagonal, e on its first subdiagonal and zeros above. e_k = -sign(alpha) |x|
    for the column x = [alpha; tail] (sign(0) = +1); a column whose tail is zero gets tau_k = 0 and e_k = alpha. NaN or Infinity in the
    lower triangle raises Nd4HipError with code -3. N <= 2048 (csrc/sytrd.hip)."""
    what = "tridiag_factor(S)"
    S = np.asarray(S)
    if np.iscomplexobj(S):
        raise TypeError("%s: S.dtype must be float." % what)
    N = _tridiag_s(S.ndim, S.shape, what)
    S = _asarray(S, what)
    lead, ne = S.shape[:-2], max(N - 1, 0)
    F, tau, d, e = np.empty(S.shape), np.empty(lead + (ne,)), np.empty(lead + (N,)), np.empty(lead + (ne,))
    if F.size:
        h = _lib.handle(device)
        _lib.check(h.lib.nd4hip_dsytrd_batched_host(h.ptr, int(np.prod(lead, dtype=np.int64)), N, _ptr(S), _ptr(F), _ptr(tau), _ptr(d), _ptr(e)))
    return F, tau, d, e


def tridiag_apply_q(F, tau, Z, transpose=False, device=None):
    """Q Z (transpose: Q^T Z) for the Q of tridiag_factor's (F, tau) and Z [..., N, K] with the leading dimensions of F. Q is never
    formed: N <= 128 reflector by reflector in LDS, above in compact WY blocks on the GEMM."""
    what = "tridiag_apply_q(F,tau,Z)"
    F, tau, Z = np.asarray(F), np.asarray(tau), np.asarray(Z)
    if np.iscomplexobj(F) or np.iscomplexobj(tau) or np.iscomplexobj(Z):
        raise TypeError("%s: F, tau and Z must be float." % what)
    N, K = _tridiag_fz(F.shape, tau.shape, Z.shape, what)
    F, tau = _asarray(F, what), _asarray(tau, what)
    out = np.array(Z, dtype=np.float64, order="C")                          # a copy: the product is made in place
    if out.size:
        h = _lib.handle(device)
        _lib.check(h.lib.nd4hip_dormtr_batched_host(h.ptr, int(np.prod(F.shape[:-2], dtype=np.int64)), N, K, 1 if transpose else 0, _ptr(F),
                                                    _ptr(tau), _ptr(out)))
    return out


def tridiag_decomp(S, device=None):
    """(Q [..., N, N], d [..., N], e [..., N-1]) with S = Q tridiag(d, e) Q^T: tridiag_factor, and Q = tridiag_apply_q(F, tau, I), the
    same bits."""
    F, tau, d, e = tridiag_factor(S, device)
    N = F.shape[-1]
    return tridiag_apply_q(F, tau, np.broadcast_to(np.eye(N), F.shape), False, device), d, e


def _herm_h(H, what):
    """the dtype rule of the Hermitian functions on host arrays: complex128 as it is; a real matrix is sent to eigen_sym"""
    H = np.asarray(H)
    if H.dtype.kind != "c":
        raise TypeError("%s: H.dtype must be complex128; a real symmetric matrix goes to eigen_sym / tridiag_factor." % what)
    if H.dtype != np.complex128:
        raise TypeError("%s: only complex128 runs on the GPU path, got %s" % (what, H.dtype))
    return np.ascontiguousarray(H)


def _herm_shape(H_ndim, H_shape, what):
    """the shape checks of herm_tridiag_factor / herm_tridiag_decomp, shared with dev.py; returns N"""
    if H_ndim < 2:
        raise ValueError("%s: H.ndim must be at least 2." % what)
    if H_shape[-2] != H_shape[-1]:
        raise ValueError("%s: H must be quadratic." % what)
    if H_shape[-1] > 2048:
        raise ValueError("%s: N <= 2048." % what)
    return int(H_shape[-1])


def herm_tridiag_factor(H, device=None):
    """(F complex128 [..., N, N], tau complex128 [..., max(N-1, 0)], d float64 [..., N], e float64 [..., max(N-1, 0)]) with
    H = Q tridiag(d, e) Q^H for the Hermitian complex128 H, read only where i >= j (the imaginary part of its diagonal is ignored): d and
    e are real, Q = H_0 H_1 ... H_{N-2}, H_k = I - tau_k v_k v_k^H, v_k zero in rows 0..k, 1 in row k+1, its tail in F[k+2:, k] (LAPACK's
    zhetrd, lower): N - 1 reflectors, the last with an empty tail, there to make e_{N-2} real. F carries d on its diagonal, e on its first
    subdiagonal and zeros above. NaN or Infinity in what is read raises Nd4HipError with code -3. N <= 2048 (csrc/hetrd.hip)."""
    what = "herm_tridiag_factor(H)"
    H = _herm_h(H, what)
    N = _herm_shape(H.ndim, H.shape, what)
    lead, ne = H.shape[:-2], max(N - 1, 0)
    F, tau = np.empty(H.shape, dtype=np.complex128), np.empty(lead + (ne,), dtype=np.complex128)
    d, e = np.empty(lead + (N,)), np.empty(lead + (ne,))
    if F.size:
        h = _lib.handle(device)
        _lib.check(h.lib.nd4hip_zhetrd_batched_host(h.ptr, int(np.prod(lead, dtype=np.int64)), N, _ptr(H), _ptr(F), _ptr(tau), _ptr(d), _ptr(e)))
    return F, tau, d, e


def herm_tridiag_apply_q(F, tau, Z, adjoint=False, device=None):
    """Q Z (adjoint: Q^H Z), complex128, for the Q of herm_tridiag_factor's (F, tau) and Z [..., N, K] with the leading dimensions of F; a
    float64 Z is promoted. Q is never formed: N <= 96 reflector by reflector in LDS, above in compact WY blocks on the complex GEMM."""
    what = "herm_tridiag_apply_q(F,tau,Z)"
    F, tau, Z = np.asarray(F), np.asarray(tau), np.asarray(Z)
    if F.dtype != np.complex128 or tau.dtype != np.complex128:
        raise TypeError("%s: F and tau must be complex128." % what)
    if Z.dtype != np.complex128 and Z.dtype != np.float64:
        raise TypeError("%s: Z must be complex128 or float64." % what)
    N, K = _tridiag_fz(F.shape, tau.shape, Z.shape, what)
    F, tau = np.ascontiguousarray(F), np.ascontiguousarray(tau)
    out = np.array(Z, dtype=np.complex128, order="C")                       # a copy: the product is made in place
    if out.size:
        h = _lib.handle(device)
        _lib.check(h.lib.nd4hip_zunmtr_batched_host(h.ptr, int(np.prod(F.shape[:-2], dtype=np.int64)), N, K, 1 if adjoint else 0, _ptr(F),
                                                    _ptr(tau), _ptr(out)))
    return out


def herm_tridiag_decomp(H, device=None):
    """(Q complex128 [..., N, N], d [..., N], e [..., N-1]) with H = Q tridiag(d, e) Q^H: herm_tridiag_factor, and
    Q = herm_tridiag_apply_q(F, tau, I), the same bits."""
    F, tau, d, e = herm_tridiag_factor(H, device)
    N = F.shape[-1]
    return herm_tridiag_apply_q(F, tau, np.broadcast_to(np.eye(N), F.shape), False, device), d, e


def _heev(H, what, vectors, device, subset):
    if subset is not None:
        what = what.replace("(H)", "(H, subset)")
    H = _herm_h(H, what)
    if H.ndim < 2:
        raise ValueError("%s: H.ndim must be at least 2." % what)
    if H.shape[-2] != H.shape[-1]:
        raise ValueError("%s: H must be quadratic." % what)
    N = H.shape[-1]
    batch = int(np.prod(H.shape[:-2], dtype=np.int64))
    if subset is not None:                                                  # bisection and inverse iteration on (d, e)
        i0, i1 = _subset(subset, N, what)
        L = np.empty(H.shape[:-2] + (i1 - i0,))
        V = np.empty(H.shape[:-1] + (i1 - i0,), dtype=np.complex128) if vectors else None
        if L.size:
            h = _lib.handle(device)
            _lib.check(h.lib.nd4hip_zheevx_batched_host(h.ptr, batch, N, i0, i1, _ptr(H), _ptr(L), _ptr(V) if vectors else None))
        return (L, V) if vectors else L
    L = np.empty(H.shape[:-1])
    V = np.empty(H.shape, dtype=np.complex128) if vectors else None
    h = _lib.handle(device)
    _lib.check(h.lib.nd4hip_zheevd_batched_host(h.ptr, batch, N, _ptr(H), _ptr(L), _ptr(V) if vectors else None))
    return (L, V) if vectors else L


def eigen_herm(H, device=None, subset=None):
    """(eigenvalues float64 [..., N] descending, eigenvectors complex128 [..., N, N] as columns) of the Hermitian complex128 H:
    H V = V diag(L) and V^H V = I. H is read only where i >= j and the imaginary part of its diagonal is ignored. The route is
    herm_tridiag_factor, eigen_sym(reduction='tridiag')'s real divide & conquer solver on (d, e), and herm_tridiag_apply_q on the vectors.
    The phase of a vector is what the route produces: deterministic, not normalised. subset=(i0, i1) as eigen_sym's: L[i0:i1] and the
    matching columns alone, by bisection and inverse iteration on (d, e). NaN or Infinity in what is read raises Nd4HipError with code
    -3. N <= 2048. A float64 S raises TypeError: it goes to eigen_sym."""
    return _heev(H, "eigen_herm(H)", True, device, subset)


def eigenvals_herm(H, device=None, subset=None):
    """the eigenvalues of eigen_herm alone (the same bits); no Q is applied and no eigenvector is computed"""
    return _heev(H, "eigenvals_herm(H)", False, device, subset)


def _hegv_dtype(name, what, is_complex, is_c128, dtype, real_goes_to):
    """the dtype rule of the Hermitian Cholesky and generalised functions, shared with dev.py: complex128 as it is; a real matrix is sent
    to the real function"""
    if not is_complex:
        raise TypeError("%s: %s.dtype must be complex128; a real symmetric matrix goes to %s." % (what, name, real_goes_to))
    if not is_c128:
        raise TypeError("%s: only complex128 runs on the GPU path, got %s" % (what, dtype))


def _hegv_square(shape, name, what):
    """N of a stack of square matrices, N <= 2048"""
    if len(shape) < 2:
        raise ValueError("%s: %s.ndim must be at least 2." % (what, name))
    if shape[-2] != shape[-1]:
        raise ValueError("%s: %s must be quadratic." % (what, name))
    if shape[-1] > 2048:
        raise ValueError("%s: N <= 2048." % what)
    return int(shape[-1])


def _hegv_pair(sa, sb, nb, what):
    """whether one B (or L) [N, N] serves every member of A [..., N, N]"""
    sa, sb = tuple(sa), tuple(sb)
    if sb != sa and sb != sa[-2:]:
        raise ValueError("%s: %s.shape must be A.shape or A.shape[-2:], got %s and %s." % (what, nb, list(sb), list(sa)))
    return sb != sa


def _hegv_ly(sl, sy, what):
    """(N, K, one L for all) of L [..., N, N] or [N, N] and Y [..., N, K]"""
    sl, sy = tuple(sl), tuple(sy)
    N = _hegv_square(sl, "L", what)
    if len(sy) < 2:
        raise ValueError("%s: Y.ndim must be at least 2." % what)
    if sy[-2] != N:
        raise ValueError("%s: L and Y don't match." % what)
    if sl[:-2] != sy[:-2] and len(sl) != 2:
        raise ValueError("%s: L must have the leading dimensions of Y or be [N, N], got %s and %s." % (what, list(sl), list(sy)))
    return N, int(sy[-1]), sl[:-2] != sy[:-2]


def _hegv_m(M, name, what, real_goes_to):
    M = np.asarray(M)
    _hegv_dtype(name, what, M.dtype.kind == "c", M.dtype == np.complex128, M.dtype, real_goes_to)
    return np.ascontiguousarray(M)


def herm_cholesky_decomp(H, device=None):
    """L complex128 [..., N, N] with H = L L^H for the Hermitian positive definite complex128 H (LAPACK's zpotrf, lower): exact zeros above
    the diagonal, a real diagonal > 0 with imaginary part +0. H is read only where i >= j, the imaginary part of its diagonal is ignored,
    and it is not written. A radicand that is not a finite number > 0 raises Nd4HipError with code -5 and the lowest such member.
    N <= 2048 (csrc/hegv.hip). A float64 H raises TypeError: it goes to cholesky_decomp."""
    what = "herm_cholesky_decomp(H)"
    H = _hegv_m(H, "H", what, "cholesky_decomp")
    N = _hegv_square(H.shape, "H", what)
    L = np.empty(H.shape, dtype=np.complex128)
    if L.size:
        h = _lib.handle(device)
        _lib.check(h.lib.nd4hip_zpotrf_batched_host(h.ptr, int(np.prod(H.shape[:-2], dtype=np.int64)), N, _ptr(H), _ptr(L)))
    return L


def _ztrs(L, Y, what, device, entry, *flag, twice=False):
    L, Y = np.asarray(L), np.asarray(Y)
    _hegv_dtype("L", what, L.dtype.kind == "c", L.dtype == np.complex128, L.dtype, "cholesky_solve / tril_solve")
    if Y.dtype != np.complex128 and Y.dtype != np.float64:
        raise TypeError("%s: Y must be complex128 or float64." % what)
    N, K, one_l = _hegv_ly(L.shape, Y.shape, what)
    L = np.ascontiguousarray(L)
    X = np.array(Y, dtype=np.complex128, order="C")                         # a copy: the solve is made in place
    if X.size:
        h = _lib.handle(device)
        _lib.check(getattr(h.lib, entry)(h.ptr, int(np.prod(Y.shape[:-2], dtype=np.int64)), N, K, *flag, _ptr(L), 0 if one_l else N * N,
                                         *([_ptr(X)] * (2 if twice else 1))))
    return X


def herm_cholesky_solve(L, Y, device=None):
    """X complex128 with L L^H X = Y for the L of herm_cholesky_decomp and Y [..., N, K], complex128 or float64 (promoted). L has Y's
    leading dimensions or is exactly [N, N]: one factor for every member."""
    return _ztrs(L, Y, "herm_cholesky_solve(L,Y)", device, "nd4hip_zpotrs_batched_host", twice=True)   # (Y, X) = (X, X): in place


def ztril_solve(L, Y, adjoint=False, device=None):
    """X complex128 with L X = Y (adjoint: L^H X = Y) for a complex128 lower triangular L, read only where i >= j; its diagonal may be
    complex. Shapes as herm_cholesky_solve's."""
    return _ztrs(L, Y, "ztril_solve(L,Y)", device, "nd4hip_ztrsm_batched_host", 1 if adjoint else 0)


def herm_gen_reduce(A, L, device=None):
    """C = L^-1 A L^-H (LAPACK's zhegst, itype 1, lower) for the Hermitian complex128 A [..., N, N], read only where i >= j, and the L of
    herm_cholesky_decomp, A's shape or [N, N]: the lower triangle of C, zeros above it and an exactly real diagonal, what eigen_herm reads."""
    what = "herm_gen_reduce(A,L)"
    A, L = _hegv_m(A, "A", what, "eigen_sym_gen"), _hegv_m(L, "L", what, "eigen_sym_gen")
    N = _hegv_square(A.shape, "A", what)
    _hegv_square(L.shape, "L", what)
    one_l = _hegv_pair(A.shape, L.shape, "L", what)
    C = np.empty(A.shape, dtype=np.complex128)
    if C.size:
        h = _lib.handle(device)
        _lib.check(h.lib.nd4hip_zhegst_batched_host(h.ptr, int(np.prod(A.shape[:-2], dtype=np.int64)), N, _ptr(A), _ptr(L),
                                                    0 if one_l else N * N, _ptr(C)))
    return C


def _hegv(A, B, what, vectors, device, subset):
    if subset is not None:
        what = what.replace("(A,B)", "(A,B, subset)")
    A, B = _hegv_m(A, "A", what, "eigen_sym_gen"), _hegv_m(B, "B", what, "eigen_sym_gen")
    N = _hegv_square(A.shape, "A", what)
    _hegv_square(B.shape, "B", what)
    one_b = _hegv_pair(A.shape, B.shape, "B", what)
    lead = A.shape[:-2]
    batch = int(np.prod(lead, dtype=np.int64))
    i0, i1 = _subset(subset, N, what) if subset is not None else (0, N)
    lam = np.empty(lead + (i1 - i0,))
    X = np.empty(lead + (N, i1 - i0), dtype=np.complex128) if vectors else None
    if lam.size:
        h = _lib.handle(device)
        if subset is not None:
            _lib.check(h.lib.nd4hip_zhegvx_batched_host(h.ptr, batch, N, i0, i1, _ptr(A), _ptr(B), 0 if one_b else N * N, _ptr(lam),
                                                        _ptr(X) if vectors else None))
        else:
            _lib.check(h.lib.nd4hip_zhegvd_batched_host(h.ptr, batch, N, _ptr(A), _ptr(B), 0 if one_b else N * N, _ptr(lam),
                                                        _ptr(X) if vectors else None))
    return (lam, X) if vectors else lam


def eigen_herm_gen(A, B, device=None, subset=None):
    """the generalised Hermitian-definite eigenproblem A x = lambda B x: (eigenvalues float64 [..., N] descending, eigenvectors complex128
    [..., N, N] as columns) with A X = B X diag(lam) and X^H B X = I. A [..., N, N] Hermitian complex128; B Hermitian positive definite of
    the same shape, or exactly [N, N]: one B for every member, factorised once. Both are read only where i >= j, the imaginary parts of
    their diagonals are ignored, neither is written. Route: L = herm_cholesky_decomp(B), C = herm_gen_reduce(A, L), eigen_herm(C)
    unchanged, X = L^-H Y (csrc/hegv.hip). The phase of a column is what the route produces: deterministic, not normalised.
    subset=(i0, i1) as eigen_herm's; the back-transformation then runs on the selected columns alone. B not positive definite raises
    Nd4HipError with code -5 and the lowest such member; NaN or Infinity in A's lower triangle, or overflow of C, code -3. N <= 2048.
    A float64 A or B raises TypeError: the pair goes to eigen_sym_gen."""
    return _hegv(A, B, "eigen_herm_gen(A,B)", True, device, subset)


def eigenvals_herm_gen(A, B, device=None, subset=None):
    """the eigenvalues of eigen_herm_gen alone (the same bits); no back-transformation is computed"""
    return _hegv(A, B, "eigenvals_herm_gen(A,B)", False, device, subset)


def _tridiag_args(d, e, what, ndim, shape):
    """the argument checks of tridiag_eigen / tridiag_eigenvals / tridiag_count, shared with dev.py; returns N"""
    if ndim(d) < 1 or ndim(e) < 1 or tuple(shape(d)[:-1]) != tuple(shape(e)[:-1]):
        raise ValueError("%s: d and e must have the same leading dimensions." % what)
    N = int(shape(d)[-1])
    if N < 1 or int(shape(e)[-1]) != N - 1:
        raise ValueError("%s: e must have len(d) - 1 entries." % what)
    if N > 2048:
        raise ValueError("%s: N <= 2048." % what)
    return N


def _stevx(d, e, subset, what, vectors, device, interval=None, info=None):
    if interval is not None:
        what = _interval_what(what, False, subset)
    d, e = _asarray(d, what), _asarray(e, what)
    N = _tridiag_args(d, e, what, lambda a: a.ndim, lambda a: a.shape)
    if interval is not None:                                                # the subset of each member chosen by value
        bounds = _interval(interval, d.shape[:-1], what)
        L, Z, k = _interval_call("nd4hip_dstevxv_batched_host", device, N, bounds, (d, e), d.shape[:-1] + (N, N) if vectors else None, info)
        L = np.ascontiguousarray(L[..., :k])
        return (L, np.ascontiguousarray(np.swapaxes(Z[..., :k, :], -1, -2))) if vectors else L
    i0, i1 = _subset((0, N) if subset is None else subset, N, what)
    lead = d.shape[:-1]
    L = np.empty(lead + (i1 - i0,))
    Z = np.empty(lead + (i1 - i0, N)) if vectors else None
    if L.size:
        h = _lib.handle(device)
        _lib.check(h.lib.nd4hip_dstevx_batched_host(h.ptr, int(np.prod(lead, dtype=np.int64)), N, i0, i1, _ptr(d), _ptr(e), _ptr(L),
                                                    _ptr(Z) if vectors else None))
    return (L, np.ascontiguousarray(np.swapaxes(Z, -1, -2))) if vectors else L


def tridiag_eigen(d, e, subset=None, device=None, interval=None, info=None):
    """selected eigenpairs of the symmetric tridiagonal T with diagonal d [..., N] and off-diagonal e [..., N-1], N <= 2048:
    (L [..., k] descending, Z [..., N, k] with the eigenvectors as columns) for subset=(i0, i1), the slice L[i0:i1] of the descending
    spectrum (None: all of it). Bisection on Sturm counts, inverse iteration, Gram-Schmidt inside clusters (csrc/syevx.hip). NaN or
    Infinity in d or e raises Nd4HipError with code -3.
    interval=(lo, hi) in place of subset: the eigenvalues lo < lambda <= hi of every member, as in eigen_sym: (L [..., kmax],
    Z [..., N, kmax]), member b's k_b pairs first (the bits of subset=(count(hi), count(lo)) with tridiag_count), then NaN and zero
    columns; `info` (a dict) receives 'range', int32 [..., 2]."""
    return _stevx(d, e, subset, "tridiag_eigen(d,e)", True, device, interval, info)


def tridiag_eigenvals(d, e, subset=None, device=None, interval=None, info=None):
    """the eigenvalues of tridiag_eigen alone (the same bits); no inverse iteration is made"""
    return _stevx(d, e, subset, "tridiag_eigenvals(d,e)", False, device, interval, info)


def tridiag_count(d, e, x, device=None):
    """int32 [..., M]: how many eigenvalues of tridiag(d [..., N], e [..., N-1]) are greater than each x [..., M] (the Sturm count alone).
    count(lo) and count(hi) turn the value interval (lo, hi] into subset=(count(hi), count(lo))."""
    what = "tridiag_count(d,e,x)"
    d, e, x = _asarray(d, what), _asarray(e, what), _asarray(x, what)
    N = _tridiag_args(d, e, what, lambda a: a.ndim, lambda a: a.shape)
    if x.ndim < 1 or x.shape[:-1] != d.shape[:-1]:
        raise ValueError("%s: x must have the leading dimensions of d." % what)
    if np.isnan(x).any():
        raise ValueError("%s: x contains NaN." % what)
    count = np.empty(x.shape, dtype=np.int32)
    if count.size:
        h = _lib.handle(device)
        _lib.check(h.lib.nd4hip_dstcnt_batched_host(h.ptr, int(np.prod(d.shape[:-1], dtype=np.int64)), N, x.shape[-1], _ptr(d), _ptr(e), _ptr(x),
                                                    count.ctypes.data))
    return count


def _sygv_args(A, B, what, is_float64, ndim, shape):
    """the argument checks of eigen_sym_gen / eigenvals_sym_gen, shared with dev.py; returns whether one B serves every member"""
    nb = what[what.index(",") + 1]                                          # 'B', or 'L' for _sygst(A,L)
    for name, M in (("A", A), (nb, B)):
        if not is_float64(M):
            raise TypeError("%s: %s.dtype must be float." % (what, name))
        if ndim(M) < 2:
            raise ValueError("%s: %s.ndim must be at least 2." % (what, name))
        if shape(M)[-2] != shape(M)[-1]:
            raise ValueError("%s: %s must be quadratic." % (what, name))
    sa, sb = tuple(shape(A)), tuple(shape(B))
    if sb != sa and sb != sa[-2:]:
        raise ValueError("%s: %s.shape must be A.shape or A.shape[-2:], got %s and %s." % (what, nb, list(sb), list(sa)))
    return sb != sa


def _sygv_select(what, jacobi, subset, interval, reduction):
    """(what, tridiag) of an eigen_sym_gen call after the refusals that need no operand, as eigen_sym's"""
    tr = _reduction(reduction, what, jacobi)
    if interval is not None:
        what = _interval_what(what, jacobi, subset)
    elif subset is not None and jacobi:
        _subset(subset, 0, what, True)
    return what, tr


def _sygvx(A, B, what, vectors, device, one_b, tr, subset, interval, info):
    """eigen_sym_gen with subset, interval or reduction='tridiag': nd4hip_dsygvx_batched_host (select 0: all, 1: subset, 2: interval)"""
    N, lead = A.shape[-1], A.shape[:-2]
    batch = int(np.prod(lead, dtype=np.int64))
    select, i0, i1, bounds, ranges, kmax = 0, 0, 0, None, None, ctypes.c_int64(0)
    if interval is not None:
        select, bounds, ranges = 2, _interval(interval, lead, what), np.zeros(lead + (2,), dtype=np.int32)
    elif subset is not None:
        select = 1
        i0, i1 = _subset(subset, N, what)
    K = i1 - i0 if select == 1 else N
    L = np.empty(lead + (K,))
    X = np.empty(lead + (N, K)) if vectors else None
    if L.size:
        h = _lib.handle(device)
        _lib.check(h.lib.nd4hip_dsygvx_batched_host(h.ptr, 1 if tr else 0, select, batch, N, i0, i1, N if select == 2 else 0,
                                               _ptr(bounds) if select == 2 else None, _ptr(A), _ptr(B), 0 if one_b else N * N, _ptr(L),
                                               _ptr(X) if vectors else None, _ptr(ranges) if select == 2 else None,
                                               ctypes.byref(kmax) if select == 2 else None))
    if select == 2:
        if info is not None:
            info["range"] = ranges
        L = np.ascontiguousarray(L[..., :kmax.value])
        X = np.ascontiguousarray(X[..., :kmax.value]) if vectors else None
    return (L, X) if vectors else L


def _sygvd(A, B, what, vectors, device, algo, info, subset=None, interval=None, reduction=None):
    jacobi = _eigsym_algo(algo, what)
    what, tr = _sygv_select(what, jacobi, subset, interval, reduction)
    A, B = np.asarray(A), np.asarray(B)
    one_b = _sygv_args(A, B, what, lambda M: not np.iscomplexobj(M), lambda M: M.ndim, lambda M: M.shape)
    A, B = _asarray(A, what), _asarray(B, what)
    if tr or subset is not None or interval is not None:
        return _sygvx(A, B, what, vectors, device, one_b, tr, subset, interval, info)
    N = A.shape[-1]
    L = np.empty(A.shape[:-1])
    X = np.empty(A.shape) if vectors else None
    batch = int(np.prod(A.shape[:-2], dtype=np.int64))
    sweeps = np.zeros(A.shape[:-2], dtype=np.int32) if jacobi else None
    h = _lib.handle(device)
    _lib.check(h.lib.nd4hip_dsygvd_batched(h.ptr, 1 if jacobi else 0, batch, N, _ptr(A), _ptr(B), 0 if one_b else N * N, _ptr(L),
                                           _ptr(X) if vectors else None, sweeps.ctypes.data if jacobi else None))
    if jacobi and info is not None:
        info["sweeps"] = sweeps
    return (L, X) if vectors else L


def eigen_sym_gen(A, B, device=None, algo=None, info=None, subset=None, interval=None, reduction=None):
    """the generalised symmetric-definite eigenproblem A x = lambda B x: (eigenvalues float64 [..., N] descending, eigenvectors
    float64 [..., N, N] as columns) with A X = B X diag(L) and X^T B X = I. A [..., N, N] symmetric; B of the same shape, or exactly
    [N, N]: one B for every member, factorised once. Only the lower triangles of A and B are read; neither is written.
    Route: L = chol(B), C = L^-1 A L^-T, eigen_sym(C, algo) unchanged, X = L^-T Y (csrc/sygv.hip; N <= 64 in two fused kernels).
    algo and info as for eigen_sym (N <= 2048; 'jacobi': N <= 128, info['sweeps']). B not positive definite raises Nd4HipError with
    code -5 and the lowest such member; NaN or Infinity in A's lower triangle, or overflow of C, code -3.
    subset=(i0, i1), interval=(lo, hi) and reduction='tridiag' (opt-in, not with 'jacobi') are eigen_sym's keywords applied to C:
    (L [..., k], X [..., N, k]) for a subset, ragged (L [..., kmax], X [..., N, kmax]) with info['range'] for an interval; the
    back-transformation then runs on the selected columns alone. The errors above keep their codes and members."""
    return _sygvd(A, B, "eigen_sym_gen(A,B)", True, device, algo, info, subset, interval, reduction)


def eigenvals_sym_gen(A, B, device=None, algo=None, info=None, subset=None, interval=None, reduction=None):
    """the eigenvalues of eigen_sym_gen alone (the same bits); no back-transformation is computed"""
    return _sygvd(A, B, "eigenvals_sym_gen(A,B)", False, device, algo, info, subset, interval, reduction)


def _sygst(A, L, device=None):
    """step 2 of eigen_sym_gen on its own, for the tests of both tiers: C = L^-1 A L^-T from a given lower triangular L [..., N, N] or
    [N, N]; the lower triangle of C and exact zeros above it (nd4hip_dsygst_batched)"""
    A, L = np.asarray(A), np.asarray(L)
    one_l = _sygv_args(A, L, "_sygst(A,L)", lambda M: not np.iscomplexobj(M), lambda M: M.ndim, lambda M: M.shape)
    A, L = _asarray(A, "_sygst(A,L)"), _asarray(L, "_sygst(A,L)")
    N = A.shape[-1]
    C = np.empty(A.shape)
    h = _lib.handle(device)
    _lib.check(h.lib.nd4hip_dsygst_batched(h.ptr, int(np.prod(A.shape[:-2], dtype=np.int64)), N, _ptr(A), _ptr(L), 0 if one_l else N * N,
                                           _ptr(C)))
    return C


# ---------------------------------------------------------------------------------------------------
# Pivoted symmetric indefinite LDL^T, Bunch-Kaufman (src/la/pldlp.js), csrc/pldlp.hip
# ---------------------------------------------------------------------------------------------------
PLDLP_TIERS = {None: 0, "auto": 0, "lds": 1, "global": 2, "grid": 3}
PLDLP_SINGULAR = "_pldlp_decomp(M,N, LD,LD_off, P,P_off): Zero column or NaN encountered."


def _pldlp_tier(tier):
    if tier not in PLDLP_TIERS:
        raise ValueError("pldlp_decomp(S): unknown tier %r (auto, lds, global or grid)." % (tier,))
    return PLDLP_TIERS[tier]


def pldlp_limits():
    """the kernels' size constants (needs no device): the largest N of the 'lds' and of the 'global' tier, and the edge of the
    'grid' tier's update tile"""
    a, b, c = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
    _lib.check(_lib.load().nd4hip_dsytrf_bk_limits(ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)))
    return {"lds_max_n": a.value, "global_max_n": b.value, "grid_tile": c.value}


def pldlp_tier(batch, N, tier=None, device=None):
    """the name of the tier pldlp_decomp takes for `batch` matrices of size N under `tier`"""
    h = _lib.handle(device)
    t = h.lib.nd4hip_dsytrf_bk_tier(h.ptr, int(batch), int(N), _pldlp_tier(tier))
    if t < 0:
        _ev_call(int, t)                   # raises with the library's text
    return {1: "lds", 2: "global", 3: "grid"}[t]


def pldlp_decomp(S, device=None, tier=None):
    """pldlp.js:191-222: [LD, P] of the Bunch-Kaufman factorisation S[P][:, P] = L D L^T of symmetric S [..., N, N] (lower
    triangle read): LD holds the unit-lower L below the 1x1 and 2x2 diagonal blocks of D, zeros above the diagonal; P [..., N]
    int32 is the row order with the second row of every 2x2 block complemented. The reference's bits on every tier
    ('lds', 'global', 'grid'; None or 'auto' chooses)."""
    t = _pldlp_tier(tier)
    S = np.asarray(S)
    if S.ndim < 2 or S.shape[-1] != S.shape[-2]:
        raise ValueError("Last two dimensions must be quadratic.")
    S = _asarray(S, "pldlp_decomp(S)")
    LD, P = np.empty_like(S), np.empty(S.shape[:-1], dtype=np.int32)
    h = _lib.handle(device)
    try:
        _lib.check(h.lib.nd4hip_dsytrf_bk_batched_ex(h.ptr, int(np.prod(S.shape[:-2], dtype=np.int64)), S.shape[-1], _ptr(S), _ptr(LD),
                                                     _ptr(P), t))
    except _lib.Nd4HipError as e:
        if e.code == -5:
            raise ValueError(str(e).split(": ", 1)[1])
        raise _arg_error(e)
    return [LD, P]


def _pldlp_args(LD, P, y=None, with_y=False):
    """the reference's argument checks of pldlp_l / _d / _p (pldlp.js:231-236) and pldlp_solve (:529-537)"""
    LD, P = np.asarray(LD), np.asarray(P)
    if with_y:
        y = np.asarray(y)
    if LD.ndim < 2:
        raise ValueError("pldlp_solve(LD,P,y): LD must be at least 2D.")
    if P.ndim < 1:
        raise ValueError("pldlp_solve(LD,P,y): P must be at least 1D.")
    if with_y and y.ndim < 2:
        raise ValueError("pldlp_solve(LD,P,y): y must be at least 2D.")
    N = LD.shape[-2]
    if N != LD.shape[-1]:
        raise ValueError("pldlp_solve(LD,P,y): LD must be square.")
    if N != P.shape[-1]:
        raise ValueError("pldlp_solve(LD,P,y): LD and P shape mismatch.")
    if with_y and N != y.shape[-2]:
        raise ValueError("pldlp_solve(LD,P,y): LD and y shape mismatch.")
    if P.dtype.kind not in "iu":
        raise TypeError("pldlp_solve(LD,P,y): P must be an integer array, got %s" % P.dtype)
    return LD, np.ascontiguousarray(P.astype(np.int32, copy=False)), y


def _pldlp_lead(*shapes):
    try:
        return tuple(np.broadcast_shapes(*shapes))
    except ValueError:
        raise ValueError("Shapes are not broadcast-compatible.")


def _pldlp_real(LD, what):
    if LD.dtype.kind not in "fiub":
        raise TypeError("%s: LD must be real, got %s" % (what, LD.dtype))
    return LD.astype(np.float64, copy=False)


def pldlp_l(LD, P=None):
    """pldlp.js:225-304: the unit lower triangular factor L [..., N, N] (host side, leading axes of LD and P broadcast)"""
    if P is None:
        LD, P = LD
    LD, P, _ = _pldlp_args(LD, P)
    LD = _pldlp_real(LD, "pldlp_l(LD,P)")
    N = LD.shape[-1]
    lead = _pldlp_lead(LD.shape[:-2], P.shape[:-1])
    L = np.tril(np.broadcast_to(LD, lead + (N, N)), -1)
    neg = np.broadcast_to(P < 0, lead + (N,))
    i = np.arange(1, N)
    L[..., i, i - 1] = np.where(neg[..., 1:], 0.0, L[..., i, i - 1])
    i = np.arange(N)
    L[..., i, i] = 1.0
    return L


def pldlp_d(LD, P=None):
    """pldlp.js:307-380: the block diagonal factor D [..., N, N] with its symmetric 2x2 blocks (host side)"""
    if P is None:
        LD, P = LD
    LD, P, _ = _pldlp_args(LD, P)
    LD = _pldlp_real(LD, "pldlp_d(LD,P)")
    N = LD.shape[-1]
    lead = _pldlp_lead(LD.shape[:-2], P.shape[:-1])
    LDb = np.broadcast_to(LD, lead + (N, N))
    neg = np.broadcast_to(P < 0, lead + (N,))
    D = np.zeros(lead + (N, N))
    i = np.arange(N)
    D[..., i, i] = LDb[..., i, i]
    i = np.arange(1, N)
    off = np.where(neg[..., 1:], LDb[..., i, i - 1], 0.0)
    D[..., i, i - 1] = off
    D[..., i - 1, i] = off
    return D


def _pldlp_perm(P):
    """pldlp.js:404-437: P [..., N] int32 with the complements undone, or the reference's error"""
    N = P.shape[-1]
    neg = P < 0
    Q = np.where(neg, ~P, P)
    rows = Q.reshape(-1, N)
    ok = not (N and neg[..., 0].any()) and not (neg[..., 1:] & neg[..., :-1]).any() and \
        bool(np.all(np.sort(rows, axis=1) == np.arange(N, dtype=np.int64)))
    if ok:
        return Q.astype(np.int32)
    Pf = P.reshape(-1, N)
    for b in range(Pf.shape[0] - 1, -1, -1):              # the reference's order: last matrix first, last row first
        seen = np.zeros(N, dtype=bool)
        for i in range(N - 1, -1, -1):
            p = int(Pf[b, i])
            if p < 0:
                if not (0 < i) or Pf[b, i - 1] < 0:
                    raise ValueError("pldlp_solve(LD,P,y): P is invalid.")
                p = ~p
            if not (0 <= p < N):
                raise ValueError("pldlp_solve(LD,P,y): P contains out-of-bounds indices.")
            if seen[p]:
                raise ValueError("pldlp_solve(LD,P,y): P contains duplicate indices.")
            seen[p] = True
    raise AssertionError("unreachable")


def pldlp_p(LD, P=None):
    """pldlp.js:383-438: the row permutation [..., N] int32 with the 2x2 marks removed, after a complete check of P (host side)"""
    if P is None:
        LD, P = LD
    LD, P, _ = _pldlp_args(LD, P)
    _pldlp_lead(LD.shape[:-2], P.shape[:-1])
    return _pldlp_perm(P)


def pldlp_solve(LD, P, y=None, device=None):
    """pldlp.js:519-604: x [..., N, J] with S x = y from pldlp_decomp's [LD, P]; also pldlp_solve([LD, P], y). Leading axes of LD,
    P and y broadcast. P is checked completely on the host before any device work."""
    if y is None:
        if P is None:
            raise ValueError("Assertion failed.")
        y = P
        LD, P = LD
    LD, P, y = _pldlp_args(LD, P, y, with_y=True)
    LD, y = _asarray(LD, "pldlp_solve(LD,P,y)"), _asarray(y, "pldlp_solve(LD,P,y)")
    N, J = LD.shape[-1], y.shape[-1]
    lead = _pldlp_lead(LD.shape[:-2], P.shape[:-1], y.shape[:-2])
    _pldlp_perm(P)
    X = np.empty(lead + (N, J))
    h = _lib.handle(device)
    for cnt, (oL, oP, oY), (sL, sP, sY), b0 in _bcast_groups_n(lead, [LD.shape[:-2], P.shape[:-1], y.shape[:-2]], [N * N, N, N * J]):
        _ev_call(h.lib.nd4hip_dsytrs_bk_batched, h.ptr, cnt, N, J, _off(LD, oL), sL, _off(P, oP, 4), sP, _off(y, oY), sY, _off(X, b0 * N * J))
    return X


# ---------------------------------------------------------------------------------------------------
# structure functions: NDArray.T, tri.js:23-42, diag.js:23-88, permute.js:23-306 (csrc/struct.hip)
# ---------------------------------------------------------------------------------------------------
def _struct_real(A, what):
    A = np.asarray(A)
    if A.dtype != np.float64:
        raise TypeError("%s: only float64 runs on the GPU path, got %s" % (what, A.dtype))
    return np.ascontiguousarray(A)


def _diag_args(shape, offset):
    """diag.js:55-72 on a shape: (rows, cols, L); the second message prints A.shape after A became its data, as the reference does."""
    if len(shape) < 2:
        raise ValueError("diag(A, offset): A.ndim=%d is less than 2." % len(shape))
    rows, cols = int(shape[-2]), int(shape[-1])
    if isinstance(offset, (bool, np.bool_)) or not isinstance(offset, (int, np.integer)):
        raise TypeError("diag(A, offset): offset must be an integer")
    if not (-rows < offset < cols):
        raise ValueError("diag(A, offset): offset=%s out of A.shape=[undefined]." % _js_num(offset))
    return rows, cols, min(rows, rows + offset, cols, cols - offset)


def _diag_mat_args(shape):
    """diag.js:25-36 on a shape"""
    if len(shape) < 1:
        raise ValueError("diag_mat(diag): diag.ndim=%d is less than 1." % len(shape))
    if int(shape[-1]) <= 0:
        raise ValueError("Assertion Failed!")
    return int(shape[-1])


def _tri_k(k):
    if isinstance(k, (bool, np.bool_)) or not isinstance(k, (int, np.integer)):
        raise TypeError("k must be an integer")
    return max(-2 ** 63, min(2 ** 63 - 1, int(k)))


def _permute_plan(name, a_shape, p_shape, p_is_int32, cols):
    """permute.js:25-48 on shapes: the checks in the reference's order and with its texts, then (M, N, L, lead, groups), groups as
    _bcast_groups_n cuts the broadcast leading axes of A and P into runs of stride 0 / M N and 0 / L."""
    if len(a_shape) < 2:
        raise ValueError("%s(A,P): A.ndim must be at least 2." % name)
    if len(p_shape) < 1:
        raise ValueError("%s(A,P): P.ndim must be at least 1." % name)
    if not p_is_int32:
        raise TypeError('%s(A,P): P.dtype must be "int32".' % name)
    M, N = int(a_shape[-2]), int(a_shape[-1])
    L = N if cols else M
    if L != int(p_shape[-1]):
        raise ValueError("%s(A,P): A.shape[%d] and P.shape[-1] must match." % (name, -1 if cols else -2))
    try:
        lead = tuple(int(x) for x in np.broadcast_shapes(tuple(a_shape[:-2]), tuple(p_shape[:-1])))
    except ValueError:
        raise ValueError("%s(A,P): A and P not broadcast-compatible." % name)
    la_, lp = tuple(int(x) for x in a_shape[:-2]), tuple(int(x) for x in p_shape[:-1])
    total = int(np.prod(lead, dtype=np.int64)) if lead else 1
    na, npm = (int(np.prod(s, dtype=np.int64)) if s else 1 for s in (la_, lp))
    # _bcast_groups_n walks the members one by one in Python (0.5 ms for 1024 members of 64 x 64, against 16 us of kernel).
    # When each operand is either dense over the whole result or one block for all of it, what that walk returns is known: one run.
    if na in (1, total) and npm in (1, total):
        groups = [(total, [0, 0], [M * N if na == total and total > 1 else 0, L if npm == total and total > 1 else 0], 0)]
    else:
        groups = _bcast_groups_n(lead, [la_, lp], [M * N, L])
    return M, N, L, lead, groups


def _as_index(P):
    """P as the reference's asarray sees it: nested lists of integers are int32; an array keeps its dtype"""
    if not isinstance(P, np.ndarray):
        P = np.asarray(P)
        if P.dtype.kind in "iu" and P.size and np.all(P == P.astype(np.int32)):
            P = P.astype(np.int32)
    return P


def transpose(A, device=None):
    """NDArray.T: the last two axes swapped; fewer than two axes: A itself."""
    A = _struct_real(A, "transpose")
    if A.ndim < 2:
        return A
    M, N = A.shape[-2:]
    B = np.empty(A.shape[:-2] + (N, M))
    h = _lib.handle(device)
    _lib.check(h.lib.nd4hip_dtranspose_batched(h.ptr, int(np.prod(A.shape[:-2], dtype=np.int64)), M, N, _ptr(A), _ptr(B)))
    return B


def _tri(upper, A, k, device):
    A = np.asarray(A)
    if A.ndim < 2:
        raise ValueError("Input must be at least 2D.")
    A = _struct_real(A, "triu" if upper else "tril")
    k = _tri_k(k)
    M, N = A.shape[-2:]
    B = np.empty(A.shape)
    h = _lib.handle(device)
    _lib.check(h.lib.nd4hip_dtri_batched(h.ptr, upper, k, int(np.prod(A.shape[:-2], dtype=np.int64)), M, N, _ptr(A), _ptr(B)))
    return B


def tril(A, k=0, device=None):
    """tri.js:23-31: zero where i < j - k"""
    return _tri(0, A, k, device)


def triu(A, k=0, device=None):
    """tri.js:34-42: zero where i > j - k"""
    return _tri(1, A, k, device)


def diag(A, offset=0, device=None):
    """diag.js:53-88: the offset-th diagonal of every matrix, [..., L]"""
    A = np.asarray(A)
    M, N, L = _diag_args(A.shape, offset)
    A = _struct_real(A, "diag")
    d = np.empty(A.shape[:-2] + (L,))
    h = _lib.handle(device)
    _lib.check(h.lib.nd4hip_ddiag_batched(h.ptr, int(np.prod(A.shape[:-2], dtype=np.int64)), M, N, int(offset), _ptr(A), _ptr(d)))
    return d


def diag_mat(d, device=None):
    """diag.js:23-50: [..., N] -> [..., N, N]"""
    d = np.asarray(d)
    N = _diag_mat_args(d.shape)
    d = _struct_real(d, "diag_mat")
    D = np.empty(d.shape + (N,))
    h = _lib.handle(device)
    _lib.check(h.lib.nd4hip_ddiagmat_batched(h.ptr, int(np.prod(d.shape[:-1], dtype=np.int64)), N, _ptr(d), _ptr(D)))
    return D


def _permute(cols, inverse, A, P, device):
    name = ("unpermute_" if inverse else "permute_") + ("cols" if cols else "rows")
    A = np.asarray(A)
    P = _as_index(P)
    M, N, L, lead, groups = _permute_plan(name, A.shape, P.shape, P.dtype == np.int32, cols)
    A = _struct_real(A, name)
    P = np.ascontiguousarray(P)
    B = np.empty(lead + (M, N))
    h = _lib.handle(device)
    for cnt, (oA, oP), (sA, sP), b0 in groups:
        try:
            _lib.check(h.lib.nd4hip_dpermute_batched(h.ptr, cols, inverse, cnt, M, N, _off(A, oA), sA, _off(P, oP, 4), sP, _off(B, b0 * M * N)))
        except _lib.Nd4HipError as e:
            raise _arg_error(e)
    return B


def permute_rows(A, P, device=None):
    """permute.js:23-92: B[i,:] = A[P[i],:]"""
    return _permute(0, 0, A, P, device)


def permute_cols(A, P, device=None):
    """permute.js:95-163: B[:,j] = A[:,P[j]]"""
    return _permute(1, 0, A, P, device)


def unpermute_rows(A, P, device=None):
    """permute.js:166-235: B[P[i],:] = A[i,:]; a later i overwrites an earlier one, rows no i names are zero"""
    return _permute(0, 1, A, P, device)


def unpermute_cols(A, P, device=None):
    """permute.js:238-306: B[:,P[j]] = A[:,j]"""
    return _permute(1, 1, A, P, device)


# planners of the strided N-d copy (csrc/gather.hip): NDArray.sliceElems (nd_array.js:531-642), transpose(...axes)
# (nd_array.js:375-436), reshape (nd_array.js:438-462), concat (concat.js) and stack (stack.js) on shapes alone. Pure host code:
# each returns what one nd4hip_gather_nd_dev call needs, in elements of a C-ordered operand, or raises the reference's text.
def _c_strides(shape):
    strides, s = [0] * len(shape), 1
    for d in range(len(shape) - 1, -1, -1):
        strides[d] = s
        s *= int(shape[d])
    return strides


def _js_list(shape):
    return ",".join(_js_num(s) for s in shape)


def _check_shape(shape, n):
    """the NDArray constructor (nd_array.js:135-139) on a new shape over n elements"""
    if any(s < 1 for s in shape):
        raise ValueError("Invalid shape: %s." % _js_list(shape))
    total = 1
    for s in shape:
        total *= s
    if total != n:
        raise ValueError("Shape [%s] does not match array length of %d." % (_js_list(shape), n))


def _integral(x):
    return isinstance(x, (int, np.integer)) and not isinstance(x, (bool, np.bool_)) or (isinstance(x, (float, np.floating)) and float(x).is_integer())


def _slice_plan(shape, slices):
    """sliceElems on a shape: (out_shape, off, strides) with out[i] = data[off + sum i_d strides[d]]. A slice is an integer (the
    axis disappears), '...' or Ellipsis, 'new' (a new axis of extent 1, stride 0) or [start, end, step] / [start, end] / [] with
    None for an omitted entry; negative start / end count from the end, a negative step reverses."""
    shape = [int(s) for s in shape]
    slices = ["..." if s is Ellipsis else s for s in slices]
    ndim = len(shape)
    n_ell = n_red = n_sl = 0
    for s in slices:
        if isinstance(s, str) and s == "...":
            n_ell += 1
        elif isinstance(s, str) and s == "new":
            pass
        elif isinstance(s, (int, float, np.integer, np.floating)) and not isinstance(s, (bool, np.bool_)):
            if not _integral(s):
                raise ValueError("Only integral indices allowed.")
            n_red += 1
        else:
            if not isinstance(s, (list, tuple)) or len(s) > 3 or len(s) == 1:
                raise ValueError("Illegal argument(s).")
            if any(x is not None and not _integral(x) for x in s):
                raise TypeError("slice entries must be integers or None")
            n_sl += 1
    if n_ell > 1:
        raise ValueError("Highlander! There can be only one ... (ellipsis).")
    if n_ell == 0:
        slices = slices + ["..."]
    if n_red + n_sl > ndim:
        raise ValueError("Cannot sliced more dimensions than available.")
    off, d, stride = 0, ndim, 1
    out_shape, strides = [], []                              # innermost first, as the reference builds them
    for s in reversed(slices):
        if isinstance(s, str) and s == "new":
            strides.append(0)
            out_shape.append(1)
        elif isinstance(s, str):
            for _ in range(n_red + n_sl, ndim):
                d -= 1
                strides.append(stride)
                out_shape.append(shape[d])
                stride *= shape[d]
        else:
            d -= 1
            n = shape[d]
            if not isinstance(s, (list, tuple)):
                i = int(s)
                if i < 0:
                    i += n
                if i < 0 or i >= n:
                    raise ValueError("Index out of bounds.")
                off += stride * i
            else:
                start, end, step = (list(s) + [None, None, None])[:3]
                start = None if start is None else int(start)
                end = None if end is None else int(end)
                step = 1 if step is None else int(step)
                if end is not None and end < 0:
                    end += n
                if start is not None and start < 0:
                    start += n
                if start is not None and (start < 0 or start >= n):
                    raise ValueError("Slice start out of bounds.")
                if step == 0:
                    raise ValueError("Stride/step cannot be zero.")
                if step < 0:
                    start = n - 1 if start is None else start
                    end = -1 if end is None else end
                    if end < -1 or end >= n:
                        raise ValueError("Slice end out of bounds.")
                else:
                    start = 0 if start is None else start
                    end = n if end is None else end
                    if end < 0 or end > n:
                        raise ValueError("Slice end out of bounds.")
                strides.append(stride * step)
                off += stride * start
                num = (1 if step < 0 else -1) + end - start
                out_shape.append(1 + (abs(num) // abs(step)) * (1 if (num < 0) == (step < 0) else -1))      # Math.trunc
            stride *= n
    out_shape.reverse()
    strides.reverse()
    count = 1
    for s in out_shape:
        count *= s
    if count < 0:                                            # an empty range the wrong way round: the engine's text, before the constructor
        raise ValueError("Invalid typed array length: %d" % count)
    if any(s < 1 for s in out_shape):
        raise ValueError("Invalid shape: %s." % _js_list(out_shape))
    return out_shape, off, strides


def _transpose_plan(shape, axes):
    """transpose(...axes) on a shape: (out_shape, strides). No axes: the last two swapped. Axes that are not named follow the
    named ones in their own order."""
    shape = [int(s) for s in shape]
    ndim = len(shape)
    old = _c_strides(shape)
    axes = list(axes)
    if not axes:
        order = list(range(ndim))
        if ndim > 1:
            order[-2:] = [ndim - 1, ndim - 2]
    else:
        if any(not _integral(j) for j in axes):
            raise TypeError("axes must be integers")
        axes = [int(j) for j in axes]
        if len(set(axes)) != len(axes):
            raise ValueError("Duplicate axes are not allowed.")
        if any(j < 0 or j >= ndim for j in axes):
            raise ValueError("Axis out of bounds.")
        order = axes + [i for i in range(ndim) if i not in axes]
    return [shape[j] for j in order], [old[j] for j in order]


def _reshape_shape(shape, n, new_shape):
    """reshape(...new_shape) of an array of `shape` holding n elements: the new shape, one -1 inferred"""
    if any(not _integral(s) for s in new_shape):
        raise TypeError("shape entries must be integers")
    new_shape = [int(s) for s in new_shape]
    rest, infer = 1, -1
    for i in range(len(new_shape) - 1, -1, -1):
        if new_shape[i] < 0:
            if new_shape[i] != -1:
                raise ValueError("Invalid dimension: %d" % new_shape[i])
            if infer != -1:
                raise ValueError("At most on dimension may be -1.")
            infer = i
        else:
            rest *= new_shape[i]
    if infer != -1:
        if rest == 0 or n % rest != 0:
            raise ValueError("Shape cannot be inferred.")
        new_shape[infer] = n // rest
    _check_shape(new_shape, n)
    return new_shape


def _concat_plan(axis, shapes):
    """concat on shapes: (out_shape, strides of the result, [offset of each piece in the result]); piece k, read in its own
    C order, lands at out[offset_k + sum i_d strides[d]]"""
    shapes = [[int(s) for s in sh] for sh in shapes]
    if not shapes:
        raise ValueError("concat: no arrays")
    axis = 0 if axis is None else int(axis)
    ndim = len(shapes[0])
    if axis < 0:
        axis += ndim
    if axis < 0 or axis >= ndim:
        raise ValueError("Axis out of bounds.")
    out = list(shapes[0])
    for sh in reversed(shapes[1:]):
        if len(sh) != ndim:
            raise ValueError("All shapes must have the same length.")
        if any(out[d] != sh[d] and d != axis for d in range(ndim)):
            raise ValueError("Shape along all axes but the concatentation axis must match.")
        out[axis] += sh[axis]
    strides = _c_strides(out)
    offs, at = [], 0
    for sh in shapes:
        offs.append(at * strides[axis])
        at += sh[axis]
    return out, strides, offs


def _stack_plan(axis, shapes):
    """stack on shapes: the shapes with the new axis of extent 1 inserted, then _concat_plan"""
    shapes = [[int(s) for s in sh] for sh in shapes]
    if not shapes:
        raise ValueError("stack: no arrays")
    axis = 0 if axis is None else int(axis)
    if axis < 0:
        axis += len(shapes[0]) + 1
    if axis < 0 or axis > len(shapes[0]):
        raise ValueError("Axis out of bounds.")
    return (axis,) + _concat_plan(axis, [sh[:axis] + [1] + sh[axis:] for sh in shapes])


GATHER_MAX_ND = 8


def _reduce_box(shape, src_strides, dst_strides):
    """the box of one strided copy, reduced for the kernel: extent-1 axes dropped, neighbours d, d+1 merged where
    stride_d == stride_{d+1} shape_{d+1} on both sides, and what is left beyond GATHER_MAX_ND axes peeled off the outer end into a
    host loop. Returns (shape, src_strides, dst_strides, loop): loop lists the (src offset, dst offset) of every launch."""
    axes = [[int(n), int(s), int(t)] for n, s, t in zip(shape, src_strides, dst_strides) if int(n) != 1]
    merged = []
    for n, s, t in axes:
        if merged and merged[-1][1] == s * n and merged[-1][2] == t * n:
            merged[-1] = [merged[-1][0] * n, s, t]
        else:
            merged.append([n, s, t])
    peel, kept = merged[:max(0, len(merged) - GATHER_MAX_ND)], merged[max(0, len(merged) - GATHER_MAX_ND):]
    loop = [(0, 0)]
    for n, s, t in peel:
        loop = [(a + i * s, b + i * t) for a, b in loop for i in range(n)]
    return [a[0] for a in kept], [a[1] for a in kept], [a[2] for a in kept], loop


def _box_reach(shape, strides, off):
    """the lowest and the highest element a box reaches from `off` (the bounds rule of nd4hip_gather_nd_dev)"""
    lo = hi = int(off)
    for n, s in zip(shape, strides):
        span = (int(n) - 1) * int(s)
        if span < 0:
            lo += span
        else:
            hi += span
    return lo, hi


# planners of the elementwise kernels (csrc/elem.hip): nd.zip_elems' broadcast rule (zip_elems.js:43-53) and NDArray.reduceElems'
# axes (nd_array.js:479-497) on shapes alone, with the reference's texts. Pure host code.
EW_OPS = {"add": 0, "sub": 1, "mul": 2, "div": 3, "min": 4, "max": 5, "neg": 16, "abs": 17}
EW_UNARY = ("neg", "abs")
EW_REDUCERS = ("add", "mul", "min", "max")
EW_MAX_ND = 8


def _zip_plan(shapes):
    """zip_elems on shapes: (shape, strides, box). shape is the broadcast result; strides[k][d] is operand k's stride along result
    axis d in elements of its own C order, 0 where it is broadcast; box = (box_shape, box_strides, loop) is the same reduced for
    nd4hip_dzip_nd_dev: extent-1 axes dropped, neighbours merged where every operand (and the dense result) allows, what exceeds
    EW_MAX_ND axes peeled off the outer end into `loop`, a list of (offset of each operand ..., offset in the result)."""
    shapes = [[int(s) for s in sh] for sh in shapes]
    ndim = max([len(sh) for sh in shapes] + [0])
    shape = [1] * ndim
    for sh in shapes:
        for i, j in zip(range(ndim - 1, -1, -1), range(len(sh) - 1, -1, -1)):
            if shape[i] == 1:
                shape[i] = sh[j]
            elif shape[i] != sh[j] and sh[j] != 1:
                raise ValueError("Shapes are not broadcast-compatible.")
    strides = []
    for sh in shapes:
        own, pad = _c_strides(sh), ndim - len(sh)
        strides.append([0 if d < pad or sh[d - pad] == 1 else own[d - pad] for d in range(ndim)])
    axes = [[shape[d], _c_strides(shape)[d]] + [st[d] for st in strides] for d in range(ndim) if shape[d] != 1]
    merged = []
    for ax in axes:
        if merged and all(p == s * ax[0] for p, s in zip(merged[-1][1:], ax[1:])):
            merged[-1] = [merged[-1][0] * ax[0]] + ax[1:]
        else:
            merged.append(list(ax))
    cut = max(0, len(merged) - EW_MAX_ND)
    loop = [tuple([0] * (len(shapes) + 1))]
    for ax in merged[:cut]:
        loop = [tuple(o + i * s for o, s in zip(offs, ax[2:] + ax[1:2])) for offs in loop for i in range(ax[0])]
    kept = merged[cut:]
    box = ([ax[0] for ax in kept], [[ax[2 + k] for ax in kept] for k in range(len(shapes))], loop)
    return shape, strides, box


def _reduce_axes(ndim, axes):
    """the set of reduced axes as nd_array.js:479-493 reads them: a number, a list, or a 1-D int32 array; negative axes wrap,
    duplicates collapse"""
    if isinstance(axes, np.ndarray):
        if axes.dtype != np.int32:
            raise ValueError("Invalid dtype %s for axes." % ("object" if axes.dtype == object else axes.dtype.name))
        if axes.ndim != 1:
            raise ValueError("Only 1D nd.Array allowed for axes.")
        axes = axes.tolist()
    elif isinstance(axes, (int, float, np.integer, np.floating)) and not isinstance(axes, (bool, np.bool_)):
        axes = [axes]
    out = set()
    for ax in axes:
        if not _integral(ax):
            raise TypeError("axes must be integers")
        ax = int(ax)
        if ax < 0:
            ax += ndim
        if ax < 0 or ax >= ndim:
            raise ValueError("Reduction axis %d out of bounds." % ax)
        out.add(ax)
    return out


def _reduce_plan(shape, axes):
    """reduceElems on a shape: (out_shape, box_shape, box_flags, loop). box is what nd4hip_dreduce_nd_dev takes: extent-1 axes
    dropped and neighbours of one kind merged, so that kept (flag 0) and reduced (flag 1) axes alternate; kept axes beyond
    EW_MAX_ND are peeled off the outer end into `loop`, a list of (offset in the operand, offset in the result)."""
    shape = [int(s) for s in shape]
    red = _reduce_axes(len(shape), axes)
    out_shape = [n for d, n in enumerate(shape) if d not in red]
    merged = []
    for d, n in enumerate(shape):
        if n == 1:
            continue
        f = 1 if d in red else 0
        if merged and merged[-1][1] == f:
            merged[-1][0] *= n
        else:
            merged.append([n, f])
    loop = [(0, 0)]
    while len(merged) > EW_MAX_ND and merged[0][1] == 0:
        n = merged.pop(0)[0]
        a_step, c_step = 1, 1
        for m, f in merged:
            a_step *= m
            if not f:
                c_step *= m
        loop = [(a + i * a_step, c + i * c_step) for a, c in loop for i in range(n)]
    if len(merged) > EW_MAX_ND:
        raise ValueError("reduceElems: more than %d alternating kept and reduced axes are not accelerated." % EW_MAX_ND)
    return out_shape, [m[0] for m in merged], [m[1] for m in merged], loop
