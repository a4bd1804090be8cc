"""Device-resident form of the hot path: the same C ABI (`*_dev` entry points) on torch CUDA tensors.

PyTorch is plumbing only (device memory + the current HIP stream + torch.distributed); every
kernel that runs is from libnd4hip.so. Tensors must be float64, contiguous, on a HIP device.
"""
import ctypes

import torch

from . import _lib


def _h(t):
    h = _lib.handle(t.device.index)
    h.set_stream(torch.cuda.current_stream(t.device).cuda_stream)
    return h


def _chk(t, name):
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float64 and t.is_contiguous()):
        raise TypeError("%s must be a contiguous float64 CUDA tensor" % name)
    return t


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _batch(shape):
    n = 1
    for s in shape:
        n *= int(s)
    return n


def fill_uniform(seed, shape, device="cuda", offset=0):
    out = torch.empty(shape, dtype=torch.float64, device=device)
    h = _h(out)
    _lib.check(h.lib.nd4hip_fill_uniform_dev(h.ptr, seed, offset, out.numel(), _p(out)))
    return out


def _chk_mm(t, name):
    """an operand of the complex path: its values as stored. torch's lazy conjugate / negative views (x.conj(), ...) share
    the storage of x and only flag it, so they are materialised here (the kernels read the storage)."""
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype in (torch.float64, torch.complex128) and t.is_contiguous()):
        raise TypeError("%s must be a contiguous float64 or complex128 CUDA tensor" % name)
    return t.resolve_conj().resolve_neg()


def matmul2(a, b, out=None):
    """[..., I, K] x [..., K, J]; leading dims must be equal or one operand plain 2-D (broadcast).
    float64 x float64 -> float64; complex128 with complex128 or float64, in either order -> complex128."""
    if getattr(a, "dtype", None) == torch.complex128 or getattr(b, "dtype", None) == torch.complex128:
        return _zmatmul2(a, b, out)
    _chk(a, "a"), _chk(b, "b")
    I, K = a.shape[-2:]
    J = b.shape[-1]
    if b.shape[-2] != K:
        raise ValueError("The last dimension of A and the 2nd to last dimension of B do not match.")
    la, lb = tuple(a.shape[:-2]), tuple(b.shape[:-2])
    if la == lb:
        lead, sA, sB = la, I * K, K * J
    elif _batch(lb) == 1:
        lead, sA, sB = la, I * K, 0
    elif _batch(la) == 1:
        lead, sA, sB = lb, 0, K * J
    else:
        raise ValueError("Shapes are not broadcast-compatible.")   # general broadcasting: host wrapper (la.py)
    batch = _batch(lead)
    if out is None:
        out = torch.empty(lead + (I, J), dtype=torch.float64, device=a.device)
    h = _h(a)
    _lib.check(h.lib.nd4hip_dgemm_batched_dev(h.ptr, batch, I, K, J, _p(a), sA if batch > 1 else 0,
                                              _p(b), sB if batch > 1 else 0, _p(_chk(out, "out"))))
    return out


def _zmatmul2(a, b, out):
    a, b = _chk_mm(a, "a"), _chk_mm(b, "b")
    I, K = a.shape[-2:]
    J = b.shape[-1]
    if b.shape[-2] != K:
        raise ValueError("The last dimension of A and the 2nd to last dimension of B do not match.")
    la, lb = tuple(a.shape[:-2]), tuple(b.shape[:-2])
    if la == lb:
        lead, sA, sB = la, I * K, K * J
    elif _batch(lb) == 1:
        lead, sA, sB = la, I * K, 0
    elif _batch(la) == 1:
        lead, sA, sB = lb, 0, K * J
    else:
        raise ValueError("Shapes are not broadcast-compatible.")
    batch = _batch(lead)
    if out is None:
        out = torch.empty(lead + (I, J), dtype=torch.complex128, device=a.device)
    elif not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.complex128 and out.is_contiguous()
              and tuple(out.shape) == lead + (I, J) and not out.is_conj() and not out.is_neg()):
        # (a conjugate or negative view would read back what the kernel writes conjugated / negated)
        raise TypeError("out must be a contiguous complex128 CUDA tensor of shape %r without a conjugate or negative bit"
                        % (lead + (I, J),))
    h = _h(a)
    _lib.check(h.lib.nd4hip_zgemm_batched_dev(h.ptr, int(a.dtype == torch.complex128), int(b.dtype == torch.complex128),
                                              batch, I, K, J, _p(a), sA if batch > 1 else 0,
                                              _p(b), sB if batch > 1 else 0, _p(out)))
    return out


def gemm_ex(transA, transB, alpha, A, B, beta, C, M, N, K, lda, ldb, ldc):
    h = _h(C)
    _lib.check(h.lib.nd4hip_dgemm_ex_dev(h.ptr, int(transA), int(transB), M, N, K, alpha, _p(A), lda, _p(B), ldb,
                                         beta, _p(C), ldc))
    return C


def lu_decomp(A):
    _chk(A, "A")
    N = A.shape[-1]
    if A.dim() < 2 or A.shape[-2] != N:
        raise ValueError("Last two dimensions must be quadratic.")
    LU = torch.empty_like(A)
    P = torch.empty(A.shape[:-1], dtype=torch.int32, device=A.device)
    h = _h(A)
    _lib.check(h.lib.nd4hip_dgetrf_batched_dev(h.ptr, _batch(A.shape[:-2]), N, _p(A), _p(LU), ctypes.c_void_p(P.data_ptr())))
    return LU, P


def qr_decomp(A):
    _chk(A, "A")
    if A.dim() < 2:
        raise ValueError("qr_decomp(A): A.ndim must be at least 2.")
    M, N = A.shape[-2:]
    L = min(M, N)
    Q = torch.empty(tuple(A.shape[:-2]) + (M, L), dtype=torch.float64, device=A.device)
    R = torch.empty(tuple(A.shape[:-2]) + (L, N), dtype=torch.float64, device=A.device)
    h = _h(A)
    _lib.check(h.lib.nd4hip_dgeqrf_q_batched_dev(h.ptr, _batch(A.shape[:-2]), M, N, _p(A), _p(Q), _p(R)))
    return Q, R


def _gesvdx(A, what, subset, vectors, info):
    from .la import _svd_subset
    _chk(A, "A")
    if A.dim() < 2:
        raise ValueError("%s: A.ndim must be at least 2." % what)
    M, N = A.shape[-2:]
    L = min(M, N)
    if L > 2048:
        raise ValueError("%s: min(M, N) <= 2048." % what)
    lead = tuple(A.shape[:-2])
    i0, i1 = (0, L) if subset is None else _svd_subset(subset, L, what, False)
    k = i1 - i0
    sv = torch.empty(lead + (k,), dtype=torch.float64, device=A.device)
    U = torch.empty(lead + (M, k), dtype=torch.float64, device=A.device) if vectors else None
    V = torch.empty(lead + (k, N), dtype=torch.float64, device=A.device) if vectors else None
    fb = torch.zeros(lead, dtype=torch.int32, device=A.device) if info is not None else None
    if sv.numel():
        h = _h(A)
        _lib.check(h.lib.nd4hip_dgesvdx_batched_dev(h.ptr, _batch(lead), M, N, i0, i1, _p(A), _p(U) if vectors else None, _p(sv),
                                                    _p(V) if vectors else None, _p(fb) if fb is not None else None))
    if info is not None:
        info["fallback"] = fb
    return (U, sv, V) if vectors else sv


def svd_decomp(A, info=None, algo=None, *, subset=None):
    """algo None / 'jacobi': block one-sided Jacobi (the default route); 'dc': bidiagonalisation + divide & conquer (opt-in);
    subset=(i0, i1) (opt-in, not with 'jacobi'): the triplets sv[i0:i1] alone (csrc/bdsvdx.hip)"""
    if algo not in (None, "jacobi", "dc"):
        raise ValueError("svd_decomp(A, algo): algo must be None, 'jacobi' or 'dc'.")
    if subset is not None:
        if algo == "jacobi":
            raise ValueError("svd_decomp(A, subset): subset is not available with algo='jacobi'.")
        return _gesvdx(A, "svd_decomp(A, subset)", subset, True, info)
    _chk(A, "A")
    if A.dim() < 2:
        raise ValueError("svd_decomp(A): A.ndim must be at least 2.")
    M, N = A.shape[-2:]
    L = min(M, N)
    lead = tuple(A.shape[:-2])
    U = torch.empty(lead + (M, L), dtype=torch.float64, device=A.device)
    sv = torch.empty(lead + (L,), dtype=torch.float64, device=A.device)
    V = torch.empty(lead + (L, N), dtype=torch.float64, device=A.device)
    sweeps, off = ctypes.c_int(0), ctypes.c_double(0.0)
    h = _h(A)
    if algo == "dc":
        _lib.check(h.lib.nd4hip_dgesdd_batched_dev(h.ptr, _batch(lead), M, N, _p(A), _p(U), _p(sv), _p(V)))
        return U, sv, V
    _lib.check(h.lib.nd4hip_dgesvdj_batched_dev(h.ptr, _batch(lead), M, N, _p(A), _p(U), _p(sv), _p(V),
                                                ctypes.byref(sweeps), ctypes.byref(off)))
    if info is not None:
        info["sweeps"], info["offnorm"] = sweeps.value, off.value
        info["rotations"] = h.svd_last_info()["rotations"]
    return U, sv, V


def svd_vals(A, info=None, subset=None):
    """device-resident la.svd_vals: sv [..., k] alone, the bits of svd_decomp(A, subset)'s"""
    return _gesvdx(A, "svd_vals(A)", subset, False, info)


def _bdsvdx(d, e, what, subset, vectors, info):
    from .la import _bidiag_operands, _subset
    d, e, K, J = _bidiag_operands(d, e, what, lambda t, w: _chk(t, w[:w.index("(")] + " operand"))
    if K > 2048:
        raise ValueError("%s: K <= 2048." % what)
    i0, i1 = (0, K) if subset is None else _subset(subset, K, what)
    lead, k = tuple(d.shape[:-1]), i1 - i0
    sv = torch.empty(lead + (k,), dtype=torch.float64, device=d.device)
    U2 = torch.empty(lead + (K, k), dtype=torch.float64, device=d.device) if vectors else None
    V2 = torch.empty(lead + (k, J), dtype=torch.float64, device=d.device) if vectors else None
    fb = torch.zeros(lead, dtype=torch.int32, device=d.device) if info is not None else None
    if sv.numel():
        h = _h(d)
        _lib.check(h.lib.nd4hip_dbdsvdx_batched_dev(h.ptr, _batch(lead), K, J, i0, i1, _p(d), _p(e), _p(U2) if vectors else None, _p(sv),
                                                    _p(V2) if vectors else None, _p(fb) if fb is not None else None))
    if info is not None:
        info["fallback"] = fb
    return (U2, sv, V2) if vectors else sv


def bidiag_svd(d, e, subset=None, info=None):
    """device-resident la.bidiag_svd: d [..., K], e [..., J-1] (J = K or K + 1) -> U2 [..., K, K], sv [..., K], V2 [..., J, J];
    subset=(i0, i1) (opt-in): U2 [..., K, k], sv [..., k], V2 [..., k, J] (csrc/bdsvdx.hip), info['fallback'] int32 [...]"""
    if subset is not None:
        return _bdsvdx(d, e, "bidiag_svd(d,e, subset)", subset, True, info)
    _chk(d, "d"), _chk(e, "e")
    if d.dim() < 1 or e.dim() < 1 or tuple(d.shape[:-1]) != tuple(e.shape[:-1]):
        raise ValueError("bidiag_svd(d,e): d and e must have the same leading dimensions.")
    K, J = d.shape[-1], e.shape[-1] + 1
    if K < 1 or J not in (K, K + 1):
        raise ValueError("bidiag_svd(d,e): e must have len(d) - 1 or len(d) entries.")
    lead = tuple(d.shape[:-1])
    U2 = torch.empty(lead + (K, K), dtype=torch.float64, device=d.device)
    sv = torch.empty(lead + (K,), dtype=torch.float64, device=d.device)
    V2 = torch.empty(lead + (J, J), dtype=torch.float64, device=d.device)
    h = _h(d)
    _lib.check(h.lib.nd4hip_dbdsdc_batched_dev(h.ptr, _batch(lead), K, J, _p(d), _p(e), _p(U2), _p(sv), _p(V2)))
    return U2, sv, V2


def bidiag_svdvals(d, e, subset=None, info=None):
    """device-resident la.bidiag_svdvals: sv [..., k] by bisection alone, the bits of bidiag_svd(d, e, subset)'s"""
    return _bdsvdx(d, e, "bidiag_svdvals(d,e)", subset, False, info)


def lu_solve(LU, P, Y):
    """device-resident lu_solve (lu.js:84-177): LU [..., N, N], P [..., N] int32, Y [..., N, J] with equal leading dims"""
    _chk(LU, "LU"), _chk(Y, "Y")
    N, J = Y.shape[-2:]
    if LU.shape[-1] != N or LU.shape[-2] != N:
        raise ValueError("LU and y don't match.")
    lead = tuple(Y.shape[:-2])
    if tuple(LU.shape[:-2]) != lead or tuple(P.shape[:-1]) != lead:
        raise ValueError("LU and y are not broadcast-compatible.")   # general broadcasting: host wrapper (la.py)
    X = torch.empty(lead + (N, J), dtype=torch.float64, device=Y.device)
    h = _h(Y)
    b = _batch(lead)
    _lib.check(h.lib.nd4hip_dgetrs_batched_dev(h.ptr, b, N, J, _p(LU), N * N if b > 1 else 0, ctypes.c_void_p(P.data_ptr()), N if b > 1 else 0,
                                               _p(Y), N * J if b > 1 else 0, _p(X)))
    return X


def tri_solve(T, Y, upper, unit_diag=False):
    _chk(T, "T"), _chk(Y, "Y")
    M, J = Y.shape[-2:]
    lead = tuple(Y.shape[:-2])
    if tuple(T.shape[:-2]) != lead or T.shape[-1] != M or T.shape[-2] != M:
        raise ValueError("T and Y don't match.")
    X = torch.empty_like(Y)
    h = _h(Y)
    b = _batch(lead)
    _lib.check(h.lib.nd4hip_dtrsm_batched_dev(h.ptr, int(bool(upper)), int(bool(unit_diag)), b, M, J, _p(T), M * M if b > 1 else 0,
                                              _p(Y), M * J if b > 1 else 0, _p(X)))
    return X


def qr_lstsq(Q, R, Y):
    """device-resident qr_lstsq (qr.js:186-273): Q [..., N, M], R [..., M, I], Y [..., N, J] with equal leading dims"""
    _chk(Q, "Q"), _chk(R, "R"), _chk(Y, "Y")
    N, M = Q.shape[-2:]
    I, J = R.shape[-1], Y.shape[-1]
    if N != Y.shape[-2]:
        raise ValueError("qr_lstsq(Q,R,y): Q and y don't match.")
    if M != R.shape[-2]:
        raise ValueError("qr_lstsq(Q,R,y): Q and R don't match.")
    if I > N:
        raise ValueError("qr_lstsq(Q,R,y): Under-determined systems not supported. Use rrqr instead.")
    lead = tuple(Y.shape[:-2])
    if tuple(Q.shape[:-2]) != lead or tuple(R.shape[:-2]) != lead:
        raise ValueError("Q, R, y are not broadcast-compatible.")      # general broadcasting: host wrapper (la.py)
    X = torch.empty(lead + (I, J), dtype=torch.float64, device=Y.device)
    h = _h(Y)
    b = _batch(lead)
    _lib.check(h.lib.nd4hip_dqrls_batched_dev(h.ptr, b, N, M, I, J, _p(Q), N * M if b > 1 else 0, _p(R), M * I if b > 1 else 0,
                                              _p(Y), N * J if b > 1 else 0, _p(X)))
    return X


def svd_lstsq(U, sv, V, Y):
    """device-resident svd_lstsq (svd.js:100-228); singular values are not checked for NaN/Inf here (no host read-back)"""
    _chk(U, "U"), _chk(sv, "sv"), _chk(V, "V"), _chk(Y, "Y")
    N, M = U.shape[-2:]
    I, J = V.shape[-1], Y.shape[-1]
    if N != Y.shape[-2]:
        raise ValueError("svd_lstsq(U,sv,V, y): U and y don't match.")
    if M != sv.shape[-1]:
        raise ValueError("svd_lstsq(U,sv,V, y): U and sv don't match.")
    if M != V.shape[-2]:
        raise ValueError("svd_lstsq(U,sv,V, y): V and sv don't match.")
    lead = tuple(Y.shape[:-2])
    if tuple(U.shape[:-2]) != lead or tuple(V.shape[:-2]) != lead or tuple(sv.shape[:-1]) != lead:
        raise ValueError("svd_lstsq(U,sv,V, y): U,sv,V,y not broadcast-compatible.")
    X = torch.empty(lead + (I, J), dtype=torch.float64, device=Y.device)
    h = _h(Y)
    b = _batch(lead)
    _lib.check(h.lib.nd4hip_dsvdls_batched_dev(h.ptr, b, N, M, I, J, _p(U), N * M if b > 1 else 0, _p(sv), M if b > 1 else 0,
                                               _p(V), M * I if b > 1 else 0, _p(Y), N * J if b > 1 else 0, _p(X)))
    return X


def qr_decomp_full(A):
    _chk(A, "A")
    M, N = A.shape[-2:]
    lead = tuple(A.shape[:-2])
    Q = torch.empty(lead + (M, M), dtype=torch.float64, device=A.device)
    R = torch.empty(lead + (M, N), dtype=torch.float64, device=A.device)
    h = _h(A)
    _lib.check(h.lib.nd4hip_dgeqrf_full_batched_dev(h.ptr, _batch(lead), M, N, _p(A), _p(Q), _p(R)))
    return Q, R


def qr_decomp_inplace(A, Y):
    """_qr_decomp_inplace (qr.js:146-183) on device tensors, in place: A <- R, Y <- Q^T Y"""
    _chk(A, "A"), _chk(Y, "Y")
    if tuple(A.shape[:-1]) != tuple(Y.shape[:-1]):
        raise ValueError("Assertion failed.")
    M, N = A.shape[-2:]
    h = _h(A)
    _lib.check(h.lib.nd4hip_dgeqrf_qty_batched_dev(h.ptr, _batch(A.shape[:-2]), M, N, Y.shape[-1], _p(A), _p(Y)))
    return A, Y


def cholesky_decomp(S):
    """device-resident cholesky_decomp (cholesky.js:51-71); one flag read-back decides the reference's singularity error"""
    _chk(S, "S")
    N = S.shape[-1]
    if S.dim() < 2 or S.shape[-2] != N:
        raise ValueError("Last two dimensions must be quadratic.")
    L = torch.empty_like(S)
    h = _h(S)
    try:
        _lib.check(h.lib.nd4hip_dpotrf_batched_dev(h.ptr, _batch(S.shape[:-2]), N, _p(S), _p(L)))
    except _lib.Nd4HipError as e:
        if e.code == -5:
            raise ValueError("Matrix contains NaNs or is (near) singular.")
        raise
    return L


def cholesky_solve(L, Y):
    _chk(L, "L"), _chk(Y, "Y")
    N, J = Y.shape[-2:]
    if L.shape[-1] != L.shape[-2]:
        raise ValueError("Last two dimensions of L must be quadratic.")
    if L.shape[-1] != N:
        raise ValueError("L and y don't match.")
    lead = tuple(Y.shape[:-2])
    if tuple(L.shape[:-2]) != lead:
        raise ValueError("Shapes are not broadcast-compatible.")       # general broadcasting: host wrapper (la.py)
    X = torch.empty_like(Y)
    h = _h(Y)
    b = _batch(lead)
    _lib.check(h.lib.nd4hip_dpotrs_batched_dev(h.ptr, b, N, J, _p(L), N * N if b > 1 else 0, _p(Y), N * J if b > 1 else 0, _p(X)))
    return X


def ldl_decomp(S):
    _chk(S, "S")
    N = S.shape[-1]
    if S.dim() < 2 or S.shape[-2] != N:
        raise ValueError("Last two dimensions must be quadratic.")
    LD = torch.empty_like(S)
    h = _h(S)
    _lib.check(h.lib.nd4hip_dldltrf_batched_dev(h.ptr, _batch(S.shape[:-2]), N, _p(S), _p(LD)))
    return LD


def ldl_solve(LD, Y):
    _chk(LD, "LD"), _chk(Y, "Y")
    N, J = Y.shape[-2:]
    if LD.shape[-1] != LD.shape[-2]:
        raise ValueError("ldl_solve(LD,y): Last two dimensions of LD must be quadratic.")
    if LD.shape[-1] != N:
        raise ValueError("ldl_solve(LD,y): LD and y don't match.")
    lead = tuple(Y.shape[:-2])
    if tuple(LD.shape[:-2]) != lead:
        raise ValueError("Shapes are not broadcast-compatible.")       # general broadcasting: host wrapper (la.py)
    X = torch.empty_like(Y)
    h = _h(Y)
    b = _batch(lead)
    _lib.check(h.lib.nd4hip_dldltrs_batched_dev(h.ptr, b, N, J, _p(LD), N * N if b > 1 else 0, _p(Y), N * J if b > 1 else 0, _p(X)))
    return X


def pldlp_decomp(S, tier=None, out=None):
    """[LD, P] (P int32) of symmetric S [..., N, N] by Bunch-Kaufman pivoting, the reference's bits (la.pldlp_decomp); out=S
    factorises in place. A singular member raises ValueError with the reference's text and the member."""
    from .la import _arg_error, _pldlp_tier
    _chk(S, "S")
    N = S.shape[-1]
    if S.dim() < 2 or S.shape[-2] != N:
        raise ValueError("Last two dimensions must be quadratic.")
    LD = torch.empty_like(S) if out is None else _chk(out, "out")
    P = torch.empty(S.shape[:-1], dtype=torch.int32, device=S.device)
    h = _h(S)
    try:
        _lib.check(h.lib.nd4hip_dsytrf_bk_batched_ex_dev(h.ptr, _batch(S.shape[:-2]), N, _p(S), _p(LD), _p(P), _pldlp_tier(tier)))
    except _lib.Nd4HipError as e:
        if e.code == -5:
            raise ValueError(str(e).split(": ", 1)[1])
        raise _arg_error(e)
    return [LD, P]


def pldlp_solve(LD, P, Y, out=None):
    """X with S X = Y from pldlp_decomp's LD [..., N, N] and P [..., N] (int32); LD and P may be one pair for a batch of Y.
    out=Y solves in place. An index of P out of range raises ValueError (nothing is read or written out of bounds)."""
    from .la import _arg_error
    _chk(LD, "LD"), _chk(Y, "Y")
    if not (isinstance(P, torch.Tensor) and P.is_cuda and P.dtype == torch.int32 and P.is_contiguous()):
        raise TypeError("P must be a contiguous int32 CUDA tensor")
    N, J = Y.shape[-2:]
    if LD.dim() < 2 or LD.shape[-1] != LD.shape[-2]:
        raise ValueError("pldlp_solve(LD,P,y): LD must be square.")
    if P.dim() < 1 or P.shape[-1] != LD.shape[-1] or tuple(P.shape[:-1]) != tuple(LD.shape[:-2]):
        raise ValueError("pldlp_solve(LD,P,y): LD and P shape mismatch.")
    if LD.shape[-1] != N:
        raise ValueError("pldlp_solve(LD,P,y): LD and y shape mismatch.")
    lead = tuple(Y.shape[:-2])
    one = _batch(LD.shape[:-2]) == 1
    if tuple(LD.shape[:-2]) != lead and not one:
        raise ValueError("Shapes are not broadcast-compatible.")       # general broadcasting: host wrapper (la.py)
    X = torch.empty_like(Y) if out is None else _chk(out, "out")
    h = _h(Y)
    b = _batch(lead)
    try:
        _lib.check(h.lib.nd4hip_dsytrs_bk_batched_dev(h.ptr, b, N, J, _p(LD), 0 if one else N * N, _p(P), 0 if one else N, _p(Y),
                                                      N * J if b > 1 else 0, _p(X)))
    except _lib.Nd4HipError as e:
        raise _arg_error(e)
    return X


def hessenberg_decomp(A):
    _chk(A, "A")
    N = A.shape[-1]
    if A.dim() < 2 or A.shape[-2] != N:
        raise ValueError("hessenberg_decomp(A): A must be square.")
    U, H = torch.empty_like(A), torch.empty_like(A)
    h = _h(A)
    _lib.check(h.lib.nd4hip_dgehrd_batched_dev(h.ptr, _batch(A.shape[:-2]), N, _p(A), _p(U), _p(H)))
    return U, H


def bidiag_decomp(A):
    _chk(A, "A")
    if A.dim() < 2:
        raise ValueError("bidiag_decomp(A): A must be at least 2D.")
    M, N = A.shape[-2:]
    I = min(M, N)
    J = I if M >= N else I + 1
    lead = tuple(A.shape[:-2])
    U = torch.empty(lead + (M, I), dtype=torch.float64, device=A.device)
    B = torch.empty(lead + (I, J), dtype=torch.float64, device=A.device)
    V = torch.empty(lead + (J, N), dtype=torch.float64, device=A.device)
    h = _h(A)
    _lib.check(h.lib.nd4hip_dgebrd_batched_dev(h.ptr, _batch(lead), M, N, _p(A), _p(U), _p(B), _p(V)))
    return U, B, V


def _rrqr(A, full):
    _chk(A, "A")
    if A.dim() < 2:
        raise ValueError("A must be at least 2D.")
    M, N = A.shape[-2:]
    L = M if full else min(M, N)
    lead = tuple(A.shape[:-2])
    Q = torch.empty(lead + (M, L), dtype=torch.float64, device=A.device)
    R = torch.empty(lead + (L, N), dtype=torch.float64, device=A.device)
    P = torch.empty(lead + (N,), dtype=torch.int32, device=A.device)
    h = _h(A)
    fn = h.lib.nd4hip_dgeqp3_full_batched_dev if full else h.lib.nd4hip_dgeqp3_batched_dev
    _lib.check(fn(h.ptr, _batch(lead), M, N, _p(A), _p(Q), _p(R), _p(P)))
    return Q, R, P


def rrqr_decomp(A):
    """device-resident rrqr_decomp (rrqr.js:278-395): Q [..., M, L], R [..., L, N], P [..., N] int32"""
    return _rrqr(A, False)


def rrqr_decomp_full(A):
    """device-resident rrqr_decomp_full (rrqr.js:88-184)"""
    return _rrqr(A, True)


def rrqr_rank(R):
    """device-resident rrqr_rank (rrqr.js:398-414): int32 tensor; -1 where the reference would throw (no host read-back here)"""
    _chk(R, "R")
    M, N = R.shape[-2:]
    r = torch.empty(tuple(R.shape[:-2]), dtype=torch.int32, device=R.device)
    h = _h(R)
    _lib.check(h.lib.nd4hip_dqp3rank_batched_dev(h.ptr, _batch(R.shape[:-2]), M, N, _p(R), _p(r)))
    return r


def rrqr_lstsq(Q, R, P, Y, rank=None):
    """device-resident rrqr_lstsq (rrqr.js:447-580): Q [..., N, M], R [..., M, I], P [..., I] int32, Y [..., N, J] with equal
    leading dims; `rank` (optional int32 tensor of the batch shape) receives each matrix's rank (-1: non-finite). No host read-back."""
    _chk(Q, "Q"), _chk(R, "R"), _chk(Y, "Y")
    if not (isinstance(P, torch.Tensor) and P.is_cuda and P.dtype == torch.int32 and P.is_contiguous()):
        raise ValueError('rrqr_lstsq(Q,R,P, y): P.dtype must be "int32".')
    N, M = Q.shape[-2:]
    I, J = R.shape[-1], Y.shape[-1]
    if N != Y.shape[-2]:
        raise ValueError("rrqr_lstsq(Q,R,P,y): Q and y don't match.")
    if M != R.shape[-2]:
        raise ValueError("rrqr_lstsq(Q,R,P,y): Q and R don't match.")
    if I != P.shape[-1]:
        raise ValueError("rrqr_lstsq(Q,R,P,y): R and P don't match.")
    lead = tuple(Y.shape[:-2])
    if tuple(Q.shape[:-2]) != lead or tuple(R.shape[:-2]) != lead or tuple(P.shape[:-1]) != lead:
        raise ValueError("rrqr_lstsq(Q,R,P,y): Q,R,P,y not broadcast-compatible.")   # general broadcasting: host wrapper (la.py)
    X = torch.empty(lead + (I, J), dtype=torch.float64, device=Y.device)
    h = _h(Y)
    b = _batch(lead)
    _lib.check(h.lib.nd4hip_dqp3ls_batched_dev(h.ptr, b, N, M, I, J, _p(Q), N * M if b > 1 else 0, _p(R), M * I if b > 1 else 0,
                                               _p(P), I if b > 1 else 0, _p(Y), N * J if b > 1 else 0, _p(X),
                                               _p(rank) if rank is not None else None))
    return X


def srrqr_decomp_full(A, dtol=1.01, ztol=None):
    """device-resident srrqr_decomp_full (srrqr.js:58-802): Q [..., M, M], R [..., M, N], P [..., N] int32, r [...] int32.
    No host read-back: r is -1 where ||A||_F is not finite and -2 where the swap cap was hit."""
    _chk(A, "A")
    if A.dim() < 2:
        raise ValueError("srrqr_decomp_full(A,opt): A must be at least 2D.")
    from .la import _srrqr_opts
    dtol, ztol = _srrqr_opts(None, dtol, ztol)
    M, N = A.shape[-2:]
    lead = tuple(A.shape[:-2])
    Q = torch.empty(lead + (M, M), dtype=torch.float64, device=A.device)
    R = torch.empty(lead + (M, N), dtype=torch.float64, device=A.device)
    P = torch.empty(lead + (N,), dtype=torch.int32, device=A.device)
    r = torch.empty(lead, dtype=torch.int32, device=A.device)
    h = _h(A)
    _lib.check(h.lib.nd4hip_dsrrqr_batched_dev(h.ptr, _batch(lead), M, N, _p(A), dtol, ztol, _p(Q), _p(R), _p(P), _p(r)))
    return Q, R, P, r


def urv_decomp_full(A):
    """device-resident urv_decomp_full (urv.js:100-135): U [..., M, M], R [..., M, N], V [..., N, N], r [...] int32 with A = U R V.
    No host read-back: r is -1 / -3 where ||A||_F is Infinity / NaN and -2 where the swap cap was hit."""
    _chk(A, "A")
    if A.dim() < 2:
        raise ValueError("srrqr_decomp_full(A,opt): A must be at least 2D.")
    M, N = A.shape[-2:]
    lead = tuple(A.shape[:-2])
    U = torch.empty(lead + (M, M), dtype=torch.float64, device=A.device)
    R = torch.empty(lead + (M, N), dtype=torch.float64, device=A.device)
    V = torch.empty(lead + (N, N), dtype=torch.float64, device=A.device)
    r = torch.empty(lead, dtype=torch.int32, device=A.device)
    h = _h(A)
    _lib.check(h.lib.nd4hip_durv_batched_dev(h.ptr, _batch(lead), M, N, _p(A), _p(U), _p(R), _p(V), _p(r)))
    return U, R, V, r


def urv_lstsq(U, R, V, ranks, Y):
    """device-resident urv_lstsq (urv.js:138-323): U [..., I, J], R [..., J, K], V [..., K, L], ranks [...] int32, Y [..., I, Jc]
    with equal leading dims -> X [..., L, Jc] (minimum-norm least squares). No host read-back."""
    _chk(U, "U"), _chk(R, "R"), _chk(V, "V"), _chk(Y, "Y")
    if not (isinstance(ranks, torch.Tensor) and ranks.is_cuda and ranks.dtype == torch.int32 and ranks.is_contiguous()):
        raise TypeError("ranks must be a contiguous int32 CUDA tensor")
    I, J = U.shape[-2:]
    K, L = V.shape[-2:]
    Jc = Y.shape[-1]
    lead = tuple(U.shape[:-2])
    if tuple(R.shape) != lead + (J, K) or tuple(V.shape[:-2]) != lead or tuple(Y.shape) != lead + (I, Jc) or tuple(ranks.shape) != lead:
        raise ValueError("urv_lstsq( U,R,V,ranks, Y ): Matrix dimensions incompatible.")
    X = torch.empty(lead + (L, Jc), dtype=torch.float64, device=U.device)
    h = _h(U)
    _lib.check(h.lib.nd4hip_durvls_batched_dev(h.ptr, _batch(lead), I, J, K, L, Jc, _p(U), I * J, _p(R), J * K, _p(V), K * L,
                                               _p(ranks), 1, _p(Y), I * Jc, _p(X)))
    return X


def _det_dev(A, log_form):
    _chk(A, "A")
    if A.dim() < 2:
        raise ValueError("qr_decomp(A): A.ndim must be at least 2.")
    M, N = A.shape[-2:]
    if M < N:
        raise ValueError("det_tri(A): A must be square matrices." if log_form else "det_tri(a): a must be square matrices.")
    lead = tuple(A.shape[:-2])
    D = torch.empty(lead, dtype=torch.float64, device=A.device)
    h = _h(A)
    if log_form:
        L = torch.empty(lead, dtype=torch.float64, device=A.device)
        _lib.check(h.lib.nd4hip_dslogdet_batched_dev(h.ptr, _batch(lead), M, N, _p(A), _p(D), _p(L)))
        return [D, L]
    _lib.check(h.lib.nd4hip_ddet_batched_dev(h.ptr, _batch(lead), M, N, _p(A), _p(D)))
    return D


def det(A):
    """device-resident det (det.js:95-99): float64 [...]. No host read-back: a matrix where the reference's Givens rotation
    asserts ('Assertion failed: NaN') gets the NaN with the bits ND4HIP_DET_ASSERT_NAN_BITS (include/nd4hip.h)."""
    return _det_dev(A, False)


def slogdet(A):
    """device-resident slogdet (det.js:102-106): [sign, logdet]."""
    return _det_dev(A, True)


def _dettri_dev(A, log_form):
    _chk(A, "A")
    if A.dim() < 2:
        raise ValueError("det_tri(A): A.ndim must be at least 2." if log_form else
                         "det_tri(a): a.shape=[%s]; a.ndim must be at least 2." % ",".join(str(s) for s in A.shape))
    M, N = A.shape[-2:]
    if M != N:
        raise ValueError("det_tri(A): A must be square matrices." if log_form else "det_tri(a): a must be square matrices.")
    lead = tuple(A.shape[:-2])
    D = torch.empty(lead, dtype=torch.float64, device=A.device)
    h = _h(A)
    if log_form:
        L = torch.empty(lead, dtype=torch.float64, device=A.device)
        _lib.check(h.lib.nd4hip_dslogdettri_batched_dev(h.ptr, _batch(lead), N, _p(A), _p(D), _p(L)))
        return [D, L]
    _lib.check(h.lib.nd4hip_ddettri_batched_dev(h.ptr, _batch(lead), N, _p(A), _p(D)))
    return D


def det_tri(A):
    """device-resident det_tri (det.js:24-50)."""
    return _dettri_dev(A, False)


def slogdet_tri(A):
    """device-resident slogdet_tri (det.js:53-92): [sign, logdet]."""
    return _dettri_dev(A, True)


def rank(A):
    """rank.js:23-27 on the device: svd_rank of the device SVD's singular values (U and V stay on the device and are dropped)."""
    from .la import svd_rank
    return svd_rank(svd_decomp(A)[1].cpu().numpy())


def lstsq(A, Y):
    """lstsq.js:22-26 on the device: svd_lstsq(svd_decomp(A), Y) with equal leading dims (the host wrapper broadcasts)."""
    U, sv, V = svd_decomp(A)
    return svd_lstsq(U, sv, V, Y)


def norm(A, ord="fro", axis=None):
    """norm.js:74-85 of a device tensor: a Python float (the one number is read back)."""
    if not (isinstance(ord, str) and ord == "fro"):
        from .la import _js_num
        raise ValueError("norm(A,ord,axis): Unsupported ord: %s." % ("null" if ord is None else ord if isinstance(ord, str) else _js_num(ord)))
    if axis is not None:
        raise ValueError("norm(A,ord,axis): axis argument not yet supported.")
    _chk(A, "A")
    out = torch.zeros((), dtype=torch.float64, device=A.device)
    h = _h(A)
    _lib.check(h.lib.nd4hip_dnrmfro_dev(h.ptr, A.numel(), _p(A), _p(out)))
    return float(out.item())


def _ev_sq(T, what):
    _chk(T, "T")
    if T.dim() < 2 or T.shape[-2] != T.shape[-1]:
        raise ValueError(what)
    return tuple(T.shape[:-2]), int(T.shape[-1])


def _ev_call(fn, *args):
    from .la import _arg_error
    try:
        _lib.check(fn(*args))
    except _lib.Nd4HipError as e:
        raise _arg_error(e)


def schur_eigenvals(T):
    """device-resident schur_eigenvals (schur.js:31-87): complex128 [..., N]. The per-matrix flags are read back (one small
    copy): a real-eigenvalued 2x2 block raises the reference's error."""
    lead, N = _ev_sq(T, "T is not square.")
    L = torch.empty(lead + (N,), dtype=torch.complex128, device=T.device)
    h = _h(T)
    _ev_call(h.lib.nd4hip_dtreval_batched_dev, h.ptr, _batch(lead), N, _p(T), _p(L))
    return L


def schur_eigen(Q, T):
    """device-resident schur_eigen (schur.js:90-370): [eigenvalues [..., N], Q V [..., N, N]], both complex128. Synchronises: the
    per-matrix flags are read back (the reference's errors), and for N > 64 the block structure is."""
    _chk(Q, "Q"), _chk(T, "T")
    if Q.device != T.device:
        raise ValueError("Q and T must be on the same device")
    if Q.dim() != T.dim():
        raise ValueError("Q.ndim != T.ndim.")
    if tuple(Q.shape) != tuple(T.shape):
        raise ValueError("Q.shape != T.shape.")
    lead, N = _ev_sq(T, "Q is not square.")
    L = torch.empty(lead + (N,), dtype=torch.complex128, device=T.device)
    V = torch.empty(lead + (N, N), dtype=torch.complex128, device=T.device)
    h = _h(T)
    _ev_call(h.lib.nd4hip_dtrevc_batched_dev, h.ptr, _batch(lead), N, _p(Q), _p(T), _p(L), _p(V))
    return [L, V]


def eigen_balance_pre(A, p=2):
    """device-resident eigen_balance_pre (eigen.js:91-226): [D [..., N], B [..., N, N]]. Synchronises: the per-matrix flags are read
    back ('NaN encountered.')."""
    from .la import _js_num
    p = 2.0 if p is None else float(p)
    if not p >= 1:
        raise ValueError("Invalid norm p=%s;" % _js_num(p))
    lead, N = _ev_sq(A, "A is not square")
    D = torch.empty(lead + (N,), dtype=torch.float64, device=A.device)
    B = torch.empty(lead + (N, N), dtype=torch.float64, device=A.device)
    h = _h(A)
    _ev_call(h.lib.nd4hip_dgebal_batched_dev, h.ptr, _batch(lead), N, p, _p(A), _p(D), _p(B))
    return [D, B]


def eigen_balance_post(D, V):
    """device-resident eigen_balance_post (eigen.js:229-270): D [..., N] float64, V [..., N, N] complex128 with equal leading
    dims -> diag(D) V with unit columns."""
    _chk(D, "D")
    V = _chk_mm(V, "V")
    if V.dim() < 2:
        raise ValueError("eigen_balance_post(D,V): V.ndim must be at least 2.")
    if V.shape[-2] != V.shape[-1]:
        raise ValueError("eigen_balance_post(D,V): V must be square.")
    if V.dtype != torch.complex128:
        V = V.to(torch.complex128)
    if tuple(D.shape) != tuple(V.shape[:-1]):
        raise ValueError("eigen_balance_post(D,V): D.shape must be V.shape[:-1].")
    N = int(V.shape[-1])
    W = torch.empty_like(V)
    h = _h(V)
    _ev_call(h.lib.nd4hip_zgebak_batched_dev, h.ptr, _batch(V.shape[:-2]), N, _p(D), _p(V), _p(W))
    return W


def schur_qrfrancis(U, H, tier=None, sweeps=False):
    """device-resident Francis iteration of schur_decomp (schur.js:388-683): [Q, T] from a Hessenberg decomposition (U, H), the
    reference's bits; `tier` as in la.schur_qrfrancis. Synchronises: the per-matrix flags and sweep counts are read back."""
    from .la import _schur_tier
    _chk(U, "U"), _chk(H, "H")
    if U.device != H.device:
        raise ValueError("U and H must be on the same device")
    if U.dim() < 2 or U.shape[-2] != U.shape[-1]:
        raise ValueError("Q is not square.")
    if U.dim() != H.dim():
        raise ValueError("Q.ndim != H.ndim.")
    if tuple(U.shape) != tuple(H.shape):
        raise ValueError("Q.shape != H.shape.")
    t = _schur_tier(tier)
    N = int(U.shape[-1])
    Q, T = torch.empty_like(U), torch.empty_like(H)
    sw = ctypes.c_int(0)
    h = _h(U)
    _ev_call(h.lib.nd4hip_dhseqr_batched_ex_dev, h.ptr, _batch(U.shape[:-2]), N, _p(U), _p(H), _p(Q), _p(T), ctypes.byref(sw), t)
    return [Q, T, sw.value] if sweeps else [Q, T]


def schur_decomp(A, sweeps=False):
    """device-resident schur_decomp (schur.js:372-381): [Q, T]. Synchronises (flags and sweep counts)."""
    _chk(A, "A")
    if A.dim() < 2:
        raise ValueError("hessenberg_decomp(A): A must at least be 2D.")
    N = int(A.shape[-1])
    if A.shape[-2] != N:
        raise ValueError("hessenberg_decomp(A): A must be square.")
    Q, T = torch.empty_like(A), torch.empty_like(A)
    sw = ctypes.c_int(0)
    h = _h(A)
    _ev_call(h.lib.nd4hip_dgees_batched_dev, h.ptr, _batch(A.shape[:-2]), N, _p(A), _p(Q), _p(T), ctypes.byref(sw))
    return [Q, T, sw.value] if sweeps else [Q, T]


def eigen(A):
    """device-resident eigen (eigen.js:33-80): [eigenvalues [..., N], unit eigenvectors [..., N, N]], both complex128."""
    lead, N = _ev_sq(A, "A is not square")
    L = torch.empty(lead + (N,), dtype=torch.complex128, device=A.device)
    V = torch.empty(lead + (N, N), dtype=torch.complex128, device=A.device)
    h = _h(A)
    _ev_call(h.lib.nd4hip_dgeev_batched_dev, h.ptr, _batch(lead), N, _p(A), _p(L), _p(V))
    return [L, V]


def eigenvals(A):
    """device-resident eigenvals (eigen.js:83-88): complex128 [..., N]."""
    lead, N = _ev_sq(A, "A is not square")
    L = torch.empty(lead + (N,), dtype=torch.complex128, device=A.device)
    h = _h(A)
    _ev_call(h.lib.nd4hip_dgeev_batched_dev, h.ptr, _batch(lead), N, _p(A), _p(L), None)
    return L


def _interval(interval, lead, what, device):
    """la._interval on the device: bounds float64 [..., 2] = (lo, hi); lo and hi are numbers, arrays or tensors that broadcast to the
    leading dimensions. The NaN and lo <= hi checks read one flag back before the call: an interval call through dev synchronises
    twice, here and at the read-back of the ranges inside the library (the C _dev form alone would see lo > hi only after the count,
    and a NaN bound not at all: it selects nothing)."""
    try:
        lo, hi = interval
        lo, hi = (torch.as_tensor(x, dtype=torch.float64, device=device) for x in (lo, hi))
    except (TypeError, ValueError, RuntimeError):
        raise ValueError("%s: interval must be (lo, hi), got %r." % (what, interval)) from None
    try:
        bounds = torch.stack((lo.broadcast_to(lead), hi.broadcast_to(lead)), dim=-1).contiguous()
    except RuntimeError:
        raise ValueError("%s: interval must broadcast to the leading dimensions %r." % (what, tuple(lead))) from None
    bad = torch.stack((torch.isnan(bounds).any(), (bounds[..., 0] > bounds[..., 1]).any())).tolist() if bounds.numel() else (False, False)
    if bad[0]:
        raise ValueError("%s: interval contains NaN." % what)
    if bad[1]:
        raise ValueError("%s: interval must satisfy lo <= hi." % what)
    return bounds


def _interval_call(name, N, bounds, operands, vshape, info):
    """la._interval_call on the device: (L [..., N], vectors of shape vshape or None, kmax) of the entry point `name` with kcap = N;
    info['range'] = int32 [..., 2] on the device"""
    lead, dv = tuple(bounds.shape[:-1]), bounds.device
    L = torch.empty(lead + (N,), dtype=torch.float64, device=dv)
    Zs = torch.empty(vshape, dtype=torch.float64, device=dv) if vshape is not None else None
    ranges = torch.zeros(lead + (2,), dtype=torch.int32, device=dv)
    kmax = ctypes.c_int64(0)
    if L.numel():
        h = _h(bounds)
        _lib.check(getattr(h.lib, name)(h.ptr, _batch(lead), N, N, _p(bounds), *[_p(a) for a in operands], _p(L),
                                        _p(Zs) if Zs is not None else None, _p(ranges), ctypes.byref(kmax)))
    if info is not None:
        info["range"] = ranges
    return L, Zs, kmax.value


def _syevd(S, what, vectors, algo=None, info=None, subset=None, reduction=None, interval=None):
    from .la import _eigsym_algo, _interval_what, _reduction, _subset
    jacobi = _eigsym_algo(algo, what)
    tr = _reduction(reduction, what, jacobi)
    if interval is not None:
        what = _interval_what(what, jacobi, subset)
    elif subset is not None:
        what = what.replace("(S)", "(S, subset)")
        if jacobi:
            _subset(subset, 0, what, True)
    if isinstance(S, torch.Tensor) and S.dtype != torch.float64:
        raise TypeError("%s: S.dtype must be float." % what)
    _chk(S, "S")
    if S.dim() < 2:
        raise ValueError("%s: S.ndim must be at least 2." % what)
    N = S.shape[-1]
    if S.shape[-2] != N:
        raise ValueError("%s: S must be quadratic." % what)
    lead = tuple(S.shape[:-2])
    if interval is not None:                                                # the same, the subset of each member chosen by value
        bounds = _interval(interval, lead, what, S.device)
        L, V, k = _interval_call("nd4hip_dsyevxv_tr_batched_dev" if tr else "nd4hip_dsyevxv_batched_dev", N, bounds, (S,),
                                 tuple(S.shape) if vectors else None, info)
        L = L[..., :k].contiguous()
        return (L, V[..., :k].contiguous()) if vectors else L
    if subset is not None:                                                  # bisection and inverse iteration (csrc/syevx.hip)
        i0, i1 = _subset(subset, N, what)
        L = torch.empty(lead + (i1 - i0,), dtype=torch.float64, device=S.device)
        V = torch.empty(lead + (N, i1 - i0), dtype=torch.float64, device=S.device) if vectors else None
        if L.numel():
            h = _h(S)
            fn = h.lib.nd4hip_dsyevx_tr_batched_dev if tr else h.lib.nd4hip_dsyevx_batched_dev
            _lib.check(fn(h.ptr, _batch(lead), N, i0, i1, _p(S), _p(L), _p(V) if vectors else None))
        return (L, V) if vectors else L
    L = torch.empty(lead + (N,), dtype=torch.float64, device=S.device)
    V = torch.empty(lead + (N, N), dtype=torch.float64, device=S.device) if vectors else None
    h = _h(S)
    if tr:                                                                  # the symmetric reduction (csrc/sytrd.hip)
        _lib.check(h.lib.nd4hip_dsyevd_tr_batched_dev(h.ptr, _batch(lead), N, _p(S), _p(L), _p(V) if vectors else None))
    elif jacobi:
        sweeps = torch.zeros(lead, dtype=torch.int32, device=S.device)
        _lib.check(h.lib.nd4hip_dsyevj_batched_dev(h.ptr, _batch(lead), N, _p(S), _p(L), _p(V) if vectors else None, _p(sweeps)))
        if info is not None:
            info["sweeps"] = sweeps
    else:
        _lib.check(h.lib.nd4hip_dsyevd_batched_dev(h.ptr, _batch(lead), N, _p(S), _p(L), _p(V) if vectors else None))
    return (L, V) if vectors else L


def eigen_sym(S, algo=None, info=None, subset=None, reduction=None, interval=None):
    """device-resident la.eigen_sym: (eigenvalues [..., N] descending, eigenvectors [..., N, N] as columns), float64; only the
    lower triangle of S is read and S is not written. algo='jacobi' (N <= 128): the one-launch Jacobi route; `info` then
    receives 'sweeps', an int32 tensor [...] on the device. subset=(i0, i1): L[i0:i1] and the matching columns alone, [..., k] and
    [..., N, k], by bisection and inverse iteration. reduction='tridiag': the reduction of tridiag_factor and the vectors by
    tridiag_apply_q in place of the Hessenberg reduction and its U. interval=(lo, hi): the eigenvalues lo < lambda <= hi of every
    member, ragged: (L [..., kmax], V [..., N, kmax]), NaN and zero columns after a member's own k_b pairs; `info` receives 'range', an
    int32 tensor [..., 2] on the device. The ranges are read back once inside the call, after one flag for the NaN and lo <= hi checks
    of the bounds (two synchronisations in all)."""
    return _syevd(S, "eigen_sym(S)", True, algo, info, subset, reduction, interval)


def eigenvals_sym(S, algo=None, info=None, subset=None, reduction=None, interval=None):
    """device-resident la.eigenvals_sym: the eigenvalues of eigen_sym alone, the same bits"""
    return _syevd(S, "eigenvals_sym(S)", False, algo, info, subset, reduction, interval)


def tridiag_factor(S):
    """device-resident la.tridiag_factor: (F [..., N, N], tau [..., N-1], d [..., N], e [..., N-1]), the same bits"""
    from .la import _tridiag_s
    what = "tridiag_factor(S)"
    if isinstance(S, torch.Tensor) and S.dtype != torch.float64:
        raise TypeError("%s: S.dtype must be float." % what)
    _chk(S, "S")
    N = _tridiag_s(S.dim(), tuple(S.shape), what)
    lead, ne = tuple(S.shape[:-2]), max(N - 1, 0)
    F, tau, d, e = (torch.empty(lead + tail, dtype=torch.float64, device=S.device) for tail in ((N, N), (ne,), (N,), (ne,)))
    if F.numel():
        h = _h(S)
        _lib.check(h.lib.nd4hip_dsytrd_batched_dev(h.ptr, _batch(lead), N, _p(S), _p(F), _p(tau), _p(d), _p(e)))
    return F, tau, d, e


def tridiag_apply_q(F, tau, Z, transpose=False):
    """device-resident la.tridiag_apply_q: Q Z (transpose: Q^T Z) as a new tensor, the same bits; only enqueued"""
    from .la import _tridiag_fz
    what = "tridiag_apply_q(F,tau,Z)"
    for a in (F, tau, Z):
        if isinstance(a, torch.Tensor) and a.dtype != torch.float64:
            raise TypeError("%s: F, tau and Z must be float." % what)
    _chk(F, "F"), _chk(tau, "tau")
    N, K = _tridiag_fz(tuple(F.shape), tuple(tau.shape), tuple(Z.shape), what)
    out = _chk(Z.clone(memory_format=torch.contiguous_format), "Z")       # the product is made in place
    if out.numel():
        h = _h(F)
        _lib.check(h.lib.nd4hip_dormtr_batched_dev(h.ptr, _batch(F.shape[:-2]), N, K, 1 if transpose else 0, _p(F), _p(tau), _p(out)))
    return out


def tridiag_decomp(S):
    """device-resident la.tridiag_decomp: (Q [..., N, N], d, e), Q = tridiag_apply_q(F, tau, I)"""
    F, tau, d, e = tridiag_factor(S)
    N = F.shape[-1]
    eye = torch.eye(N, dtype=torch.float64, device=F.device).expand(F.shape)
    return tridiag_apply_q(F, tau, eye), d, e


def _chk_herm(t, name, what):
    """a contiguous complex128 CUDA tensor without a lazy conjugate or negative bit (the kernels read the stored numbers); a
    float64 tensor is sent to eigen_sym"""
    if isinstance(t, torch.Tensor) and not t.is_complex():
        raise TypeError("%s: %s.dtype must be complex128; a real symmetric matrix goes to eigen_sym / tridiag_factor." % (what, name))
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.complex128 and t.is_contiguous()):
        raise TypeError("%s: %s must be a contiguous complex128 CUDA tensor" % (what, name))
    return t.resolve_conj().resolve_neg()


def herm_tridiag_factor(H):
    """device-resident la.herm_tridiag_factor: (F complex128 [..., N, N], tau complex128 [..., N-1], d float64 [..., N], e float64
    [..., N-1]), the same bits"""
    from .la import _herm_shape
    what = "herm_tridiag_factor(H)"
    H = _chk_herm(H, "H", what)
    N = _herm_shape(H.dim(), tuple(H.shape), what)
    lead, ne = tuple(H.shape[:-2]), max(N - 1, 0)
    F, tau = (torch.empty(lead + tail, dtype=torch.complex128, device=H.device) for tail in ((N, N), (ne,)))
    d, e = (torch.empty(lead + tail, dtype=torch.float64, device=H.device) for tail in ((N,), (ne,)))
    if F.numel():
        h = _h(H)
        _lib.check(h.lib.nd4hip_zhetrd_batched_dev(h.ptr, _batch(lead), N, _p(H), _p(F), _p(tau), _p(d), _p(e)))
    return F, tau, d, e


def herm_tridiag_apply_q(F, tau, Z, adjoint=False):
    """device-resident la.herm_tridiag_apply_q: Q Z (adjoint: Q^H Z) as a new complex128 tensor, the same bits; a float64 Z is promoted;
    only enqueued"""
    from .la import _tridiag_fz
    what = "herm_tridiag_apply_q(F,tau,Z)"
    for a in (F, tau):
        if not (isinstance(a, torch.Tensor) and a.is_cuda and a.dtype == torch.complex128 and a.is_contiguous()):
            raise TypeError("%s: F and tau must be contiguous complex128 CUDA tensors." % what)
    if not (isinstance(Z, torch.Tensor) and Z.is_cuda and Z.dtype in (torch.float64, torch.complex128)):
        raise TypeError("%s: Z must be a complex128 or float64 CUDA tensor." % what)
    F, tau = F.resolve_conj().resolve_neg(), tau.resolve_conj().resolve_neg()
    N, K = _tridiag_fz(tuple(F.shape), tuple(tau.shape), tuple(Z.shape), what)
    out = Z.to(torch.complex128).resolve_conj().resolve_neg().clone(memory_format=torch.contiguous_format)   # the product is made in place
    if out.numel():
        h = _h(F)
        _lib.check(h.lib.nd4hip_zunmtr_batched_dev(h.ptr, _batch(F.shape[:-2]), N, K, 1 if adjoint else 0, _p(F), _p(tau), _p(out)))
    return out


def herm_tridiag_decomp(H):
    """device-resident la.herm_tridiag_decomp: (Q complex128 [..., N, N], d, e), Q = herm_tridiag_apply_q(F, tau, I)"""
    F, tau, d, e = herm_tridiag_factor(H)
    N = F.shape[-1]
    eye = torch.eye(N, dtype=torch.float64, device=F.device).expand(F.shape)
    return herm_tridiag_apply_q(F, tau, eye), d, e


def _heev(H, what, vectors, subset):
    from .la import _subset
    if subset is not None:
        what = what.replace("(H)", "(H, subset)")
    H = _chk_herm(H, "H", what)
    if H.dim() < 2:
        raise ValueError("%s: H.ndim must be at least 2." % what)
    N = H.shape[-1]
    if H.shape[-2] != N:
        raise ValueError("%s: H must be quadratic." % what)
    lead = tuple(H.shape[:-2])
    if subset is not None:                                                  # bisection and inverse iteration on (d, e)
        i0, i1 = _subset(subset, N, what)
        L = torch.empty(lead + (i1 - i0,), dtype=torch.float64, device=H.device)
        V = torch.empty(lead + (N, i1 - i0), dtype=torch.complex128, device=H.device) if vectors else None
        if L.numel():
            h = _h(H)
            _lib.check(h.lib.nd4hip_zheevx_batched_dev(h.ptr, _batch(lead), N, i0, i1, _p(H), _p(L), _p(V) if vectors else None))
        return (L, V) if vectors else L
    L = torch.empty(lead + (N,), dtype=torch.float64, device=H.device)
    V = torch.empty(lead + (N, N), dtype=torch.complex128, device=H.device) if vectors else None
    h = _h(H)
    _lib.check(h.lib.nd4hip_zheevd_batched_dev(h.ptr, _batch(lead), N, _p(H), _p(L), _p(V) if vectors else None))
    return (L, V) if vectors else L


def eigen_herm(H, subset=None):
    """device-resident la.eigen_herm: (eigenvalues float64 [..., N] descending, eigenvectors complex128 [..., N, N] as columns) of the
    Hermitian complex128 H, read only where i >= j and not written; subset=(i0, i1) as eigen_sym's. The same bits."""
    return _heev(H, "eigen_herm(H)", True, subset)


def eigenvals_herm(H, subset=None):
    """device-resident la.eigenvals_herm: the eigenvalues of eigen_herm alone, the same bits"""
    return _heev(H, "eigenvals_herm(H)", False, subset)


def _chk_c128(t, name, what, real_goes_to):
    """a contiguous complex128 CUDA tensor with its stored numbers (no lazy conjugate or negative bit); la's dtype errors"""
    from .la import _hegv_dtype
    if isinstance(t, torch.Tensor):
        _hegv_dtype(name, what, t.is_complex(), t.dtype == torch.complex128, t.dtype, real_goes_to)
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.is_contiguous()):
        raise TypeError("%s: %s must be a contiguous complex128 CUDA tensor" % (what, name))
    return t.resolve_conj().resolve_neg()


def herm_cholesky_decomp(H):
    """device-resident la.herm_cholesky_decomp: L complex128 [..., N, N] with H = L L^H, the same bits"""
    from .la import _hegv_square
    what = "herm_cholesky_decomp(H)"
    H = _chk_c128(H, "H", what, "cholesky_decomp")
    N = _hegv_square(tuple(H.shape), "H", what)
    L = torch.empty_like(H)
    if L.numel():
        h = _h(H)
        _lib.check(h.lib.nd4hip_zpotrf_batched_dev(h.ptr, _batch(H.shape[:-2]), N, _p(H), _p(L)))
    return L


def _ztrs(L, Y, what, entry, *flag, twice=False):
    from .la import _hegv_ly
    L = _chk_c128(L, "L", what, "cholesky_solve / tril_solve")
    if not (isinstance(Y, torch.Tensor) and Y.is_cuda and Y.dtype in (torch.float64, torch.complex128)):
        raise TypeError("%s: Y must be a complex128 or float64 CUDA tensor." % what)
    N, K, one_l = _hegv_ly(tuple(L.shape), tuple(Y.shape), what)
    if L.device != Y.device:
        raise ValueError("%s: both operands must be on the same device." % what)
    X = Y.to(torch.complex128).resolve_conj().resolve_neg().clone(memory_format=torch.contiguous_format)   # the solve is made in place
    if X.numel():
        h = _h(L)
        _lib.check(getattr(h.lib, entry)(h.ptr, _batch(Y.shape[:-2]), N, K, *flag, _p(L), 0 if one_l else N * N, *([_p(X)] * (2 if twice else 1))))
    return X


def herm_cholesky_solve(L, Y):
    """device-resident la.herm_cholesky_solve: X with L L^H X = Y, the same bits; only enqueued"""
    return _ztrs(L, Y, "herm_cholesky_solve(L,Y)", "nd4hip_zpotrs_batched_dev", twice=True)   # (Y, X) = (X, X): in place


def ztril_solve(L, Y, adjoint=False):
    """device-resident la.ztril_solve: X with L X = Y (adjoint: L^H X = Y), the same bits; only enqueued"""
    return _ztrs(L, Y, "ztril_solve(L,Y)", "nd4hip_ztrsm_batched_dev", 1 if adjoint else 0)


def _hegv_ab(A, B, nb, what):
    from .la import _hegv_pair, _hegv_square
    A, B = _chk_c128(A, "A", what, "eigen_sym_gen"), _chk_c128(B, nb, what, "eigen_sym_gen")
    N = _hegv_square(tuple(A.shape), "A", what)
    _hegv_square(tuple(B.shape), nb, what)
    one = _hegv_pair(A.shape, B.shape, nb, what)
    if B.device != A.device:
        raise ValueError("%s: both operands must be on the same device." % what)
    return A, B, N, one


def herm_gen_reduce(A, L):
    """device-resident la.herm_gen_reduce: C = L^-1 A L^-H, lower triangle, zeros above, a real diagonal; the same bits; only enqueued"""
    A, L, N, one_l = _hegv_ab(A, L, "L", "herm_gen_reduce(A,L)")
    C = torch.empty_like(A)
    if C.numel():
        h = _h(A)
        _lib.check(h.lib.nd4hip_zhegst_batched_dev(h.ptr, _batch(A.shape[:-2]), N, _p(A), _p(L), 0 if one_l else N * N, _p(C)))
    return C


def _hegv(A, B, what, vectors, subset):
    from .la import _subset
    if subset is not None:
        what = what.replace("(A,B)", "(A,B, subset)")
    A, B, N, one_b = _hegv_ab(A, B, "B", what)
    lead = tuple(A.shape[:-2])
    i0, i1 = _subset(subset, N, what) if subset is not None else (0, N)
    lam = torch.empty(lead + (i1 - i0,), dtype=torch.float64, device=A.device)
    X = torch.empty(lead + (N, i1 - i0), dtype=torch.complex128, device=A.device) if vectors else None
    if lam.numel():
        h = _h(A)
        if subset is not None:
            _lib.check(h.lib.nd4hip_zhegvx_batched_dev(h.ptr, _batch(lead), N, i0, i1, _p(A), _p(B), 0 if one_b else N * N, _p(lam),
                                                       _p(X) if vectors else None))
        else:
            _lib.check(h.lib.nd4hip_zhegvd_batched_dev(h.ptr, _batch(lead), N, _p(A), _p(B), 0 if one_b else N * N, _p(lam),
                                                       _p(X) if vectors else None))
    return (lam, X) if vectors else lam


def eigen_herm_gen(A, B, subset=None):
    """device-resident la.eigen_herm_gen: A x = lambda B x with A Hermitian and B Hermitian positive definite, complex128: (eigenvalues
    float64 [..., N] descending, eigenvectors complex128 [..., N, N] as columns, X^H B X = I). B has A's shape or is exactly [N, N] (one B
    for every member, factorised once). Only i >= j is read; A and B are not written. The same bits as through la."""
    return _hegv(A, B, "eigen_herm_gen(A,B)", True, subset)


def eigenvals_herm_gen(A, B, subset=None):
    """device-resident la.eigenvals_herm_gen: the eigenvalues of eigen_herm_gen alone, the same bits"""
    return _hegv(A, B, "eigenvals_herm_gen(A,B)", False, subset)


def _stevx(d, e, subset, what, vectors, interval=None, info=None):
    from .la import _interval_what, _subset, _tridiag_args
    if interval is not None:
        what = _interval_what(what, False, subset)
    _chk(d, "d"), _chk(e, "e")
    N = _tridiag_args(d, e, what, lambda a: a.dim(), lambda a: a.shape)
    if interval is not None:                                                # the subset of each member chosen by value
        lead = tuple(d.shape[:-1])
        bounds = _interval(interval, lead, what, d.device)
        L, Z, k = _interval_call("nd4hip_dstevxv_batched_dev", N, bounds, (d, e), lead + (N, N) if vectors else None, info)
        L = L[..., :k].contiguous()
        return (L, Z[..., :k, :].transpose(-1, -2).contiguous()) if vectors else L
    i0, i1 = _subset((0, N) if subset is None else subset, N, what)
    lead = tuple(d.shape[:-1])
    L = torch.empty(lead + (i1 - i0,), dtype=torch.float64, device=d.device)
    Z = torch.empty(lead + (i1 - i0, N), dtype=torch.float64, device=d.device) if vectors else None
    if L.numel():
        h = _h(d)
        _lib.check(h.lib.nd4hip_dstevx_batched_dev(h.ptr, _batch(lead), N, i0, i1, _p(d), _p(e), _p(L), _p(Z) if vectors else None))
    return (L, Z.transpose(-1, -2).contiguous()) if vectors else L


def tridiag_eigen(d, e, subset=None, interval=None, info=None):
    """device-resident la.tridiag_eigen: (L [..., k] descending, Z [..., N, k] with the eigenvectors as columns), the same bits;
    interval=(lo, hi) and `info` as in eigen_sym"""
    return _stevx(d, e, subset, "tridiag_eigen(d,e)", True, interval, info)


def tridiag_eigenvals(d, e, subset=None, interval=None, info=None):
    """device-resident la.tridiag_eigenvals: the eigenvalues of tridiag_eigen alone, the same bits"""
    return _stevx(d, e, subset, "tridiag_eigenvals(d,e)", False, interval, info)


def tridiag_count(d, e, x):
    """device-resident la.tridiag_count: int32 [..., M], how many eigenvalues of tridiag(d, e) are greater than each x [..., M].
    The NaN check of x reads one flag back; the count itself is only enqueued."""
    from .la import _tridiag_args
    what = "tridiag_count(d,e,x)"
    _chk(d, "d"), _chk(e, "e"), _chk(x, "x")
    N = _tridiag_args(d, e, what, lambda a: a.dim(), lambda a: a.shape)
    if x.dim() < 1 or tuple(x.shape[:-1]) != tuple(d.shape[:-1]):
        raise ValueError("%s: x must have the leading dimensions of d." % what)
    if bool(torch.isnan(x).any()):
        raise ValueError("%s: x contains NaN." % what)
    count = torch.empty(tuple(x.shape), dtype=torch.int32, device=x.device)
    if count.numel():
        h = _h(d)
        _lib.check(h.lib.nd4hip_dstcnt_batched_dev(h.ptr, _batch(d.shape[:-1]), N, int(x.shape[-1]), _p(d), _p(e), _p(x), _p(count)))
    return count


def _sygv_chk(A, B, what):
    from .la import _sygv_args
    named = ((what[what.index("(") + 1], A), (what[what.index(",") + 1], B))
    for name, M in named:
        if isinstance(M, torch.Tensor) and M.dtype != torch.float64:
            raise TypeError("%s: %s.dtype must be float." % (what, name))
    for name, M in named:
        _chk(M, name)
    one = _sygv_args(A, B, what, lambda M: True, lambda M: M.dim(), lambda M: M.shape)
    if B.device != A.device:
        raise ValueError("%s: both operands must be on the same device." % what)
    return one


def _sygvx(A, B, what, vectors, one_b, tr, subset, interval, info):
    """la._sygvx on the device: nd4hip_dsygvx_batched_dev"""
    from .la import _subset
    N, lead = A.shape[-1], tuple(A.shape[:-2])
    select, i0, i1, bounds, ranges, kmax = 0, 0, 0, None, None, ctypes.c_int64(0)
    if interval is not None:
        select, bounds = 2, _interval(interval, lead, what, A.device)
        ranges = torch.zeros(lead + (2,), dtype=torch.int32, device=A.device)
    elif subset is not None:
        select = 1
        i0, i1 = _subset(subset, N, what)
    K = i1 - i0 if select == 1 else N
    L = torch.empty(lead + (K,), dtype=torch.float64, device=A.device)
    X = torch.empty(lead + (N, K), dtype=torch.float64, device=A.device) if vectors else None
    if L.numel():
        h = _h(A)
        _lib.check(h.lib.nd4hip_dsygvx_batched_dev(h.ptr, 1 if tr else 0, select, _batch(lead), N, i0, i1, N if select == 2 else 0,
                                                   _p(bounds) if select == 2 else None, _p(A), _p(B), 0 if one_b else N * N, _p(L),
                                                   _p(X) if vectors else None, _p(ranges) if select == 2 else None,
                                                   ctypes.byref(kmax) if select == 2 else None))
    if select == 2:
        if info is not None:
            info["range"] = ranges
        L = L[..., :kmax.value].contiguous()
        X = X[..., :kmax.value].contiguous() if vectors else None
    return (L, X) if vectors else L


def _sygvd(A, B, what, vectors, algo, info, subset=None, interval=None, reduction=None):
    from .la import _eigsym_algo, _sygv_select
    jacobi = _eigsym_algo(algo, what)
    what, tr = _sygv_select(what, jacobi, subset, interval, reduction)
    one_b = _sygv_chk(A, B, what)
    if tr or subset is not None or interval is not None:
        return _sygvx(A, B, what, vectors, one_b, tr, subset, interval, info)
    N = A.shape[-1]
    lead = tuple(A.shape[:-2])
    L = torch.empty(lead + (N,), dtype=torch.float64, device=A.device)
    X = torch.empty(lead + (N, N), dtype=torch.float64, device=A.device) if vectors else None
    sweeps = torch.zeros(lead, dtype=torch.int32, device=A.device) if jacobi else None
    h = _h(A)
    _lib.check(h.lib.nd4hip_dsygvd_batched_dev(h.ptr, 1 if jacobi else 0, _batch(lead), N, _p(A), _p(B), 0 if one_b else N * N, _p(L),
                                               _p(X) if vectors else None, _p(sweeps) if jacobi else None))
    if jacobi and info is not None:
        info["sweeps"] = sweeps
    return (L, X) if vectors else L


def eigen_sym_gen(A, B, algo=None, info=None, subset=None, interval=None, reduction=None):
    """device-resident la.eigen_sym_gen: A x = lambda B x with A symmetric and B symmetric positive definite, (eigenvalues [..., N]
    descending, eigenvectors [..., N, N] as columns, X^T B X = I), float64. B has A's shape or is exactly [N, N] (one B for every
    member, factorised once). Only the lower triangles are read; A and B are not written. The same bits as through la. subset,
    interval and reduction as in la.eigen_sym_gen; info['range'] is an int32 tensor on the device."""
    return _sygvd(A, B, "eigen_sym_gen(A,B)", True, algo, info, subset, interval, reduction)


def eigenvals_sym_gen(A, B, algo=None, info=None, subset=None, interval=None, reduction=None):
    """device-resident la.eigenvals_sym_gen: the eigenvalues of eigen_sym_gen alone, the same bits"""
    return _sygvd(A, B, "eigenvals_sym_gen(A,B)", False, algo, info, subset, interval, reduction)


def _sygst(A, L):
    """device-resident la._sygst: C = L^-1 A L^-T, lower triangle, zeros above"""
    one_l = _sygv_chk(A, L, "_sygst(A,L)")
    N = A.shape[-1]
    C = torch.empty_like(A)
    h = _h(A)
    _lib.check(h.lib.nd4hip_dsygst_batched_dev(h.ptr, _batch(A.shape[:-2]), N, _p(A), _p(L), 0 if one_l else N * N, _p(C)))
    return C


# ---- structure functions (csrc/struct.hip): values are moved, never computed; nothing leaves the device ----
def _struct_call(fn, *args):
    from .la import _arg_error
    try:
        _lib.check(fn(*args))
    except _lib.Nd4HipError as e:
        raise _arg_error(e)


def transpose(A, *axes, pairs=False):
    """no axes: the last two axes swapped (NDArray.T); fewer than two axes: A itself. With axes: NDArray.transpose(...axes), any
    permutation of the axes (csrc/gather.hip), also of int32 tensors and, with pairs=True, of complex128 stored as float64 [..., 2]."""
    if axes or pairs:
        return _transpose_axes(A, axes, pairs)
    _chk(A, "A")
    if A.dim() < 2:
        return A
    M, N = A.shape[-2:]
    B = torch.empty(tuple(A.shape[:-2]) + (N, M), dtype=torch.float64, device=A.device)
    h = _h(A)
    _struct_call(h.lib.nd4hip_dtranspose_batched_dev, h.ptr, _batch(A.shape[:-2]), M, N, _p(A), _p(B))
    return B


def _tri(upper, A, k):
    from .la import _tri_k
    _chk(A, "A")
    if A.dim() < 2:
        raise ValueError("Input must be at least 2D.")
    M, N = A.shape[-2:]
    B = torch.empty_like(A)
    h = _h(A)
    _struct_call(h.lib.nd4hip_dtri_batched_dev, h.ptr, upper, _tri_k(k), _batch(A.shape[:-2]), M, N, _p(A), _p(B))
    return B


def tril(A, k=0):
    return _tri(0, A, k)


def triu(A, k=0):
    return _tri(1, A, k)


def diag(A, offset=0):
    from .la import _diag_args
    _chk(A, "A")
    M, N, L = _diag_args(tuple(A.shape), offset)
    d = torch.empty(tuple(A.shape[:-2]) + (L,), dtype=torch.float64, device=A.device)
    h = _h(A)
    _struct_call(h.lib.nd4hip_ddiag_batched_dev, h.ptr, _batch(A.shape[:-2]), M, N, int(offset), _p(A), _p(d))
    return d


def diag_mat(d):
    from .la import _diag_mat_args
    _chk(d, "d")
    N = _diag_mat_args(tuple(d.shape))
    D = torch.empty(tuple(d.shape) + (N,), dtype=torch.float64, device=d.device)
    h = _h(d)
    _struct_call(h.lib.nd4hip_ddiagmat_batched_dev, h.ptr, _batch(d.shape[:-1]), N, _p(d), _p(D))
    return D


def _permute(cols, inverse, A, P):
    """la._permute on device tensors: the same shape rule (leading axes of A and P broadcast against each other), one call per
    stride-0 / dense run. A bad index raises ValueError with the reference's text (the call reads one flag word back)."""
    from .la import _permute_plan
    name = ("unpermute_" if inverse else "permute_") + ("cols" if cols else "rows")
    _chk(A, "A")
    if not (isinstance(P, torch.Tensor) and P.is_cuda and P.is_contiguous()):
        raise TypeError("P must be a contiguous CUDA tensor")
    M, N, L, lead, groups = _permute_plan(name, tuple(A.shape), tuple(P.shape), P.dtype == torch.int32, cols)
    B = torch.empty(lead + (M, N), dtype=torch.float64, device=A.device)
    h = _h(A)
    for cnt, (oA, oP), (sA, sP), b0 in groups:
        _struct_call(h.lib.nd4hip_dpermute_batched_dev, h.ptr, cols, inverse, cnt, M, N, ctypes.c_void_p(A.data_ptr() + 8 * oA), sA,
                     ctypes.c_void_p(P.data_ptr() + 4 * oP), sP, ctypes.c_void_p(B.data_ptr() + 8 * b0 * M * N))
    return B


def permute_rows(A, P):
    return _permute(0, 0, A, P)


def permute_cols(A, P):
    return _permute(1, 0, A, P)


def unpermute_rows(A, P):
    return _permute(0, 1, A, P)


def unpermute_cols(A, P):
    return _permute(1, 1, A, P)


# ---- slices, axis permutations, concat and stack (csrc/gather.hip): one strided N-d copy, planned by la._*_plan ----
_GATHER_BYTES = {torch.float64: 8, torch.int32: 4}


def _chk_g(t, name, pairs=False):
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype in _GATHER_BYTES and t.is_contiguous()):
        raise TypeError("%s must be a contiguous float64 or int32 CUDA tensor" % name)
    if pairs and not (t.dtype == torch.float64 and t.dim() >= 1 and t.shape[-1] == 2):
        raise TypeError("%s must be float64 [..., 2] (complex128 as pairs)" % name)
    return t


def strided_copy(dst, dst_off, dst_strides, src, src_off, src_strides, shape):
    """dst.flat[dst_off + sum i_d dst_strides[d]] = src.flat[src_off + sum i_d src_strides[d]] for every i of the box `shape`
    (nd4hip_gather_nd_dev as it is: at most 8 axes, offsets and strides in elements, the box inside both tensors, the two sides
    disjoint; otherwise ValueError and nothing is written). Enqueues on the current stream."""
    _chk_g(src, "src")
    _chk_g(dst, "dst")
    if src.dtype != dst.dtype or src.device != dst.device:
        raise TypeError("src and dst must have one dtype and one device")
    nd = len(shape)
    if not (len(src_strides) == nd and len(dst_strides) == nd):
        raise ValueError("shape and strides must have one length")
    arr = ctypes.c_int64 * max(nd, 1)
    h = _h(src)
    _struct_call(h.lib.nd4hip_gather_nd_dev, h.ptr, _GATHER_BYTES[src.dtype], nd, arr(*[int(s) for s in shape]),
                 _p(src), src.numel(), int(src_off), arr(*[int(s) for s in src_strides]),
                 _p(dst), dst.numel(), int(dst_off), arr(*[int(s) for s in dst_strides]))
    return dst


def _gather(dst, dst_off, dst_strides, src, src_off, src_strides, shape, pairs):
    """strided_copy of a planned box: complex pairs become one more innermost axis, the box is reduced (la._reduce_box) and what
    exceeds 8 axes is a loop of launches"""
    from .la import _reduce_box
    shape, ss, ds = list(shape), list(src_strides), list(dst_strides)
    if pairs:
        shape, ss, ds = shape + [2], [2 * s for s in ss] + [1], [2 * s for s in ds] + [1]
        src_off, dst_off = 2 * src_off, 2 * dst_off
    shape, ss, ds, loop = _reduce_box(shape, ss, ds)
    for so, do in loop:
        strided_copy(dst, dst_off + do, ds, src, src_off + so, ss, shape)
    return dst


def _plain(shape, pairs):
    return tuple(shape[:-1]) if pairs else tuple(shape)


def _fresh(like, shape, pairs):
    return torch.empty(tuple(shape) + ((2,) if pairs else ()), dtype=like.dtype, device=like.device)


def slice_elems(A, *slices, pairs=False):
    """NDArray.sliceElems on a device tensor: a fresh tensor. pairs=True: A is complex128 stored as float64 [..., 2] and the
    slices address A.shape[:-1]."""
    from .la import _c_strides, _slice_plan
    _chk_g(A, "A", pairs)
    out_shape, off, strides = _slice_plan(_plain(A.shape, pairs), list(slices))
    B = _fresh(A, out_shape, pairs)
    return _gather(B, 0, _c_strides(out_shape), A, off, strides, out_shape, pairs)


def _transpose_axes(A, axes, pairs):
    from .la import _c_strides, _transpose_plan
    _chk_g(A, "A", pairs)
    out_shape, strides = _transpose_plan(_plain(A.shape, pairs), axes)
    B = _fresh(A, out_shape, pairs)
    return _gather(B, 0, _c_strides(out_shape), A, 0, strides, out_shape, pairs)


def reshape(A, *shape, pairs=False):
    """NDArray.reshape: a view of the same storage (no kernel runs); one entry may be -1"""
    from .la import _reshape_shape
    _chk_g(A, "A", pairs)
    plain = _plain(A.shape, pairs)
    new_shape = _reshape_shape(plain, _batch(plain), shape)
    return A.view(tuple(new_shape) + ((2,) if pairs else ()))


def _concat(fn, plan, axis, tensors, pairs):
    from .la import _c_strides
    tensors = list(tensors)
    for i, t in enumerate(tensors):
        _chk_g(t, "%s: array %d" % (fn, i), pairs)
    if not tensors:
        raise ValueError("%s: no arrays" % fn)
    if any(t.dtype != tensors[0].dtype or t.device != tensors[0].device for t in tensors):
        raise TypeError("%s: the arrays must have one dtype and one device" % fn)
    out_shape, strides, offs, shapes = plan(axis, [_plain(t.shape, pairs) for t in tensors])
    B = _fresh(tensors[0], out_shape, pairs)
    for t, sh, off in zip(tensors, shapes, offs):
        _gather(B, off, strides, t, 0, _c_strides(sh), sh, pairs)
    return B


def concat(axis, tensors, pairs=False):
    """nd.concat on device tensors of one dtype"""
    from .la import _concat_plan
    return _concat("concat", lambda ax, shapes: _concat_plan(ax, shapes) + ([list(s) for s in shapes],), axis, tensors, pairs)


def stack(axis, tensors, pairs=False):
    """nd.stack on device tensors of one dtype"""
    from .la import _stack_plan

    def plan(ax, shapes):
        ax, out_shape, strides, offs = _stack_plan(ax, shapes)
        return out_shape, strides, offs, [list(s[:ax]) + [1] + list(s[ax:]) for s in shapes]
    return _concat("stack", plan, axis, tensors, pairs)


# ---- elementwise arithmetic and ordered reductions (csrc/elem.hip), planned by la._zip_plan / la._reduce_plan ----
def _chk_e(t, name):
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float64 and t.is_contiguous()):
        raise TypeError("%s must be a contiguous float64 CUDA tensor" % name)
    return t


def _ew_op(op, allowed, what):
    from .la import EW_OPS
    if op not in allowed:
        raise ValueError("%s: op must be one of %s" % (what, ", ".join(allowed)))
    return EW_OPS[op]


def _zip(code, tensors):
    from .la import _zip_plan
    if any(t.device != tensors[0].device for t in tensors):
        raise TypeError("zip_elems: the tensors must be on one device")
    shape, _, (bshape, bstrides, loop) = _zip_plan([tuple(t.shape) for t in tensors])
    C = torch.empty(tuple(shape), dtype=torch.float64, device=tensors[0].device)
    nd = len(bshape)
    arr = ctypes.c_int64 * max(nd, 1)
    count = 1
    for n in bshape:
        count *= n
    A, B = tensors[0], tensors[1] if len(tensors) > 1 else None
    h = _h(A)
    for offs in loop:
        _struct_call(h.lib.nd4hip_dzip_nd_dev, h.ptr, code, nd, arr(*bshape), _p(A), A.numel(), offs[0], arr(*bstrides[0]),
                     _p(B) if B is not None else None, B.numel() if B is not None else 0, offs[1] if B is not None else 0,
                     arr(*bstrides[1]) if B is not None else None, ctypes.c_void_p(C.data_ptr() + 8 * offs[-1]), count)
    return C


def zip_elems(tensors, op):
    """nd.zip_elems(tensors, 'float64', nd.math.<op>) on two device tensors, broadcast by the reference's rule: op is 'add', 'sub',
    'mul', 'div', 'min' or 'max' (Math.min / Math.max: NaN wins, -0 < +0). A fresh tensor; every non-NaN result has the
    reference's bits."""
    from .la import EW_OPS, EW_UNARY
    tensors = list(tensors)
    code = _ew_op(op, [k for k in EW_OPS if k not in EW_UNARY], "zip_elems")
    if len(tensors) != 2:
        raise ValueError("zip_elems: %s takes two tensors" % op)
    for i, t in enumerate(tensors):
        _chk_e(t, "zip_elems: tensor %d" % i)
    return _zip(code, tensors)


def map_elems(t, op=None):
    """NDArray.mapElems('float64', nd.math.<op>) on a device tensor: op is 'neg' or 'abs'; None: a copy"""
    from .la import EW_UNARY
    _chk_e(t, "t")
    if op is None:
        C = torch.empty_like(t)
        return strided_copy(C.view(-1), 0, [1], t.view(-1), 0, [1], [t.numel()]).view(t.shape)
    return _zip(_ew_op(op, list(EW_UNARY), "map_elems"), [t])


def reduce_elems(t, axes, op):
    """NDArray.reduceElems(axes, 'float64', nd.math.<op>) on a device tensor: op is 'add', 'mul', 'min' or 'max'; axes is a number,
    a list or a 1-D int32 numpy array. Each output folds its elements in the reference's order (row-major over the reduced axes,
    the first one copied), so sums and products have its bits. A fresh tensor."""
    from .la import EW_REDUCERS, _reduce_plan
    _chk_e(t, "t")
    code = _ew_op(op, list(EW_REDUCERS), "reduce_elems")
    out_shape, bshape, flags, loop = _reduce_plan(tuple(t.shape), axes)
    C = torch.empty(tuple(out_shape), dtype=torch.float64, device=t.device)
    nd = len(bshape)
    a_n = c_n = 1
    for n, f in zip(bshape, flags):
        a_n *= n
        c_n *= 1 if f else n
    h = _h(t)
    for a_off, c_off in loop:
        _struct_call(h.lib.nd4hip_dreduce_nd_dev, h.ptr, code, nd, (ctypes.c_int64 * max(nd, 1))(*bshape), (ctypes.c_int32 * max(nd, 1))(*flags),
                     ctypes.c_void_p(t.data_ptr() + 8 * a_off), a_n, ctypes.c_void_p(C.data_ptr() + 8 * c_off), c_n)
    return C
