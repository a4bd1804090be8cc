"""Shared by the tests of the Hermitian tridiagonal reduction and eigenproblem (test_herm_host.py, test_gpu_herm.py,
test_node_herm.py): a plain numpy model of the recurrence of csrc/hetrd.hip, the inputs, the bounds, and the argument rows of the
four new C operations.

The model is not bit-exact: the device's sums are wave reductions whose order the tests do not pin. It fixes the convention
(LAPACK's zhetrd, lower, on row-major members):
  H = Q tridiag(d, e) Q^H, d and e real, Q = H_0 H_1 ... H_{N-2}, H_k = I - tau_k v_k v_k^H, v_k zero in rows 0..k, 1 in row k+1, tail
  in F[k+2:, k]; N - 1 reflectors, the last with an empty tail. For the column x = [alpha; tail], sigma = |tail|^2:
    sigma = 0 and Im alpha = 0: tau_k = 0, e_k = Re alpha;
    else beta = -sign(Re alpha) sqrt(Re alpha^2 + Im alpha^2 + sigma) (sign(0) = +1), tau_k = ((beta - Re alpha) / beta, -Im alpha / beta),
         tail / (alpha - beta), e_k = beta;
    p = tau A v, w = p - (tau / 2)(p^H v) v, A -= v w^H + w v^H on the trailing block.
  A column whose sum of squares falls below 2^-900 (the member's maximum is scaled into [0.5, 1)) takes it again on 2^450 x, then on
  2^900 x, and divides the root by that factor: the reflector of a tiny column stays unitary and finite.

Bounds (the project's 1e-12 norm-wise gates, as in eigsym_common.py and tridiag_common.py), nrm = ||H||_F of the Hermitian completion:
  ||H - Q T Q^H||_F <= 1e-12 nrm,   ||Q^H Q - I||_F <= 1e-12 sqrt(N),   max |lambda(T) - lambda_LAPACK(H)| <= 1e-12 nrm,
  max |lambda - numpy.linalg.eigvalsh(H)| <= 1e-12 nrm,   ||H V - V diag(lambda)||_F <= 1e-12 nrm,   ||V^H V - I||_F <= 1e-12 sqrt(k)."""
import ctypes
import functools

import numpy as np

import eigsym_common as C
from nd4js_amd import _lib, rng

TOL = 1e-12
SEED = 8800
CAP = 96                                                        # tier A of csrc/hetrd.hip: N <= CAP stays in LDS


def herm(H):
    """the Hermitian completion of what the device reads: the lower triangle, the real part of the diagonal"""
    H = np.asarray(H, dtype=np.complex128)
    L = np.tril(H, -1)
    D = np.real(np.diagonal(H, 0, -2, -1))
    out = L + np.conj(np.swapaxes(L, -1, -2))
    idx = np.arange(H.shape[-1])
    out[..., idx, idx] = D
    return out


def tridiag(d, e):
    return np.diag(d) + np.diag(e, 1) + np.diag(e, -1)


def exponent(H):
    """e1: the frexp exponent of max(|Re h_ij|, |Im h_ij|) over what is read, 0 for the zero matrix"""
    A = np.tril(herm(H))
    mx = max(np.abs(A.real).max(), np.abs(A.imag).max()) if A.size else 0.0
    return int(np.frexp(mx)[1]) if mx > 0.0 and np.isfinite(mx) else 0


def _ldexp(z, k):
    return np.ldexp(z.real, k) + 1j * np.ldexp(z.imag, k)


def model(H):
    """(F, tau, d, e) of one Hermitian H [N, N] by the recurrence of the module's docstring on 2^-e1 H; d and e get 2^e1 back"""
    N = np.asarray(H).shape[0]
    e1 = exponent(H)
    A = _ldexp(herm(H), -e1)
    F, tau, e = np.zeros((N, N), dtype=np.complex128), np.zeros(max(N - 1, 0), dtype=np.complex128), np.zeros(max(N - 1, 0))
    for k in range(N - 1):
        alpha, tail = A[k + 1, k], A[k + 2:, k].copy()
        # a column below 2^-450 of the member's maximum: its squares lose bits or vanish; it takes them again on c x, c = 2^450, 2^900
        c = 1.0
        for _ in range(3):
            ta, al = tail * c, alpha * c
            sigma = float(np.sum(ta.real * ta.real + ta.imag * ta.imag))
            s2 = al.real * al.real + al.imag * al.imag + sigma
            if s2 >= 2.0 ** -900 or c == 2.0 ** 900 or not (tail.any() or alpha != 0.0):
                break
            c *= 2.0 ** 450
        if sigma == 0.0 and alpha.imag == 0.0:
            tau[k], e[k] = 0.0, alpha.real
            continue
        nrm = np.sqrt(s2) / c
        beta = -nrm if alpha.real >= 0.0 else nrm
        tau[k], e[k] = complex((beta - alpha.real) / beta, -alpha.imag / beta), beta
        v = np.concatenate(([1.0 + 0.0j], tail / (alpha - beta)))
        sub = A[k + 1:, k + 1:]
        p = tau[k] * (sub @ v)
        w = p - (0.5 * tau[k] * np.vdot(p, v)) * v
        sub -= np.outer(v, np.conj(w)) + np.outer(w, np.conj(v))
        idx = np.arange(sub.shape[0])
        sub[idx, idx] = sub[idx, idx].real
        F[k + 2:, k] = v[1:]
    d = np.ldexp(np.diag(A).real.copy(), e1)
    e = np.ldexp(e, e1)
    F[np.arange(N), np.arange(N)] = d
    F[np.arange(1, N), np.arange(N - 1)] = e
    return F, tau, d, e


def apply_q(F, tau, Z, adjoint=False):
    """Q Z or Q^H Z from the stored reflectors, one after the other"""
    N = F.shape[0]
    Z = np.array(Z, dtype=np.complex128)
    ks = range(N - 1) if adjoint else range(N - 2, -1, -1)
    for k in ks:
        v = np.zeros(N, dtype=np.complex128)
        v[k + 1] = 1.0
        v[k + 2:] = F[k + 2:, k]
        t = np.conj(tau[k]) if adjoint else tau[k]
        Z -= t * np.outer(v, np.conj(v) @ Z)
    return Z


def form_q(F, tau):
    return apply_q(F, tau, np.eye(F.shape[0]))


def norm_of(H):
    return max(np.linalg.norm(herm(H)), 1e-300)


def shares(H, Q, d, e, lam_ref=None):
    """(reconstruction, orthogonality, eigenvalues of T) as fractions of the three reduction bounds for one member; a missing part is 0"""
    N = H.shape[0]
    H = herm(H)
    nrm = norm_of(H)
    sc = np.ldexp(1.0, -np.frexp(nrm)[1])                       # keeps the products of a 2^+-500 member in range
    out = [0.0, 0.0, 0.0]
    if Q is not None:
        T = tridiag(d * sc, e * sc)
        out[0] = np.linalg.norm(H * sc - Q @ T @ np.conj(Q.T)) / (TOL * nrm * sc)
        out[1] = np.linalg.norm(np.conj(Q.T) @ Q - np.eye(N)) / (TOL * np.sqrt(N))
    if lam_ref is not None:
        from scipy.linalg import eigvalsh_tridiagonal
        lam = eigvalsh_tridiagonal(d * sc, e * sc) if N > 1 else d * sc
        out[2] = np.abs(np.sort(lam) - np.sort(lam_ref) * sc).max() / (TOL * nrm * sc)
    return tuple(out)


def check(H, Q, d, e, lam_ref=None, what=""):
    assert d.dtype == np.float64 and e.dtype == np.float64, what
    sh = shares(H, Q, d, e, lam_ref)
    print("%s: shares of the bounds (reconstruction, unitarity, values of T): %.3g %.3g %.3g" % ((what,) + sh))
    assert sh[0] <= 1.0, "%s: ||H - Q T Q^H||_F is %.3g of its bound" % (what, sh[0])
    assert sh[1] <= 1.0, "%s: ||Q^H Q - I||_F is %.3g of its bound" % (what, sh[1])
    assert sh[2] <= 1.0, "%s: max|lambda(T) - lambda(H)| is %.3g of its bound" % (what, sh[2])
    return sh


def check_layout(F, tau, d, e, what=""):
    """F carries d and e on its diagonals, with zero imaginary part, and zeros above"""
    N = F.shape[-1]
    assert F.dtype == np.complex128 and tau.dtype == np.complex128 and tau.shape == F.shape[:-2] + (max(N - 1, 0),), what
    dg = np.diagonal(F, 0, -2, -1)
    assert np.array_equal(dg.real, d) and not dg.imag.any(), what
    if N > 1:
        sg = np.diagonal(F, -1, -2, -1)
        assert np.array_equal(sg.real, e) and not sg.imag.any(), what
    assert not np.triu(F, 1).any(), what


def eig_shares(H, lam, V, lam_ref, lam_idx=None):
    """(values, residual, orthonormality) as fractions of the three eigen bounds, the largest over the members; lam [..., k] and
    V [..., N, k] (or None) are the columns lam_idx (a slice) of the descending spectrum lam_ref [..., N]"""
    N = H.shape[-1]
    k = lam.shape[-1]
    sl = lam_idx if lam_idx is not None else slice(0, N)
    out = [0.0, 0.0, 0.0]
    Vs = [None] * len(lam.reshape(-1, k)) if V is None else V.reshape(-1, N, k)
    for h, l, v, lr in zip(H.reshape(-1, N, N), lam.reshape(-1, k), Vs, lam_ref.reshape(-1, N)):
        h = herm(h)
        nrm = norm_of(h)
        out[0] = max(out[0], np.abs(l - lr[sl]).max() / (TOL * nrm) if k else 0.0)
        if v is not None and k:
            out[1] = max(out[1], np.linalg.norm(h @ v - v * l) / (TOL * nrm))
            out[2] = max(out[2], np.linalg.norm(np.conj(v.T) @ v - np.eye(k)) / (TOL * np.sqrt(k)))
    return tuple(out)


def eig_check(H, lam, V, lam_ref, lam_idx=None, what=""):
    assert lam.dtype == np.float64 and np.all(np.isfinite(lam)), what
    assert V is None or V.dtype == np.complex128, what
    if lam.shape[-1] > 1:
        assert np.all(lam[..., :-1] >= lam[..., 1:]), "%s: lambda is not descending" % what
    sh = eig_shares(H, lam, V, lam_ref, lam_idx)
    print("%s: shares of the bounds (values, residual, orthonormality): %.3g %.3g %.3g" % ((what,) + sh))
    assert sh[0] <= 1.0, "%s: max|lambda - eigvalsh| is %.3g of its bound" % (what, sh[0])
    assert sh[1] <= 1.0, "%s: ||H V - V L||_F is %.3g of its bound" % (what, sh[1])
    assert sh[2] <= 1.0, "%s: ||V^H V - I||_F is %.3g of its bound" % (what, sh[2])
    return sh


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def descending(H):
    """numpy.linalg.eigvalsh of the Hermitian completion, descending, per member"""
    return np.ascontiguousarray(np.linalg.eigvalsh(herm(H))[..., ::-1])


# ---- inputs -----------------------------------------------------------------------------------------------------------------------
def herm_uniform(seed, N):
    """a dense Hermitian matrix of seeded uniform parts in [-1, 1), real diagonal"""
    return herm(rng.matrix(seed, N, N) + 1j * rng.matrix(seed + 50000, N, N))


@functools.lru_cache(maxsize=None)
def dense(N):
    """(H, eigenvalues of LAPACK ascending); read-only, shared"""
    H = herm_uniform(SEED + N, N)
    lam = np.linalg.eigvalsh(H)
    H.setflags(write=False)
    lam.setflags(write=False)
    return H, lam


def complex_tridiag(N, seed=SEED + 4000):
    """a tridiagonal H with complex off-diagonals (every one with a non-zero imaginary part): all tails are zero, every step is a pure
    phase reflector"""
    d = rng.fill_uniform(seed + N, N)
    o = rng.fill_uniform(seed + 1 + N, max(N - 1, 0)) + 1j * (0.25 + 0.5 * np.abs(rng.fill_uniform(seed + 2 + N, max(N - 1, 0))))
    return np.diag(d).astype(np.complex128) + np.diag(o, -1) + np.diag(np.conj(o), 1)


def tiny_coupling(alpha):
    """two 1 x 1 blocks coupled by a tiny complex entry: [[1, .], [alpha, 1]]; |alpha|^2 underflows"""
    return np.array([[1.0, 0.0], [alpha, 1.0]], dtype=np.complex128)


def check_tiny_coupling(factor):
    """`factor(H)` -> (F, tau, d, e) on the two tiny couplings: finite, e_0 = -|alpha| and tau_0 = 1 - alpha / e_0 as for any other size"""
    eps = np.finfo(float).eps
    F, tau, d, e = factor(tiny_coupling(1e-170j))
    assert tau[0] == 1.0 + 1.0j and e[0] == -1e-170 and np.array_equal(d, [1.0, 1.0])
    F, tau, d, e = factor(tiny_coupling((3.0 + 4.0j) * 1e-160))
    assert np.all(np.isfinite(d)) and abs(e[0] + 5e-160) <= 4 * eps * 5e-160 and abs(tau[0] - (1.6 + 0.8j)) <= 8 * eps
    assert np.abs(d - 1.0).max() <= 4 * eps


def block_diagonal(N, cut):
    """two dense blocks, the second starting at row `cut`: column cut-1 has a zero tail and a zero alpha in the middle of the run"""
    H = np.zeros((N, N), dtype=np.complex128)
    H[:cut, :cut] = herm_uniform(SEED + 1000 + N, cut)
    H[cut:, cut:] = herm_uniform(SEED + 2000 + N, N - cut)
    return H


def real_symmetric(N):
    return C.sym_uniform(SEED + 5000 + N, N).astype(np.complex128)


def mixed_batch(N, k=500):
    """five members: dense, diagonal, zero, complex tridiagonal and 2^k times the dense one"""
    D = np.array(dense(N)[0])
    return np.stack([D, np.diag(C.half_steps(SEED + 3000 + N, N)).astype(np.complex128), np.zeros((N, N), dtype=np.complex128),
                     complex_tridiag(N), _ldexp(D, k)])


def kron_pairs(N2):
    """A (x) I_2 of a real symmetric A of order N2, as complex: every eigenvalue twice"""
    return np.kron(C.sym_uniform(SEED + 6000 + N2, N2), np.eye(2)).astype(np.complex128)


def rank5(N):
    x = rng.matrix(SEED + 6100 + N, N, 5) + 1j * rng.matrix(SEED + 6101 + N, N, 5)
    return herm(x @ np.conj(x.T))


def negdef(N):
    x = rng.matrix(SEED + 6200 + N, N, N) + 1j * rng.matrix(SEED + 6201 + N, N, N)
    return herm(-(x @ np.conj(x.T)) - N * np.eye(N))


def batch_5x40():
    return np.stack([herm_uniform(SEED + 7000 + b, 40) for b in range(5)])


def with_unread(H, fill=np.nan):
    """H with NaN in its strict upper triangle and garbage in the imaginary part of its diagonal: nothing of that is read"""
    out = np.array(H, dtype=np.complex128)
    N = H.shape[-1]
    iu = np.triu_indices(N, 1)
    out[..., iu[0], iu[1]] = complex(fill, fill)
    idx = np.arange(N)
    out[..., idx, idx] = out[..., idx, idx].real + 1j * (1.0 + idx)
    return out


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------
_buf = (ctypes.c_double * 64)()
P = ctypes.cast(_buf, ctypes.c_void_p)
Z = None
SUBSET = ": subset must satisfy 0 <= i0 <= i1 <= N"
# (operation, kind, arguments after the handle, return code, nd4hip_last_error()): every row ends inside the validation, which
# stands before the handle is looked at, so the rows hold with a NULL handle and the buffers are never read. The checks run in the
# family's order: negative extent, subset / selector, N <= 2048, empty call, NULL pointer
ROWS = [
    ("zhetrd_batched", "extent", (-1, 1, P, P, P, P, P), -1, "nd4hip_zhetrd_batched: negative extent"),
    ("zhetrd_batched", "extent", (1, -1, P, P, P, P, P), -1, "nd4hip_zhetrd_batched: negative extent"),
    ("zhetrd_batched", "extent", (1, 2049, P, P, P, P, P), -1, "nd4hip_zhetrd_batched: N <= 2048"),
    ("zhetrd_batched", "extent", (0, 2049, Z, Z, Z, Z, Z), -1, "nd4hip_zhetrd_batched: N <= 2048"),
    ("zhetrd_batched", "empty", (0, 1, Z, Z, Z, Z, Z), 0, None),
    ("zhetrd_batched", "empty", (1, 0, Z, Z, Z, Z, Z), 0, None),
    ("zhetrd_batched", "null", (1, 1, Z, Z, Z, Z, Z), -1, "nd4hip_zhetrd_batched: NULL pointer"),
    ("zhetrd_batched", "null", (1, 2, P, P, Z, P, P), -1, "nd4hip_zhetrd_batched: NULL pointer"),
    ("zhetrd_batched", "null", (1, 2, P, P, P, P, Z), -1, "nd4hip_zhetrd_batched: NULL pointer"),
    ("zhetrd_batched", "null", (1, 2, P, P, P, Z, P), -1, "nd4hip_zhetrd_batched: NULL pointer"),
    ("zunmtr_batched", "extent", (-1, 1, 1, 0, P, P, P), -1, "nd4hip_zunmtr_batched: negative extent"),
    ("zunmtr_batched", "extent", (1, 1, -1, 0, P, P, P), -1, "nd4hip_zunmtr_batched: negative extent"),
    ("zunmtr_batched", "extent", (1, 2049, 1, 0, P, P, P), -1, "nd4hip_zunmtr_batched: N <= 2048"),
    ("zunmtr_batched", "selector", (1, 4, 1, 2, P, P, P), -1, "nd4hip_zunmtr_batched: adjoint must be 0 or 1"),
    ("zunmtr_batched", "selector", (1, 4, 1, -1, P, P, P), -1, "nd4hip_zunmtr_batched: adjoint must be 0 or 1"),
    ("zunmtr_batched", "empty", (0, 1, 1, 0, Z, Z, Z), 0, None),
    ("zunmtr_batched", "empty", (1, 3, 0, 1, Z, Z, Z), 0, None),
    ("zunmtr_batched", "null", (1, 1, 1, 0, Z, Z, Z), -1, "nd4hip_zunmtr_batched: NULL pointer"),
    ("zunmtr_batched", "null", (1, 3, 1, 0, P, Z, P), -1, "nd4hip_zunmtr_batched: NULL pointer"),
    ("zheevd_batched", "extent", (-1, 1, P, P, P), -1, "nd4hip_zheevd_batched: negative extent"),
    ("zheevd_batched", "extent", (1, -1, P, P, P), -1, "nd4hip_zheevd_batched: negative extent"),
    ("zheevd_batched", "extent", (1, 2049, P, P, P), -1, "nd4hip_zheevd_batched: N <= 2048"),
    ("zheevd_batched", "empty", (0, 1, Z, Z, Z), 0, None),
    ("zheevd_batched", "empty", (1, 0, Z, Z, Z), 0, None),
    ("zheevd_batched", "null", (1, 1, Z, Z, Z), -1, "nd4hip_zheevd_batched: NULL pointer"),
    ("zheevd_batched", "null", (1, 1, P, Z, P), -1, "nd4hip_zheevd_batched: NULL pointer"),
    ("zheevx_batched", "extent", (-1, 1, 0, 1, P, P, P), -1, "nd4hip_zheevx_batched: negative extent"),
    ("zheevx_batched", "extent", (1, -1, 0, 0, P, P, P), -1, "nd4hip_zheevx_batched: negative extent"),
    ("zheevx_batched", "selector", (1, 4, 3, 2, P, P, P), -1, "nd4hip_zheevx_batched" + SUBSET),
    ("zheevx_batched", "selector", (1, 4, 0, 5, P, P, P), -1, "nd4hip_zheevx_batched" + SUBSET),
    ("zheevx_batched", "selector", (1, 2049, 0, 2050, P, P, P), -1, "nd4hip_zheevx_batched" + SUBSET),
    ("zheevx_batched", "extent", (1, 2049, 0, 1, P, P, P), -1, "nd4hip_zheevx_batched: N <= 2048"),
    ("zheevx_batched", "empty", (0, 1, 0, 1, Z, Z, Z), 0, None),
    ("zheevx_batched", "empty", (1, 0, 0, 0, Z, Z, Z), 0, None),
    ("zheevx_batched", "empty", (1, 4, 4, 4, Z, Z, Z), 0, None),
    ("zheevx_batched", "null", (1, 1, 0, 1, Z, Z, Z), -1, "nd4hip_zheevx_batched: NULL pointer"),
    ("zheevx_batched", "null", (1, 1, 0, 1, P, Z, P), -1, "nd4hip_zheevx_batched: NULL pointer"),
]
NEW = ("nd4hip_zhetrd_batched", "nd4hip_zunmtr_batched", "nd4hip_zheevd_batched", "nd4hip_zheevx_batched")
# a valid call of each operation (arguments after the handle): refused only for the NULL handle
VALID = {"zhetrd_batched": (1, 1, P, P, Z, P, Z), "zunmtr_batched": (1, 1, 1, 0, P, Z, P), "zheevd_batched": (1, 1, P, P, Z),
         "zheevx_batched": (1, 1, 0, 1, P, P, Z)}


def mismatches(handle):
    """the rows that a form answers differently, for test_gpu_herm.py too"""
    lib, bad = _lib.load(), []
    for op, kind, args, rc, text in ROWS:
        for form in ("_host", "_dev"):
            got = getattr(lib, "nd4hip_" + op + form)(handle, *args)
            err = lib.nd4hip_last_error().decode() if got != 0 else None
            if (got, err) != (rc, text):
                bad.append("nd4hip_%s%s%r [%s]: expected %r, got %r" % (op, form, args, kind, (rc, text), (got, err)))
    return bad
