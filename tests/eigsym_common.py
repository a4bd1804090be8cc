"""Shared by the symmetric-eigenproblem tests (test_eigsym_host.py, test_gpu_eigsym.py, test_node_eigsym.py): the catalogue of
inputs, LAPACK's results for them (computed once per input and never modified), the bounds, and a numpy model of the two steps
of csrc/syev.hip that are new arithmetic (the shift-and-Cholesky recurrence and the back-transformation of the values), with
numpy.linalg.svd standing in for the device's bidiagonal solver and a plain Householder tridiagonalisation for hess.hip.
For test_eigsym_paths_host.py and test_gpu_eigsym_paths.py: the inputs that reach every path of syev.hip's own kernels (PATHS,
HESS_ROUTES) and compose(), the route restated from the device's public pieces with syev.hip's own part in numpy.

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


def model_batch(S):
    """model() per member of S [..., N, N] with lambda put in descending order: (lambda, V, smallest radicand of all)"""
    N = S.shape[-1]
    lam, V, low = np.empty(S.shape[:-1]).reshape(-1, N), np.empty(S.shape).reshape(-1, N, N), np.inf
    for b, s in enumerate(S.reshape(-1, N, N)):
        l, v, lo = model(s)
        order = np.argsort(-l, kind="stable")
        lam[b], V[b], low = l[order], v[:, order], min(low, lo)
    return lam.reshape(S.shape[:-1]), V.reshape(S.shape), low


# ---- the route stage by stage (test_eigsym_paths_host.py, test_gpu_eigsym_paths.py) --------------------------------------------------
PATH_SEED = 7400
SCALE_KS = (-1000, -500, -1, 0, 3, 500, 1000)
PAIR_ROWS = (1, 64, 65, 129)                         # the row i of the single pair s_i,i-1 of pair_130: e_i-1 is the only non-zero of e


def base_40():
    return sym_uniform(7300, 40)


def half_steps(seed, N):
    """rint(8 u) / 2 of N seeded uniform u in [-1, 1): the 17 multiples of 0.5 in [-4, 4], unsorted, with negatives; ties for N > 17"""
    return np.rint(8.0 * rng.fill_uniform(seed, N)) / 2.0


def diag_half(N):
    return np.diag(half_steps(PATH_SEED + 100 + N, N))


def diag_among_dense(N):
    """diag_half(N) between two dense members"""
    return np.stack([sym_uniform(PATH_SEED + 200 + N, N), diag_half(N), sym_uniform(PATH_SEED + 300 + N, N)])


def pair_130(i):
    """diag_half(130) with the single off-diagonal pair s_i,i-1 = s_i-1,i = 0.375"""
    S = diag_half(130)
    S[i, i - 1] = S[i - 1, i] = 0.375
    return S


def mixed_7x40():
    D = sym_uniform(PATH_SEED + 40, 40)
    return np.stack([D, np.ldexp(D, 500), np.ldexp(D, -500), D * 3.0, np.diag(half_steps(PATH_SEED + 41, 40)), np.zeros((40, 40)),
                     _tri_zeros(PATH_SEED + 42, 40)])


def mixed_3x65():
    return np.stack([sym_uniform(PATH_SEED + 65, 65), np.diag(half_steps(PATH_SEED + 66, 65)), np.ldexp(sym_uniform(PATH_SEED + 67, 65), -3)])


def scaled_batch(ks=SCALE_KS):
    """member b is 2^ks[b] base_40()"""
    return np.stack([np.ldexp(base_40(), k) for k in ks])


def grid_20(N):
    """symmetric integers of up to 20 bits: rint(2^20 u); 2^-1074 times it is exact, every entry a subnormal number"""
    return np.rint(np.ldexp(sym_uniform(PATH_SEED + 500 + N, N), 20))


def top_tridiag(N):
    """tridiag(0.625, 0.125): 2^1024 times it is finite (0.625 2^1024 < DBL_MAX), its eigenvalues lie inside +-0.875"""
    return tridiag(np.full(N, 0.625), np.full(N - 1, 0.125))


def _batch_256(B):
    return np.stack([sym_uniform(PATH_SEED + 600 + 10 * B + b, 256) for b in range(B)])


# name -> builder: the finite inputs of the composition test. singles: the LDS tile edges of syev_symm (63, 64, 65: one tile, a
# partial one, a 2 x 2 tiling with a one-wide edge; 129: the same on a 3 x 3 tiling) and the leaves N = 2, 3.
PATHS = {}
for _N in (2, 3, 63, 64, 65, 129):
    PATHS["single_%d" % _N] = functools.partial(sym_uniform, PATH_SEED + _N, _N)
PATHS.update({"mixed_7x40": mixed_7x40, "mixed_3x65": mixed_3x65, "scaled_7x40": scaled_batch})
for _N in (2, 5, 64, 65, 130):
    PATHS["diag_%d" % _N] = functools.partial(diag_half, _N)
    PATHS["diag_in_batch_%d" % _N] = functools.partial(diag_among_dense, _N)
for _i in PAIR_ROWS:
    PATHS["pair_130_at_%d" % _i] = functools.partial(pair_130, _i)
for _N in (5, 40):
    PATHS["grid_%d" % _N] = functools.partial(grid_20, _N)
for _N in (3, 65):
    PATHS["top_base_%d" % _N] = functools.partial(top_tridiag, _N)
# name -> (builder, ND4HIP_HESS_NO_PERSIST set?): the routes of the reduction that eigen_sym reaches (hess.hip, nd4_gehrd)
HESS_ROUTES = {
    "one_launch_1x256": (functools.partial(_batch_256, 1), False),
    "blocked_1x512": (lambda: sym_uniform(PATH_SEED + 512, 512)[None], True),
    "per_step_wy_2x256": (functools.partial(_batch_256, 2), False),
    "per_step_u_5x256": (functools.partial(_batch_256, 5), False),
}
PATH_NAMES = tuple(PATHS)


@functools.lru_cache(maxsize=None)
def path_reference(name):
    """(S, lambda descending) of LAPACK for an input of PATHS or HESS_ROUTES; read-only, shared by every test"""
    S = np.ascontiguousarray((PATHS[name] if name in PATHS else HESS_ROUTES[name][0])(), dtype=np.float64)
    assert np.array_equal(S, np.swapaxes(S, -1, -2))
    return _freeze(S, np.ascontiguousarray(np.linalg.eigvalsh(S)[..., ::-1]))


def member_exponents(S):
    """e1 [batch] of syev_absmax_lower / syev_exp: the frexp exponent of max|s_ij| over the lower triangle, 0 for a zero member"""
    N = S.shape[-1]
    mx = np.abs(np.tril(S.reshape(-1, N, N))).max(axis=(1, 2))
    assert np.all(np.isfinite(mx))
    return np.where(mx > 0.0, np.frexp(mx)[1], 0).astype(np.int64)


def check_scaled(S, lam, V, lam_ref, what=""):
    """check() on every member times 2^-e1: the same shares of the same bounds (the scaling is exact), also where ||S||_F itself
    would overflow (2^1000, 2^1024) or its squares underflow (2^-1000, subnormal input)"""
    N = S.shape[-1]
    assert lam.shape == S.shape[:-1] and (V is None or V.shape == S.shape), what
    e1 = member_exponents(S)
    up = lambda a, extra: np.ldexp(a.reshape((-1,) + a.shape[-extra:]), -e1.reshape((-1,) + (1,) * extra)).reshape(a.shape)
    return check(up(S, 2), up(lam, 1), V, up(lam_ref, 1), what)


def _device_calls():
    """the three public device entry points compose() is made of, on host arrays: hessenberg_decomp on the whole batch in one call
    (nd4_gehrd picks its route by batch and N), bidiag_svd on the whole batch, nd4hip_dgemm_ex_dev(0, 1, ...) per member"""
    import torch
    from nd4js_amd import dev

    def up(a):
        return torch.from_numpy(np.ascontiguousarray(a)).cuda()

    def hess(W):
        U, H = dev.hessenberg_decomp(up(W))
        return U.cpu().numpy(), H.cpu().numpy()

    def bsvd(p, q):
        _, sv, V2 = dev.bidiag_svd(up(p), up(q))
        return sv.cpu().numpy(), V2.cpu().numpy()

    def gemm_nt(U, V2):
        N = U.shape[0]
        out = torch.empty((N, N), dtype=torch.float64, device="cuda")
        return dev.gemm_ex(0, 1, 1.0, up(U), up(V2), 0.0, out, N, N, N, N, N, N).cpu().numpy()
    return hess, bsvd, gemm_nt


def compose(S, calls=None):
    """csrc/syev.hip restated from its public pieces: (lambda, V, parts) for S [N, N] or [batch, N, N], N >= 2. Everything that
    syev.hip computes itself is exact or rounded once (ldexp, one +, /, sqrt, *, - each, no contraction) and is done here in
    numpy; the reduction, the bidiagonal solver and the product U V2^T are `calls` = (hess, bsvd, gemm_nt), by default the device's
    own entry points. A member whose e is zero throughout (a diagonal T, the zero matrix included) takes 2^e1 d by descending
    rank, ties by index, and the unit vectors in that order for the rows of V2, as syev_values writes them. parts: the
    intermediate results by name (V2 with that replacement)."""
    hess, bsvd, gemm_nt = calls if calls is not None else _device_calls()
    N = S.shape[-1]
    S3 = np.asarray(S, dtype=np.float64).reshape(-1, N, N)
    B = S3.shape[0]
    e1 = member_exponents(S3)
    W = np.tril(S3)
    iu = np.triu_indices(N, 1)
    W[:, iu[0], iu[1]] = W[:, iu[1], iu[0]]                         # mirrored, not added: a -0.0 keeps its sign
    W = np.ldexp(W, -e1[:, None, None])
    U, H = hess(W)
    d = np.ascontiguousarray(np.diagonal(H, 0, -2, -1))
    e = np.ascontiguousarray(np.diagonal(H, -1, -2, -1))
    p, q = np.ones((B, N)), np.zeros((B, N - 1))                   # a zero member: the bidiagonal of the identity
    c, k, kind = np.zeros(B), np.zeros(B, dtype=np.int64), []
    for b in range(B):
        f = shift_chol(d[b], e[b])
        if f is None:
            kind.append("zero")
            continue
        p[b], q[b], c[b], k[b] = f[:4]
        kind.append("dense" if np.any(e[b]) else "diag")
    sv, V2 = bsvd(p, q)
    lam, V = np.empty((B, N)), np.empty((B, N, N))
    V2 = np.array(V2)
    for b in range(B):
        if kind[b] == "dense":
            lam[b] = np.ldexp(sv[b] * sv[b] - c[b], e1[b] - k[b])
        else:                                                        # d by descending rank, ties by index, and the unit vectors
            order = np.argsort(-d[b], kind="stable")                 # in that order (a zero member: d = 0, the identity)
            lam[b] = np.ldexp(d[b][order], e1[b])
            V2[b] = np.eye(N)[order]
        V[b] = gemm_nt(U[b], V2[b])
    parts = {"e1": e1, "W": W, "U": U, "H": H, "d": d, "e": e, "p": p, "q": q, "c": c, "k": k, "kind": tuple(kind), "sv": sv, "V2": V2}
    return lam.reshape(S.shape[:-1]), V.reshape(S.shape), parts


def numpy_calls():
    """numpy stand-ins for the three device calls of compose(): the model's Householder tridiagonalisation, numpy.linalg.svd and @"""
    def hess(W):
        U, H = np.empty_like(W), np.empty_like(W)
        for b in range(W.shape[0]):
            U[b], d, e = householder_tridiag(W[b])
            H[b] = tridiag(d, e)
        return U, H

    def bsvd(p, q):
        sv, V2 = np.empty_like(p), np.empty(p.shape + p.shape[-1:])
        for b in range(p.shape[0]):
            _, sv[b], V2[b] = np.linalg.svd(np.diag(p[b]) + np.diag(q[b], 1))
        return sv, V2
    return hess, bsvd, lambda U, V2: U @ V2.T


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


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
