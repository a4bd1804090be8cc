"""Shared by the divide & conquer SVD tests (test_gpu_svd_dc.py, test_node_svd_dc.py, test_svd_dc_host.py): the inputs, the
oracle's results (computed once per input and never modified) and the project's SVD bounds.

The yardstick is oracle.svd_dc, the line-cited C restatement of the reference's svd_dc.js. The device adds across lanes where
the reference adds sequentially, so nothing is compared bit for bit; the bounds are those of tests/test_gpu_svd.py:
sv within 1e-12 sigma_max, the reference's acceptance bounds (check_properties, slack 1), and for dense inputs with distinct
singular values sign-aligned U and V within 1e-11 / max(gap, 1e-6)."""
import functools

import numpy as np

import oracle
from nd4js_amd import rng

EPS = 2.0 ** -52


def check_properties(a, u, sv, v, slack=1.0):
    """_generic_test_svd_decomp.js:85-154 (copied from tests/test_gpu_svd.py)"""
    M, N = a.shape[-2:]
    L = min(M, N)
    assert u.shape == a.shape[:-2] + (M, L) and sv.shape == a.shape[:-2] + (L,) and v.shape == a.shape[:-2] + (L, N)
    assert np.all(sv >= 0) and np.all(np.diff(sv, axis=-1) <= 0), "sv must be non-negative and descending"
    a2, u2, s2, v2 = a.reshape((-1, M, N)), u.reshape((-1, M, L)), sv.reshape((-1, L)), v.reshape((-1, L, N))
    for b in range(a2.shape[0]):
        rec = (u2[b] * s2[b]) @ v2[b]
        assert np.linalg.norm(rec - a2[b]) <= slack * 48 * EPS * max(M, N) * max(np.linalg.norm(a2[b]), 1e-300)
        assert np.abs(u2[b].T @ u2[b] - np.eye(L)).max() <= slack * 4 * EPS * M
        assert np.abs(v2[b] @ v2[b].T - np.eye(L)).max() <= slack * 4 * EPS * N


def align_signs(u, v, ur, vr):
    """flip (u_k, v_k) pairs so they point like the reference's; returns aligned copies"""
    s = np.sign(np.einsum("...ik,...ik->...k", u, ur))
    s[s == 0] = 1.0
    return u * s[..., None, :], v * s[..., :, None]


def check_values(sv, ref):
    assert np.abs(sv - ref).max() <= 1e-12 * max(ref.max(), 1e-300)


def check_vectors(u, v, ur, vr, ref):
    """dense inputs with distinct singular values: what test_golden_svd_decomp asserts"""
    if ref.shape[-1] < 2:
        gaps = 1.0
    else:
        gaps = np.abs(np.diff(ref, axis=-1)).min() / ref.max()
    ua, va = align_signs(u, v, ur, vr)
    tol = 1e-11 / max(gaps, 1e-6)                      # singular vector sensitivity ~ eps / gap
    assert np.abs(ua - ur).max() <= tol and np.abs(va - vr).max() <= tol


def bidiag_dense(d, e):
    """(d [K], e [J-1]) as the dense upper bidiagonal K x J matrix"""
    K, J = d.shape[-1], e.shape[-1] + 1
    B = np.zeros(d.shape[:-1] + (K, J))
    i = np.arange(K)
    B[..., i, i] = d
    j = np.arange(J - 1)
    B[..., j, j + 1] = e
    return B


# ---- inputs of the bidiagonal solver -------------------------------------------------------------------------------------
BIDIAG_SIZES = (2, 3, 4, 5, 6, 7, 9, 17, 33, 64, 65, 129, 257)


def _u(seed, n, lo, hi):
    return np.random.default_rng(seed).uniform(lo, hi, n)


def _bidiag_cases():
    c = {}
    for n in BIDIAG_SIZES:                                     # leaves, first merges, wave / workgroup / tile boundaries
        for J in (n, n + 1):
            c["rand_%d_%d" % (n, J)] = (_u(5000 + 2 * n + J, n, -1, 1), _u(6000 + 2 * n + J, J - 1, -1, 1))
    d20, e20 = _u(7001, 20, 0.5, 1), _u(7002, 20, 0.5, 1)      # deflation by z = 0: K = 20, J = 21
    c["zdefl_none"] = (d20, e20)
    for name, ks in (("one", (7,)), ("several", (2, 3, 11, 19)), ("all", tuple(range(20)))):
        e = e20.copy()
        e[list(ks)] = 0.0
        c["zdefl_" + name] = (d20, e)
    dd = np.array([3, 3, 3, 2, 2, 1, 1, 1, 0, 0], dtype=np.float64)   # deflation by equal diagonal entries
    c["eqdiag_e0"] = (dd, np.zeros(9))
    c["eqdiag_e1e-3"] = (dd, 1e-3 * _u(7003, 9, -1, 1))
    c["identity_16"] = (np.ones(16), np.zeros(15))
    c["zero_8"] = (np.zeros(8), np.zeros(7))
    return c


BIDIAG_CASES = _bidiag_cases()


@functools.lru_cache(maxsize=None)
def bidiag_reference(name):
    d, e = BIDIAG_CASES[name]
    B = bidiag_dense(d, e)
    u, sv, v = oracle.svd_dc(B)
    for x in (B, u, sv, v):
        x.setflags(write=False)
    return B, u, sv, v


# ---- inputs of svd_decomp(A, algo='dc') ----------------------------------------------------------------------------------
SQUARE_SIZES = (1, 2, 3, 4, 5, 7, 8, 9, 16, 17, 33, 64, 65, 130, 257, 513)
DENSE_SHAPES = {"wide_5x9": (5, 9), "wide_33x130": (33, 130), "tall_70x33": (70, 33), "batch_3x2x9x9": (3, 2, 9, 9)}


def _with_sv(seed, n, sv):
    g = np.random.default_rng(seed)
    q1, _ = np.linalg.qr(g.standard_normal((n, n)))
    q2, _ = np.linalg.qr(g.standard_normal((n, n)))
    return (q1 * np.asarray(sv, dtype=np.float64)) @ q2


def _low_rank(seed, n, r):
    g = np.random.default_rng(seed)
    return g.uniform(-1, 1, (n, r)) @ g.uniform(-1, 1, (r, n))


def _dense_cases():
    c = {}
    for n in SQUARE_SIZES:
        c["sq_%d" % n] = rng.matrix(8000 + n, n, n)
    for name, shape in DENSE_SHAPES.items():
        c[name] = rng.matrix(8100 + sum(shape), *shape)
    c["scaled_1e+150"] = rng.matrix(8017, 17, 17) * 1e150
    c["scaled_1e-150"] = rng.matrix(8017, 17, 17) * 1e-150
    return c


def _structured_cases():
    i = np.arange(12, dtype=np.float64)
    return {
        "rank2_16": _low_rank(8201, 16, 2),
        "rank5_64": _low_rank(8202, 64, 5),
        "clustered_32": _with_sv(8203, 32, [1.0] * 16 + [0.5] * 8 + [1e-8] * 8),
        "graded_32": _with_sv(8204, 32, 10.0 ** -np.arange(32)),
        "hilbert_12": 1.0 / (i[:, None] + i[None, :] + 1.0),
    }


DENSE_CASES = _dense_cases()                # distinct singular values: values, properties and vectors
STRUCTURED_CASES = _structured_cases()      # values and properties
RANKS = {"rank2_16": 2, "rank5_64": 5}


@functools.lru_cache(maxsize=None)
def dense_reference(name):
    a = DENSE_CASES[name] if name in DENSE_CASES else STRUCTURED_CASES[name]
    u, sv, v = oracle.svd_dc(a)
    for x in (a, u, sv, v):
        x.setflags(write=False)
    return a, u, sv, v


# ---- the level list --------------------------------------------------------------------------------------------------------
def recursion_nodes(n, off=0):
    """the nodes _svd_dc_bidiag visits (svd_dc.js:666-824): (off, n, is_leaf), children before their parent"""
    if n <= 3:
        return [(off, n, True)]
    n0 = n >> 1
    return recursion_nodes(n0, off) + recursion_nodes(n - n0, off + n0) + [(off, n, False)]
