"""Shared by the divide & conquer SVD tests (test_gpu_svd_dc.py, test_gpu_svd_dc_paths.py, test_node_svd_dc.py, test_svd_dc_host.py,
test_svd_dc_paths_host.py): the inputs, the
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


# ---- inputs named for the path each selects (test_svd_dc_paths_host.py, test_gpu_svd_dc_paths.py) -------------------------------
# What a merge does depends on two counts the data decide: n0 values deflated because z = 0, n1 - n0 deflated by a rotation
# because two diagonal entries are equal; m - n1 secular roots remain. The cases below are built so that the reference takes a
# given path at a given size; test_svd_dc_paths_host.py asserts that from the oracle's own records (oracle.bidiag_svd_dc,
# stats=True), so a catalogue entry cannot silently stop reaching what it is named for.
def twin(seed, h, lo, hi, zeros=()):
    """K = 2 h + 1, J = K + 1: the same block twice around one middle row. Both children of the top merge are computed by the
    same operations from the same numbers, so every singular value of one meets its twin with a non-zero z: rotations.
    zeros: entries of the block's super-diagonal set to 0 in both copies."""
    dl, el = _u(seed, h, lo, hi), _u(seed + 1, h, lo, hi)
    el[list(zeros)] = 0.0
    return np.concatenate([dl, [0.7], dl]), np.concatenate([el, [-0.6], el])


def quad(seed, h, inner=1.0):
    """K = 4 h + 3, J = K + 1: a twin of twins. With inner = 1 every value of a half meets its twin once more at the top, in
    pairs: a rotation deflates one of the two and the other becomes a pole, whose root differs from it. With a weak inner middle
    row (inner = 1e-9) that root moves by the square of the coupling, less than a rounding, so each half hands BOTH copies of a
    value up, with vectors that reach the half's boundary: the top merge meets four equal values with z of order 1 and its
    rotations chain through them."""
    dl, el = _u(seed, h, -1, 1), _u(seed + 1, h, -1, 1)
    hd, he = np.concatenate([dl, [0.8 * inner], dl]), np.concatenate([el, [0.55 * inner], el])
    return np.concatenate([hd, [0.7], hd]), np.concatenate([he, [-0.6], he])


TINY_VALUES = (-1.5, 0.0, 0.75)
TINY_SHAPES = ((1, 1), (1, 2), (2, 2), (2, 3))


def tiny_problems(K, J):
    """every (d [K], e [J-1]) with entries from TINY_VALUES, as one batch: one leaf each, no merge; every zero and sign branch
    of the two closed forms (svd_dc.js:37-143)"""
    g = np.array(np.meshgrid(*[TINY_VALUES] * (K + J - 1), indexing="ij")).reshape(K + J - 1, -1).T
    return np.ascontiguousarray(g[:, :K]), np.ascontiguousarray(g[:, K:])


def _path_cases():
    c = {}
    c["quad_16"] = quad(9400, 16)                              # two m = 33 merges full of rotations; all three lists at the top
    c["quad_16_weak"] = quad(9400, 16, inner=1e-9)             # rotations that chain through three and four equal values
    d, e = quad(9400, 16)
    d[[5, 39]] = 0.0
    c["quad_16_singular"] = (d, e[:-1])                        # J = K: zero middle rows; a rotation whose partner is m - 1
    d, e = _u(21, 69, -1, 1), _u(22, 68, -1, 1)
    d[[10, 50]] = 0.0
    c["sing_69"] = (d, e)                                      # the same without any symmetry
    c["twin_130"] = twin(9430, 130, 0.5, 1)                    # m = 261: rotations in the columns c >= 256
    c["twin_34_zeros"] = twin(9100, 34, -1, 1, zeros=(5, 20))  # z = 0 deflates at both GEMM levels, roots remain
    d, e = twin(9100, 34, -1, 1, zeros=(5, 20))
    e[34] = 0.0
    c["twin_34_zeros_b2"] = (d, e)
    d, e = _u(11, 69, -1, 1), _u(12, 69, -1, 1)
    d[34] = e[34] = 0.0
    c["zero_middle_69"] = (d, e)                               # the top merge deflates everything but one root
    c["rand_70_71"] = (_u(1, 70, -1, 1), _u(2, 70, -1, 1))     # merges of m = 34 and m = 35 in one level: zero padding
    # Graded by 2^-12 per row. Not more steeply: at 2^-16 per row the reference itself loses orthogonality completely
    # (U^T U - I of order 1). That is how the reference behaves and nothing the device could be held to.
    k = np.arange(40, dtype=np.float64)
    c["graded_40"] = (2.0 ** (-12 * k), 2.0 ** (-12 * k - 1))
    c["max_2048"] = (_u(1, 2048, -1, 1), _u(2, 2048, -1, 1))   # the largest K: every LDS array full
    return c


PATH_CASES = _path_cases()


@functools.lru_cache(maxsize=None)
def path_reference(name):
    """(B, U2, sv, V2, records) of oracle.bidiag_svd_dc for a PATH_CASES entry"""
    d, e = PATH_CASES[name]
    B = bidiag_dense(d, e)
    u, sv, v, rec = oracle.bidiag_svd_dc(d, e, stats=True)
    for x in (B, u, sv, v):
        x.setflags(write=False)
    return B, u, sv, v, tuple(rec)


def mixed_members(name):
    """the members of the two batches whose members take different paths at a level that runs gather, GEMM and scatter"""
    if name == "mixed_67_68":
        d, e = _u(31, 67, -1, 1), _u(32, 67, -1, 1)
        d[33] = e[33] = 0.0
        return [PATH_CASES["quad_16"], (_u(33, 67, -1, 1), _u(34, 67, -1, 1)), (d, e), twin(9100, 33, -1, 1, zeros=(5, 20))]
    assert name == "mixed_69_69"
    return [PATH_CASES["sing_69"], (_u(35, 69, -1, 1), _u(36, 68, -1, 1))]


def error_inputs():
    """K = 20, J = 21, all ones but one entry: the reference's bisection meets a sum that is not finite (svd_dc.js:429)"""
    out = []
    for which, k, val in (("d", 3, np.nan), ("d", 3, np.inf), ("e", 0, np.inf), ("e", 19, np.nan)):
        d, e = np.ones(20), np.ones(20)
        (d if which == "d" else e)[k] = val
        out.append((d, e))
    return out


def check_bidiag(d, e, u2, sv, v2, ref):
    """what every bidiag_svd result is held to: the project's bounds, and all J rows of V2 orthonormal"""
    B = bidiag_dense(d, e)
    K, J = B.shape
    assert u2.shape == (K, K) and sv.shape == (K,) and v2.shape == (J, J)
    check_values(sv, ref)
    check_properties(B, u2, sv, v2[:K])
    assert np.abs(v2 @ v2.T - np.eye(J)).max() <= 4 * EPS * J


def used(a, u2, sv, v2, ref):
    """the share of each bound a result uses (values, reconstruction, U, V), for reports; asserts nothing"""
    M, N = a.shape
    L = min(M, N)
    return (np.abs(sv - ref).max() / (1e-12 * max(ref.max(), 1e-300)),
            np.linalg.norm((u2 * sv) @ v2[:L] - a) / (48 * EPS * max(M, N) * max(np.linalg.norm(a), 1e-300)),
            np.abs(u2.T @ u2 - np.eye(L)).max() / (4 * EPS * M),
            np.abs(v2 @ v2.T - np.eye(v2.shape[0])).max() / (4 * EPS * N))


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


def _path_dense_cases():
    """min(M, N) > 32, so the deflations these spectra cause are applied by gather, GEMM and scatter"""
    return {
        "clustered_96": _with_sv(8303, 96, [1.0] * 48 + [0.5] * 24 + [1e-8] * 24),
        "rank3_80": _low_rank(8301, 80, 3),
        "zero_40": np.zeros((40, 40)),
        "eye_70": np.eye(70),
        "batch_2x40x70": rng.matrix(8340, 2, 40, 70),          # the wide and the tall route with m = 40: d and e are read
        "batch_2x70x40": rng.matrix(8370, 2, 70, 40),          # at the stride of the bidiagonal matrix from two members
    }


DENSE_CASES = _dense_cases()                # distinct singular values: values, properties and vectors
STRUCTURED_CASES = _structured_cases()      # values and properties
PATH_DENSE_CASES = _path_dense_cases()      # values and properties
RANKS = {"rank2_16": 2, "rank5_64": 5, "rank3_80": 3}


@functools.lru_cache(maxsize=None)
def dense_reference(name):
    a = next(c[name] for c in (DENSE_CASES, STRUCTURED_CASES, PATH_DENSE_CASES) if name in c)
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
