"""Shared helpers of the DGEMM path tests (test_gemm_ref_host.py, test_gpu_gemm_paths.py): a reference product of higher precision
than the kernels, the two elementwise checks, NaN-guarded operand buffers, the two input families and the rank-k case selection.

The reference is `np.longdouble` where that type carries a 64-bit mantissa (x87 extended); anywhere else it is a compensated product
(Ogita / Rump / Oishi Dot2: TwoProduct by Veltkamp splitting, TwoSum) kept as an unevaluated float64 pair, so the suite never silently
compares a float64 kernel with a float64 reference.

Bound check: for C = alpha op(A) op(B) + beta C0 with inner extent K, every element of a float64 result computed in ANY summation
order, with or without FMA, over at most 32 split-K partial sums, satisfies

    |got - exact| <= gamma_n * E,   gamma_n = n u / (1 - n u),  u = 2^-53,  n = K + 35,
    E = |alpha| (|op A| |op B|) + |beta| |C0|

(Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., section 3.1: a length-K inner product costs gamma_K whatever the
order; the 35 covers the <= 32 partial sums, the product with alpha and the beta C0 term). It is derived, not measured, and does not
depend on tile shape, K-step or accumulation order. The reference's own error is <= (K + 2) 2^-64 E, 2^-11 of the budget.

Exact check: operands and C0 are integers in [-4, 4], alpha and beta are dyadic, so every partial sum in every order is a dyadic
rational far below 2^53 and the kernel must reproduce the integer result bit for bit."""
import random

import numpy as np

from nd4js_amd import rng

U = 2.0 ** -53
LD = np.longdouble
HAVE_LD = np.finfo(np.longdouble).nmant >= 63             # x87 extended or better; otherwise the Dot2 pair below
ALPHAS = (1.0, -1.0, 2.0, -0.5, 0.75)                     # the integer family's scalars: dyadic, so alpha * integer is exact
BETAS = (0.0, 1.0, -1.0, 2.0, -0.5)
SMALLK_AB = ((1.0, 0.0), (-1.0, 0.0), (1.0, 1.0), (1.0, -1.0), (-1.0, 1.0), (-1.0, -1.0))   # gemm.hip: smallk_ok


class Pair(np.ndarray):
    """float64 array `hi` with a correction `lo` of the same shape: the value is hi + lo, unevaluated"""
    lo = None


# ------------------------------------------------------------------------------------------------------------------------ inputs
def uniform(seed, *shape):
    return rng.matrix(seed, *shape)


def integers(seed, *shape):
    """the seeded generator's [-1, 1) mapped to the integers -4 .. 4 (as float64)"""
    return np.rint(rng.matrix(seed, *shape) * 4.0)


FAMILIES = {"int": integers, "uni": uniform}


def op(t, X):
    return X.T if t else X


# --------------------------------------------------------------------------------------------------------------------- reference
def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def _split(a):
    c = 134217729.0 * a                                     # 2^27 + 1
    hi = c - (c - a)
    return hi, a - hi


def _two_prod(a, b):
    p = a * b
    ah, al = _split(a)
    bh, bl = _split(b)
    return p, al * bl - (((p - ah * bh) - al * bh) - ah * bl)


def _dot2(A, B):
    """A @ B as an unevaluated pair (s, c): error <= u |result| + gamma_K^2 |A| |B|"""
    M, K = A.shape
    s = np.zeros((M, B.shape[1]))
    c = np.zeros_like(s)
    for k in range(K):
        p, e = _two_prod(A[:, k, None], B[None, k, :])
        s, q = _two_sum(s, p)
        c += e + q
    return s, c


def _ref_dot2(alpha, A, B, beta, C0):
    s, c = _dot2(A, B)
    # alpha and beta are applied to both halves; the products with alpha are themselves split so that nothing is rounded at u
    p, e = _two_prod(np.float64(alpha), s)
    lo = e + alpha * c
    if beta != 0.0:
        q, f = _two_prod(np.float64(beta), C0)
        p, g = _two_sum(p, q)
        lo = lo + (f + g)
    out = p.view(Pair)
    out.lo = lo
    return out


def ref_gemm(ta, tb, alpha, A, B, beta, C0, force_dot2=False):
    """(ref, E): alpha op(A) op(B) + beta C0 and the envelope |alpha| |op A| |op B| + |beta| |C0| in the reference precision.
    beta == 0 means C0 is not read (it may be None or hold NaN), as in the kernels."""
    a, b = op(ta, np.asarray(A, dtype=np.float64)), op(tb, np.asarray(B, dtype=np.float64))
    with np.errstate(invalid="ignore", over="ignore"):
        aa, ab = np.abs(a).astype(LD), np.abs(b).astype(LD)
        E = LD(abs(alpha)) * (aa @ ab) if a.shape[1] else np.zeros((a.shape[0], b.shape[1]), dtype=LD)
        if beta != 0.0:
            E = E + LD(abs(beta)) * np.abs(C0).astype(LD)
        if HAVE_LD and not force_dot2:
            ref = LD(alpha) * (a.astype(LD) @ b.astype(LD)) if a.shape[1] else np.zeros(E.shape, dtype=LD)
            if beta != 0.0:
                ref = ref + LD(beta) * np.asarray(C0).astype(LD)
        else:
            ref = _ref_dot2(alpha, np.ascontiguousarray(a), np.ascontiguousarray(b), beta, None if beta == 0.0 else np.asarray(C0, dtype=np.float64))
    return ref, E


def exact_gemm(ta, tb, alpha, A, B, beta, C0, blas=False):
    """the integer family's result: int64 product converted to float64 (`blas`: float64 BLAS, which is exact on these inputs too
    and is what the few cases above 2e8 multiply-adds use), then the exact dyadic scaling"""
    a, b = op(ta, A), op(tb, B)
    if blas:
        p = a @ b
    else:
        ai, bi = a.astype(np.int64), b.astype(np.int64)
        assert np.array_equal(ai, a) and np.array_equal(bi, b)
        p = (ai @ bi).astype(np.float64)
    out = alpha * p
    if beta != 0.0:
        out = out + beta * C0
    assert np.abs(out).max(initial=0.0) < 2.0 ** 40
    return out


# ------------------------------------------------------------------------------------------------------------------------ checks
def gamma(n):
    return LD(n) * LD(U) / (LD(1) - LD(n) * LD(U))


def _where(mask, limit=8):
    idx = np.argwhere(mask)
    return "%d element(s), first at %s" % (len(idx), [tuple(int(v) for v in i) for i in idx[:limit]])


def bound_ratio(got, ref, E, K):
    """per element |got - ref| / (gamma_{K+35} E) on the finite elements (0 on the others), after the non-finite ones were compared
    by position and kind. An element with E == 0 must be reproduced exactly (its ratio is inf otherwise)."""
    got = np.asarray(got)
    assert got.dtype == np.float64 and got.shape == E.shape, (got.dtype, got.shape, E.shape)
    hi = np.asarray(ref, dtype=np.float64) if isinstance(ref, Pair) else ref
    for name, f in (("nan", np.isnan), ("+inf", np.isposinf), ("-inf", np.isneginf)):
        bad = f(got) != f(hi)
        assert not bad.any(), "%s mask differs from the reference: %s" % (name, _where(bad))
    fin = np.isfinite(hi)
    with np.errstate(invalid="ignore", divide="ignore"):
        if isinstance(ref, Pair):
            err = np.abs((got.astype(LD) - hi.astype(LD)) - np.asarray(ref.lo).astype(LD))
        else:
            err = np.abs(got.astype(LD) - ref)
        lim = gamma(K + 35) * E
        return np.where(fin, np.where(err == 0, LD(0), err / lim), LD(0))


def assert_within_bound(got, ref, E, K):
    """every element: |got - ref| <= gamma_{K+35} E. Returns the largest |err| / (gamma E) for the record."""
    ratio = bound_ratio(got, ref, E, K)
    bad = ~(ratio <= 1)
    if bad.any():
        i = np.unravel_index(np.argmax(np.where(np.isnan(ratio), np.inf, ratio)), ratio.shape)
        raise AssertionError("outside gamma_%d * E: %s; worst %s: got %r, ratio %.3g"
                             % (K + 35, _where(bad), tuple(int(v) for v in i), got[i], float(ratio[i])))
    return float(ratio.max(initial=0))


def assert_exact(got, want):
    got = np.asarray(got)
    assert got.shape == want.shape, (got.shape, want.shape)
    if not np.array_equal(got, want):
        bad = ~(got == want)
        i = tuple(np.argwhere(bad)[0])
        raise AssertionError("not exact: %s; at %s got %r, want %r" % (_where(bad), tuple(int(v) for v in i), got[i], want[i]))


# ------------------------------------------------------------------------------------------------------------- NaN-guarded buffers
class Padded:
    """`batch` operands of rows x cols with leading dimension `ld`, `stride` elements apart, laid out inside a flat buffer that holds
    NaN everywhere else: `lead_rows` rows before the first, `tail_rows` after the last, the ld - cols padding of every row, whatever
    lies between two members, and `offset` extra elements in front, which shift the base by 8 bytes each. `win` is the host view of the
    window(s); upload() / download() move the WHOLE buffer."""

    def __init__(self, rows, cols, ld, lead_rows=2, tail_rows=2, offset=0, batch=1, stride=None):
        assert ld >= cols and rows >= 0 and cols >= 0 and batch >= 1
        self.rows, self.cols, self.ld, self.batch = rows, cols, ld, batch
        self.stride = rows * ld if stride is None else stride
        assert batch == 1 or self.stride >= rows * ld
        self.start = lead_rows * max(ld, 1) + offset
        n = self.start + (batch - 1) * self.stride + (rows + tail_rows) * max(ld, 1) + 2
        self.buf = np.full(n, np.nan)
        self.win = self._window(self.buf)
        self.dev = self.sent = None

    def _window(self, flat, squeeze=True):
        s = flat.strides[0]
        w = np.lib.stride_tricks.as_strided(flat[self.start:], (self.batch, self.rows, self.cols), (self.stride * s, self.ld * s, s))
        return w[0] if squeeze and self.batch == 1 else w

    def upload(self):
        import torch
        self.sent = self.buf.copy()
        self.dev = torch.from_numpy(self.sent).cuda()
        return self

    @property
    def ptr(self):
        import ctypes
        return ctypes.c_void_p(self.dev.data_ptr() + 8 * self.start)

    def download(self):
        """the window(s) as the device holds them now; everything outside must still hold the bits that were uploaded"""
        now = self.dev.cpu().numpy()
        outside = np.ones(now.shape, dtype=bool)
        self._window(outside)[...] = False
        changed = outside & (now.view(np.uint64) != self.sent.view(np.uint64))
        assert not changed.any(), "written outside the window: flat offsets from the window's first element %s" % (
            (np.flatnonzero(changed)[:8] - self.start).tolist(),)
        return self._window(now).copy()

    def assert_unchanged(self):
        """an input: the whole buffer, window included, bit-identical to what was uploaded"""
        assert np.array_equal(self.dev.cpu().numpy().view(np.uint64), self.sent.view(np.uint64)), "an input operand was written"


def padded(rows, cols, ld, lead_rows=2, tail_rows=2, offset=0):
    return Padded(rows, cols, ld, lead_rows, tail_rows, offset)


# ------------------------------------------------------------------------------------------------- model of the kernel's tile map
def tile_of(bid, tiles_m, tiles_n, nxcd=8, group_m=8):
    """workgroup -> (tm, tn) exactly as gemm.hip: dgemm_kernel computes it ("XCD-aware tile assignment"): blocks b, b + 8, ... share
    an XCD and get a contiguous chunk of the tile sequence, which is rasterised in groups of 8 tile-rows. A model, not the kernel."""
    nwg = tiles_m * tiles_n
    xcd, within = bid % nxcd, bid // nxcd
    q, r = nwg // nxcd, nwg % nxcd
    wg = (xcd * (q + 1) if xcd < r else r * (q + 1) + (xcd - r) * q) + within
    per_group = group_m * tiles_n
    first_m = (wg // per_group) * group_m
    gsz = min(tiles_m - first_m, group_m)
    return first_m + (wg % per_group) % gsz, (wg % per_group) // gsz


# ------------------------------------------------------------------------------------------------- rank-k kernel: case selection
SMALLK_K = (1, 2, 3, 4, 5, 7, 8, 15, 16, 17, 31, 32)
SMALLK_M = (1, 15, 16, 17, 63, 64, 65, 130)
SMALLK_N = (1, 31, 32, 33, 100)
SMALLK_AXES = (SMALLK_K, SMALLK_M, SMALLK_N, (0, 1), SMALLK_AB)


def smallk_cases():
    """(K, M, N, tb, (alpha, beta)): a seeded greedy selection that covers every PAIR of values of two different axes (so every
    value of every axis meets both transposes, beta = 0 and beta != 0); about a hundred cases instead of the 5760 of the full product"""
    axes = SMALLK_AXES
    pairs = lambda c: {(i, c[i], j, c[j]) for i in range(5) for j in range(i + 1, 5)}
    need = sorted({(i, a, j, b) for i in range(5) for j in range(i + 1, 5) for a in axes[i] for b in axes[j]}, key=repr)
    left = set(need)
    r = random.Random(20240)
    out = []
    for seed_pair in need:                                  # every candidate holds one uncovered pair: progress is certain
        if seed_pair not in left:
            continue
        i, a, j, b = seed_pair
        best, gain = None, -1
        for _ in range(40):
            c = [r.choice(ax) for ax in axes]
            c[i], c[j] = a, b
            g = len(pairs(c) & left)
            if g > gain:
                best, gain = tuple(c), g
        out.append(best)
        left -= pairs(best)
    return out
