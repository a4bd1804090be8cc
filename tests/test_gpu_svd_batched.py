"""Batched kernel paths of svd_decomp, member isolation, host chunking and extreme scales, checked member by member.

The one-sided Jacobi SVD (svd.hip: nd4_gesvdj / jacobi_square, svd_block.hip: nd4_jacobi_block_sweep) chooses its kernels from the
BATCH SIZE as well as from N, so a batched member can be wrong in one member's offset, in a per-member stride of the block scratch
(Gpart, Qt2, flags2) or in a noise floor shared across members while every single-matrix test passes. The `dev` form hands the
batch to the kernels unchanged, so the cases below reach each path by shape alone.

Notation: L = min(M, N) (the Jacobi size after the QR front end of rectangular input), Np = L rounded up to a multiple of 64
(zero-padded when L % 64 != 0, for L > 64), npairs = Np / 64, P = batch * npairs.

  case (batch x M x N)                         path                                                   condition in the source
  16x512, 96x512, 40x300, 64x100, 12x1000,     fused Gram + eigen: jacb_eigen<true, 8>                Np <= 1024, 128 <= P <= 768
  70 x 96x80
  15x512, 20x300, 63x100, 5x1000, 4x1100,      step 0 jacb_gram2 + jacb_eigen<false, 2>, then         P <= 256, not fused, not deferred
  9x512, 24 x 600x272, 24 x 272x600            jacb_eigen_p; jacb_apply
  97x512, 160x300, 400x128, 16x1100            step 0 jacb_eigen<false, 8>, then jacb_eigen_p          P > 256, not fused
  8x512, 3x1000, 2x1100, 1x512,                deferred U update: jacb_eigen_pu + jacb_apply_w<1>     P <= 64, Np >= 512, Np <= 2048
  3 x 1500x700
  1x2100 (Np = 2112)                           the same with the one-chain jacb_apply_w<2>            P <= 64, Np > 2048, nblk % 4 != 0
  64x32, 9x2 / 50x33, 40x64, 40 x 200x48       jac_small<32> / jac_small<64>                          1 < L <= 64
  dense phase (precheck off in early sweeps)   every block case with Np >= 512                        svd.hip: dense_phase
  completion of null-space rows of V           jac_complete (L < 128), one QR per member (L >= 128)   svd.hip epilogue

The host form (la.svd_decomp) cuts a batch into calls first (nd4hip_host.hip: min_chunk 128, 256 MB chunks; `_host_chunk`):
300 x 256^2 runs as 2 fused calls of 150 (P = 600) while the device form of all 300 is <false, 8> (P = 1200).

Checks on every member: the reference's acceptance bounds (_generic_test_svd_decomp.js:85-154, as check_properties in
test_gpu_svd.py) relative to the member's OWN |A|_F and sigma_max. On a fixed sample of members (first, last and seeded others, at
least 8): sv within 1e-12 sigma_max of oracle.svd_dc (the reference's svd_decomp; at most 2 members at L >= 1000, the rest of the
sample against LAPACK) and U / V after per-triplet sign alignment within 1e-11 / gap where singular values are separated. The audit
(include/nd4hip.h: nd4hip_dgesvdj_last_info) must hold for every call: 1 <= sweeps <= 30, rotations > 0, offnorm <= L * 2.3e-16.

Member isolation: for Np < 512 there is no dense phase and converged members are skipped, so a member's U, sv and V do not depend on
its companions at all; that is asserted bit for bit. For Np >= 512 the dense-phase switch (svd.hip: dense_phase) reads the rotation
count summed over the batch, so a member's last bits legitimately depend on its companions; there only the tolerances are asserted.

Extreme scales: each member is scaled by an exact power of two 2^-e (e = frexp exponent of max|a|) before the Jacobi sweeps and sv by
2^e afterwards, so the sums of squares neither overflow nor underflow for any finite input, and svd_decomp(2^k A) returns bit for bit
the U and V of svd_decomp(A) and sv times 2^k.
"""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import oracle
from nd4js_amd import rng

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -52
_POOL = ThreadPoolExecutor(8)          # the oracle is plain C behind ctypes (the GIL is released): sample members in parallel


# ------------------------------------------------------------------------------------------------------------------------ helpers
def _dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _host(*ts):
    out = tuple(t.cpu().numpy() for t in ts)
    return out if len(out) > 1 else out[0]


def _sample(batch, seed, k=8):
    """first, last and seeded others: at least k members (all of them for batch <= k)"""
    if batch <= k:
        return list(range(batch))
    idx = {0, batch - 1}
    r = rng.matrix(seed, 4 * k).ravel()
    for u in r:
        if len(idx) >= k:
            break
        idx.add(int((u + 1.0) / 2.0 * batch) % batch)
    return sorted(idx)


def _host_chunk(batch, per_item_bytes, chunk_bytes=256 << 20, max_chunks=8, min_chunk=128):
    """members per kernel call of la.svd_decomp on one device: nd4hip_host.hip run_block with the SVD Plan"""
    n = -(-per_item_bytes * batch // chunk_bytes)
    n = max(1, min(n, max_chunks, batch // min_chunk))
    return -(-batch // n)


def _pow2(x):
    """the power of two of max|x| (frexp), 1 for a zero member: dividing by it is exact and brings the member to unit scale"""
    m = np.abs(x).max() if x.size else 0.0
    return 1.0 if m == 0 or not np.isfinite(m) else float(np.ldexp(1.0, int(np.frexp(m)[1])))


def dev_svd(a):
    """dev.svd_decomp of a host batch: (U, sv, V) on the host and the audit"""
    from nd4js_amd import dev
    info = {}
    U, sv, V = dev.svd_decomp(_dev(a), info=info)
    return _host(U, sv, V) + (info,)


def check_audit(info, L, trivial=False):
    assert 1 <= info["sweeps"] <= 30, info
    assert trivial or info["rotations"] > 0, info
    assert info["offnorm"] <= L * 2.3e-16, info


def check_member(a, u, sv, v, slack=1.0):
    """test_gpu_svd.check_properties for ONE member, evaluated at unit scale (exact power-of-two scaling) so that members at
    1e+-150 .. 1e+-300 are held to the same bounds as the ordinary ones"""
    M, N = a.shape
    L = min(M, N)
    assert u.shape == (M, L) and sv.shape == (L,) and v.shape == (L, N)
    assert np.all(sv >= 0) and np.all(np.diff(sv) <= 0), "sv must be non-negative and descending"
    s = _pow2(a)
    a1, sv1 = a / s, sv / s
    rec = (u * sv1) @ v
    assert np.linalg.norm(rec - a1) <= slack * 48 * EPS * max(M, N) * max(np.linalg.norm(a1), 1e-300)
    assert np.abs(u.T @ u - np.eye(L)).max() <= slack * 4 * EPS * M
    assert np.abs(v @ v.T - np.eye(L)).max() <= slack * 4 * EPS * N


def align_signs(u, v, ur, vr):
    """flip (u_k, v_k) pairs so they point like the reference's; returns aligned copies"""
    s = np.sign(np.einsum("ik,ik->k", u, ur))
    s[s == 0] = 1.0
    return u * s[None, :], v * s[:, None]


def _svd_dc_or_lapack(x):
    """oracle.svd_dc; LAPACK where the reference's own algorithm stops at one of its assertions (svd_dc.js:583 trips on some
    exactly degenerate members: zero, all-ones, diagonal with repeated entries)"""
    try:
        return oracle.svd_dc(x)
    except RuntimeError:
        return np.linalg.svd(x, full_matrices=False)


def _ref_jobs(a, members):
    """reference SVDs of the sample, started before the device runs: svd_dc (the reference's algorithm) for at most 2 members at
    L >= 1000 (single core, ~6 s at 1100^2), LAPACK as the third opinion for the rest"""
    L = min(a.shape[-2:])
    jobs = {}
    for i, m in enumerate(members):
        if L < 1000 or i < 2:
            jobs[m] = _POOL.submit(_svd_dc_or_lapack, a[m])
        else:
            jobs[m] = _POOL.submit(np.linalg.svd, a[m], False)
    return jobs


def check_against_reference(a, u, sv, v, ref, uv=True):
    """sv within 1e-12 sigma_max of the reference; U / V after sign alignment where the singular values are well separated"""
    ru, rsv, rv = ref
    s = _pow2(a)
    assert np.abs(sv / s - rsv / s).max() <= 1e-12 * max(rsv.max() / s, 1e-300)
    if uv and min(a.shape) > 1 and rsv[-1] > 1e-6 * rsv[0]:
        gaps = np.abs(np.diff(rsv)).min() / rsv.max()
        ua, va = align_signs(u, v, ru, rv)
        tol = 1e-11 / max(gaps, 1e-6)                  # eigenvector sensitivity ~ eps / gap (test_golden_svd_decomp)
        assert np.abs(ua - ru).max() <= tol and np.abs(va - rv).max() <= tol


def run_checked(a, seed, slack=None, uv=True, trivial=False):
    """dev.svd_decomp of the batch a: bounds on every member, reference on the sample; returns U, sv, V, info"""
    members = _sample(len(a), seed)
    jobs = _ref_jobs(a, members)
    u, sv, v, info = dev_svd(a)
    check_audit(info, min(a.shape[-2:]), trivial)
    for m in range(len(a)):
        check_member(a[m], u[m], sv[m], v[m], 1.0 if slack is None else slack[m])
    for m in members:
        check_against_reference(a[m], u[m], sv[m], v[m], jobs[m].result(), uv and (slack is None or slack[m] == 1.0))
    return u, sv, v, info


# ------------------------------------------------------------------------------------------------------ every path, dense members
PATH_CASES = [
    # fused jacb_eigen<true, 8>: both ends of P, padded, Np = 128, Np = 1024 padded
    (16, 512, 512), (96, 512, 512), (40, 300, 300), (64, 100, 100), (12, 1000, 1000),
    # jacb_eigen<false, 2>, not deferred: dense phase, padded without dense phase, P = 126 below fused, Np = 1024, Np = 1152 > 1024
    (15, 512, 512), (20, 300, 300), (63, 100, 100), (5, 1000, 1000), (4, 1100, 1100),
    # jacb_eigen<false, 8>: P = 776 above fused, P = 800 below the dense-phase size, Np = 128, Np > 1024
    (97, 512, 512), (160, 300, 300), (400, 128, 128), (16, 1100, 1100),
    # deferred U update (jacb_eigen_pu + jacb_apply_w<1>): P = 64, P = 72 (not deferred), padded, Np > 1024
    (8, 512, 512), (9, 512, 512), (3, 1000, 1000), (2, 1100, 1100),
    # one-chain jacb_apply_w<2>: a single matrix with 2048 < Np < 4096
    (1, 2100, 2100),
    # jac_small<32> / <64>
    (64, 32, 32), (50, 33, 33), (40, 64, 64), (9, 2, 2),
    # rectangular front end (QR first), batched: tall / wide <false, 2>, fused + jac_complete, jac_small, deferred after QR
    (24, 600, 272), (24, 272, 600), (70, 96, 80), (40, 200, 48), (3, 1500, 700),
]


@pytest.mark.parametrize("batch,M,N", PATH_CASES)
def test_svd_paths(batch, M, N):
    """every member of a dense batch on each kernel path against the acceptance bounds, the sample against the reference"""
    a = rng.matrix(21000 + 7 * batch + M + 3 * N, batch, M, N)
    run_checked(a, 21100 + M + N)


def test_small_path_against_mpmath():
    """jac_small<32>: singular values of 3 members against a 40-digit SVD"""
    mpmath = pytest.importorskip("mpmath")
    a = rng.matrix(21300, 64, 32, 32)
    u, sv, v, info = dev_svd(a)
    check_audit(info, 32)
    with mpmath.workdps(40):
        for m in (0, 31, 63):
            ref = np.array([float(x) for x in mpmath.svd_r(mpmath.matrix(a[m].tolist()), compute_uv=False)])
            ref = np.sort(ref)[::-1]
            assert np.abs(sv[m] - ref).max() <= 1e-12 * ref[0]
    b = rng.matrix(21301, 9, 2, 2)
    _, svb, _, _ = dev_svd(b)
    with mpmath.workdps(40):
        for m in range(9):
            ref = np.sort(np.array([float(x) for x in mpmath.svd_r(mpmath.matrix(b[m].tolist()), compute_uv=False)]))[::-1]
            assert np.abs(svb[m] - ref).max() <= 1e-12 * ref[0]


# --------------------------------------------------------------------------------------------------------- heterogeneous batches
KINDS = ("dense", "zero", "orth", "diag", "rank1", "rankhalf", "zerorow", "zerocol", "graded", "tiny", "huge", "tail")


def _member(kind, seed, M, N):
    L = min(M, N)
    g = rng.matrix(seed, M, N)
    if kind == "dense":
        return g
    if kind == "zero":
        return np.zeros((M, N))
    if kind == "orth":                                          # every sv = 1: converges in the first sweep
        q, _ = np.linalg.qr(rng.matrix(seed, max(M, N), L))
        return q if M >= N else q.T.copy()
    if kind == "diag":
        out = np.zeros((M, N))
        out[np.arange(L), np.arange(L)] = 4.0 * g[0, :L] if M <= N else 4.0 * g[:L, 0]
        return out
    if kind == "ones":                                          # rank 1 with the longest rows a member at its scale can have
        return np.ones((M, N))
    if kind == "rank1":
        return np.outer(g[:, 0], g[0, :])
    if kind == "rankhalf":
        r = max(1, L // 2)
        return rng.matrix(seed + 1, M, r) @ rng.matrix(seed + 2, r, N)
    if kind == "zerorow":
        g[M // 3, :] = 0.0
        return g
    if kind == "zerocol":
        g[:, N // 3] = 0.0
        return g
    if kind == "graded":
        return g * np.logspace(0, -8, M)[:, None]
    if kind == "tiny":
        return g * 1e-150
    if kind == "huge":
        return g * 1e150
    if kind == "tail":
        # diagonal: one entry 1, the others -4 L eps. Legit singular values 4x above this member's OWN noise floor
        # (L eps max_i |a_i| = L eps) but below the floor of a member with long rows ("ones": L eps sqrt(N) / 2 after scaling),
        # so a floor shared with such a member would replace their rows of V: |A - U S V|_F ~ 8 L^1.5 eps > 48 eps L |A|_F
        out = np.zeros((M, N))
        out[np.arange(L), np.arange(L)] = -4.0 * L * EPS
        out[0, 0] = 1.0
        return out
    raise ValueError(kind)


def mixed_batch(seed, batch, M, N, first=None, kinds=KINDS):
    """members cycle through `kinds`; member 0 is `first` when given"""
    out = np.empty((batch, M, N))
    names = []
    for m in range(batch):
        k = first if (m == 0 and first is not None) else kinds[(m + seed) % len(kinds)]
        out[m] = _member(k, seed + 31 * m, M, N)
        names.append(k)
    return out, names


RANK_DEFICIENT = ("zero", "rank1", "rankhalf", "ones")

MIXED_CASES = [
    (40, 300, 300), (64, 100, 100), (20, 300, 300), (15, 512, 512), (160, 300, 300), (97, 512, 512), (8, 512, 512), (3, 1000, 1000),
    (64, 32, 32), (50, 33, 33), (24, 600, 272), (24, 272, 600), (70, 96, 80), (40, 200, 48),
]


@pytest.mark.parametrize("batch,M,N", MIXED_CASES)
def test_mixed_members(batch, M, N):
    """zero, orthogonal, diagonal, rank 1, rank L/2, zero row / column, graded, 1e-150, 1e150 and dense members in ONE batch on each
    path: every member meets its own bounds (slack 4 for the rank-deficient ones with L >= 128, as
    test_rank_deficient_completion_by_qr), the sample matches the reference. Member 0 has the longest rows (all ones): a noise floor
    taken from it would swallow the legit small singular values of the `tail` members, and in a rectangular batch its identical
    columns drive the QR front end's column norms into the subnormal range (test_input_with_identical_columns)"""
    a, kinds = mixed_batch(22000 + batch + M, batch, M, N, first="ones")
    L = min(M, N)
    slack = [4.0 if (k in RANK_DEFICIENT and L >= 128) else 1.0 for k in kinds]
    u, sv, v, _ = run_checked(a, 22100 + M, slack=slack, uv=False)
    for m, k in enumerate(kinds):
        if k == "zero":
            assert np.array_equal(sv[m], np.zeros(L))
            if M >= N:                                          # (the wide path returns Vr Q^T: orthonormal, not the identity)
                assert np.array_equal(v[m], np.eye(L)), "rank 0: V is the identity completion"
        elif k == "orth":
            assert np.abs(sv[m] - 1.0).max() <= 4 * EPS * max(M, N)
        elif k in ("rank1", "ones"):
            assert np.all(sv[m][1:] <= 1e-12 * sv[m][0]) and sv[m][0] > 0
        elif k == "tail":
            assert abs(sv[m][0] - 1.0) <= 4 * EPS * max(M, N) and np.abs(sv[m][1:] / (4.0 * L * EPS) - 1.0).max() <= 1e-8


@pytest.mark.parametrize("N", [100, 300, 512])
def test_mixed_rank_completion(N):
    """r = N, r = 0, 0 < r < N side by side: jac_complete (N < 128) and the per-member QR completion loop (svd.hip, N >= 128) must
    each write their own member's V. Member 0 is full rank, so a completion written to the wrong member breaks member 0."""
    ranks = [N, 0, N // 3, N, 1, N - 1, 0, N]
    a = np.zeros((len(ranks), N, N))
    for m, r in enumerate(ranks):
        if r > 0:                                   # orthonormal factors, singular values in [1, 2]: rank r, well conditioned
            q1, _ = np.linalg.qr(rng.matrix(22200 + 5 * m + N, N, r))
            q2, _ = np.linalg.qr(rng.matrix(22300 + 5 * m + N, N, r))
            a[m] = (q1 * (1.5 + 0.5 * rng.matrix(22350 + m + N, r).ravel())) @ q2.T
    slack = [1.0 if r == N else (4.0 if N >= 128 else 1.0) for r in ranks]
    u, sv, v, _ = run_checked(a, 22400 + N, slack=slack, uv=False)
    for m, r in enumerate(ranks):
        if r == 0:
            assert np.array_equal(sv[m], np.zeros(N)) and np.array_equal(v[m], np.eye(N))
        elif r < N:
            assert np.all(sv[m][r:] <= 1e-10 * sv[m][0]) and sv[m][r - 1] > 1e-6 * sv[m][0]


# ---------------------------------------------------------------------------------------------------- companions do not matter
ISOLATION_CASES = [(40, 300, 300), (20, 300, 300), (160, 300, 300), (64, 100, 100), (64, 32, 32), (50, 33, 33), (24, 600, 272)]


@pytest.mark.parametrize("batch,M,N", ISOLATION_CASES)
def test_member_independent_of_companions(batch, M, N):
    """Np < 512 (fused, <false, 2>, <false, 8>, jac_small, and the tall front end): the same member k in two batches of the same size
    and shape whose other members are different and shuffled comes out bit for bit the same, wherever it sits"""
    a, _ = mixed_batch(23000 + M, batch, M, N)
    k = batch // 3
    b, _ = mixed_batch(23100 + M, batch, M, N)
    b = b[rng.matrix(23200, batch).ravel().argsort()]
    k2 = batch - 2
    b[k2] = a[k]
    u1, s1, v1, _ = dev_svd(a)
    u2, s2, v2, _ = dev_svd(b)
    assert np.array_equal(s1[k], s2[k2]) and np.array_equal(u1[k], u2[k2]) and np.array_equal(v1[k], v2[k2])


def test_member_with_other_companions_dense_phase():
    """Np >= 512: the dense-phase switch reads the rotation count summed over the batch, so the last bits of a member may depend on
    its companions; the tolerances still hold and the two results agree to them"""
    batch, N = 9, 512
    a = rng.matrix(23300, batch, N, N)
    b, _ = mixed_batch(23400, batch, N, N)
    b[5] = a[2]
    u1, s1, v1, _ = dev_svd(a)
    u2, s2, v2, _ = dev_svd(b)
    check_member(b[5], u2[5], s2[5], v2[5])
    assert np.abs(s1[2] - s2[5]).max() <= 1e-12 * s1[2][0]


# -------------------------------------------------------------------------------------------------------------- host chunking
def test_host_chunk_size():
    per_item = 8 * (3 * 256 * 256 + 256)                      # A in, U, sv, V out
    assert _host_chunk(300, per_item) == 150
    assert _host_chunk(255, per_item) == 255                  # below 2 * min_chunk: never cut


def test_host_chunks_equal_device_slices():
    """la.svd_decomp of 300 x 256^2 = two calls of 150 (fused, P = 600): each equals dev.svd_decomp of exactly that slice bit for
    bit; every member (149 | 150 across the cut included) meets the bounds; the device form of all 300 (<false, 8>, P = 1200)
    agrees within the tolerances (a different path: not bitwise). la's default handle (device=None) is ONE device, the current
    one, so the batch is not sharded over peers: only a handle created over a list of devices is (nd4js_amd/_lib.py: Handle)"""
    from nd4js_amd import la
    B, N = 300, 256
    c = _host_chunk(B, 8 * (3 * N * N + N))
    a, kinds = mixed_batch(24000, B, N, N)
    a[:: 2] = rng.matrix(24001, B // 2, N, N)
    info = {}
    u, sv, v = la.svd_decomp(a, info=info)
    check_audit(info, N)
    for lo in range(0, B, c):
        us, ss, vs, _ = dev_svd(a[lo:lo + c])
        assert np.array_equal(u[lo:lo + c], us) and np.array_equal(sv[lo:lo + c], ss) and np.array_equal(v[lo:lo + c], vs)
    rd = [k in RANK_DEFICIENT and m % 2 for m, k in enumerate(kinds)]
    for m in range(B):
        check_member(a[m], u[m], sv[m], v[m], 4.0 if rd[m] else 1.0)
    u2, s2, v2, info2 = dev_svd(a)
    check_audit(info2, N)
    for m in range(B):
        assert np.abs(sv[m] - s2[m]).max() <= 1e-12 * max(sv[m][0], 1e-300)
    for m in (0, 149, 150, 299):
        assert np.abs(sv[m] - np.linalg.svd(a[m], compute_uv=False)).max() <= 1e-12 * max(sv[m][0], 1e-300)


# ------------------------------------------------------------------------------------------------------------- extreme scales
SCALES = [2.0 ** 600, 2.0 ** -600, 1e200, 1e-200, 1e300, 1e-300]
SCALE_SHAPES = [(48, 48), (100, 100), (300, 300), (512, 512), (200, 48), (48, 200), (600, 272)]


@pytest.mark.parametrize("scale", SCALES, ids=["2^600", "2^-600", "1e200", "1e-200", "1e300", "1e-300"])
@pytest.mark.parametrize("M,N", SCALE_SHAPES)
def test_extreme_scale(M, N, scale):
    """sums of squares of unscaled entries overflow above ~1e154 and underflow below ~1e-154: the result must not notice"""
    a = rng.matrix(25000 + M + N, M, N) * scale
    ref = _POOL.submit(oracle.svd_dc, a)
    u, sv, v, info = dev_svd(a[None])
    check_audit(info, min(M, N))
    assert np.all(np.isfinite(sv)) and np.all(np.isfinite(u)) and np.all(np.isfinite(v))
    check_member(a, u[0], sv[0], v[0])
    check_against_reference(a, u[0], sv[0], v[0], ref.result())


@pytest.mark.parametrize("batch,N", [(12, 300), (12, 48), (6, 512)])
def test_mixed_scale_batch(batch, N):
    """1e-200, 1 and 1e200 members in one batch: each at its own scale"""
    a = rng.matrix(25100 + N, batch, N, N) * np.array([1e-200, 1.0, 1e200] * (batch // 3))[:, None, None]
    run_checked(a, 25200 + N)


EQUI_KINDS = tuple(k for k in KINDS if k not in ("tiny", "huge"))       # (2^+-600 times those would leave the normal range)
EQUI_CASES = [(8, 48, 48), (40, 300, 300), (1, 512, 512), (24, 600, 272), (24, 272, 600), (40, 200, 48), (3, 1500, 700)]


@pytest.mark.parametrize("batch,M,N", EQUI_CASES)
def test_power_of_two_equivariance(batch, M, N):
    """the scaling by 2^-e is exact and canonical: svd_decomp(2^k A) is svd_decomp(A) with sv times 2^k, bit for bit"""
    a, _ = mixed_batch(25300 + M, batch, M, N, kinds=EQUI_KINDS)
    a[::3] = rng.matrix(25301 + N, len(a[::3]), M, N)
    u0, s0, v0, _ = dev_svd(a)
    for k in (-600, 3, 600):
        u, s, v, _ = dev_svd(np.ldexp(a, k))
        assert np.array_equal(u, u0) and np.array_equal(v, v0), k
        assert np.array_equal(s, np.ldexp(s0, k)), k


@pytest.mark.parametrize("scale", [1e-170, 1e170])
def test_rank_and_lstsq_at_extreme_scales(scale):
    """rank and lstsq are built on svd_decomp (rank.js, lstsq.js): they must not change with the scale of A"""
    from nd4js_amd import la
    A = rng.matrix(25400, 100, 37) @ rng.matrix(25401, 37, 100)
    r = la.rank(A)
    assert r == 37
    assert la.rank(A * scale) == r
    B = rng.matrix(25402, 4, 60, 40)
    y = rng.matrix(25403, 4, 60, 3)
    x = la.lstsq(B * scale, y)
    for m in range(4):
        ref = np.linalg.pinv(B[m] * scale) @ y[m]
        assert np.linalg.norm(x[m] - ref) <= 1e-10 * np.linalg.norm(ref)


# ------------------------------------------------------------------------------------------------------------- QR front end
@pytest.mark.parametrize("M,N", [(200, 48), (96, 80), (600, 272), (272, 600), (1500, 700)])
def test_input_with_identical_columns(M, N):
    """identical columns: each Householder step leaves the next column at eps times the previous one, so after ~10 columns the sums
    of squares of the QR front end are subnormal (qr_internal.h: QR_SIGMA_MIN). U / V must stay orthogonal, alone and batched"""
    from nd4js_amd import la
    a = np.ones((3, M, N))
    a[1] *= -0.5
    u, sv, v, _ = dev_svd(a)
    for m in range(3):
        check_member(a[m], u[m], sv[m], v[m], slack=4.0 if min(M, N) >= 128 else 1.0)
        assert np.all(sv[m][1:] <= 1e-12 * sv[m][0])
    L = min(M, N)
    q, r = la.qr_decomp(a[0] if M >= N else a[0].T.copy())
    assert np.abs(q.T @ q - np.eye(L)).max() <= 4 * EPS * max(M, N)
    assert np.abs(q @ r - (a[0] if M >= N else a[0].T)).max() <= 1e-13 * max(M, N)
@pytest.mark.parametrize("batch,M,r", [(3, 1500, 350), (24, 1500, 350), (3, 1000, 350), (24, 2048, 350)])
def test_batched_tall_rank_deficient_members(batch, M, r):
    """rank-deficient tall members (N = 700): the row-split QR panel that straddles the rank is flagged and factorised by the classic
    kernel, so the next panel needs X = V^T C over all rows. It used to form X inside its own launch while the other row workgroups
    of that launch were already updating their rows of C: with a batch (more workgroups than run at once) columns from 352 on came
    out wrong (|QR - A| up to 0.5) for some members, identical members included. qr_decomp and svd_decomp, every member"""
    from nd4js_amd import la
    N = 700
    a = np.stack([rng.matrix(26000 + m % 3, M, r) @ rng.matrix(26100 + m % 3, r, N) for m in range(batch)])
    q, rr = la.qr_decomp(a)
    for m in range(batch):
        assert np.abs(q[m] @ rr[m] - a[m]).max() <= 1e-12 * np.abs(a[m]).max() * M
        assert np.abs(q[m].T @ q[m] - np.eye(N)).max() <= 4 * EPS * M
    u, sv, v, _ = dev_svd(a)
    for m in range(batch):
        check_member(a[m], u[m], sv[m], v[m], slack=4.0)
        assert np.all(sv[m][r:] <= 1e-10 * sv[m][0])
