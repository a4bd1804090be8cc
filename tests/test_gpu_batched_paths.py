"""Batched kernel paths of cholesky_decomp, ldl_decomp, hessenberg_decomp and bidiag_decomp (and of the two triangular solves behind
cholesky_solve / ldl_solve), checked member by member against the oracle.

These four factorisations choose their kernels from the BATCH SIZE as well as from N, so a multi-matrix path can be wrong in one
member's offset or share one member's scratch with another while every single-matrix test passes. The `dev` forms hand the batch to
the kernels unchanged, so the cases below reach each path by shape alone. The host forms (`la.*`) cut a batch into chunks first
(`_host_chunk`); the last group of tests relies on that.

Case -> path -> condition in the source (CB = 32):

  cholesky_decomp (chol.hip: nd4_potrf)
    (8, 256^2), (16, 512^2), (256, 256^2)       look-ahead: chol_diag_la + fused chol_trsm_narrow     N >= 128, N % 32 == 0, batch*N <= 65536
    (8, 300^2)                                  look-ahead: chol_diag_la + chol_trsm + narrow GEMM    N >= 128, N % 32 != 0, batch*N <= 65536
    (300, 300^2), (70, 1100^2), (257, 256^2),   chol_diag + chol_trsm + nd4_syrk_lower over several    batch*N > 65536
    (160, 512^2)                                128^2 tiles
  ldl_decomp (chol.hip: nd4_ldltrf)
    (8, 256^2), (256, 256^2)                    look-ahead: chol_diag_la<true> + chol_trsm_narrow     N >= 128, N % 32 == 0, batch*N <= 65536
    (6, 300^2)                                  ldl_diag + ldl_trsm + nd4_gemm_nt_lower               N % 32 != 0
    (300, 256^2), (257, 256^2), (160, 512^2)    ldl_diag + ldl_trsm + nd4_gemm_nt_lower               batch*N > 65536
  hessenberg_decomp (hess.hip: nd4_gehrd; a batch of 2 or more never takes the one-launch or the blocked single-matrix form)
    (2, 256^2), (3, 256^2), (4, 256^2),         hess_vec / hess_pass_a / hess_reduce / hess_pass_b,    2 <= batch <= 4, N >= 256
    (3, 257^2), (4, 512^2), (4, 1024^2)         U formed by nd4_wy_form per member
    (5, 256^2), (6, 256^2), (8, 256^2),         the same step kernels, U updated in every step         batch > 4 or N < 256
    (6, 384^2), (3, 255^2), (12, 768^2)
  bidiag_decomp (bidiag.hip: nd4_gebrd; a batch of 2 or more always takes the unfused bd_vec_col / bd_vec_row loop)
    (3, 256^2), (4, 256^2), (2, 300x260),       U, V formed by nd4_wy_form per member (shared VRt /    batch <= 4, K = min(M, N) >= 256
    (4, 260x300), (2, 512^2)                    Vt scratch)
    (5, 256^2), (6, 256^2), (8, 256^2),         U, V accumulated by reflect_left / reflect_right       batch > 4 or K < 256
    (6, 300x280), (8, 270x300), (3, 255^2), (12, 768^2)
  host forms (la.*; chunk sizes derived above test_host_chunk_sizes)
    hessenberg 12 x 768^2 -> calls of 4 (WY), bidiag 12 x 768^2 -> calls of 3 (WY), cholesky / ldl 160 x 512^2 -> calls of 20 (look-ahead)
  cholesky_solve / ldl_solve (trsm.hip: nd4_trsm_ld, nd4_trsm_t_ex), 6 members, 7 columns
    N = 256, 512                                one launch per panel: trsm_cols (+ tri_inv_blocks)    N >= 256, N % 32 == 0, J*batch >= 32
    N = 300                                     tri_block_solve + GEMM per 32 rows                    N % 32 != 0

Tolerances are those of the single-matrix test of the same op (test_gpu_chol.py, test_gpu_hess.py, test_gpu_bidiag.py), never
looser. The oracle runs on a fixed sample of members (first, last and seeded others, at least 8); the properties hold on every member.
"""
import numpy as np
import pytest

import oracle
from nd4js_amd import rng

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -52


# ------------------------------------------------------------------------------------------------------------------------ helpers
def _dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _host(*ts):
    out = tuple(t.cpu().numpy() for t in ts)
    return out if len(out) > 1 else out[0]


def _fro(x):
    """Frobenius norm without overflow at 1e150 scales"""
    s = np.abs(x).max() if x.size else 0.0
    return 0.0 if s == 0 else float(s * np.linalg.norm((x / s).ravel()))


def relerr(x, ref):
    return _fro(x - ref) / max(_fro(ref), 1e-300)


def _scale(x):
    """1 for the ordinary members, the magnitude of a member scaled by 1e150 or 1e-150"""
    s = np.abs(x).max()
    return 1.0 if s == 0 or 1e-100 < s < 1e100 else s


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


def _host_chunk(batch, per_item_bytes, chunk_bytes=64 << 20, max_chunks=8, min_chunk=1):
    """members per kernel call of a host-pointer entry point on one device: nd4hip_host.hip run_block with the default Plan"""
    n = -(-per_item_bytes * batch // chunk_bytes)
    n = max(1, min(n, max_chunks, batch // min_chunk))
    return -(-batch // n)


# ------------------------------------------------------------------------------------------------------------------- Cholesky
def _spd(seed, batch, N):
    """S = B B^T + N I (as test_cholesky_sizes); only the lower triangle is read by both the kernels and the oracle"""
    B = rng.matrix(seed, batch, N, N)
    S = B @ np.swapaxes(B, -1, -2)
    S[:, np.arange(N), np.arange(N)] += N
    return S


def _cond_spd(S):
    w = np.linalg.eigvalsh(S / _scale(S))
    return w[-1] / w[0]


def _check_chol(S, L, with_oracle):
    """test_cholesky_golden / test_cholesky_sizes: exact zeros above the diagonal, ||L L^T - S|| <= 8 eps N ||S||, L against the oracle"""
    N = S.shape[-1]
    assert np.array_equal(np.triu(L, 1), np.zeros_like(L)) and np.all(np.diag(L) > 0)
    assert _fro(L @ L.T - S) <= 8 * EPS * N * _fro(S)
    if with_oracle:
        assert relerr(L, oracle.cholesky_decomp(S)) <= 1e-14 * max(_cond_spd(S), 10)


def _chol_batch_checked(S, seed):
    L = _host(_dev_chol(S))
    samp = set(_sample(len(S), seed))
    for m in range(len(S)):
        _check_chol(S[m], L[m], m in samp)
    return L


def _dev_chol(S):
    from nd4js_amd import dev
    return dev.cholesky_decomp(_dev(S))


CHOL_CASES = [(8, 256), (16, 512), (8, 300), (300, 300), (70, 1100)]


@pytest.mark.parametrize("batch,N", CHOL_CASES)
def test_cholesky_paths(batch, N):
    """every member of a batch on each of the three Cholesky paths; the reversed batch gives every member bit for bit"""
    S = _spd(11000 + N + batch, batch, N)
    L = _chol_batch_checked(S, 11100 + N)
    Lr = _host(_dev_chol(S[::-1]))
    assert np.array_equal(Lr[::-1], L)


def _chol_specials(N, seed):
    """positive definite members that are not dense: identity, 1e150 / 1e-150 scales, rank 8 update of I, a diagonal matrix, zero rows
    and columns off the diagonal (a zero or rank-deficient member is not positive definite and raises: test_cholesky_not_pd)"""
    base = _spd(seed, 1, N)[0]
    W = rng.matrix(seed + 1, N, 8)
    zrc = base.copy()
    for k in (3, 40, N - 1):
        d = zrc[k, k]
        zrc[k, :] = 0.0
        zrc[:, k] = 0.0
        zrc[k, k] = d
    return [np.eye(N), base * 1e150, base * 1e-150, np.eye(N) + W @ W.T, np.diag(1.0 + np.abs(rng.matrix(seed + 2, N).ravel())), zrc]


@pytest.mark.parametrize("batch,N", [(8, 256), (8, 300), (257, 256)])
def test_cholesky_mixed_batch(batch, N):
    """special members beside dense ones on each path: each meets the single-matrix check"""
    S = _spd(11200 + N + batch, batch, N)
    sp = _chol_specials(N, 11300 + N)
    pos = np.linspace(0, batch - 1, len(sp)).astype(int)
    for p, s in zip(pos, sp):
        S[p] = s
    L = _host(_dev_chol(S))
    samp = set(_sample(batch, 11400)) | set(pos.tolist())
    for m in range(batch):
        _check_chol(S[m], L[m], m in samp)
    assert np.array_equal(L[pos[0]], np.eye(N))


@pytest.mark.parametrize("where", ["first", "middle", "last"])
@pytest.mark.parametrize("batch,N", [(8, 256), (8, 300), (257, 256)])
def test_cholesky_not_pd(batch, N, where):
    """one member not positive definite raises the reference's error on each path; the next call on the same handle is right"""
    S = _spd(11500 + N, batch, N)
    good = _host(_dev_chol(S))
    k = {"first": 0, "middle": batch // 2, "last": batch - 1}[where]
    bad = S.copy()
    bad[k, N // 2 + 1, N // 2 + 1] = -1.0
    with pytest.raises(ValueError, match="Matrix contains NaNs or is \\(near\\) singular."):
        _dev_chol(bad)
    assert np.array_equal(_host(_dev_chol(S)), good)
    for m in _sample(batch, 11600, k=3):
        _check_chol(S[m], good[m], True)


# ------------------------------------------------------------------------------------------------------------------------ LDL^T
def _ldl_factors(seed, batch, N):
    """L0 unit lower (entries / 4), D0 = +-(1 + |u|): test_ldl_sizes's construction for N <= 512"""
    r = rng.matrix(seed, batch, N, N)
    idx = np.arange(N)
    L0 = np.tril(r * 0.25, -1) + np.eye(N)
    dr = r[:, idx, idx]
    d0 = np.where(dr >= 0, 1 + dr, -1 + dr)
    return L0, d0


def _ldl_compose(L0, d0):
    return (L0 * d0[..., None, :]) @ np.swapaxes(L0, -1, -2)


def _unpack(LD):
    N = LD.shape[-1]
    idx = np.arange(N)
    L = np.tril(LD, -1)
    L[..., idx, idx] = 1.0
    return L, LD[..., idx, idx]


def _check_ldl(S, LD, L0, d0, with_oracle):
    """test_ldl_sizes: exact zeros above, ||L D L^T - S|| <= 64 eps N ||S||, (L, D) recovered to 1e-9 (relative to |D| for a scaled
    member), LD against the oracle to 4 eps cond"""
    N = S.shape[-1]
    L, d = _unpack(LD)
    assert np.array_equal(np.triu(LD, 1), np.zeros_like(LD))
    assert _fro((L * d) @ L.T - S) <= 64 * EPS * N * _fro(S)
    assert np.abs(L - L0).max() <= 1e-9 and np.abs(d - d0).max() <= 1e-9 * _scale(d0)
    if with_oracle:
        assert relerr(LD, oracle.ldl_decomp(S)) <= 4 * EPS * max(np.linalg.cond(S / _scale(S)), 100)


def _dev_ldl(S):
    from nd4js_amd import dev
    return dev.ldl_decomp(_dev(S))


def _ldl_batch_checked(S, L0, d0, seed, extra=()):
    LD = _host(_dev_ldl(S))
    samp = set(_sample(len(S), seed)) | set(extra)
    for m in range(len(S)):
        _check_ldl(S[m], LD[m], L0[m], d0[m], m in samp)
    return LD


LDL_CASES = [(8, 256), (6, 300), (300, 256)]


@pytest.mark.parametrize("batch,N", LDL_CASES)
def test_ldl_paths(batch, N):
    L0, d0 = _ldl_factors(12000 + N + batch, batch, N)
    S = _ldl_compose(L0, d0)
    LD = _ldl_batch_checked(S, L0, d0, 12100 + N)
    assert np.array_equal(_host(_dev_ldl(S[::-1]))[::-1], LD)


@pytest.mark.parametrize("batch,N", [(8, 256), (6, 300), (257, 256)])
def test_ldl_mixed_batch(batch, N):
    """identity, a diagonal D with both signs, 1e150 / 1e-150 scales, L with a rank 8 strict lower part, zero rows and columns off the
    diagonal: every one with known (L0, D0)"""
    L0, d0 = _ldl_factors(12200 + N + batch, batch, N)
    idx = np.arange(N)
    sp_L, sp_d = [], []
    sp_L.append(np.eye(N)); sp_d.append(np.ones(N))
    sp_L.append(np.eye(N)); sp_d.append(d0[1].copy())
    sp_L.append(L0[2].copy()); sp_d.append(d0[2] * 1e150)
    sp_L.append(L0[3].copy()); sp_d.append(d0[3] * 1e-150)
    lr = np.tril(0.05 * rng.matrix(12300, N, 8) @ rng.matrix(12301, 8, N), -1) + np.eye(N)
    sp_L.append(lr); sp_d.append(d0[4].copy())
    zl = L0[5].copy()
    for k in (3, 40, N - 1):
        zl[k, :] = 0.0
        zl[:, k] = 0.0
        zl[k, k] = 1.0
    sp_L.append(zl); sp_d.append(d0[5].copy())
    pos = np.linspace(0, batch - 1, len(sp_L)).astype(int)
    for p, l, d in zip(pos, sp_L, sp_d):
        L0[p], d0[p] = l, d
    S = _ldl_compose(L0, d0)
    assert np.array_equal(S[pos[0]], np.eye(N)) and np.all(S[pos[1]][~np.eye(N, dtype=bool)] == 0)
    LD = _ldl_batch_checked(S, L0, d0, 12400, extra=pos.tolist())
    assert np.array_equal(LD[pos[0]], np.eye(N)) and np.array_equal(LD[pos[1]][idx, idx], d0[pos[1]])


def test_cholesky_ldl_batchN_boundary():
    """batch*N = 65536 (look-ahead) against 65792 (chol_diag / ldl_diag + tile-skipping GEMM) at 256^2, the same 256 members on both
    sides plus one; each side against the oracle at the single-matrix tolerances (Cholesky 1e-14 cond, LDL^T 4 eps cond)"""
    N = 256
    S = _spd(12500, 257, N)
    _chol_batch_checked(S[:256], 12501)
    _chol_batch_checked(S, 12501)
    L0, d0 = _ldl_factors(12502, 257, N)
    T = _ldl_compose(L0, d0)
    _ldl_batch_checked(T[:256], L0[:256], d0[:256], 12503)
    _ldl_batch_checked(T, L0, d0, 12503, extra=(256,))


# ------------------------------------------------------------------------------------------------------------------ Hessenberg
def hess_props(a, u, h):
    """test_gpu_hess.check_props on one member; a scaled member is checked on its unscaled twin (a / s, h / s)"""
    from test_gpu_hess import check_props
    s = _scale(a)
    check_props(a / s, u, h / s)


def hess_oracle(a, u, h):
    """test_one_launch_reduction_sizes's bounds"""
    N = a.shape[-1]
    uo, ho = oracle.hessenberg_decomp(a)
    assert np.abs(h - ho).max() <= 64 * EPS * N * np.abs(a).max() * N ** 0.5
    assert np.abs(u - uo).max() <= 64 * EPS * N


def _dev_hess(a):
    from nd4js_amd import dev
    return _host(*dev.hessenberg_decomp(_dev(a)))


def _hess_batch_checked(a, seed, extra=()):
    u, h = _dev_hess(a)
    samp = set(_sample(len(a), seed)) | set(extra)
    for m in range(len(a)):
        hess_props(a[m], u[m], h[m])
        if m in samp:
            hess_oracle(a[m], u[m], h[m])
    return u, h


HESS_CASES = [(2, 256), (3, 257), (4, 512), (4, 1024), (5, 256), (6, 384)]


@pytest.mark.parametrize("batch,N", HESS_CASES)
def test_hessenberg_paths(batch, N):
    a = rng.matrix(13000 + N + batch, batch, N, N)
    u, h = _hess_batch_checked(a, 13100)
    ur, hr = _dev_hess(a[::-1])
    assert np.array_equal(ur[::-1], u) and np.array_equal(hr[::-1], h)


def test_hessenberg_batch_boundary():
    """batch 4 (WY-formed U) against 5 (explicit U) at 256^2, and N = 255 (explicit) against 256 (WY) at batch 3: same members on both
    sides, each side against the oracle at test_one_launch_reduction_sizes's bounds"""
    a = rng.matrix(13200, 5, 256, 256)
    _hess_batch_checked(a[:4], 13201)
    _hess_batch_checked(a, 13201)
    b = rng.matrix(13202, 3, 256, 256)
    _hess_batch_checked(np.ascontiguousarray(b[:, :255, :255]), 13203)
    _hess_batch_checked(b, 13203)


def _square_specials(N, seed, skip_form):
    """zero, identity, 1e150 / 1e-150 scales, rank 8, zero rows and columns, and a member in which every step is skipped"""
    base = rng.matrix(seed, N, N)
    zc = base.copy()
    zc[:, 5] = 0.0
    zc[17, :] = 0.0
    zc[:, 200:210] = 0.0
    return {"zeros": np.zeros((N, N)), "identity": np.eye(N), "1e150": base * 1e150, "1e-150": base * 1e-150,
            "rank 8": rng.matrix(seed + 1, N, 8) @ rng.matrix(seed + 2, 8, N), "zero rows and columns": zc, "skip": skip_form(base)}


def _hess_special_check(name, a, u, h):
    """test_one_launch_reduction_special_inputs, plus test_hessenberg_golden's every-step-skipped member: nothing changes"""
    N = a.shape[-1]
    sc = max(np.abs(a).max(), 1e-300)
    assert np.isfinite(h).all() and np.isfinite(u).all(), name
    assert np.abs(u @ h @ u.T - a).max() <= 256 * EPS * N * sc, name
    assert np.abs(u @ u.T - np.eye(N)).max() <= 16 * EPS * N, name
    assert np.abs(np.tril(h, -2)).max() == 0.0, name
    if name == "skip":
        assert np.array_equal(h, a) and np.array_equal(u, np.eye(N)), name


@pytest.mark.parametrize("batch", [4, 8])
def test_hessenberg_mixed_batch(batch):
    """special members beside dense ones; batch 4 (WY, two calls to place all seven specials) and 8 (explicit U)"""
    N = 256
    sp = list(_square_specials(N, 13300, lambda b: np.triu(b, -1)).items())
    dense = rng.matrix(13310, batch, N, N)
    groups = [sp[:3], sp[3:6], sp[6:]] if batch == 4 else [sp]
    for g in groups:
        a = dense.copy()
        pos = np.arange(1, 1 + len(g))
        for p, (_, x) in zip(pos, g):
            a[p] = x
        u, h = _dev_hess(a)
        for m in range(batch):
            if m in pos:
                name = g[m - 1][0]
                _hess_special_check(name, a[m], u[m], h[m])
            else:
                hess_props(a[m], u[m], h[m])
                hess_oracle(a[m], u[m], h[m])


@pytest.mark.parametrize("batch", [3, 6])
def test_hessenberg_nan_member_stays_in_its_member(batch):
    """NaN in one member (WY path at batch 3, explicit at 6): every other member bit-identical to the call without it"""
    N = 256
    a = rng.matrix(13400 + batch, batch, N, N)
    u, h = _dev_hess(a)
    k = batch // 2
    bad = a.copy()
    bad[k, N - 1, 7] = np.nan
    ub, hb = _dev_hess(bad)
    others = [m for m in range(batch) if m != k]
    assert np.array_equal(ub[others], u[others]) and np.array_equal(hb[others], h[others])
    assert not np.array_equal(hb[k], h[k])


# --------------------------------------------------------------------------------------------------------------- bidiagonal
def bd_props(a, u, b, v):
    """test_gpu_bidiag.check_props on one member, a scaled member on its unscaled twin"""
    from test_gpu_bidiag import check_props
    s = _scale(a)
    check_props(a / s, u, b / s, v)


def bd_oracle(a, u, b, v):
    """test_bidiag_shapes_vs_oracle's bounds: B, U, V against the oracle, singular values against LAPACK's"""
    M, N = a.shape
    uo, bo, vo = oracle.bidiag_decomp(a)
    n = max(M, N)
    assert np.abs(b - bo).max() <= 1e-11 * n and np.abs(u - uo).max() <= 1e-10 and np.abs(v - vo).max() <= 1e-10
    sv = np.linalg.svd(b, compute_uv=False)
    assert np.abs(sv - np.linalg.svd(a, compute_uv=False)[: len(sv)]).max() <= 1e-11 * max(np.abs(a).max() * n, 1)


def _dev_bd(a):
    from nd4js_amd import dev
    return _host(*dev.bidiag_decomp(_dev(a)))


def _bd_batch_checked(a, seed):
    u, b, v = _dev_bd(a)
    samp = set(_sample(len(a), seed))
    for m in range(len(a)):
        bd_props(a[m], u[m], b[m], v[m])
        if m in samp:
            bd_oracle(a[m], u[m], b[m], v[m])
    return u, b, v


BD_CASES = [(3, 256, 256), (2, 300, 260), (4, 260, 300), (2, 512, 512), (5, 256, 256), (6, 300, 280), (8, 270, 300)]


@pytest.mark.parametrize("batch,M,N", BD_CASES)
def test_bidiag_paths(batch, M, N):
    a = rng.matrix(14000 + M + N + batch, batch, M, N)
    u, b, v = _bd_batch_checked(a, 14100)
    ur, br, vr = _dev_bd(a[::-1])
    assert np.array_equal(ur[::-1], u) and np.array_equal(br[::-1], b) and np.array_equal(vr[::-1], v)


def test_bidiag_batch_boundary():
    """batch 4 (WY-formed U, V) against 5 (explicit) at 256^2, K = 255 (explicit) against 256 (WY) at batch 3: same members on both
    sides, each side against the oracle at test_bidiag_shapes_vs_oracle's bounds.
    (Seed 14200 is not used: its member 3 is not forward stable at these bounds. A relative perturbation of one ulp of the input
    moves the oracle's own B by up to 8e-9 and U, V by 7e-10, and the kernels differ from the oracle by as much on both sides.)"""
    a = rng.matrix(14204, 5, 256, 256)
    _bd_batch_checked(a[:4], 14201)
    _bd_batch_checked(a, 14201)
    b = rng.matrix(14202, 3, 256, 256)
    _bd_batch_checked(np.ascontiguousarray(b[:, :255, :255]), 14203)
    _bd_batch_checked(b, 14203)


def _bd_special_check(name, a, u, b, v):
    """test_gpu_bidiag.test_one_launch_reduction_special_inputs; an already bidiagonal member comes back unchanged (U = V = I)"""
    N = a.shape[-1]
    sc = max(np.abs(a).max(), 1e-300)
    assert np.isfinite(b).all() and np.isfinite(u).all() and np.isfinite(v).all(), name
    assert np.abs(u @ b @ v - a).max() <= 256 * EPS * N * sc, name
    assert np.abs(u.T @ u - np.eye(N)).max() <= 16 * EPS * N and np.abs(v @ v.T - np.eye(N)).max() <= 16 * EPS * N, name
    assert np.abs(np.tril(b, -1)).max() == 0.0 and np.abs(np.triu(b, 2)).max() == 0.0, name
    if name == "skip":
        assert np.array_equal(b, a) and np.array_equal(u, np.eye(N)) and np.array_equal(v, np.eye(N)), name


@pytest.mark.parametrize("batch", [4, 8])
def test_bidiag_mixed_batch(batch):
    N = 256
    sp = list(_square_specials(N, 14300, lambda b: np.triu(np.tril(b, 1))).items())
    dense = rng.matrix(14310, batch, N, N)
    groups = [sp[:3], sp[3:6], sp[6:]] if batch == 4 else [sp]
    for g in groups:
        a = dense.copy()
        pos = np.arange(1, 1 + len(g))
        for p, (_, x) in zip(pos, g):
            a[p] = x
        u, b, v = _dev_bd(a)
        for m in range(batch):
            if m in pos:
                name = g[m - 1][0]
                _bd_special_check(name, a[m], u[m], b[m], v[m])
            else:
                bd_props(a[m], u[m], b[m], v[m])
                bd_oracle(a[m], u[m], b[m], v[m])


@pytest.mark.parametrize("batch", [3, 6])
def test_bidiag_nan_member_stays_in_its_member(batch):
    N = 256
    a = rng.matrix(14400 + batch, batch, N, N)
    u, b, v = _dev_bd(a)
    k = batch // 2
    bad = a.copy()
    bad[k, 7, 0] = np.nan
    ub, bb, vb = _dev_bd(bad)
    others = [m for m in range(batch) if m != k]
    assert np.array_equal(ub[others], u[others]) and np.array_equal(bb[others], b[others]) and np.array_equal(vb[others], v[others])
    assert not np.array_equal(bb[k], b[k])


# ---------------------------------------------------------------------------------------------------------------- batched solves
SOLVE_FORMS = {"batched L, shared y": ((6,), ()), "shared L, batched y": ((), (6,)), "both batched": ((6,), (6,))}


@pytest.mark.parametrize("form", list(SOLVE_FORMS))
@pytest.mark.parametrize("N", [256, 512, 300])
def test_cholesky_solve_batched(N, form):
    """J * batch = 42 >= 32: N = 256, 512 take the one-launch trsm_cols path (shared L: one inverse of the diagonal blocks for all
    members), N = 300 the blocked one; test_cholesky_solve_vs_oracle's tolerances per member"""
    from families import spd
    from nd4js_amd import la
    lL, ly = SOLVE_FORMS[form]
    S = spd(15000 + N, lL + (N, N))
    L = np.linalg.cholesky(S)
    y = rng.matrix(15100 + N, *(ly + (N, 7)))
    x = la.cholesky_solve(L, y)
    want = oracle.cholesky_solve(L, y)
    Sb, yb = np.broadcast_to(S, (6, N, N)), np.broadcast_to(y, (6, N, 7))
    xb, wb = np.broadcast_to(x, (6, N, 7)), np.broadcast_to(want, (6, N, 7))
    assert x.shape == want.shape == (6, N, 7)
    for m in range(6):
        assert relerr(xb[m], wb[m]) <= 1e-14
        assert np.abs(Sb[m] @ xb[m] - yb[m]).max() <= 1e-12 * N
    if form == "both batched":
        from nd4js_amd import dev
        assert np.array_equal(_host(dev.cholesky_solve(_dev(L), _dev(y))), x)


@pytest.mark.parametrize("form", list(SOLVE_FORMS))
@pytest.mark.parametrize("N", [256, 512, 300])
def test_ldl_solve_batched(N, form):
    """as test_cholesky_solve_batched, at test_ldl_solve_vs_oracle's tolerances"""
    from families import sym_indefinite
    from nd4js_amd import la
    lL, ly = SOLVE_FORMS[form]
    S = sym_indefinite(15200 + N, lL + (N, N))
    LD = oracle.ldl_decomp(S)
    y = rng.matrix(15300 + N, *(ly + (N, 7)))
    x = la.ldl_solve(LD, y)
    want = oracle.ldl_solve(LD, y)
    Sb, yb = np.broadcast_to(S, (6, N, N)), np.broadcast_to(y, (6, N, 7))
    xb, wb = np.broadcast_to(x, (6, N, 7)), np.broadcast_to(want, (6, N, 7))
    assert x.shape == want.shape == (6, N, 7)
    for m in range(6):
        assert relerr(xb[m], wb[m]) <= 1e-13
        assert np.abs(Sb[m] @ xb[m] - yb[m]).max() <= 1e-10 * N
    if form == "both batched":
        from nd4js_amd import dev
        assert np.array_equal(_host(dev.ldl_solve(_dev(LD), _dev(y))), x)


# ------------------------------------------------------------------------------------------------- host forms: chunked batches
# run_block (nd4hip_host.hip, default Plan: chunk_bytes = 64 MiB, max_chunks = 8, min_chunk = 1) cuts a batch of n members moving
# p bytes each into c = min(ceil(n p / 64 MiB), 8, n) chunks of ceil(n / c) members (one device):
#   hessenberg_decomp 12 x 768^2: p = 3 N^2 8 B = 13.5 MiB -> c = ceil(162 / 64) = 3 -> 4 members per call: WY path (dev: 12, explicit)
#   bidiag_decomp     12 x 768^2: p = 4 N^2 8 B = 18 MiB   -> c = ceil(216 / 64) = 4 -> 3 members per call: WY path (dev: 12, explicit)
#   cholesky / ldl   160 x 512^2: p = 2 N^2 8 B = 4 MiB    -> c = min(10, 8) = 8   -> 20 members per call: 20 * 512 <= 65536, look-ahead
#                                                             (dev: 160 * 512 = 81920 > 65536, chol_diag / ldl_diag + tiled GEMM)
def test_host_chunk_sizes():
    assert _host_chunk(12, 3 * 768 * 768 * 8) == 4
    assert _host_chunk(12, 4 * 768 * 768 * 8) == 3
    assert _host_chunk(160, 2 * 512 * 512 * 8) == 20


def test_hessenberg_host_chunks():
    from nd4js_amd import la
    N = 768
    a = rng.matrix(16000, 12, N, N)
    u, h = la.hessenberg_decomp(a)
    ud, hd = _dev_hess(a)
    for m in range(12):
        hess_props(a[m], u[m], h[m])
        assert np.abs(h[m] - hd[m]).max() <= 64 * EPS * N * np.abs(a[m]).max() * N ** 0.5
        assert np.abs(u[m] - ud[m]).max() <= 64 * EPS * N
    for m in _sample(12, 16001):
        hess_oracle(a[m], u[m], h[m])


def test_bidiag_host_chunks():
    from nd4js_amd import la
    N = 768
    a = rng.matrix(16100, 12, N, N)
    u, b, v = la.bidiag_decomp(a)
    ud, bd, vd = _dev_bd(a)
    for m in range(12):
        bd_props(a[m], u[m], b[m], v[m])
        assert np.abs(b[m] - bd[m]).max() <= 1e-11 * N and np.abs(u[m] - ud[m]).max() <= 1e-10 and np.abs(v[m] - vd[m]).max() <= 1e-10
    for m in _sample(12, 16101):
        bd_oracle(a[m], u[m], b[m], v[m])


def test_cholesky_host_chunks():
    from nd4js_amd import la
    N = 512
    S = _spd(16200, 160, N)
    L = la.cholesky_decomp(S)
    Ld = _host(_dev_chol(S))
    samp = set(_sample(160, 16201))
    for m in range(160):
        _check_chol(S[m], L[m], m in samp)
        _check_chol(S[m], Ld[m], False)
    for m in samp:
        assert relerr(L[m], Ld[m]) <= 1e-14 * max(_cond_spd(S[m]), 10)


def test_ldl_host_chunks():
    from nd4js_amd import la
    N = 512
    L0, d0 = _ldl_factors(16300, 160, N)
    S = _ldl_compose(L0, d0)
    LD = la.ldl_decomp(S)
    LDd = _host(_dev_ldl(S))
    samp = set(_sample(160, 16301))
    for m in range(160):
        _check_ldl(S[m], LD[m], L0[m], d0[m], m in samp)
        if m in samp:
            assert relerr(LD[m], LDd[m]) <= 4 * EPS * max(np.linalg.cond(S[m]), 100)
