"""Pins the CPU oracle (oracle/nd4_oracle.c) to the REAL reference: every golden fixture under
tests/golden/ was produced by /root/reference/dist/nd.js (oracle/gen_golden.js).

matmul / Givens-QR / LU restate the reference's exact operation order -> bit-identical.
The two-sided Jacobi SVD calls libm atan2/cos/sin (V8 uses its own fdlibm port) -> 1e-12.
"""
import numpy as np
import pytest

import oracle
from conftest import golden_cases
from families import make_input
from nd4js_amd import rng


def test_rng_matches_js_and_c(golden):
    g = golden("rng")
    u_js = g["u"]
    assert np.array_equal(rng.fill_uniform(g.seed, g.n, g.offset), u_js)
    assert np.array_equal(oracle.fill_uniform(g.seed, g.n, g.offset), u_js)
    big = rng.fill_uniform(7, 1 << 16)
    assert np.array_equal(big, oracle.fill_uniform(7, 1 << 16))
    assert big.min() >= -1.0 and big.max() < 1.0 and abs(big.mean()) < 0.02


@pytest.mark.parametrize("name", [c for c in golden_cases(op="matmul2") if not c.startswith("c2_")])
def test_matmul_bit_exact(golden, name):
    g = golden(name)
    a = rng.matrix(g.seedA, *g.shapeA)
    b = rng.matrix(g.seedB, *g.shapeB)
    c = oracle.matmul2(a, b)
    ref = g["C"]
    assert c.shape == ref.shape == tuple(g.shapeC)
    assert np.array_equal(c, ref)


def test_matmul_errors():
    with pytest.raises(ValueError, match="do not match"):
        oracle.matmul2(np.ones((2, 3)), np.ones((4, 2)))
    with pytest.raises(ValueError, match="broadcast"):
        oracle.matmul2(np.ones((2, 2, 3)), np.ones((3, 3, 2)))


@pytest.mark.parametrize("name", [c for c in golden_cases(op="qr_decomp") if not c.startswith(("c3_", "c3b_"))])
def test_qr_bit_exact(golden, name):
    g = golden(name)
    a = make_input(g.seed, g.shape, g.family)
    q, r = oracle.qr_decomp(a)
    assert q.shape == g["Q"].shape and r.shape == g["R"].shape
    assert np.array_equal(q, g["Q"])
    assert np.array_equal(r, g["R"])


@pytest.mark.parametrize("name", golden_cases(op="qr_decomp_full"))
def test_qr_full_bit_exact(golden, name):
    g = golden(name)
    a = make_input(g.seed, g.shape, g.family)
    q, r = oracle.qr_decomp_full(a)
    assert np.array_equal(q, g["Q"])
    assert np.array_equal(r, g["R"])


@pytest.mark.parametrize("name", [c for c in golden_cases(op="lu_decomp") if not c.startswith(("c3_", "c3b_"))])
def test_lu_bit_exact(golden, name):
    g = golden(name)
    a = make_input(g.seed, g.shape, g.family)
    lu, p = oracle.lu_decomp(a)
    assert np.array_equal(p, g["P"])
    assert np.array_equal(lu, g["LU"], equal_nan=True)


@pytest.mark.parametrize("name", golden_cases(op="svd_jac_2sided"))
def test_svd_jac_2sided_matches_reference(golden, name):
    g = golden(name)
    a = make_input(g.seed, g.shape, g.family)
    u, sv, v, _ = oracle.svd_jac_2sided(a)
    ref_sv = g["sv"]
    smax = max(ref_sv.max(), 1e-300)
    assert np.abs(sv - ref_sv).max() <= 1e-12 * smax
    if g.family in ("dense", "sparse10"):          # unique vectors: compare values too
        assert np.abs(u - g["U"]).max() <= 1e-9
        assert np.abs(v - g["V"]).max() <= 1e-9
    # always: the reference's own acceptance properties (_generic_test_svd_decomp.js:85-154)
    N = a.shape[-1]
    eps = 2.0 ** -52
    rec = np.einsum("...ik,...k,...kj->...ij", u, sv, v)
    assert np.linalg.norm(rec - a) <= 48 * eps * N * max(np.linalg.norm(a), 1e-300) * np.sqrt(a.size / (N * N))
    assert np.all(sv >= 0) and np.all(np.diff(sv, axis=-1) <= 0)
    eye = np.eye(N)
    assert np.abs(np.swapaxes(u, -1, -2) @ u - eye).max() <= 4 * eps * N
    assert np.abs(v @ np.swapaxes(v, -1, -2) - eye).max() <= 4 * eps * N


@pytest.mark.parametrize("name", [c for c in golden_cases(op="svd_decomp") if not c.startswith(("c4_", "c5_"))])
def test_svd_dc_matches_reference(golden, name):
    """oracle/nd4_oracle_svd_dc.c restates the reference's svd_decomp (= svd_dc, svd_dc.js:37-932: bidiagonalisation + divide &
    conquer) statement by statement; against the reference's own U, sv, V on square, wide, tall, batched and edge-family inputs.
    Bit-identical wherever the 2 x 3 base case's atan2 / sin / cos agree between V8 and libm (c1_svd32, wide, diagonal, 1 x 1);
    elsewhere 1e-13 — including the SIGNS of every singular vector (nothing is re-normalised)."""
    g = golden(name)
    a = make_input(g.seed, g.shape, g.family)
    u, sv, v = oracle.svd_dc(a)
    smax = max(g["sv"].max(), 1e-300)
    assert u.shape == g["U"].shape and v.shape == g["V"].shape
    assert np.abs(sv - g["sv"]).max() <= 1e-13 * smax
    assert np.abs(u - g["U"]).max() <= 1e-13 and np.abs(v - g["V"]).max() <= 1e-13


def test_svd_dc_c5_members(golden):
    """Members 0, 16, 32 of BASELINE configs[4] (512 x 512, seeds 1000 + b) against the reference's singular values."""
    from nd4js_amd import rng
    g = golden("c5_svd512")
    members, ref = g["members"], g["sv"]
    for k in range(3):
        a = rng.matrix(g.seed_base + int(members[k]), 512, 512)
        _, sv, _ = oracle.svd_dc(a)
        assert np.abs(sv - ref[k]).max() <= 1e-12 * ref[k].max()


@pytest.mark.parametrize("name", [c for c in golden_cases(op="svd_decomp") if c.startswith(("c1_", "mid_svd96", "b_svd", "edge_svd_"))])
def test_jacobi_sv_equal_svd_decomp_sv(golden, name):
    """The oracle's Jacobi sv must equal the sv of svd_decomp (= svd_dc, the public function)."""
    g = golden(name)
    if g.shape[-1] != g.shape[-2]:
        pytest.skip("square only")
    a = make_input(g.seed, g.shape, g.family)
    _, sv, _, _ = oracle.svd_jac_2sided(a)
    ref = g["sv"]
    assert np.abs(sv - ref).max() <= 1e-12 * ref.max()


def test_big_configs_sampled(golden):
    """C3 (2048^2 LU): the oracle reproduces the reference's permutation and sampled entries exactly
    (the full C2/C4/C5 runs are too slow for the CPU suite; their fixtures gate the GPU tests)."""
    g = golden("c3_lu2048")
    a = rng.matrix(g.seed, *g.shape)
    lu, p = oracle.lu_decomp(a)
    assert np.array_equal(p, g["P"])
    assert np.array_equal(lu.reshape(-1)[g["LUidx"]], g["LUval"])
    assert np.isclose(np.linalg.norm(lu), g.froLU, rtol=1e-14)


# ---- solve-side consumers (lu.js:84-177, tri.js:45-290) ----
from families import triangle  # noqa: E402


@pytest.mark.parametrize("name", golden_cases(op="lu_solve"))
def test_lu_solve_bit_exact(golden, name):
    g = golden(name)
    lu, p = oracle.lu_decomp(rng.matrix(g.seedA, *g.shapeA))
    x = oracle.lu_solve(lu, p, rng.matrix(g.seedY, *g.shapeY))
    assert x.shape == g["X"].shape and np.array_equal(x, g["X"])


@pytest.mark.parametrize("name", golden_cases(op="triu_solve") + golden_cases(op="tril_solve"))
def test_tri_solve_bit_exact(golden, name):
    g = golden(name)
    upper = g.op == "triu_solve"
    t = triangle(g.seedT, g.shapeT, upper)
    x = (oracle.triu_solve if upper else oracle.tril_solve)(t, rng.matrix(g.seedY, *g.shapeY))
    assert x.shape == g["X"].shape and np.array_equal(x, g["X"])


# ---- least-squares consumers (qr.js:186-273, svd.js:66-228) ----
@pytest.mark.parametrize("name", golden_cases(op="qr_lstsq"))
def test_qr_lstsq_bit_exact(golden, name):
    g = golden(name)
    a = rng.matrix(g.seedA, *g.shapeA)
    q, r = (oracle.qr_decomp_full if g.full else oracle.qr_decomp)(a)
    x = oracle.qr_lstsq(q, r, rng.matrix(g.seedY, *g.shapeY))
    assert x.shape == g["X"].shape and np.array_equal(x, g["X"])


@pytest.mark.parametrize("name", golden_cases(op="svd_lstsq") + golden_cases(op="svd_solve"))
def test_svd_lstsq_bit_exact(golden, name):
    g = golden(name)
    x = oracle.svd_lstsq(g["U"], g["sv"], g["V"], rng.matrix(g.seedY, *g.shapeY))
    assert x.shape == g["X"].shape and np.array_equal(x, g["X"])


def test_lstsq_errors():
    with pytest.raises(ValueError, match="Q and y don't match"):
        oracle.qr_lstsq(np.ones((4, 3)), np.ones((3, 3)), np.ones((5, 1)))
    with pytest.raises(ValueError, match="Under-determined"):
        oracle.qr_lstsq(np.ones((3, 3)), np.ones((3, 5)), np.ones((3, 1)))
    with pytest.raises(ValueError, match="NaN or Infinity"):
        oracle.svd_lstsq(np.eye(2), np.array([1.0, np.nan]), np.eye(2), np.ones((2, 1)))


# ---- _qr_decomp_inplace (qr.js:146-183), pinned through the reference's own test oracle ----
@pytest.mark.parametrize("name", golden_cases(op="qr_decomp_inplace"))
def test_qr_decomp_inplace_matches_reference_test_oracle(golden, name):
    g = golden(name)
    M, N = g.shapeA
    a = rng.matrix(g.seedA, M, N)
    if g.sparse:
        a[rng.matrix(g.seedA + 1000, M, N) > 0.8] = 0.0
    y = rng.matrix(g.seedY, M, g.L)
    r, qty = oracle.qr_decomp_inplace(a, y)
    assert np.array_equal(np.tril(r, -1), np.zeros_like(r))             # toBeUpperTriangular (qr_test.js:223)
    assert np.array_equal(r, g["R"])                                      # same rotations as qr_decomp_full -> same bits
    assert np.abs(qty - g["QtY"]).max() <= 1e-13 * max(np.abs(y).max(), 1) * M
    qf, rf = oracle.qr_decomp_full(a)                                     # and the oracle's own qr_decomp_full is the reference's
    assert np.array_equal(qf, g["Q"]) and np.array_equal(rf, g["R"])


# ---- Cholesky (cholesky.js:27-150) ----
from families import spd  # noqa: E402


@pytest.mark.parametrize("name", golden_cases(op="cholesky_decomp"))
def test_cholesky_bit_exact(golden, name):
    g = golden(name)
    L = oracle.cholesky_decomp(spd(g.seed, tuple(g.shape)))
    assert np.array_equal(L, g["L"])
    if "X" in g.files:
        x = oracle.cholesky_solve(L, rng.matrix(g.seedY, *g.shapeY))
        assert x.shape == g["X"].shape and np.array_equal(x, g["X"])


def test_cholesky_errors():
    with pytest.raises(ValueError, match="near\\) singular"):
        oracle.cholesky_decomp(np.array([[1.0, 2.0], [2.0, 1.0]]))
    with pytest.raises(ValueError, match="quadratic"):
        oracle.cholesky_decomp(np.ones((2, 3)))
    with pytest.raises(ValueError, match="L and y don't match"):
        oracle.cholesky_solve(np.eye(3), np.ones((4, 1)))


# ---- LDL^T (ldl.js:47-201) ----
from families import sym_indefinite  # noqa: E402


@pytest.mark.parametrize("name", golden_cases(op="ldl_decomp"))
def test_ldl_bit_exact(golden, name):
    g = golden(name)
    LD = oracle.ldl_decomp(sym_indefinite(g.seed, tuple(g.shape)))
    assert np.array_equal(LD, g["LD"])
    if "X" in g.files:
        x = oracle.ldl_solve(LD, rng.matrix(g.seedY, *g.shapeY))
        assert x.shape == g["X"].shape and np.array_equal(x, g["X"])


# ---- hessenberg_decomp (hessenberg.js:27-115) ----
from families import hess_input  # noqa: E402


@pytest.mark.parametrize("name", golden_cases(op="hessenberg_decomp"))
def test_hessenberg_bit_exact(golden, name):
    g = golden(name)
    u, h = oracle.hessenberg_decomp(hess_input(g.seed, tuple(g.shape), g.family))
    assert np.array_equal(u, g["U"]) and np.array_equal(h, g["H"])


# ---- bidiag_decomp (bidiag.js:32-319) ----
def bidiag_input(g):
    a = rng.matrix(g.seed, *g.shape)
    if g.sparse:
        a[rng.matrix(g.seed + 1000, *g.shape) > 0.6] = 0.0
    return a


@pytest.mark.parametrize("name", golden_cases(op="bidiag_decomp"))
def test_bidiag_bit_exact(golden, name):
    g = golden(name)
    u, b, v = oracle.bidiag_decomp(bidiag_input(g))
    assert u.shape == g["U"].shape and b.shape == g["B"].shape and v.shape == g["V"].shape
    assert np.array_equal(b, g["B"]) and np.array_equal(u, g["U"]) and np.array_equal(v, g["V"])


# ---- 2048^2-class fixtures of the reductions (gen_golden.js c6): sampled, the full factors are 32 MB each ----
def test_hessenberg_2048_sampled(golden):
    """The oracle's Hessenberg reduction reproduces the reference's at 2048^2 bit for bit: both diagonals in full, entries sampled from
    the band j >= i - 1 of H and from U, the row sums of 64 rows. The GPU tests at this size compare with these fixtures, and at
    1025 / 1536 with the oracle directly."""
    g = golden("c6_hess2048")
    u, h = oracle.hessenberg_decomp(rng.matrix(g.seed, *g.shape))
    assert np.array_equal(np.diagonal(h), g["diagH"]) and np.array_equal(np.diagonal(h, -1), g["subH"])
    assert np.array_equal(h.reshape(-1)[g["Hidx"]], g["Hval"]) and np.array_equal(u.reshape(-1)[g["Uidx"]], g["Uval"])
    rows = g["rows"]
    assert np.array_equal(np.cumsum(h[rows], axis=1)[:, -1], g["Hrowsum"])          # summed left to right, as the generator does
    assert np.array_equal(np.cumsum(u[rows], axis=1)[:, -1], g["Urowsum"])
    assert np.isclose(np.linalg.norm(h), g.froH, rtol=1e-14)


def test_bidiag_2048_sampled(golden):
    """The same for the bidiagonal reduction at 2048^2: both diagonals of B in full, sampled entries of U and V."""
    g = golden("c6_bidiag2048")
    u, b, v = oracle.bidiag_decomp(rng.matrix(g.seed, *g.shape))
    assert b.shape == tuple(g.shapeB)
    assert np.array_equal(np.diagonal(b), g["diagB"]) and np.array_equal(np.diagonal(b, 1), g["superB"])
    assert np.array_equal(u.reshape(-1)[g["Uidx"]], g["Uval"]) and np.array_equal(v.reshape(-1)[g["Vidx"]], g["Vval"])
    assert np.isclose(np.linalg.norm(b), g.froB, rtol=1e-14)
