"""GPU parity of the matmul path through the C ABI.

Tolerance: fp64, norm-wise relative error <= 1e-10 (BASELINE.json north_star); the MFMA k-ordered
FMA chain differs from the reference's unfused i-k-j sum only in rounding, so we assert a much
tighter 1e-13 here and keep 1e-10 as the documented gate."""
import numpy as np
import pytest

import oracle
from conftest import golden_cases
from nd4js_amd import rng

pytestmark = pytest.mark.gpu
GATE = 1e-10
TIGHT = 1e-13


def relerr(x, ref):
    return np.linalg.norm((x - ref).ravel()) / max(np.linalg.norm(ref.ravel()), 1e-300)


@pytest.fixture(scope="module")
def la():
    from nd4js_amd import la as _la
    return _la


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available()
    from nd4js_amd import dev as _dev
    return _dev


@pytest.mark.parametrize("name", [c for c in golden_cases(op="matmul2") if not c.startswith("c2_")])
def test_golden_host_api(la, golden, name):
    g = golden(name)
    a = rng.matrix(g.seedA, *g.shapeA)
    b = rng.matrix(g.seedB, *g.shapeB)
    c = la.matmul2(a, b)
    ref = g["C"]
    assert c.shape == ref.shape
    assert relerr(c, ref) <= TIGHT


@pytest.mark.parametrize("shape", [(1, 1, 1), (2, 3, 5), (17, 31, 13), (128, 128, 128), (129, 17, 255),
                                   (301, 97, 203), (256, 512, 384), (100, 1000, 50), (640, 48, 640)])
def test_vs_oracle_odd_and_even_shapes(la, shape):
    I, K, J = shape
    a = rng.matrix(100 + I, I, K)
    b = rng.matrix(200 + J, K, J)
    assert relerr(la.matmul2(a, b), oracle.matmul2(a, b)) <= TIGHT


def test_batched_and_broadcast_vs_oracle(la):
    cases = [((4, 3, 33, 20), (20, 18)), ((33, 20), (5, 20, 18)), ((2, 1, 16, 8), (1, 3, 8, 24)), ((7, 40, 40), (7, 40, 40))]
    for k, (sa, sb) in enumerate(cases):
        a = rng.matrix(300 + k, *sa)
        b = rng.matrix(400 + k, *sb)
        c = la.matmul2(a, b)
        ref = oracle.matmul2(a, b)
        assert c.shape == ref.shape and relerr(c, ref) <= TIGHT


def chain_operands(g):
    if g.meta.get("hand"):
        return [g["M%d" % k] for k in range(g.n)]
    return [rng.matrix(g.seed0 + k, *s) for k, s in enumerate(g.shapes)]


@pytest.mark.parametrize("name", golden_cases(op="matmul"))
def test_matmul_chain_vs_reference_golden(la, golden, name):
    """matmul(...ms) (matmul.js:150-236) against the reference's own results: the three value-pinned cases of
    matmul_test.js:32-79 and seeded 1-5 operand chains with broadcast leading axes."""
    g = golden(name)
    c = la.matmul(*chain_operands(g))
    ref = g["C"]
    assert c.shape == ref.shape
    assert relerr(c, ref) <= TIGHT


def test_matmul_chain_hand_case_exact(la):
    assert np.array_equal(la.matmul([[1, 2, 3, 4]], [[11, 12, 13], [21, 22, 23], [31, 32, 33], [41, 42, 43]], [[5, 6], [7, 8], [9, 10]]),
                          [[6760.0, 7720.0]])          # matmul_test.js:64-79


def test_inputs_untouched_and_zero_extent(la):
    a = rng.matrix(1, 20, 20)
    b = rng.matrix(2, 20, 20)
    a0, b0 = a.copy(), b.copy()
    la.matmul2(a, b)
    assert np.array_equal(a, a0) and np.array_equal(b, b0)
    # zero extents: I = 0 and J = 0 give empty results, K = 0 an empty sum, that is zeros (also over an `out` that held NaN)
    for sa, sb, sc in (((0, 20), (20, 20), (0, 20)), ((20, 20), (20, 0), (20, 0)), ((20, 0), (0, 20), (20, 20)),
                       ((3, 5, 0), (3, 0, 7), (3, 5, 7)), ((3, 5, 0), (0, 7), (3, 5, 7)), ((2, 0, 4), (4, 7), (2, 0, 7))):
        c = la.matmul2(np.zeros(sa), np.zeros(sb))
        assert c.shape == sc and c.dtype == np.float64 and np.array_equal(c, np.zeros(sc)), (sa, sb)
        assert np.array_equal(la.matmul2(np.zeros(sa), np.zeros(sb), out=np.full(sc, np.nan)), np.zeros(sc)), (sa, sb)


def test_special_values_propagate(la):
    a = rng.matrix(3, 40, 40)
    b = rng.matrix(4, 40, 40)
    a[3, 7] = np.inf
    b[5, 9] = np.nan
    c = la.matmul2(a, b)
    ref = oracle.matmul2(a, b)
    assert np.array_equal(np.isnan(c), np.isnan(ref))
    assert np.array_equal(np.isinf(c), np.isinf(ref))


def test_device_fill_is_bit_identical(dev):
    x = dev.fill_uniform(12345, (1000,), offset=1000).cpu().numpy()
    assert np.array_equal(x, rng.fill_uniform(12345, 1000, 1000))


@pytest.mark.parametrize("ta,tb", [(0, 0), (1, 0), (0, 1), (1, 1)])
def test_gemm_ex_transposes_alpha_beta(dev, ta, tb):
    import torch
    M, N, K = 150, 94, 70
    A = rng.matrix(600, K, M) if ta else rng.matrix(600, M, K)
    B = rng.matrix(601, N, K) if tb else rng.matrix(601, K, N)
    C0 = rng.matrix(602, M, N)
    ref = 0.75 * ((A.T if ta else A) @ (B.T if tb else B)) - 0.5 * C0
    dA, dB, dC = (torch.from_numpy(x).cuda() for x in (A, B, C0))
    dev.gemm_ex(ta, tb, 0.75, dA, dB, -0.5, dC, M, N, K, A.shape[1], B.shape[1], N)
    assert relerr(dC.cpu().numpy(), ref) <= 1e-13


def test_gemm_ex_submatrix_views(dev):
    """Strided sub-blocks, as the LU/QR trailing updates use them (odd offsets -> scalar load path)."""
    import torch
    big = rng.matrix(610, 200, 200)
    d = torch.from_numpy(big.copy()).cuda()
    r0, c0, m, n, k = 33, 65, 120, 101, 32
    ref = big.copy()
    ref[r0:r0 + m, c0:c0 + n] -= big[r0:r0 + m, 1:1 + k] @ big[1:1 + k, c0:c0 + n]
    import ctypes
    from nd4js_amd import _lib
    h = _lib.handle(0)
    h.set_stream(torch.cuda.current_stream().cuda_stream)
    base = d.data_ptr()
    off = lambda r, c: ctypes.c_void_p(base + 8 * (r * 200 + c))
    _lib.check(h.lib.nd4hip_dgemm_ex_dev(h.ptr, 0, 0, m, n, k, -1.0, off(r0, 1), 200, off(1, c0), 200, 1.0, off(r0, c0), 200))
    assert relerr(d.cpu().numpy(), ref) <= 1e-13


def test_c2_4096_against_reference_samples(dev, golden):
    """BASELINE config 2: 4096^2 fp64 matmul, inputs regenerated on the device from the seeds,
    checked against entries / row sums / Frobenius norm of the real reference's output."""
    import torch
    g = golden("c2_matmul4096")
    N = 4096
    A = dev.fill_uniform(g.seedA, (N, N))
    B = dev.fill_uniform(g.seedB, (N, N))
    C = dev.matmul2(A, B)
    torch.cuda.synchronize()
    flat = C.reshape(-1)
    idx = torch.from_numpy(g["idx"].astype(np.int64)).cuda()
    got = flat[idx].cpu().numpy()
    val = g["val"]
    assert np.linalg.norm(got - val) / np.linalg.norm(val) <= TIGHT
    rows = torch.from_numpy(g["rows"].astype(np.int64)).cuda()
    rs = C[rows].sum(dim=1).cpu().numpy()
    assert np.abs(rs - g["rowsum"]).max() <= 1e-9 * C[rows].abs().sum(dim=1).max().item()
    assert abs(torch.linalg.norm(C).item() - g.fro) <= 1e-12 * g.fro
    # size-independent property at full size: linearity  (A)(2B) == 2(AB) exactly (power of two)
    C2 = dev.matmul2(A, B * 2.0)
    assert torch.equal(C2, C * 2.0)


@pytest.mark.parametrize("ta,tb", [(0, 0), (1, 0), (0, 1), (1, 1)])
@pytest.mark.parametrize("M,N,K", [(64, 200, 4096), (130, 70, 2001), (16, 16, 5000), (300, 300, 700)])
def test_split_k_products(dev, ta, tb, M, N, K):
    """few output tiles and a long K: K is split over blockIdx.z and the partials are added in a fixed order"""
    import torch
    A = rng.matrix(610, K, M) if ta else rng.matrix(610, M, K)
    B = rng.matrix(611, N, K) if tb else rng.matrix(611, K, N)
    C0 = rng.matrix(612, M, N)
    ref = -1.25 * ((A.T if ta else A) @ (B.T if tb else B)) + 0.5 * C0
    dA, dB, dC = (torch.from_numpy(x).cuda() for x in (A, B, C0))
    dev.gemm_ex(ta, tb, -1.25, dA, dB, 0.5, dC, M, N, K, A.shape[1], B.shape[1], N)
    out = dC.cpu().numpy()
    assert relerr(out, ref) <= 1e-13
    dC2 = torch.from_numpy(C0).cuda()                      # deterministic: same bits on a second run
    dev.gemm_ex(ta, tb, -1.25, dA, dB, 0.5, dC2, M, N, K, A.shape[1], B.shape[1], N)
    assert np.array_equal(dC2.cpu().numpy(), out)


def test_split_k_batched_matmul2(la):
    a, b = rng.matrix(620, 3, 100, 2000), rng.matrix(621, 2000, 60)      # 3 tiles in total, K = 2000
    c = la.matmul2(a, b)
    assert relerr(c, a @ b) <= 1e-13
