"""The buffer path of dgemm_kernel (gemm.hip: the BUF instantiations), at the places where it can go wrong.

FULL products (M, N multiples of 128, K a multiple of 16, 16-byte loads) whose tiles span less than 2^31 bytes load their operands
through buffer resources: the base of a resource is the first element of one tile of one K-step, a thread's share of the address is a
32-bit byte offset computed once, the row offsets are scalars; and the loop body of these instantiations is scheduled instruction by
instruction (every LDS access and every load behind an MFMA), with up to three K-steps following it. What can break, and the case
that shows it:

  prologue and drain   the loop body always loads two tiles ahead, so one to three K-steps are left behind it: every condition of
                       the prologue and the drain flips somewhere in nk = 1 .. 5; nk = 6 .. 9 run the loop body once to three
                       times with both parities of what is left. A tile behind the last one must never be loaded: the rows
                       behind every operand hold NaN
  resource base        per batch member (blockIdx.y) and per tile: 3 members with NaN between them, 2 x 3 tiles
  scalar row offsets   ld = extent, extent + 2 and 2^20 (a row offset of 256 MiB), bases shifted by two elements
  host predicate       buf_fits(): a 128-row tile of an x-major operand with ld = 2^21 - 2 spans 2^31 - 2048 bytes (buffer path), with
                       ld = 2^21 it spans 2^31 (pointer loads). Both give the bits of the same product at ld = K
  nd4_gemm_nt_lower    the workgroup of the tile above the diagonal returns before its first load: that tile of C keeps its value

Checks and operands are those of gemm_common.py / test_gpu_gemm_paths.py: the integer family must be reproduced exactly, the uniform
family within gamma_{K+35} E of the longdouble reference, operands lie inside NaN-filled buffers, beta = 0 runs over a NaN C. The
cases with a huge ld build their operands on the device (a strided view into a NaN-filled buffer): only the C window is read back."""
import ctypes

import numpy as np
import pytest

import gemm_common as gc
import test_gpu_gemm_paths as paths

pytestmark = pytest.mark.gpu
TRANSPOSES = paths.TRANSPOSES
TNAME = paths.TNAME
AB = ((2.0, 1.0), (0.75, 0.0))                              # neither is a rank-k pair (gemm.hip: smallk_ok), so K <= 32 stays on this kernel
c_i64, c_dp = ctypes.c_int64, ctypes.c_void_p
# the two internal entry points behind every caller inside the library (nd4hip_internal.h), by their C++ names
ND4_GEMM = ("_Z8nd4_gemmP13nd4hip_handlebbllldPKdllS2_lldPdlll",
            [c_dp, ctypes.c_bool, ctypes.c_bool, c_i64, c_i64, c_i64, ctypes.c_double, c_dp, c_i64, c_i64, c_dp, c_i64, c_i64,
             ctypes.c_double, c_dp, c_i64, c_i64, c_i64])
ND4_GEMM_NT_LOWER = ("_Z17nd4_gemm_nt_lowerP13nd4hip_handlelldPKdllS2_lldPdlll",
                     [c_dp, c_i64, c_i64, ctypes.c_double, c_dp, c_i64, c_i64, c_dp, c_i64, c_i64, ctypes.c_double, c_dp, c_i64, c_i64, c_i64])


@pytest.fixture(scope="module")
def h():
    import torch
    assert torch.cuda.is_available()
    from nd4js_amd import _lib
    hd = _lib.handle(0)
    hd.set_stream(torch.cuda.current_stream().cuda_stream)
    return hd


def _internal(h, entry):
    name, argtypes = entry
    fn = getattr(h.lib, name)
    fn.restype, fn.argtypes = ctypes.c_int, argtypes
    return fn


# ------------------------------------------------------------------------------------------------------------ prologue and drain
@pytest.mark.parametrize("ta,tb", TRANSPOSES, ids=TNAME.values())
@pytest.mark.parametrize("M,N", [(128, 128), (256, 384)])
@pytest.mark.parametrize("nk", range(1, 10))
def test_full_k_steps_1_to_9(h, nk, M, N, ta, tb):
    for alpha, beta in AB:
        paths.check_ex(h, "prefetch FULL", ta, tb, M, N, 16 * nk, alpha, beta, seed=4000 + nk)


# --------------------------------------------------------------------------------------------------------------------------- batch
@pytest.mark.parametrize("ta,tb", TRANSPOSES, ids=TNAME.values())
def test_batch_of_three_with_gaps(h, ta, tb):
    """nd4_gemm with 3 members, member strides larger than the matrices and NaN in the gaps, ld = extent + 2"""
    from nd4js_amd import _lib
    gemm = _internal(h, ND4_GEMM)
    batch, M, N, K = 3, 128, 128, 48
    ar, ac = (K, M) if ta else (M, K)
    br, bc = (N, K) if tb else (K, N)
    for alpha, beta in AB:
        for fam in ("int", "uni"):
            gen = gc.FAMILIES[fam]
            pa = gc.Padded(ar, ac, ac + 2, batch=batch, stride=ar * (ac + 2) + 38)
            pb = gc.Padded(br, bc, bc + 2, batch=batch, stride=br * (bc + 2) + 70)
            pc = gc.Padded(M, N, N + 2, batch=batch, stride=M * (N + 2) + 6)
            pa.win[...] = gen(4100, batch, ar, ac)
            pb.win[...] = gen(4101, batch, br, bc)
            C0 = gen(4102, batch, M, N)
            pc.win[...] = np.nan if beta == 0.0 else C0
            A, B = pa.win.copy(), pb.win.copy()
            for p in (pa, pb, pc):
                p.upload()
                assert p.dev.data_ptr() % 16 == 0 and p.start % 2 == 0 and p.stride % 2 == 0      # the 16-byte path
            _lib.check(gemm(h.ptr, bool(ta), bool(tb), M, N, K, alpha, pa.ptr, pa.ld, pa.stride, pb.ptr, pb.ld, pb.stride,
                            beta, pc.ptr, pc.ld, pc.stride, batch))
            got = pc.download()
            pa.assert_unchanged()
            pb.assert_unchanged()
            for b in range(batch):
                if fam == "int":
                    gc.assert_exact(got[b], gc.exact_gemm(ta, tb, alpha, A[b], B[b], beta, C0[b]))
                else:
                    ref, E = gc.ref_gemm(ta, tb, alpha, A[b], B[b], beta, C0[b])
                    gc.assert_within_bound(got[b], ref, E, K)


# -------------------------------------------------------------------------------------------------------------- leading dimensions
def _on_device(X, ld, shift):
    """X (rows x cols on the host) as a view with leading dimension ld, `shift` elements into a NaN-filled device buffer that ends
    two elements behind X -> (buffer, pointer to X[0, 0])"""
    import torch
    rows, cols = X.shape
    buf = torch.full(((rows - 1) * ld + cols + shift + 2,), float("nan"), dtype=torch.float64, device="cuda")
    buf.as_strided((rows, cols), (ld, 1), shift).copy_(torch.from_numpy(np.ascontiguousarray(X)).cuda())
    assert buf.data_ptr() % 16 == 0
    return buf, ctypes.c_void_p(buf.data_ptr() + 8 * shift)


def strided_product(h, ta, tb, M, N, K, alpha, beta, A, B, C0, lda, ldb, shift=2):
    """alpha op(A) op(B) + beta C0 through nd4hip_dgemm_ex_dev with A and B (as stored) at leading dimensions lda / ldb on the device"""
    from nd4js_amd import _lib
    bufa, ptra = _on_device(A, lda, shift)
    bufb, ptrb = _on_device(B, ldb, shift)
    pc = gc.padded(M, N, N + 2)
    pc.win[...] = np.nan if beta == 0.0 else C0
    pc.upload()
    _lib.check(h.lib.nd4hip_dgemm_ex_dev(h.ptr, ta, tb, M, N, K, alpha, ptra, lda, ptrb, ldb, beta, pc.ptr, pc.ld))
    got = pc.download()
    del bufa, bufb
    return got


@pytest.mark.parametrize("ta,tb", TRANSPOSES, ids=TNAME.values())
@pytest.mark.parametrize("pad", [0, 2, "2^20"])
def test_leading_dimensions_and_shifted_bases(h, pad, ta, tb):
    """(128, 128, 48) with both operands two elements into their buffers (still 16-byte aligned)"""
    M, N, K = 128, 128, 48
    ac, bc = (M if ta else K), (K if tb else N)
    for alpha, beta in AB:
        if pad != "2^20":
            paths.check_ex(h, "prefetch ld", ta, tb, M, N, K, alpha, beta, seed=4200, lda=ac + pad, ldb=bc + pad, offA=2, offB=2)
            continue
        for fam in ("int", "uni"):
            gen = gc.FAMILIES[fam]
            A, B, C0 = gen(4200, *((K, M) if ta else (M, K))), gen(4201, *((N, K) if tb else (K, N))), gen(4202, M, N)
            got = strided_product(h, ta, tb, M, N, K, alpha, beta, A, B, C0, 1 << 20, 1 << 20)
            if fam == "int":
                gc.assert_exact(got, gc.exact_gemm(ta, tb, alpha, A, B, beta, C0))
            else:
                ref, E = gc.ref_gemm(ta, tb, alpha, A, B, beta, C0)
                gc.assert_within_bound(got, ref, E, K)


# ------------------------------------------------------------------------------------------------------------------ host predicate
def test_buffer_path_boundary_of_an_x_major_operand(h):
    """A of NN, 128 x 48: lda = 2^21 - 2 is the largest even ld whose 128-row tile spans less than 2^31 bytes (128 * lda * 8 =
    2^31 - 2048), lda = 2^21 is the first that does not (= 2^31: the FULL instantiation with pointer loads). Each operand is a view
    into a NaN-filled buffer of 2 GiB; both must give the bits of the same product at lda = 48, which is checked against the reference."""
    M, N, K = 128, 128, 48
    for alpha, beta in AB:
        A, B, C0 = gc.uniform(4300, M, K), gc.uniform(4301, K, N), gc.uniform(4302, M, N)
        base = strided_product(h, 0, 0, M, N, K, alpha, beta, A, B, C0, K, N, shift=0)
        ref, E = gc.ref_gemm(0, 0, alpha, A, B, beta, C0)
        gc.assert_within_bound(base, ref, E, K)
        for lda in ((1 << 21) - 2, 1 << 21):
            assert (128 * lda * 8 < 1 << 31) == (lda < 1 << 21)
            got = strided_product(h, 0, 0, M, N, K, alpha, beta, A, B, C0, lda, N)
            assert np.array_equal(got.view(np.uint64), base.view(np.uint64)), "lda = %d differs from lda = %d" % (lda, K)
        Ai, Bi, Ci = gc.integers(4303, M, K), gc.integers(4304, K, N), gc.integers(4305, M, N)
        for lda in ((1 << 21) - 2, 1 << 21):
            gc.assert_exact(strided_product(h, 0, 0, M, N, K, alpha, beta, Ai, Bi, Ci, lda, N), gc.exact_gemm(0, 0, alpha, Ai, Bi, beta, Ci))


# ---------------------------------------------------------------------------------------------------------------- nd4_gemm_nt_lower
@pytest.mark.parametrize("K", [48, 144])
def test_nt_lower_skips_the_tile_above_the_diagonal(h, K):
    """C[lower tiles] = alpha A B^T + beta C for N = 256: tiles (0, 0), (1, 0), (1, 1) are computed in full, tile (0, 1) belongs to
    a workgroup that returns before the first barrier and must issue nothing: its part of C keeps the value it was given"""
    from nd4js_amd import _lib
    lower = _internal(h, ND4_GEMM_NT_LOWER)
    N = 256
    for alpha, beta in AB:
        for fam in ("int", "uni"):
            gen = gc.FAMILIES[fam]
            pa, pb, pc = gc.padded(N, K, K + 2), gc.padded(N, K, K + 2), gc.padded(N, N, N + 2)
            pa.win[...] = gen(4400, N, K)
            pb.win[...] = gen(4401, N, K)
            C0 = gen(4402, N, N)
            pc.win[...] = np.nan if beta == 0.0 else C0
            pc.win[:128, 128:] = 12345.0
            A, B = pa.win.copy(), pb.win.copy()
            for p in (pa, pb, pc):
                p.upload()
                assert p.dev.data_ptr() % 16 == 0
            _lib.check(lower(h.ptr, N, K, alpha, pa.ptr, pa.ld, 0, pb.ptr, pb.ld, 0, beta, pc.ptr, pc.ld, 0, 1))
            got = pc.download()
            pa.assert_unchanged()
            pb.assert_unchanged()
            assert (got[:128, 128:] == 12345.0).all(), "the tile above the diagonal was written"
            for rows, cols in ((slice(0, 128), slice(0, 128)), (slice(128, 256), slice(0, 256))):
                if fam == "int":
                    gc.assert_exact(got[rows, cols], gc.exact_gemm(0, 1, alpha, A[rows], B[cols], beta, C0[rows, cols]))
                else:
                    ref, E = gc.ref_gemm(0, 1, alpha, A[rows], B[cols], beta, C0[rows, cols])
                    gc.assert_within_bound(got[rows, cols], ref, E, K)
