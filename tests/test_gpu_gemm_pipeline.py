"""The software pipeline of dgemm_kernel's K loop (gemm.hip), at the places where a pipelined loop goes wrong.

The loop keeps two sets of MFMA fragments, reads group g + 1 from LDS under the MFMAs of group g, carries that across the barrier of
every K-step (group 0 of tile t + 1 is read before the MFMAs of group 3 of tile t) and is unrolled by two so that the LDS buffer
index is a constant. A mistake there is a fragment read from the wrong buffer or a group skipped or doubled at a loop boundary, and
it shows at few K-steps: the prologue, the drain and the odd tail of the unroll are all of the loop at nk = 1, 2, 3. The existing
cases of test_gpu_gemm_paths.py have nk = 3, 4 and 10 on the FULL instantiation; here every instantiation runs nk = 1 .. 7, split-K
chunks of both parities, and one product through all three instantiations, which must agree BIT FOR BIT: every element is
accumulated by the same instruction over k in ascending groups of four, whatever the instantiation.

Checks and operands are those of gemm_common.py / test_gpu_gemm_paths.py: the integer family must be reproduced exactly, the uniform
family within gamma_{K+35} E of the longdouble reference, operands lie inside NaN-filled buffers, beta = 0 runs over a NaN C."""
import ctypes

import numpy as np
import pytest

import gemm_common as gc
import test_gpu_gemm_paths as paths

pytestmark = pytest.mark.gpu
TRANSPOSES = paths.TRANSPOSES
TNAME = paths.TNAME
KSTEPS = (1, 2, 3, 4, 5, 6, 7)                              # K = 16 .. 112
AB = ((2.0, 1.0), (0.75, 0.0))                              # neither is a rank-k pair (gemm.hip: smallk_ok), so K <= 32 stays on this kernel


@pytest.fixture(scope="module")
def h():
    import torch
    assert torch.cuda.is_available()
    from nd4js_amd import _lib
    hd = _lib.handle(0)
    hd.set_stream(torch.cuda.current_stream().cuda_stream)
    return hd


def _odd(e):
    return (e + 2) | 1


@pytest.mark.parametrize("ta,tb", TRANSPOSES, ids=TNAME.values())
@pytest.mark.parametrize("M,N", [(128, 128), (256, 384)])
@pytest.mark.parametrize("nk", KSTEPS)
def test_full_few_k_steps(h, nk, M, N, ta, tb):
    for alpha, beta in AB:
        paths.check_ex(h, "pipeline FULL", ta, tb, M, N, 16 * nk, alpha, beta, seed=3000 + nk)


@pytest.mark.parametrize("ta,tb", TRANSPOSES, ids=TNAME.values())
@pytest.mark.parametrize("nk", KSTEPS)
def test_edge_vector_few_k_steps(h, nk, ta, tb):
    """(130, 258, K): two tile rows and three tile columns with 2 rows / 2 columns in the last ones, ld = extent + 2"""
    for alpha, beta in AB:
        paths.check_ex(h, "pipeline edge", ta, tb, 130, 258, 16 * nk, alpha, beta, seed=3100 + nk)


@pytest.mark.parametrize("ta,tb", TRANSPOSES, ids=TNAME.values())
@pytest.mark.parametrize("nk", KSTEPS)
def test_scalar_few_k_steps(h, nk, ta, tb):
    """the same shape with an odd lda: 8-byte loads"""
    K = 16 * nk
    for alpha, beta in AB:
        paths.check_ex(h, "pipeline scalar", ta, tb, 130, 258, K, alpha, beta, seed=3200 + nk, lda=_odd(130 if ta else K))


def split_chunks(M, N, K, batch=1):
    """K-steps of every split-K chunk, by the formula of gemm.hip: nd4_gemm ([] when the product is not split)"""
    tiles = -(-M // 128) * -(-N // 128) * batch
    if not (tiles <= 160 and K >= 512):
        return []
    want = min(384 // tiles, K // 256, 32)
    if want < 2:
        return []
    kc = -(-(-(-K // want)) // 16) * 16
    return [-(-(min(K, z + kc) - z) // 16) for z in range(0, K, kc)]


@pytest.mark.parametrize("M,N,K,main,last", [(16, 16, 9001, 18, 5), (16, 16, 8592, 17, 10), (130, 70, 8592, 17, 10)])
@pytest.mark.parametrize("beta", [0.0, 0.5])
def test_split_k_chunk_parity(h, M, N, K, main, last, beta):
    """kbeg / kend drive the same loop: chunks with an even and with an odd number of K-steps in one launch"""
    steps = split_chunks(M, N, K)
    assert len(steps) == 32 and set(steps[:-1]) == {main} and steps[-1] == last and (main + last) % 2 == 1
    for ta, tb in TRANSPOSES:
        paths.check_ex(h, "pipeline split-K", ta, tb, M, N, K, 0.75, beta, seed=3300, ldc=N + 6)


def _product(h, ta, tb, M, N, K, alpha, beta, A, B, C0, ld_pad, offA=0):
    """alpha op(A)[:M] op(B) + beta C0[:M] with A, B (as stored, for the whole 256-row product) inside NaN-filled buffers"""
    from nd4js_amd import _lib
    pa = gc.padded(A.shape[0], A.shape[1], A.shape[1] + ld_pad, offset=offA)
    pb = gc.padded(B.shape[0], B.shape[1], B.shape[1] + ld_pad)
    pc = gc.padded(M, N, N + 2)
    pa.win[...] = A
    pb.win[...] = B
    pc.win[...] = np.nan if beta == 0.0 else C0[:M]
    for p in (pa, pb, pc):
        p.upload()
        assert p.dev.data_ptr() % 16 == 0
    _lib.check(h.lib.nd4hip_dgemm_ex_dev(h.ptr, ta, tb, M, N, K, alpha, pa.ptr, pa.ld, pb.ptr, pb.ld, beta, pc.ptr, pc.ld))
    pa.assert_unchanged()
    pb.assert_unchanged()
    return pc.download()


@pytest.mark.parametrize("ta,tb", TRANSPOSES, ids=TNAME.values())
@pytest.mark.parametrize("alpha,beta", AB)
def test_same_bits_on_every_instantiation(h, ta, tb, alpha, beta):
    """one seeded uniform (256, 256, 208) product: FULL; vec / edge (the first 254 rows of the same operands, so M % 128 != 0);
    scalar (A's base shifted by 8 bytes). 13 K-steps, no k padding: the same MFMAs on the same numbers in the same order."""
    M = N = 256
    K = 208
    A = gc.uniform(3400, *((K, M) if ta else (M, K)))
    B = gc.uniform(3401, *((N, K) if tb else (K, N)))
    C0 = gc.uniform(3402, M, N)
    full = _product(h, ta, tb, M, N, K, alpha, beta, A, B, C0, 2)
    ref, E = gc.ref_gemm(ta, tb, alpha, A, B, beta, C0)
    gc.assert_within_bound(full, ref, E, K)
    edge = _product(h, ta, tb, M - 2, N, K, alpha, beta, A, B, C0, 2)     # lda unchanged: op(A)'s first 254 rows
    scalar = _product(h, ta, tb, M, N, K, alpha, beta, A, B, C0, 2, offA=1)
    assert edge.shape == (M - 2, N) and np.array_equal(edge.view(np.uint64), full[:M - 2].view(np.uint64)), "vec / edge path differs from FULL"
    assert np.array_equal(scalar.view(np.uint64), full.view(np.uint64)), "scalar path differs from FULL"


def test_4096_cubed_integers(h):
    """the headline shape (256 K-steps, 1024 tiles: two full rounds of workgroups), integer family only, against float64 BLAS on the
    host, which is exact on these inputs"""
    paths.check_ex(h, "pipeline 4096", 0, 0, 4096, 4096, 4096, 1.0, 0.0, seed=3500, families=("int",), blas=True)
