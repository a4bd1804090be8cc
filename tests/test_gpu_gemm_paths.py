"""Every kernel path of the fp64 GEMM (gemm.hip: nd4_gemm), checked ELEMENT BY ELEMENT against a reference of higher precision.

nd4_gemm is the headline kernel and the trailing-update engine of LU, QR, Cholesky, LDL^T, the blocked triangular solves, the block
Jacobi SVD and the real-by-complex product. It picks one of three kernels (and one of three instantiations of the tiled one) from the
shape, the scalars, the transposes and the alignment of its operands, so a path can be wrong while every norm-wise test at friendly
shapes passes. Each case below runs twice (helpers and the derivation of the bound: gemm_common.py):

  integer family   operands and C0 integers in [-4, 4], dyadic alpha / beta: the result must EQUAL the integer result (no tolerance);
                   this is what names a dropped, doubled or misplaced term at an edge
  uniform family   seeded uniform [-1, 1): every element within gamma_{K+35} E of the longdouble reference; this is what catches
                   lost precision. The bound holds for any summation order, so a rewrite of the main loop must still meet it.

Operands are views inside device buffers that hold NaN everywhere else (rows before and after, the ld - extent padding of each row,
an optional 8-byte shift of the base). One out-of-range element that is loaded and used makes the result NaN; C's buffer is read back
whole and everything outside the M x N window must be bit-identical to what was uploaded; A's and B's buffers must be unchanged.
Whenever beta == 0, C is filled with NaN first: beta = 0 must not read C.

Case -> kernel -> condition in nd4_gemm that sends it there (BM = BN = 128, BK = 16):

  rank-k      dgemm_smallk_kernel<TB>            K <= 32, A plain, alpha = +-1, beta in {0, +-1}
    K in 1..32 x M in 1..130 x N in 1..100 x B plain / transposed x the six (alpha, beta): 96 cases that cover every pair of values
      (K % 4 != 0: the kk*4+fk < K predicate, nk = (K+3)>>2; M = 1, 15..17: waves that leave early, rbase >= M; N % 32 != 0: the
      col < N predicates), odd lda / ldb, ldc > N, every base shifted by 8 bytes (no vector path here: nothing may change)
    K = 33; K = 16 with (alpha, beta) = (2, 1); K = 16 with A transposed     the neighbours that smallk_ok refuses -> tiled kernel
    batch 5 of 70 x 24 x 50 through nd4hip_dgemm_batched_dev: equal strides, A broadcast, B broadcast, strides with NaN between members
  tiled FULL  dgemm_kernel<TA, TB, true, true>   vec && M % 128 == 0 && N % 128 == 0 && K % 16 == 0: no predicate anywhere
    (128, 128, 48), (256, 384, 64), (384, 256, 160) x four transposes
    NN (1408, 1664, 48): 11 x 13 = 143 tiles, short last group of tile rows, count % 8 != 0 (the XCD map); (1152, 128, 48),
    (128, 1152, 48), (2176, 384, 48): 9 x 1, 1 x 9, 17 x 3 tiles
  tiled edge  dgemm_kernel<TA, TB, true, false>  vec (aligned bases, even lda / ldb / contiguous extents) but not FULL
    (130, 258, 34), (254, 126, 50), (2, 2, 34), (130, 258, 46), (1410, 1666, 36) x four transposes: K % 16 in {2, 4, 14}, ld > extent
  tiled scalar dgemm_kernel<TA, TB, false, false>  !vec, one trigger at a time from the even, aligned (150, 94, 70):
    A shifted by 8 bytes | B shifted | lda odd | ldb odd                     x four transposes
    contiguous extent of A odd: K = 71 (NN), M = 151 (TN, TT); of B odd: N = 95 (NN, TN), K = 71 (TT)
    strideA odd | strideB odd in a batch of 3 (50 x 40 x 30, nd4hip_dgemm_batched_dev)
    all odd: (129, 17, 255), (301, 97, 203) x four transposes
  split-K     dgemm_kernel (raw partials) + dgemm_splitk_reduce   tiles * batch <= 160 && K >= 512, chunks = min(384 / tiles, K / 256, 32)
    (64, 200, 511) no split | (64, 200, 512) 2 chunks; (1280, 2048, 512) 160 tiles, FULL, 2 chunks | (1280, 2176, 512) 170 tiles, none
    (16, 16, 8192) 32 chunks of 256; (16, 16, 9001) 32 chunks of 288, last one 73; (130, 70, 2001) 7 chunks of 288, last one 273
    FULL with split: (128, 128, 4096), (256, 256, 2048) x four transposes; beta in {0, 0.5}, ldc > N; the same bits on a second run
    batched: 3 x (100 x 2000 x 60), B per member and B broadcast; 4 | 5 x (1280 x 1024 x 512): 160 tiles split | 200 tiles not
  K = 0       dgemm_kernel<.., false>, no K step: C = beta C
  special     +inf in op(A)[M-1, K-1], NaN in op(B)[K-1, N-1] (last row / column / k of an edge tile), once per kernel

The cases marked "integer only" in the source exceed 2e8 multiply-adds; they run the integer family alone, against float64 BLAS on
the host, which is exact on these inputs. The largest |err| / (gamma E) of the uniform family is printed per path at the end of the
module (pytest -s) as a record of the margin; the assertion is the derived bound."""

import numpy as np
import pytest

import gemm_common as gc

pytestmark = pytest.mark.gpu
TRANSPOSES = [(0, 0), (1, 0), (0, 1), (1, 1)]
TNAME = {(0, 0): "NN", (1, 0): "TN", (0, 1): "NT", (1, 1): "TT"}
# scalars of the tiled cases, taken in turn: every group meets beta = 0 and beta != 0
AB = ((0.75, -0.5), (2.0, 1.0), (-0.5, 2.0), (-1.0, 0.0), (1.0, -1.0), (0.75, 0.0), (2.0, -0.5), (-0.5, 1.0))
STATS = {}


@pytest.fixture(scope="module")
def h():
    import torch
    assert torch.cuda.is_available()
    from nd4js_amd import _lib
    hd = _lib.handle(0)
    hd.set_stream(torch.cuda.current_stream().cuda_stream)
    return hd


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    print("\npath: runs, largest |err| / (gamma_{K+35} E) of the uniform family")
    for path, (runs, worst) in STATS.items():
        print("  %-16s %4d  %.4f" % (path, runs, worst))


def _even_ld(extent):
    return extent + 2 - (extent & 1)


def _record(path, ratio=None):
    s = STATS.setdefault(path, [0, 0.0])
    s[0] += 1
    if ratio is not None:
        s[1] = max(s[1], ratio)


def _upload(p):
    p.upload()
    assert p.dev.data_ptr() % 16 == 0                       # so that the base is 16-byte aligned exactly when p.start is even
    return p


def run_ex(h, ta, tb, M, N, K, alpha, beta, fam, seed, lda=None, ldb=None, ldc=None, offA=0, offB=0, offC=0, special=False):
    """one nd4hip_dgemm_ex_dev call on NaN-guarded operands -> (result window, A, B, C0) with A, B as stored"""
    from nd4js_amd import _lib
    gen = gc.FAMILIES[fam]
    ar, ac = (K, M) if ta else (M, K)
    br, bc = (N, K) if tb else (K, N)
    pa = gc.padded(ar, ac, _even_ld(ac) if lda is None else lda, offset=offA)
    pb = gc.padded(br, bc, _even_ld(bc) if ldb is None else ldb, offset=offB)
    pc = gc.padded(M, N, _even_ld(N) if ldc is None else ldc, offset=offC)
    pa.win[...] = gen(seed, ar, ac)
    pb.win[...] = gen(seed + 1, br, bc)
    if special:
        gc.op(ta, pa.win)[M - 1, K - 1] = np.inf
        gc.op(tb, pb.win)[K - 1, N - 1] = np.nan
    C0 = gen(seed + 2, M, N)
    pc.win[...] = np.nan if beta == 0.0 else C0             # beta = 0 must not read C
    A, B = pa.win.copy(), pb.win.copy()
    for p in (pa, pb, pc):
        _upload(p)
    _lib.check(h.lib.nd4hip_dgemm_ex_dev(h.ptr, ta, tb, M, N, K, alpha, pa.ptr, pa.ld, pb.ptr, pb.ld, beta, pc.ptr, pc.ld))
    got = pc.download()
    pa.assert_unchanged()
    pb.assert_unchanged()
    return got, A, B, C0


def check_ex(h, path, ta, tb, M, N, K, alpha, beta, seed=700, families=("int", "uni"), blas=False, twice=False, **kw):
    for fam in families:
        got, A, B, C0 = run_ex(h, ta, tb, M, N, K, alpha, beta, fam, seed, **kw)
        if fam == "int":
            gc.assert_exact(got, gc.exact_gemm(ta, tb, alpha, A, B, beta, C0, blas=blas))
            _record(path)
        else:
            ref, E = gc.ref_gemm(ta, tb, alpha, A, B, beta, C0)
            _record(path, gc.assert_within_bound(got, ref, E, K))
        if beta == 0.0 and not kw.get("special"):
            assert np.isfinite(got).all()
        if twice:                                           # the split-K partials are added in a fixed order: the same bits again
            again = run_ex(h, ta, tb, M, N, K, alpha, beta, fam, seed, **kw)[0]
            assert np.array_equal(again.view(np.uint64), got.view(np.uint64))


def run_batched(h, batch, I, K, J, fam, seed, bcastA=False, bcastB=False, strideA=None, strideB=None):
    """nd4hip_dgemm_batched_dev (alpha = 1, beta = 0, lda = K, ldb = J, C contiguous) -> (C, A, B) with the batch axis in front"""
    from nd4js_amd import _lib
    gen = gc.FAMILIES[fam]
    na, nb = (1 if bcastA else batch), (1 if bcastB else batch)
    pa = gc.Padded(I, K, K, batch=na, stride=strideA)
    pb = gc.Padded(K, J, J, batch=nb, stride=strideB)
    pc = gc.Padded(I, J, J, batch=batch)                    # stays NaN: beta = 0
    pa.win[...] = gen(seed, na, I, K).reshape(pa.win.shape)
    pb.win[...] = gen(seed + 1, nb, K, J).reshape(pb.win.shape)
    A, B = pa.win.copy().reshape(na, I, K), pb.win.copy().reshape(nb, K, J)
    for p in (pa, pb, pc):
        _upload(p)
    _lib.check(h.lib.nd4hip_dgemm_batched_dev(h.ptr, batch, I, K, J, pa.ptr, 0 if bcastA or batch == 1 else pa.stride,
                                              pb.ptr, 0 if bcastB or batch == 1 else pb.stride, pc.ptr))
    got = pc.download().reshape(batch, I, J)
    pa.assert_unchanged()
    pb.assert_unchanged()
    return got, A, B


def check_batched(h, path, batch, I, K, J, seed=800, families=("int", "uni"), blas=False, **kw):
    for fam in families:
        got, A, B = run_batched(h, batch, I, K, J, fam, seed, **kw)
        assert np.isfinite(got).all()
        for b in range(batch):
            a, bb = A[b if len(A) > 1 else 0], B[b if len(B) > 1 else 0]
            if fam == "int":
                gc.assert_exact(got[b], gc.exact_gemm(0, 0, 1.0, a, bb, 0.0, None, blas=blas))
                _record(path)
            else:
                ref, E = gc.ref_gemm(0, 0, 1.0, a, bb, 0.0, None)
                _record(path, gc.assert_within_bound(got[b], ref, E, K))


# ------------------------------------------------------------------------------------------------------------------------ rank-k
@pytest.mark.parametrize("K,M,N,tb,ab", gc.smallk_cases(), ids=lambda v: "%g_%g" % v if isinstance(v, tuple) else str(v))
def test_rank_k_kernel(h, K, M, N, tb, ab):
    ldb = ((K if tb else N) + 2) | 1
    check_ex(h, "rank-k", 0, tb, M, N, K, ab[0], ab[1], seed=1000 + 7 * K + M, lda=(K + 2) | 1, ldb=ldb, ldc=N + 3, offA=1, offB=1, offC=1)


@pytest.mark.parametrize("tb", [0, 1])
@pytest.mark.parametrize("ta,K,alpha,beta", [(0, 33, -1.0, 1.0), (0, 33, 1.0, 0.0), (0, 16, 2.0, 1.0), (1, 16, -1.0, 1.0), (1, 32, 1.0, 0.0)])
def test_rank_k_neighbours_take_the_tiled_kernel(h, ta, tb, K, alpha, beta):
    """K = 33, alpha = 2 and a transposed A are what smallk_ok refuses: the tiled kernel gives the same exact integers"""
    for M, N in ((65, 33), (130, 100)):
        check_ex(h, "rank-k neighbours", ta, tb, M, N, K, alpha, beta, seed=1100 + K, ldc=N + 3, offC=1)


@pytest.mark.parametrize("kw", [dict(), dict(bcastA=True), dict(bcastB=True), dict(strideA=70 * 24 + 5, strideB=24 * 50 + 3)],
                         ids=["equal", "bcastA", "bcastB", "gaps"])
def test_rank_k_batched(h, kw):
    check_batched(h, "rank-k batched", 5, 70, 24, 50, **kw)


# ------------------------------------------------------------------------------------------------------------------ tiled, FULL
@pytest.mark.parametrize("ta,tb", TRANSPOSES, ids=TNAME.values())
@pytest.mark.parametrize("n,M,N,K", [(0, 128, 128, 48), (1, 256, 384, 64), (2, 384, 256, 160)])
def test_tiled_full_transposes(h, ta, tb, n, M, N, K):
    alpha, beta = AB[(3 * n + 2 * ta + tb) % len(AB)]
    check_ex(h, "tiled FULL", ta, tb, M, N, K, alpha, beta, seed=1200 + n)


@pytest.mark.parametrize("n,M,N,K", [(0, 1408, 1664, 48), (1, 1152, 128, 48), (2, 128, 1152, 48), (3, 2176, 384, 48)])
def test_tiled_full_tile_map(h, n, M, N, K):
    """tile grids of 11 x 13, 9 x 1, 1 x 9 and 17 x 3: short last groups of tile rows, tile counts that are not multiples of 8"""
    alpha, beta = AB[n]
    check_ex(h, "tiled FULL", 0, 0, M, N, K, alpha, beta, seed=1300 + n)


# ------------------------------------------------------------------------------------------------------ tiled, 16-byte edge path
@pytest.mark.parametrize("ta,tb", TRANSPOSES, ids=TNAME.values())
@pytest.mark.parametrize("n,M,N,K", [(0, 130, 258, 34), (1, 254, 126, 50), (2, 2, 2, 34), (3, 130, 258, 46), (4, 1410, 1666, 36)])
def test_tiled_edge_vector_path(h, ta, tb, n, M, N, K):
    alpha, beta = AB[(n + 2 * ta + tb) % len(AB)]
    check_ex(h, "tiled edge", ta, tb, M, N, K, alpha, beta, seed=1400 + n)


# ------------------------------------------------------------------------------------------------------------ tiled, scalar path
BASE = (150, 94, 70)
SCALAR_TRIGGERS = (
    [("A shifted", t, BASE, dict(offA=1)) for t in TRANSPOSES] + [("B shifted", t, BASE, dict(offB=1)) for t in TRANSPOSES] +
    [("lda odd", t, BASE, dict(lda=(151 if t[0] else 71))) for t in TRANSPOSES] +
    [("ldb odd", t, BASE, dict(ldb=(71 if t[1] else 95))) for t in TRANSPOSES] +
    [("K odd, A plain", (0, 0), (150, 94, 71), {}), ("M odd, A transposed", (1, 0), (151, 94, 70), {}),
     ("M odd, A transposed", (1, 1), (151, 94, 70), {}), ("N odd, B plain", (0, 0), (150, 95, 70), {}),
     ("N odd, B plain", (1, 0), (150, 95, 70), {}), ("K odd, B transposed", (1, 1), (150, 94, 71), {})])


def test_scalar_base_case_is_on_the_vector_path():
    """the case the triggers start from: nothing odd, so that each of them is the only reason for the scalar path"""
    M, N, K = BASE
    assert all(v % 2 == 0 for v in (M, N, K, _even_ld(M), _even_ld(N), _even_ld(K))) and gc.padded(4, 4, 6).start % 2 == 0


@pytest.mark.parametrize("what,t,shape,kw", SCALAR_TRIGGERS, ids=["%s %s" % (w, TNAME[t]) for w, t, _, _ in SCALAR_TRIGGERS])
def test_tiled_scalar_path_one_trigger(h, what, t, shape, kw):
    """the NaN right behind each odd extent is the point: a wrongly granted 16-byte load takes it in"""
    M, N, K = shape
    alpha, beta = AB[(len(what) + 2 * t[0] + t[1]) % len(AB)]
    check_ex(h, "tiled scalar", t[0], t[1], M, N, K, alpha, beta, seed=1500, **kw)


@pytest.mark.parametrize("ta,tb", TRANSPOSES, ids=TNAME.values())
@pytest.mark.parametrize("n,M,N,K", [(0, 150, 94, 70), (1, 129, 17, 255), (2, 301, 97, 203)])
def test_tiled_scalar_path_all_odd(h, ta, tb, n, M, N, K):
    """(the first shape is the even base case itself with every operand shifted and every ld odd)"""
    alpha, beta = AB[(n + 4 + 2 * ta + tb) % len(AB)]
    odd = lambda e: (e + 2) | 1
    check_ex(h, "tiled scalar", ta, tb, M, N, K, alpha, beta, seed=1600 + n, lda=odd(M if ta else K), ldb=odd(K if tb else N),
             ldc=odd(N), offA=1, offB=1, offC=1)


@pytest.mark.parametrize("kw", [dict(strideA=50 * 40 + 1), dict(strideB=40 * 30 + 1), dict()], ids=["strideA odd", "strideB odd", "even"])
def test_tiled_batched_stride_parity(h, kw):
    check_batched(h, "tiled scalar" if kw else "tiled edge", 3, 50, 40, 30, seed=1700, **kw)


# ----------------------------------------------------------------------------------------------------------------------- split-K
@pytest.mark.parametrize("M,N,K", [(64, 200, 511), (64, 200, 512), (16, 16, 8192), (16, 16, 9001), (130, 70, 2001)])
@pytest.mark.parametrize("beta", [0.0, 0.5])
def test_split_k_thresholds_and_chunks(h, M, N, K, beta):
    check_ex(h, "split-K", 0, 0, M, N, K, -0.5, beta, seed=1800, ldc=N + 6, twice=True)
    check_ex(h, "split-K", 1, 1, M, N, K, 0.75, beta, seed=1801, ldc=N + 6)


@pytest.mark.parametrize("ta,tb", TRANSPOSES, ids=TNAME.values())
@pytest.mark.parametrize("M,N,K", [(128, 128, 4096), (256, 256, 2048)])
def test_split_k_full(h, ta, tb, M, N, K):
    beta = 0.5 if ta == tb else 0.0
    check_ex(h, "split-K", ta, tb, M, N, K, 2.0, beta, seed=1900 + K, ldc=N + 2, twice=(ta, tb) == (0, 0))


@pytest.mark.parametrize("N", [2048, 2176])
def test_split_k_tile_count_threshold(h, N):
    """integer only: 10 x 16 = 160 tiles are split (FULL), 10 x 17 = 170 are not"""
    check_ex(h, "split-K", 0, 0, 1280, N, 512, 0.75, -0.5, seed=2000, families=("int",), blas=True)


@pytest.mark.parametrize("bcastB", [False, True])
def test_split_k_batched(h, bcastB):
    check_batched(h, "split-K", 3, 100, 2000, 60, seed=2100, bcastB=bcastB)


@pytest.mark.parametrize("batch", [4, 5])
def test_split_k_batched_tile_count_threshold(h, batch):
    """integer only: 4 x 40 = 160 tiles are split, 5 x 40 = 200 are not"""
    check_batched(h, "split-K", batch, 1280, 1024, 512, seed=2200, families=("int",), blas=True)


# ---------------------------------------------------------------------------------------------------------- beta = 0 must not read C
@pytest.mark.parametrize("name,ta,tb,M,N,K,alpha,kw", [
    ("rank-k", 0, 1, 65, 33, 17, -1.0, {}), ("tiled FULL", 0, 0, 256, 128, 64, 0.75, {}), ("tiled edge", 1, 0, 130, 70, 36, 2.0, {}),
    ("scalar", 0, 1, 129, 17, 255, -0.5, dict(offA=1)), ("split-K", 1, 1, 64, 200, 1024, 0.75, {})], ids=lambda v: v if isinstance(v, str) else None)
def test_beta_zero_over_nan(h, name, ta, tb, M, N, K, alpha, kw):
    """run_ex fills C with NaN whenever beta == 0 (and check_ex asserts a finite result); here once per kernel, by name"""
    check_ex(h, "beta = 0 over NaN", ta, tb, M, N, K, alpha, 0.0, seed=2300, **kw)


def test_beta_zero_over_nan_matmul2_out():
    import torch
    from nd4js_amd import dev
    for shape_a, shape_b in (((70, 24), (24, 50)), ((3, 130, 70), (3, 70, 36)), ((256, 64), (64, 128)), ((64, 1024), (1024, 200))):
        A, B = gc.integers(2400, *shape_a), gc.integers(2401, *shape_b)
        out = torch.full(shape_a[:-1] + shape_b[-1:], float("nan"), dtype=torch.float64, device="cuda")
        res = dev.matmul2(torch.from_numpy(A).cuda(), torch.from_numpy(B).cuda(), out=out)
        assert res is out
        gc.assert_exact(out.cpu().numpy(), (A.astype(np.int64) @ B.astype(np.int64)).astype(np.float64))
        _record("beta = 0 over NaN")


# ------------------------------------------------------------------------------------------------------------------------- K = 0
@pytest.mark.parametrize("ta,tb", TRANSPOSES, ids=TNAME.values())
@pytest.mark.parametrize("M,N", [(5, 7), (130, 129), (128, 128)])
def test_k_zero_gemm_ex(h, ta, tb, M, N):
    """C = beta C: zeros over NaN for beta = 0, exact halves of the integers for beta = 0.5, padding untouched"""
    for alpha, beta in ((1.0, 0.0), (0.75, 0.5), (-1.0, 1.0)):
        got, _, _, C0 = run_ex(h, ta, tb, M, N, 0, alpha, beta, "int", 2500, ldc=N + 3, offC=1)
        gc.assert_exact(got, np.zeros((M, N)) if beta == 0.0 else beta * C0)
        _record("K = 0")


def test_zero_extents_matmul2_dev():
    import torch
    from nd4js_amd import dev
    z = lambda *s: torch.zeros(s, dtype=torch.float64, device="cuda")
    for sa, sb, sc in (((5, 0), (0, 7), (5, 7)), ((3, 5, 0), (3, 0, 7), (3, 5, 7)), ((3, 5, 0), (0, 7), (3, 5, 7)),
                       ((0, 4), (4, 7), (0, 7)), ((5, 4), (4, 0), (5, 0)), ((2, 0, 4), (2, 4, 7), (2, 0, 7)), ((0, 5, 4), (0, 4, 7), (0, 5, 7))):
        c = dev.matmul2(z(*sa), z(*sb))
        assert tuple(c.shape) == sc and c.dtype == torch.float64
        assert np.array_equal(c.cpu().numpy(), np.zeros(sc)), (sa, sb)
        out = torch.full(sc, float("nan"), dtype=torch.float64, device="cuda")
        assert np.array_equal(dev.matmul2(z(*sa), z(*sb), out=out).cpu().numpy(), np.zeros(sc)), (sa, sb)
        _record("K = 0")


def test_zero_extents_matmul2_host():
    from nd4js_amd import la
    for sa, sb, sc in (((5, 0), (0, 7), (5, 7)), ((3, 5, 0), (3, 0, 7), (3, 5, 7)), ((3, 5, 0), (0, 7), (3, 5, 7)),
                       ((0, 4), (4, 7), (0, 7)), ((5, 4), (4, 0), (5, 0)), ((2, 0, 4), (2, 4, 7), (2, 0, 7))):
        c = la.matmul2(np.zeros(sa), np.zeros(sb))
        assert c.shape == sc and c.dtype == np.float64 and np.array_equal(c, np.zeros(sc)), (sa, sb)
        out = np.full(sc, np.nan)
        assert np.array_equal(la.matmul2(np.zeros(sa), np.zeros(sb), out=out), np.zeros(sc)), (sa, sb)
        _record("K = 0")


# ---------------------------------------------------------------------------------------------------------------- special values
@pytest.mark.parametrize("name,ta,tb,M,N,K,alpha,beta,kw", [
    ("rank-k", 0, 0, 65, 33, 17, -1.0, 1.0, {}), ("rank-k", 0, 1, 130, 100, 32, 1.0, 0.0, {}),
    ("tiled FULL", 0, 0, 256, 128, 64, 0.75, -0.5, {}), ("tiled FULL", 1, 1, 128, 256, 48, 2.0, 0.0, {}),
    ("tiled edge", 1, 0, 130, 70, 36, 2.0, 1.0, {}), ("tiled edge", 0, 1, 258, 130, 34, -0.5, 0.0, {}),
    ("scalar", 0, 0, 129, 17, 255, -0.5, 2.0, {}), ("scalar", 1, 1, 151, 95, 71, 0.75, 0.0, dict(offB=1)),
    ("split-K", 0, 0, 130, 70, 2001, 0.75, 0.5, {}), ("split-K", 1, 0, 128, 128, 4096, -1.0, 0.0, {})],
    ids=lambda v: v if isinstance(v, str) else None)
def test_special_values(h, name, ta, tb, M, N, K, alpha, beta, kw):
    """+inf in the last row of op(A) and NaN in the last column of op(B), both at the last k: the same elements are NaN, +inf and
    -inf as in the longdouble reference, and every finite one is within the bound"""
    got, A, B, C0 = run_ex(h, ta, tb, M, N, K, alpha, beta, "uni", 2600, special=True, **kw)
    ref, E = gc.ref_gemm(ta, tb, alpha, A, B, beta, C0)
    _record("special", gc.assert_within_bound(got, ref, E, K))
    assert np.isnan(got[:, N - 1]).all() and np.isinf(got[M - 1, :N - 1]).all() and np.isfinite(got[:M - 1, :N - 1]).all()
