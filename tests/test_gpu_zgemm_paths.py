"""Every kernel path of the complex GEMM (zgemm.hip: nd4_zgemm, reached through nd4hip_zgemm_batched_dev), checked ELEMENT BY ELEMENT
against a reference of higher precision.

zgemm_kernel<BC, VEC, FULL> is the second-hottest kernel after the real GEMM, from which it is derived: the same XCD-aware tile map,
double-buffered LDS and predicated edges, so a path can be wrong while every norm-wise test at friendly shapes passes. The reference
is the real embedding of the complex product (zgemm_common.py, on top of gemm_common.py). Each case runs twice:

  integer family   Re and Im integers in [-4, 4]: the result must EQUAL the integer product of the embedding (no tolerance); this is
                   what names a dropped, doubled, misplaced or sign-flipped term
  uniform family   seeded uniform [-1, 1): every element of the real view within gamma_{n+35} E of the longdouble reference, n = 2K for
                   CC and K for CR and RC. The bound holds for any summation order, so a rewrite of the main loop must still meet it.

Operands are the real views of the interleaved data inside device buffers that hold NaN everywhere else (rows before and after,
whatever lies between two members of a batch, an optional 8-byte shift of the base). One out-of-range element that is loaded and used
makes the result NaN. C is uploaded FULL OF NaN (the kernel must not read it), read back whole, and everything outside the batch of
I x 2J windows must be bit-identical to what was uploaded; A's and B's buffers must be unchanged.

Case -> instantiation -> condition in nd4_zgemm that sends it there (tile 128 x 64 complex, K step 8; shapes are I x K x J; CC and CR
unless stated; zgemm_common.path_of is the model of the condition and every case asserts the path it names against it):

  FULL    zgemm_kernel<BC, true, true>    vec && I % 128 == 0 && J % 64 == 0 && K % 8 == 0 && K > 0 (CR: B aligned, strideB even)
    128x8x64 (one K step: the prefetch branch never runs), 128x24x64, 256x40x128, 128x200x64 (25 K steps)
    1408x24x192: 11 x 3 = 33 tiles, count % 8 = 1, short last group of tile rows: every branch of the XCD map by itself
    1152x8x64, 128x8x576, 2176x8x192: 9 x 1, 1 x 9, 17 x 3 tiles
  edge    zgemm_kernel<BC, true, false>   vec (16-byte aligned bases) but not FULL
    129x9x65, 127x7x63, 1x1x1, 2x34x2, 130x17x1 (CR: the x + 1 < X predicate), 70x13x37 (odd J: a real B's rows start at odd doubles)
    1290x20x194: 11 x 4 = 44 tiles with an edge on both sides; 130 x K x 70, K in 1..7, 9, 12, 15, 17, 23: every K % 8
  scalar  zgemm_kernel<BC, false, false>  !vec, one trigger at a time: A shifted by 8 bytes | B shifted (CC) | C shifted | all three
    each at 128x16x64 (FULL otherwise) and at 150x21x94
  CR off FULL  <false, true, false>       128x16x64, A and C aligned: a real B shifted by 8 bytes; strideB = K J + 1 in a batch of 3
  batches  batch 3 of 130x19x70 and of 128x16x64: equal strides | strideA = I K + 3, strideB = K J + 5 with NaN between the members |
           strideA = 0 | strideB = 0
           batch 32770 of 2x3x2 (CC, CR, RC): the second chunk of the entry point's loop, per-member strides and strideB = 0;
           integer family only, every member compared
  RC      nd4_gemm on the real views: 37x29x45, batch 3 of 70x13x37 with an odd strideA (the rest is test_gpu_gemm_paths.py)
  K = 0   128x0x64 and batch 2 of 5x0x7, A and B NULL: C is all +0
  special +inf in Re A[I-1, K-1], NaN in Im B[K-1, J-1] (CR: in B[K-1, J-1]): the last row, column and k of an edge tile, where the
          zero-filled lanes meet them; once per instantiation. A with inf + 0i and a finite real B, once per CR instantiation: no NaN
          in Im C.
  twice   once per instantiation: a second run gives the same bits

A case above 3e7 products of the embedding would run the integer family alone, against float64 BLAS, which is exact there. The largest
|err| / (gamma E) of the uniform family is printed per path at the end of the module (pytest -s) as a record of the margin; the
assertion is the derived bound."""
import ctypes

import numpy as np
import pytest

import gemm_common as gc
import zgemm_common as zc

pytestmark = pytest.mark.gpu
STATS = {}
PATHS = ("CC full", "CC edge", "CC scalar", "CR full", "CR edge", "CR scalar", "RC")
CX = ("CC", "CR")


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
    print("\npath: runs, largest |err| / (gamma_{n+35} E) of the uniform family")
    for path in PATHS:
        runs, worst = STATS.get(path, (0, 0.0))
        print("  %-12s %6d  %.4f" % (path, runs, worst))


def _record(path, ratio=None):
    s = STATS.setdefault(path, [0, 0.0])
    s[0] += 1
    if ratio is not None:
        s[1] = max(s[1], ratio)


def _upload(p):
    p.upload()
    assert p.dev.data_ptr() % 16 == 0                       # so that the base is 16-byte aligned exactly when p.start is even
    return p


def _sid(v):
    return "x".join(map(str, v)) if isinstance(v, tuple) else None


def run(h, pairing, batch, I, K, J, fam, seed, offA=0, offB=0, offC=0, strideA=None, strideB=None, special=None, null=False):
    """one nd4hip_zgemm_batched_dev call on NaN-guarded operands -> (C, A, B) as real views with the batch axis in front (a
    broadcast operand has one member). strideA / strideB count elements of each operand: None is dense, 0 a broadcast."""
    from nd4js_amd import _lib
    ea, eb = zc.widths(pairing)
    na, nb = (1 if strideA == 0 else batch), (1 if strideB == 0 else batch)
    sA, sB = (I * K if strideA is None else strideA), (K * J if strideB is None else strideB)
    pa = gc.Padded(I, ea * K, ea * K, offset=offA, batch=na, stride=ea * sA if na > 1 else None)
    pb = gc.Padded(K, eb * J, eb * J, offset=offB, batch=nb, stride=eb * sB if nb > 1 else None)
    pc = gc.Padded(I, 2 * J, 2 * J, offset=offC, batch=batch)            # stays NaN: the kernel must not read C
    assert (pa.start % 2, pb.start % 2, pc.start % 2) == (offA % 2, offB % 2, offC % 2)
    A, B = zc.operands(pairing, fam, seed, na, nb, I, K, J)
    if special:
        A[0, I - 1, ea * (K - 1)] = np.inf
        if special == "inf only":
            A[0, I - 1, ea * (K - 1) + 1] = 0.0             # inf + 0i
        else:
            B[0, K - 1, eb * (J - 1) + eb - 1] = np.nan
    pa.win[...] = A.reshape(pa.win.shape)
    pb.win[...] = B.reshape(pb.win.shape)
    for p in (pa, pb, pc):
        _upload(p)
    nil = ctypes.c_void_p(None)
    _lib.check(h.lib.nd4hip_zgemm_batched_dev(h.ptr, ea - 1, eb - 1, batch, I, K, J, nil if null else pa.ptr, sA if na > 1 else 0,
                                              nil if null else pb.ptr, sB if nb > 1 else 0, pc.ptr))
    got = pc.download().reshape(batch, I, 2 * J)
    pa.assert_unchanged()
    pb.assert_unchanged()
    return got, A, B


def check(h, path, pairing, batch, I, K, J, seed=4000, families=("int", "uni"), twice=False, **kw):
    sB = kw.get("strideB")
    passed = 0 if batch == 1 or sB == 0 else K * J if sB is None else sB
    assert zc.path_of(pairing, I, K, J, kw.get("offA", 0), kw.get("offB", 0), kw.get("offC", 0), passed) == path
    blas = zc.products(pairing, I, K, J) > zc.BLAS_ABOVE
    for fam in (("int",) if blas else families):
        got, A, B = run(h, pairing, batch, I, K, J, fam, seed, **kw)
        if fam == "int":
            gc.assert_exact(got, zc.exact(pairing, A, B, blas=blas))
            for _ in range(batch):
                _record(path)
        else:
            for b in range(batch):
                ref, E, n = zc.ref(pairing, A[b if len(A) > 1 else 0], B[b if len(B) > 1 else 0])
                _record(path, gc.assert_within_bound(got[b], ref, E, n))
        assert np.isfinite(got).all()                       # (the comparisons above name the elements; C held NaN before the call)
        if twice:
            again = run(h, pairing, batch, I, K, J, fam, seed, **kw)[0]
            assert np.array_equal(again.view(np.uint64), got.view(np.uint64))


# -------------------------------------------------------------------------------------------------------------------------- FULL
@pytest.mark.parametrize("pairing", CX)
@pytest.mark.parametrize("shape", zc.FULL_SHAPES, ids=_sid)
def test_full(h, pairing, shape):
    check(h, pairing + " full", pairing, 1, *shape, seed=4100 + shape[0])


# -------------------------------------------------------------------------------------------------------------------------- edge
@pytest.mark.parametrize("pairing", CX)
@pytest.mark.parametrize("shape", zc.EDGE_SHAPES, ids=_sid)
def test_edge(h, pairing, shape):
    check(h, pairing + " edge", pairing, 1, *shape, seed=4200 + shape[1])


# ------------------------------------------------------------------------------------------------------------------------ scalar
SCALAR = [("CC", "A shifted", dict(offA=1)), ("CC", "B shifted", dict(offB=1)), ("CC", "C shifted", dict(offC=1)),
          ("CC", "all shifted", dict(offA=1, offB=1, offC=1)), ("CR", "A shifted", dict(offA=1)), ("CR", "C shifted", dict(offC=1)),
          ("CR", "all shifted", dict(offA=1, offB=1, offC=1))]


@pytest.mark.parametrize("pairing,what,kw", SCALAR, ids=["%s %s" % s[:2] for s in SCALAR])
@pytest.mark.parametrize("shape", [(128, 16, 64), (150, 21, 94)], ids=_sid)
def test_scalar_one_trigger(h, pairing, what, kw, shape):
    """the unshifted (128, 16, 64) is FULL and the unshifted (150, 21, 94) is on the 16-byte edge path, so each shift is the only
    reason for the 8-byte path; the NaN in front of and behind each shifted operand is what a wrongly granted 16-byte access takes in"""
    assert zc.path_of(pairing, *shape).endswith(" full" if shape[0] == 128 else " edge")
    check(h, pairing + " scalar", pairing, 1, *shape, seed=4300, **kw)


@pytest.mark.parametrize("shape", [(128, 16, 64), (150, 21, 94)], ids=_sid)
def test_cr_real_b_at_an_odd_double(h, shape):
    """vec && !full: 16-byte loads of A and stores of C, 8-byte loads of the real B"""
    check(h, "CR edge", "CR", 1, *shape, seed=4400, offB=1)


def test_cr_odd_stride_b_leaves_full(h):
    I, K, J = 128, 16, 64
    check(h, "CR edge", "CR", 3, I, K, J, seed=4500, strideB=K * J + 1)
    check(h, "CC full", "CC", 3, I, K, J, seed=4500, strideB=K * J + 1)   # (complex elements are 16 bytes whatever the stride)


# ----------------------------------------------------------------------------------------------------------------------- batches
LAYOUTS = {"equal": lambda I, K, J: {}, "gaps": lambda I, K, J: dict(strideA=I * K + 3, strideB=K * J + 5),
           "strideA=0": lambda I, K, J: dict(strideA=0), "strideB=0": lambda I, K, J: dict(strideB=0)}


@pytest.mark.parametrize("pairing", CX)
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("shape", [(130, 19, 70), (128, 16, 64)], ids=_sid)
def test_batch_of_three(h, pairing, layout, shape):
    kw = LAYOUTS[layout](*shape)
    odd_real_b = pairing == "CR" and layout == "gaps"       # strideB = K J + 5 is odd: a real B leaves FULL
    path = pairing + (" full" if shape[0] == 128 and not odd_real_b else " edge")
    check(h, path, pairing, 3, *shape, seed=4600, **kw)


@pytest.mark.parametrize("pairing", zc.PAIRINGS)
@pytest.mark.parametrize("bcast", [False, True], ids=["per member", "strideB=0"])
def test_batch_of_32770_runs_two_chunks(h, pairing, bcast):
    """members 32768 and 32769 are the second chunk: its offsets 2 b0 strideA, (2 or 1) b0 strideB and 2 b0 I J"""
    path = "RC" if pairing == "RC" else pairing + " edge"
    check(h, path, pairing, 32770, 2, 3, 2, seed=4700, families=("int",), **(dict(strideB=0) if bcast else {}))


# ---------------------------------------------------------------------------------------------------------------------------- RC
def test_rc(h):
    check(h, "RC", "RC", 1, 37, 29, 45, seed=4800)
    check(h, "RC", "RC", 3, 70, 13, 37, seed=4801, strideA=70 * 13 + 1)


# ------------------------------------------------------------------------------------------------------------------------- K = 0
@pytest.mark.parametrize("pairing", zc.PAIRINGS)
@pytest.mark.parametrize("batch,I,J", [(1, 128, 64), (2, 5, 7)])
def test_k_zero(h, pairing, batch, I, J):
    """nothing is read (A and B are NULL) and C, which held NaN, is all +0"""
    got = run(h, pairing, batch, I, 0, J, "int", 4900, null=True)[0]
    assert got.shape == (batch, I, 2 * J) and not got.view(np.uint64).any()
    _record(zc.path_of(pairing, I, 0, J))


# ------------------------------------------------------------------------------------------- once per instantiation (and once for RC)
INSTANCES = [("CC full", "CC", (256, 40, 128), {}), ("CC edge", "CC", (129, 9, 65), {}), ("CC scalar", "CC", (150, 21, 94), dict(offA=1)),
             ("CR full", "CR", (256, 40, 128), {}), ("CR edge", "CR", (129, 9, 65), {}), ("CR scalar", "CR", (150, 21, 94), dict(offC=1)),
             ("RC", "RC", (129, 9, 65), {})]
IIDS = [i[0] for i in INSTANCES]


@pytest.mark.parametrize("path,pairing,shape,kw", INSTANCES, ids=IIDS)
def test_special_values(h, path, pairing, shape, kw):
    """+inf in the last row of Re A and NaN in the last column of Im B (of B for CR), both at the last k: the same elements are NaN,
    +inf and -inf as in the longdouble reference of the embedding, and every finite one is within the bound"""
    I, K, J = shape
    assert zc.path_of(pairing, I, K, J, **kw) == path
    got, A, B = run(h, pairing, 1, I, K, J, "uni", 5000, special="inf and nan", **kw)
    ref, E, n = zc.ref(pairing, A[0], B[0])
    _record(path, gc.assert_within_bound(got[0], ref, E, n))
    c = zc.to_complex(got[0])
    assert np.isnan(c[:, J - 1].imag).all() and np.isfinite(got[0, :I - 1, :2 * (J - 1)]).all()
    # (RC: the NaN sits in Im B alone, and Re C is A Br)
    assert np.isfinite(c[:I - 1, J - 1].real).all() if pairing == "RC" else np.isnan(c[:, J - 1].real).all()
    last = c[I - 1, :J - 1]
    assert np.isinf(last.real).all() and (np.isfinite(last.imag) if pairing == "CR" else np.isinf(last.imag)).all()


@pytest.mark.parametrize("path,pairing,shape,kw", INSTANCES[3:6], ids=IIDS[3:6])
def test_cr_infinity_with_zero_imaginary_part(h, path, pairing, shape, kw):
    """A[I-1, K-1] = inf + 0i and a finite real B: Re C gets +-inf, Im C no NaN (CR is not CC with Bi = 0)"""
    I, K, J = shape
    got, A, B = run(h, pairing, 1, I, K, J, "uni", 5100, special="inf only", **kw)
    ref, E, n = zc.ref(pairing, A[0], B[0])
    _record(path, gc.assert_within_bound(got[0], ref, E, n))
    c = zc.to_complex(got[0])
    assert not np.isnan(got).any() and np.isinf(c[I - 1].real).all() and np.isfinite(c.imag).all() and np.isfinite(c[:I - 1]).all()


@pytest.mark.parametrize("path,pairing,shape,kw", INSTANCES[:6], ids=IIDS[:6])
def test_second_run_gives_the_same_bits(h, path, pairing, shape, kw):
    check(h, path, pairing, 1, *shape, seed=5200, families=("uni",), twice=True, **kw)
