"""Shared helpers of the complex GEMM path tests (test_zgemm_ref_host.py, test_gpu_zgemm_paths.py): the reference of a complex product
by REAL EMBEDDING, on top of gemm_common.py, which is used as it is.

Operands are handled as their interleaved real views, the layout the kernels read: a complex I x K matrix is an I x 2K float64 matrix
[re, im, re, im, ...]. A complex product is a real product over the same set of elementary products:

  CC   A' = [Ar | Ai] (I x 2K)  times  B' (2K x 2J): rows 0..K-1 hold Br in the even and Bi in the odd columns, rows K..2K-1 hold -Bi in
       the even and Br in the odd columns. A' @ B' is the interleaved I x 2J real view of C; inner extent 2K.
  CR   [Ar ; Ai] (2I x K) times the real B: rows 0..I-1 are Re C, rows I..2I-1 are Im C; inner extent K. Never CC with Bi = 0: that
       would add the products Ai * 0 and Ar * 0, and (inf + 0i) * x would get a NaN that the reference's loop never forms.
  RC   the real A times the K x 2J real view of B; inner extent K.

The embedding adds no product and drops none (test_zgemm_ref_host.py compares it with exact rationals), so gemm_common's longdouble
reference, its NaN / +inf / -inf mask comparison and its bound carry over: every element of the real view of a float64 result computed
in any order, with or without FMA, is within gamma_{n+35} E of the exact one, n = 2K for CC and n = K for CR and RC, E = |A'| |B'|
(Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., section 3.1). Derived, not measured.

Integer family: Re and Im are integers in [-4, 4]; the result must equal the integer product of the embedding, no tolerance."""
import numpy as np

import gemm_common as gc

PAIRINGS = ("CC", "CR", "RC")
ZBM, ZBN, ZBK = 128, 64, 8                                 # zgemm.hip: macro tile in complex elements, K step
BLAS_ABOVE = 3e7                                           # embedded products above which a case runs the integer family alone


def widths(pairing):
    """doubles per element of A and of B"""
    return (2 if pairing[0] == "C" else 1), (2 if pairing[1] == "C" else 1)


def operands(pairing, fam, seed, na, nb, I, K, J):
    """real views (na, I, ea K) and (nb, K, eb J) of the seeded family"""
    ea, eb = widths(pairing)
    gen = gc.FAMILIES[fam]
    return gen(seed, na, I, ea * K), gen(seed + 1, nb, K, eb * J)


def to_complex(view):
    return np.ascontiguousarray(view).view(np.complex128)


# --------------------------------------------------------------------------------------------------------------------- embedding
def _interleave(P, I):
    out = np.empty(P.shape[:-2] + (I, 2 * P.shape[-1]), dtype=P.dtype)
    out[..., 0::2] = P[..., :I, :]
    out[..., 1::2] = P[..., I:, :]
    return out


def _unstack(P, I):
    """(2I x J) [Re ; Im] -> the interleaved I x 2J view, for arrays and for gemm_common's (hi, lo) pairs"""
    if isinstance(P, gc.Pair):
        out = _interleave(np.asarray(P), I).view(gc.Pair)
        out.lo = _interleave(np.asarray(P.lo), I)
        return out
    return _interleave(np.asarray(P), I)


def embed(pairing, Av, Bv):
    """(A', B', n, unpack): real matrices whose product, passed through `unpack`, is the I x 2J real view of C; n is the inner extent.
    Leading (batch) axes are carried along."""
    Av, Bv = np.asarray(Av, dtype=np.float64), np.asarray(Bv, dtype=np.float64)
    if pairing == "CC":
        K, J = Bv.shape[-2], Bv.shape[-1] // 2
        Br, Bi = Bv[..., 0::2], Bv[..., 1::2]
        A2 = np.concatenate([Av[..., 0::2], Av[..., 1::2]], axis=-1)
        B2 = np.empty(Bv.shape[:-2] + (2 * K, 2 * J))
        B2[..., :K, 0::2], B2[..., :K, 1::2] = Br, Bi
        B2[..., K:, 0::2], B2[..., K:, 1::2] = -Bi, Br
        return A2, B2, 2 * K, lambda P: P
    if pairing == "CR":
        I = Av.shape[-2]
        return np.concatenate([Av[..., 0::2], Av[..., 1::2]], axis=-2), Bv, Bv.shape[-2], lambda P: _unstack(P, I)
    assert pairing == "RC"
    return Av, Bv, Bv.shape[-2], lambda P: P


def ref(pairing, Av, Bv):
    """(ref, E, n) of one product (no batch axis): the real view of C and its envelope in the reference precision"""
    A2, B2, n, unpack = embed(pairing, Av, Bv)
    r, E = gc.ref_gemm(0, 0, 1.0, A2, B2, 0.0, None)
    return unpack(r), unpack(E), n


def exact(pairing, Av, Bv, blas=False):
    """the integer family's result, real view; leading batch axes allowed (a broadcast operand keeps a leading 1)"""
    A2, B2, _, unpack = embed(pairing, Av, Bv)
    return unpack(gc.exact_gemm(0, 0, 1.0, A2, B2, 0.0, None, blas=blas))


def products(pairing, I, K, J):
    """elementary products of the embedding = cost of the reference"""
    return (4 if pairing == "CC" else 2) * I * K * J


# ------------------------------------------------------------------------------------------- model of the dispatch in zgemm.hip
def path_of(pairing, I, K, J, offA=0, offB=0, offC=0, strideB=0):
    """the instantiation nd4_zgemm picks: `off*` are the 8-byte shifts of the bases from a 16-byte boundary, strideB is the batch
    stride as passed (elements of B; 0 for one member or a broadcast). A model, not the kernel."""
    if pairing == "RC":
        return "RC"
    bc = pairing == "CC"
    al = lambda off: off % 2 == 0
    vec = al(offA) and al(offC) and (al(offB) or not bc)
    full = vec and I % ZBM == 0 and J % ZBN == 0 and K % ZBK == 0 and K > 0 and (bc or (al(offB) and strideB % 2 == 0))
    return pairing + (" full" if full else " edge" if vec else " scalar")


def map_branches(tiles_m, tiles_n, nxcd=8, group_m=8):
    """which branches of the workgroup -> tile map (zgemm.hip: the same as dgemm_kernel's, gemm_common.tile_of) a grid reaches"""
    nwg = tiles_m * tiles_n
    r = nwg % nxcd
    hit = set()
    for bid in range(nwg):
        hit.add("xcd < r" if bid % nxcd < r else "xcd >= r")
        tm, _ = gc.tile_of(bid, tiles_m, tiles_n, nxcd, group_m)
        first_m = tm // group_m * group_m
        hit.add("short group" if tiles_m - first_m < group_m else "whole group")
        if first_m:
            hit.add("second group")
    return hit


MAP_BRANCHES = {"xcd < r", "xcd >= r", "short group", "whole group", "second group"}

# ------------------------------------------------------------------------------------------------ the cases both modules speak of
FULL_SHAPES = [(128, 8, 64), (128, 24, 64), (256, 40, 128), (1408, 24, 192), (1152, 8, 64), (128, 8, 576), (2176, 8, 192), (128, 200, 64)]
EDGE_SHAPES = ([(129, 9, 65), (127, 7, 63), (1, 1, 1), (2, 34, 2), (130, 17, 1), (70, 13, 37), (1290, 20, 194)] +
               [(130, K, 70) for K in (1, 2, 3, 4, 5, 6, 7, 9, 12, 15, 17, 23)])
HOST_SHAPES = [(130, 19, 70), (257, 13, 65), (1408, 24, 192)]      # where numpy's own product is held to the bound on the CPU


def tiles(I, J):
    return (I + ZBM - 1) // ZBM, (J + ZBN - 1) // ZBN
