"""CPU tests of the complex GEMM checker itself (tests/zgemm_common.py): a check that cannot fail is worth nothing.

The real embeddings of the three complex pairings are pinned to exact rational arithmetic of the complex product as the reference's
loops define it (Re += Ar Br - Ai Bi, Im += Ar Bi + Ai Br), numpy's own complex product must pass the bound check, a list of wrong
products, each of the kind a kernel bug produces, must be refused by it, and the special-value model must reproduce the NaN / Inf masks
of the recorded `special_*` fixtures. The last tests pin the model of the dispatch and the coverage of the tile map by the cases that
test_gpu_zgemm_paths.py runs."""
import json
import os
from fractions import Fraction

import numpy as np
import pytest

from conftest import GOLDEN
import gemm_common as gc
import zgemm_common as zc
from gemm_common import LD

ZDIR = os.path.join(GOLDEN, "zmatmul")


# --------------------------------------------------------------------------------------------------------------------- embedding
def _fraction_product(pairing, Av, Bv):
    """(C, envelope) as exact rationals, both as I x 2J real views, straight from the definition of each pairing"""
    ea, eb = zc.widths(pairing)
    I, K, J = Av.shape[0], Bv.shape[0], Bv.shape[1] // eb
    F = lambda x: Fraction(float(x))
    C = [[Fraction(0)] * (2 * J) for _ in range(I)]
    E = [[Fraction(0)] * (2 * J) for _ in range(I)]
    for i in range(I):
        for j in range(J):
            for k in range(K):
                ar, ai = (F(Av[i, 2 * k]), F(Av[i, 2 * k + 1])) if ea == 2 else (F(Av[i, k]), None)
                br, bi = (F(Bv[k, 2 * j]), F(Bv[k, 2 * j + 1])) if eb == 2 else (F(Bv[k, j]), None)
                if pairing == "CC":
                    re, im = (ar * br, -(ai * bi)), (ar * bi, ai * br)
                elif pairing == "CR":
                    re, im = (ar * br,), (ai * br,)
                else:
                    re, im = (ar * br,), (ar * bi,)
                C[i][2 * j] += sum(re)
                C[i][2 * j + 1] += sum(im)
                E[i][2 * j] += sum(abs(p) for p in re)
                E[i][2 * j + 1] += sum(abs(p) for p in im)
    return C, E


def _to_fraction(x):
    hi = float(x)
    return Fraction(hi) + Fraction(float(x - LD(hi)))


SMALL = [(12, 10, 11), (3, 1, 5), (7, 17, 2), (1, 33, 1)]              # (I, K, J)


@pytest.mark.parametrize("pairing", zc.PAIRINGS)
@pytest.mark.parametrize("I,K,J", SMALL)
def test_embedding_against_exact_rationals(pairing, I, K, J):
    """|ref - exact| <= 2^-60 E elementwise and the envelope to 2^-50: the embedding holds every product of the complex product,
    once, with its sign, and no other; the inner extent it reports is the number of products per element"""
    Av, Bv = zc.operands(pairing, "uni", 3100 + K, 1, 1, I, K, J)
    ref, E, n = zc.ref(pairing, Av[0], Bv[0])
    want, env = _fraction_product(pairing, Av[0], Bv[0])
    assert n == (2 * K if pairing == "CC" else K) and ref.shape == E.shape == (I, 2 * J)
    for i in range(I):
        for j in range(2 * J):
            got = Fraction(float(ref[i, j])) + Fraction(float(ref.lo[i, j])) if isinstance(ref, gc.Pair) else _to_fraction(ref[i, j])
            assert abs(got - want[i][j]) <= Fraction(1, 2 ** 60) * env[i][j], (i, j)
            assert abs(_to_fraction(E[i, j]) - env[i][j]) <= Fraction(1, 2 ** 50) * env[i][j], (i, j)


@pytest.mark.parametrize("pairing", zc.PAIRINGS)
@pytest.mark.parametrize("I,K,J", SMALL)
def test_integer_family_is_exact(pairing, I, K, J):
    Av, Bv = zc.operands(pairing, "int", 3200 + K, 1, 1, I, K, J)
    want, _ = _fraction_product(pairing, Av[0], Bv[0])
    got = zc.exact(pairing, Av[0], Bv[0])
    assert got.shape == (I, 2 * J) and all(Fraction(float(got[i, j])) == want[i][j] for i in range(I) for j in range(2 * J))
    gc.assert_exact(zc.exact(pairing, Av[0], Bv[0], blas=True), got)
    gc.assert_exact(zc.exact(pairing, Av, Bv)[0], got)                       # with a batch axis in front


def _numpy_product(pairing, Av, Bv):
    """numpy's own product of the operands as the user holds them, as a real view"""
    a = zc.to_complex(Av) if pairing[0] == "C" else Av
    b = zc.to_complex(Bv) if pairing[1] == "C" else Bv
    if pairing == "CC":
        return np.ascontiguousarray(a @ b).view(np.float64)
    if pairing == "CR":                                      # (numpy would widen B to complex: the two real products instead)
        c = np.empty((a.shape[0], b.shape[1]), dtype=np.complex128)
        c.real, c.imag = a.real @ b, a.imag @ b
        return c.view(np.float64)
    return a @ Bv


# ------------------------------------------------------------------------------------------- correct products pass the bound check
@pytest.mark.parametrize("pairing", zc.PAIRINGS)
@pytest.mark.parametrize("I,K,J", zc.HOST_SHAPES)
def test_numpy_products_pass_the_bound_check(pairing, I, K, J):
    Av, Bv = zc.operands(pairing, "uni", 3300 + I, 1, 1, I, K, J)
    ref, E, n = zc.ref(pairing, Av[0], Bv[0])
    ratio = gc.assert_within_bound(_numpy_product(pairing, Av[0], Bv[0]), ref, E, n)
    print("%s %d x %d x %d: |err| / (gamma_%d E) = %.4f" % (pairing, I, K, J, n + 35, ratio))
    Ai, Bi = zc.operands(pairing, "int", 3300 + I, 1, 1, I, K, J)
    gc.assert_exact(_numpy_product(pairing, Ai[0], Bi[0]), zc.exact(pairing, Ai[0], Bi[0]))


# ------------------------------------------------------------------------------------------------------ wrong products are refused
def _mutants(Av, Bv, C):
    """(name, wrong CC product, real view), each what one kind of kernel bug gives. (i, j) is a complex element away from every edge."""
    I, K, J = Av.shape[0], Bv.shape[0], Bv.shape[1] // 2
    Ar, Ai, Br, Bi = Av[:, 0::2], Av[:, 1::2], Bv[:, 0::2], Bv[:, 1::2]
    i, j = I // 2, J // 3
    m = C.copy(); m[i, 2 * j] -= Ar[i, K - 1] * Br[K - 1, j]
    yield "one product of the last k dropped", m
    s = Ai[i] @ Bi
    js = int(np.argmax(np.abs(s)))                           # (integers: an element whose sum of Ai Bi is not zero)
    m = C.copy(); m[i, 2 * js] += 2.0 * s[js]
    yield "+Ai Bi in place of -Ai Bi in one element", m
    jw = int(np.argmax(np.abs(C[i, 0::2] - C[i, 1::2])))     # (integers: an element with Re != Im)
    m = C.copy(); m[i, 2 * jw], m[i, 2 * jw + 1] = C[i, 2 * jw + 1], C[i, 2 * jw]
    yield "Re and Im swapped in one element", m
    r = min(zc.ZBM, I - zc.ZBM)                              # the rows of tile row 0 and tile row 1, first tile column
    m = C.copy(); m[:r, :2 * zc.ZBN], m[zc.ZBM:zc.ZBM + r, :2 * zc.ZBN] = C[zc.ZBM:zc.ZBM + r, :2 * zc.ZBN], C[:r, :2 * zc.ZBN]
    yield "one tile's rows exchanged with another's", m


@pytest.mark.parametrize("fam", ["uni", "int"])
@pytest.mark.parametrize("I,K,J", zc.HOST_SHAPES)
def test_checks_refuse_mutants(I, K, J, fam):
    Av, Bv = zc.operands("CC", fam, 3400 + I, 1, 1, I, K, J)
    Av, Bv = Av[0], Bv[0]
    if fam == "int":                                         # (so that the dropped product is not a zero)
        Av[I // 2, 2 * (K - 1)], Bv[K - 1, 2 * (J // 3)] = 3.0, -2.0
    C = _numpy_product("CC", Av, Bv)
    if fam == "uni":
        ref, E, n = zc.ref("CC", Av, Bv)
        gc.assert_within_bound(C, ref, E, n)
        refuse = lambda wrong: gc.assert_within_bound(wrong, ref, E, n)
    else:
        want = zc.exact("CC", Av, Bv)
        gc.assert_exact(C, want)
        refuse = lambda wrong: gc.assert_exact(wrong, want)
    names = []
    for name, wrong in _mutants(Av, Bv, C):
        with pytest.raises(AssertionError):
            refuse(wrong)
        names.append(name)
    assert len(names) == 4


@pytest.mark.parametrize("I,K,J", [(6, 5, 7)] + zc.HOST_SHAPES[:2])
def test_cr_computed_as_cc_with_zero_imaginary_b_is_refused_by_the_nan_mask(I, K, J):
    """A holds inf + 0i. The CR product has +-inf in Re and finite numbers in Im; CC with Bi = 0 forms inf * 0 there."""
    Av, Bv = zc.operands("CR", "uni", 3500 + I, 1, 1, I, K, J)
    Av, Bv = Av[0], Bv[0]
    Av[I - 1, 2 * (K - 1)], Av[I - 1, 2 * (K - 1) + 1] = np.inf, 0.0
    ref, E, n = zc.ref("CR", Av, Bv)
    good = _numpy_product("CR", Av, Bv)
    gc.assert_within_bound(good, ref, E, n)
    assert np.isinf(good[I - 1, 0::2]).all() and np.isfinite(good[I - 1, 1::2]).all() and np.isfinite(good[:I - 1]).all()
    Bz = np.zeros((K, 2 * J))
    Bz[:, 0::2] = Bv
    A2, B2, _, _ = zc.embed("CC", Av, Bz)
    with np.errstate(invalid="ignore"):
        wrong = A2 @ B2
    assert np.isnan(wrong[I - 1, 1::2]).all()
    with pytest.raises(AssertionError, match="nan mask differs"):
        gc.assert_within_bound(wrong, ref, E, n)


# ------------------------------------------------------------------------------------------------ special values: the fixtures
with open(os.path.join(ZDIR, "manifest.json")) as _f:
    SPECIAL = {k: v for k, v in json.load(_f)["cases"].items() if k.startswith("special_")}


def test_the_six_special_fixtures_are_there():
    assert sorted(SPECIAL) == ["special_%s%s" % (p, s) for p in zc.PAIRINGS for s in ("", "_inf_only")]


@pytest.mark.parametrize("name", sorted(SPECIAL))
def test_model_reproduces_the_special_value_fixtures(name):
    """the recorded results of the reference's loops: the model has its NaN, +inf and -inf in the same places (real and imaginary
    parts separately) and agrees on every finite element"""
    meta = SPECIAL[name]
    A, B, C = (np.load(os.path.join(ZDIR, f)) for f in (meta["A"]["file"], meta["B"]["file"], meta["C"]))
    pairing = meta["pairing"]
    assert (A.dtype == np.complex128, B.dtype == np.complex128) == (pairing[0] == "C", pairing[1] == "C")
    Av, Bv, Cv = (np.ascontiguousarray(x).view(np.float64) for x in (A, B, C))
    ref, E, n = zc.ref(pairing, Av, Bv)
    hi = np.asarray(ref, dtype=np.float64)
    assert not np.isfinite(Cv).all()
    for f in (np.isnan, np.isposinf, np.isneginf):
        assert np.array_equal(f(hi), f(Cv)), f.__name__
    gc.assert_within_bound(Cv, ref, E, n)


# ----------------------------------------------------------------------------------------------------- buffers, dispatch, tile map
def test_padded_real_view_of_a_complex_batch():
    """Padded on the real view: cols = ld = 2K, the stride in doubles is twice the complex stride, an odd offset is the 8-byte shift"""
    I, K, sA = 3, 2, 3 * 2 + 5
    p = gc.Padded(I, 2 * K, 2 * K, offset=1, batch=3, stride=2 * sA)
    z = np.arange(3 * I * K).reshape(3, I, K) * (1 + 2j)
    p.win[...] = z.view(np.float64)
    flat = p.buf[p.start:p.start + 2 * (2 * sA + I * K)].view(np.complex128)
    assert p.start % 2 == 1 and np.array_equal(flat[2 * sA:2 * sA + I * K].reshape(I, K), z[2]) and np.isnan(flat[I * K:sA]).all()
    assert gc.Padded(I, 2 * K, 2 * K).start % 2 == 0 and gc.Padded(5, 7, 7).start % 2 == 0


def test_dispatch_model():
    f = zc.path_of
    assert [f("CC", *s) for s in zc.FULL_SHAPES] == ["CC full"] * 8 and [f("CR", *s) for s in zc.FULL_SHAPES] == ["CR full"] * 8
    assert {f(p, *s) for p in ("CC", "CR") for s in zc.EDGE_SHAPES} == {"CC edge", "CR edge"}
    assert f("CC", 128, 16, 64, offA=1) == f("CC", 128, 16, 64, offB=1) == f("CC", 128, 16, 64, offC=1) == "CC scalar"
    assert f("CR", 128, 16, 64, offA=1) == f("CR", 128, 16, 64, offC=1) == "CR scalar"
    assert f("CR", 128, 16, 64, offB=1) == f("CR", 128, 16, 64, strideB=16 * 64 + 1) == "CR edge"       # a real B only leaves FULL
    assert f("CC", 128, 16, 64, strideB=16 * 64 + 1) == "CC full" and f("CR", 128, 16, 64, strideB=16 * 64 + 2) == "CR full"
    assert f("CC", 128, 0, 64) == "CC edge" and f("RC", 128, 16, 64, offA=1) == "RC"


def test_full_cases_reach_every_branch_of_the_tile_map():
    """the XCD-aware map (gemm_common.tile_of; zgemm_kernel computes the same): a remainder of the tile count over the 8 XCDs on both
    sides of `xcd < r`, a whole and a short group of 8 tile rows, a group after the first"""
    grids = [zc.tiles(I, J) for I, _, J in zc.FULL_SHAPES]
    assert grids == [(1, 1), (1, 1), (2, 2), (11, 3), (9, 1), (1, 9), (17, 3), (1, 1)]
    assert set().union(*(zc.map_branches(*g) for g in grids)) == zc.MAP_BRANCHES
    assert zc.map_branches(11, 3) == zc.MAP_BRANCHES and 33 % 8 == 1             # the one case that reaches them all by itself
    for tm, tn in grids + [zc.tiles(1290, 194)]:
        assert {gc.tile_of(b, tm, tn) for b in range(tm * tn)} == {(m, n) for m in range(tm) for n in range(tn)}
