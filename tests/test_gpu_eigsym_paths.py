"""The default route of eigen_sym / eigenvals_sym (csrc/syev.hip, algo None / 'dc') stage by stage. test_gpu_eigsym.py holds the
route end to end to 1e-12 ||S||_F, of which the device uses a thousandth; here its own kernels (syev_absmax_lower, syev_symm,
syev_shift_chol, syev_values) are pinned bit for bit.

  composition   syev.hip's own arithmetic is exact or rounded once, so eigen_sym must equal, in every bit of lambda and V,
                eigsym_common.compose(): numpy for syev.hip's part around the device's own hessenberg_decomp, bidiag_svd and
                nd4hip_dgemm_ex_dev, on the tile edges of syev_symm, on batches that mix dense, scaled, diagonal, zero and
                tridiagonal members, and on every route of the reduction that eigen_sym reaches.
  exact scale   2^k S has 2^k lambda and the bits of V, k = -1000 ... 1000, member by member in one batch; subnormal input; the
                top of the range, max|s| = 0.625 2^1024.
  diagonal      the rank sort of syev_values and the `offdiag` flag: unsorted diagonals with ties and negatives, single and
                between dense members; one off-diagonal pair in each lane pass.
  NaN / Inf     at the corners, next to the diagonal and in every tile of the lower triangle, on a dense and on a diagonal S:
                code -3 and a usable handle. On a diagonal S a NaN below the subdiagonal never reaches d or e (hess.hip skips
                the row: fmax(0, NaN) = 0); syev_shift_chol catches it from max|s_ij| of step 1.
  accuracy      the device's shares of the three bounds within 4 x the numpy model's (the model is the reference).

Mutants of csrc/syev.hip (one at a time, on the device, not committed) and the tests that catch each:
  mx[0] for mx[b] in syev_values              test_route_equals_its_public_pieces (mixed_7x40, mixed_3x65, scaled_7x40, every
                                              diag_in_batch_N), test_scaled_batch_is_exact_member_by_member,
                                              test_diagonal_members_are_sorted_exactly (the dense neighbours)
  kexp[0] for kexp[b]                         test_route_equals_its_public_pieces (mixed_7x40, mixed_3x65, every diag_in_batch_N),
                                              test_diagonal_members_are_sorted_exactly (N >= 5)
  offdiag from the first 64 entries only      test_one_off_diagonal_pair_is_not_a_diagonal_member (65, 129) and the same inputs in
                                              test_route_equals_its_public_pieces
  rank ties broken by descending index        test_route_equals_its_public_pieces (diag_64, diag_65, diag_130, their batches and
                                              both mixed batches: the columns of V of tied values change places)
  contraction in syev_shift_chol              test_route_equals_its_public_pieces (every dense input from N = 3 up),
                                              test_every_route_of_the_reduction (all four)
  mirrored store of syev_symm: tile[r][c]     nearly everything: the compositions, the scale tests, the accuracy gate (44 tests)
  the entrance check taken out again          test_nan_or_inf_anywhere_in_the_lower_triangle_is_noconv (3, 40, 130 diagonal, and
                                              3 dense: row 2 of a 3 x 3 S has a single entry left of the subdiagonal, so a NaN
                                              at (2, 0) was passed over on dense input too)
  the unit rows of V2 of a diagonal member    test_diagonal_members_are_sorted_exactly (5, 64, 130: the solver's rows carry entries
  not written (the solver's rows instead)     like 6.1e-17 and rotated tied pairs), test_route_equals_its_public_pieces (diag_N)"""
import numpy as np
import pytest

import eigsym_common as C
from nd4js_amd import _lib, la

pytestmark = pytest.mark.gpu

MESSAGE = "eigen_sym(S): S contains NaN or Infinity in its lower triangle."


def _dev():
    import torch
    from nd4js_amd import dev
    return torch, dev


def _eigen_sym(S):
    """eigen_sym on the device tensor (the whole batch in one call of nd4_syevd), with eigenvals_sym and the host form held to
    the same bits"""
    torch, dev = _dev()
    t = torch.from_numpy(np.array(S)).cuda()
    lam, V = dev.eigen_sym(t)
    lam, V = lam.cpu().numpy(), V.cpu().numpy()
    assert C.same_bits(dev.eigenvals_sym(t).cpu().numpy(), lam), "eigenvals_sym must have eigen_sym's bits"
    l2, v2 = la.eigen_sym(S)
    assert C.same_bits(l2, lam) and C.same_bits(v2, V) and C.same_bits(la.eigenvals_sym(S), lam)
    return lam, V


def _assert_composed(S, lam, V, what):
    """lambda and V of the route against compose() on the device's own pieces, bit for bit. V = U V2^T is one call of nd4_gemm
    over the batch inside the route and one call per member in compose(); gemm.hip picks its kernel from M, N, K, the leading
    dimensions and alignment, all equal here, and splits K only for K >= 512 by the number of tiles, which differs between the
    two only for batches (none here has N >= 512): no path depends on the batch count, so V is held to the bits as well."""
    lc, Vc, parts = C.compose(S)
    assert C.same_bits(lam, lc), "%s: lambda differs from its composition by %.3g (kinds %s)" % (what, np.abs(lam - lc).max(), parts["kind"])
    assert C.same_bits(V, Vc), "%s: V differs from its composition by %.3g" % (what, np.abs(V - Vc).max())
    return parts


@pytest.mark.parametrize("name", C.PATH_NAMES)
def test_route_equals_its_public_pieces(name):
    S, lam_ref = C.path_reference(name)
    lam, V = _eigen_sym(S)
    parts = _assert_composed(S, lam, V, name)
    sh = C.check_scaled(S, lam, V, lam_ref, name)
    print("%s kinds %s e1 %s shares %.3g %.3g %.3g" % ((name, parts["kind"], parts["e1"].tolist()) + sh))
    # the upper triangle is not read
    l2, v2 = la.eigen_sym(C.with_upper(S, np.nan))
    assert C.same_bits(l2, lam) and C.same_bits(v2, V)


@pytest.mark.parametrize("name", sorted(C.HESS_ROUTES))
def test_every_route_of_the_reduction(name, monkeypatch):
    """nd4_gehrd inside nd4_syevd: one launch (one matrix, 256 <= N <= 2048), blocked (one matrix, even N >= 512, under
    ND4HIP_HESS_NO_PERSIST), per step with U formed from the stored reflectors (batch <= 4, N >= 256), per step with U dragged
    along (batch 5). compose() reduces the same batch in one call under the same setting, so it takes the same route."""
    if C.HESS_ROUTES[name][1]:
        monkeypatch.setenv("ND4HIP_HESS_NO_PERSIST", "1")
    else:
        monkeypatch.delenv("ND4HIP_HESS_NO_PERSIST", raising=False)
    S, lam_ref = C.path_reference(name)
    lam, V = _eigen_sym(S)
    _assert_composed(S, lam, V, name)
    sh = C.check(S, lam, V, lam_ref, name)
    print("%s shares %.3g %.3g %.3g" % ((name,) + sh))


def test_scaled_batch_is_exact_member_by_member():
    ks = C.SCALE_KS
    S = C.path_reference("scaled_7x40")[0]
    l0, v0 = _eigen_sym(C.base_40())
    lam, V = _eigen_sym(S)
    for b, k in enumerate(ks):
        assert C.same_bits(lam[b], np.ldexp(l0, k)), "member %d (2^%d): lambda" % (b, k)
        assert C.same_bits(V[b], v0), "member %d (2^%d): V" % (b, k)
    # other places, other neighbours, another batch size: the results follow their members
    R = np.concatenate([S[::-1], S[::-1][:2]])
    l2, v2 = _eigen_sym(R)
    for b, k in enumerate(ks[::-1] + ks[::-1][:2]):
        assert C.same_bits(l2[b], np.ldexp(l0, k)) and C.same_bits(v2[b], v0), "reversed member %d (2^%d)" % (b, k)


@pytest.mark.parametrize("N", [5, 40])
def test_subnormal_input(N):
    G = C.path_reference("grid_%d" % N)[0]
    lg, vg = _eigen_sym(G)
    lam, V = _eigen_sym(np.ldexp(G, -1074))
    assert C.same_bits(lam, np.ldexp(lg, -1074)) and C.same_bits(V, vg)


@pytest.mark.parametrize("N", [3, 65])
def test_top_of_the_range(N):
    """max|s| = 0.625 2^1024, e1 = 1024; ||S||_F would overflow and is not formed"""
    T = C.path_reference("top_base_%d" % N)[0]
    lt, vt = _eigen_sym(T)
    S = np.ldexp(T, 1024)
    lam, V = _eigen_sym(S)
    assert np.all(np.isfinite(lam)) and C.same_bits(lam, np.ldexp(lt, 1024)) and C.same_bits(V, vt)
    _assert_composed(S, lam, V, "top_%d" % N)


def _assert_diagonal_result(d, lam, V, what):
    N = len(d)
    assert np.array_equal(lam, np.sort(d)[::-1]), what
    nz = V != 0.0
    assert np.array_equal(nz.sum(axis=0), np.ones(N)) and np.array_equal(nz.sum(axis=1), np.ones(N)), what
    assert np.array_equal(np.abs(V[nz]), np.ones(N)), what
    assert np.array_equal(np.diag(d) @ V, V * lam), what                     # every product is exact: S V = V diag(lambda) elementwise


@pytest.mark.parametrize("N", [2, 5, 64, 65, 130])
def test_diagonal_members_are_sorted_exactly(N):
    S = C.path_reference("diag_%d" % N)[0]
    lam, V = _eigen_sym(S)
    _assert_diagonal_result(np.diag(S), lam, V, "diag_%d" % N)
    B = C.path_reference("diag_in_batch_%d" % N)[0]
    lb, vb = _eigen_sym(B)
    _assert_diagonal_result(np.diag(S), lb[1], vb[1], "diag_in_batch_%d" % N)
    for b in (0, 2):                                                         # the dense neighbours are their single runs
        l1, v1 = _eigen_sym(B[b])
        assert C.same_bits(lb[b], l1) and C.same_bits(vb[b], v1), "diag_in_batch_%d member %d" % (N, b)


@pytest.mark.parametrize("i", C.PAIR_ROWS)
def test_one_off_diagonal_pair_is_not_a_diagonal_member(i):
    """the only non-zero of e at index i - 1 = 0, 63, 64, 128: the first lane pass of `offdiag`, its last lane, the second pass,
    the third. Taken for diagonal, lambda is wrong by up to 0.375."""
    name = "pair_130_at_%d" % i
    S, lam_ref = C.path_reference(name)
    lam, V = _eigen_sym(S)
    C.check(S, lam, V, lam_ref, name)
    parts = _assert_composed(S, lam, V, name)
    assert np.flatnonzero(parts["e"][0]).tolist() == [i - 1] and parts["kind"] == ("dense",)


def _bad_places(N):
    places = [(0, 0), (N - 1, N - 1), (N - 1, 0), (N - 1, N - 2)]
    if N == 130:                                                             # one in each lower tile of the 64-tiling
        places += [(33, 7), (97, 9), (101, 77), (128, 31), (129, 90), (128, 128)]
    return places


@pytest.mark.parametrize("kind", ["dense", "diagonal"])
@pytest.mark.parametrize("N", [3, 40, 130])
def test_nan_or_inf_anywhere_in_the_lower_triangle_is_noconv(N, kind):
    S = np.array(C.sym_uniform(C.PATH_SEED + 700 + N, N) if kind == "dense" else np.diag(C.half_steps(C.PATH_SEED + 800 + N, N)))
    before = la.eigen_sym(S)
    for bad in (np.nan, np.inf, -np.inf):
        for r, c in _bad_places(N):
            X = S.copy()
            X[r, c] = bad
            for fn in (la.eigen_sym, la.eigenvals_sym):
                with pytest.raises(_lib.Nd4HipError) as e:
                    fn(X)
                assert e.value.code == -3 and MESSAGE in str(e.value), (bad, r, c)
            after = la.eigen_sym(S)
            assert C.same_bits(after[0], before[0]) and C.same_bits(after[1], before[1]), (bad, r, c)
        # a batch of three with the bad member in the middle
        for r, c in ((N - 1, 0), (0, 0)):
            B = np.stack([S, S, S])
            B[1, r, c] = bad
            for fn in (la.eigen_sym, la.eigenvals_sym):
                with pytest.raises(_lib.Nd4HipError) as e:
                    fn(B)
                assert e.value.code == -3 and MESSAGE in str(e.value), (bad, r, c)
        after = la.eigen_sym(np.stack([S, S, S]))
        for b in range(3):
            assert C.same_bits(after[0][b], before[0]) and C.same_bits(after[1][b], before[1])


@pytest.mark.parametrize("name", C.SMALL)
def test_device_shares_within_four_times_the_models(name):
    """Gate per input and bound: device share <= 4 x max(model share, N 2^-52 / 1e-12), the margin test_gpu_schur.py grants
    another rotation path of the same length; the floor is for inputs the model solves exactly. The model (eigsym_common.model,
    numpy) is the reference, computed here. Measured worst ratios device / gate over the catalogue: values 0.083 (dense_3), residual
    0.18 (zdiag_tri_3), orthogonality 0.21 (dense_3); every input with N > 3 stays below 0.06 of its gate."""
    S, lam_ref, _ = C.reference(name)
    N = S.shape[-1]
    lm, vm, _ = C.model_batch(S)
    model = C.shares(S, lm, vm, lam_ref)
    lam, V = la.eigen_sym(S)
    device = C.check(S, lam, V, lam_ref, name)
    floor = N * C.EPS / C.TOL
    rows = [(what, dv, md, 4.0 * max(md, floor)) for what, dv, md in zip(("values", "residual", "orthogonality"), device, model)]
    for what, dv, md, gate in rows:
        print("%s %s: device %.3g model %.3g gate %.3g ratio %.3g" % (name, what, dv, md, gate, dv / gate))
    for what, dv, md, gate in rows:
        assert dv <= gate, "%s %s: the device's share %.3g exceeds 4 x max(model %.3g, floor %.3g)" % (name, what, dv, md, floor)
