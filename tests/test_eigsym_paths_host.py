"""CPU-side premises of test_gpu_eigsym_paths.py: every new builder of tests/eigsym_common.py is symmetric and seeded, every
exactness premise the device tests rest on holds in float64 (the 2^k scalings and their inverses, the subnormal grid, the top of
the range, the half-step diagonals with their ties and negatives), the numpy model of csrc/syev.hip meets the bounds on each
new finite input and satisfies the scale identities itself, and compose() -- the route restated from its public pieces -- is run
here with numpy stand-ins for the three device calls, so that its glue is tested without a device."""
import numpy as np
import pytest

import eigsym_common as C

ALL = C.PATH_NAMES + tuple(C.HESS_ROUTES)


@pytest.mark.parametrize("name", ALL)
def test_builders_are_symmetric_seeded_and_finite(name):
    S, lam_ref = C.path_reference(name)
    build = C.PATHS[name] if name in C.PATHS else C.HESS_ROUTES[name][0]
    again = np.asarray(build(), dtype=np.float64)
    assert np.array_equal(S, again) and np.array_equal(S, np.swapaxes(S, -1, -2)) and np.all(np.isfinite(S))
    assert S.shape[-1] <= 512 and lam_ref.shape == S.shape[:-1]
    assert not S.flags.writeable


@pytest.mark.parametrize("name", C.PATH_NAMES)
def test_model_meets_the_bounds_on_the_new_inputs(name):
    S, lam_ref = C.path_reference(name)
    lam, V, low = C.model_batch(S)
    assert low > 2.0 ** -21
    C.check_scaled(S, lam, V, lam_ref, name)


@pytest.mark.parametrize("name", C.PATH_NAMES + ("one_launch_1x256",))
def test_compose_with_numpy_stand_ins(name):
    """the glue of compose(): the members' exponents, the mirrored lower triangle, d and e of H, the three kinds of member, the
    back-transformation, the shapes. With the model's own pieces it must give the model's bits on every dense member."""
    S, lam_ref = C.path_reference(name)
    N = S.shape[-1]
    lam, V, parts = C.compose(C.with_upper(S, np.nan), C.numpy_calls())       # the upper triangle is never read
    assert lam.shape == S.shape[:-1] and V.shape == S.shape
    C.check_scaled(S, lam, V, lam_ref, name)
    S3, l3, V3 = S.reshape(-1, N, N), lam.reshape(-1, N), V.reshape(-1, N, N)
    assert len(parts["kind"]) == S3.shape[0] and parts["W"].shape == S3.shape
    for b, s in enumerate(S3):
        assert np.abs(parts["W"][b]).max() < 1.0 and (np.abs(parts["W"][b]).max() >= 0.5 or not s.any())
        assert np.array_equal(parts["W"][b], np.ldexp(s, -parts["e1"][b]))
        want = "zero" if not s.any() else "diag" if not np.any(np.tril(s, -1)) else "dense"
        assert parts["kind"][b] == want, (name, b)
        m_lam, m_V, _ = C.model(s)
        if want == "dense":
            assert C.same_bits(l3[b], m_lam) and C.same_bits(V3[b], m_V), (name, b)
        elif want == "diag":
            assert np.array_equal(l3[b], np.sort(np.diag(s))[::-1])


def test_compose_kinds_of_the_mixed_batches():
    assert C.compose(C.path_reference("mixed_7x40")[0], C.numpy_calls())[2]["kind"] == ("dense",) * 4 + ("diag", "zero", "dense")
    assert C.compose(C.path_reference("mixed_3x65")[0], C.numpy_calls())[2]["kind"] == ("dense", "diag", "dense")
    parts = C.compose(C.path_reference("mixed_7x40")[0], C.numpy_calls())[2]
    assert len(set(parts["e1"][:4])) == 4 and parts["e1"][5] == 0               # reading member 0's exponent for all is visible
    assert not np.all(parts["e"][6]) and np.any(parts["e"][6])                  # zeros in e of the tridiagonal member
    e3 = C.compose(C.path_reference("mixed_3x65")[0], C.numpy_calls())[2]["e1"]
    assert e3[0] != e3[1] and e3[1] != e3[2] and e3[0] != e3[2]


def test_every_catalogue_batch_has_equal_exponents_and_the_new_ones_do_not():
    """the gap this file closes: mx[0] for mx[b] passes every batch of the catalogue"""
    for name in ("batch_5x40", "batch_2x130"):
        assert len(set(C.member_exponents(C.reference(name)[0]))) == 1
    for name in ("mixed_7x40", "mixed_3x65", "scaled_7x40"):
        assert len(set(C.member_exponents(C.path_reference(name)[0]))) >= 3
    for N in (2, 5, 64, 65, 130):
        e1 = C.member_exponents(C.path_reference("diag_in_batch_%d" % N)[0])
        assert e1[1] != e1[0] and e1[1] != e1[2], N


@pytest.mark.parametrize("k", C.SCALE_KS)
def test_scaling_premise_and_model_identity(k):
    base = C.base_40()
    assert np.array_equal(base, C.reference("batch_5x40")[0][0])
    scaled = np.ldexp(base, k)
    assert np.all(np.isfinite(scaled)) and np.array_equal(np.ldexp(scaled, -k), base)
    assert np.array_equal(C.scaled_batch()[C.SCALE_KS.index(k)], scaled)
    lam, V, _ = C.model(base)
    l2, v2, _ = C.model(scaled)
    assert C.same_bits(l2, np.ldexp(lam, k)) and C.same_bits(v2, V)


@pytest.mark.parametrize("N", [5, 40])
def test_subnormal_premise_and_model_identity(N):
    G = C.grid_20(N)
    assert np.array_equal(G, np.rint(G)) and np.abs(G).max() <= 2.0 ** 20 and np.array_equal(G, G.T)
    S = np.ldexp(G, -1074)
    tiny = np.finfo(np.float64).tiny
    assert np.all(np.abs(S) < tiny) and np.array_equal(np.ldexp(S, 1074), G)      # every entry subnormal (or zero), none rounded
    assert C.member_exponents(S[None])[0] == C.member_exponents(G[None])[0] - 1074
    lam, V, _ = C.model(G)
    l2, v2, _ = C.model(S)
    assert C.same_bits(l2, np.ldexp(lam, -1074)) and C.same_bits(v2, V)


@pytest.mark.parametrize("N", [3, 65])
def test_top_of_the_range_premise_and_model_identity(N):
    T = C.top_tridiag(N)
    S = np.ldexp(T, 1024)
    assert np.all(np.isfinite(S)) and np.array_equal(np.ldexp(S, -1024), T)
    assert C.member_exponents(S[None])[0] == 1024 and C.member_exponents(T[None])[0] == 0
    lam_ref = np.linalg.eigvalsh(T)[::-1]
    assert np.abs(lam_ref).max() < 0.875
    lam, V, _ = C.model(T)
    l2, v2, _ = C.model(S)
    assert np.all(np.isfinite(l2)) and C.same_bits(l2, np.ldexp(lam, 1024)) and C.same_bits(v2, V)
    l3, v3, _ = C.compose(S, C.numpy_calls())
    assert C.same_bits(l3, l2) and C.same_bits(v3, v2)


@pytest.mark.parametrize("N", [2, 5, 64, 65, 130])
def test_half_step_diagonals(N):
    d = np.diag(C.diag_half(N))
    assert np.array_equal(2.0 * d, np.rint(2.0 * d)) and np.abs(d).max() <= 4.0
    assert np.any(d < 0) and np.any(np.diff(d) > 0)                                      # negatives; not descending as it stands
    if N > 2:
        assert np.any(np.diff(d) < 0)                                                    # nor ascending
    if N >= 64:
        assert len(set(d)) < N                                                               # ties
    # distinct d have distinct rounded roots sqrt(2^k d + c): the solver's order is the rank order up to ties of d itself
    p = C.shift_chol(d, np.zeros(N - 1))[0]
    assert len(set(p)) == len(set(d))


@pytest.mark.parametrize("i", C.PAIR_ROWS)
def test_one_pair_premise(i):
    S = C.pair_130(i)
    off = S - np.diag(np.diag(S))
    assert np.count_nonzero(off) == 2 and S[i, i - 1] == 0.375 == S[i - 1, i]
    parts = C.compose(S, C.numpy_calls())[2]
    assert np.flatnonzero(parts["e"][0]).tolist() == [i - 1] and parts["kind"] == ("dense",)
    # treated as diagonal its eigenvalues are off by up to 0.375, far outside the bound of C.check
    lam_ref = C.path_reference("pair_130_at_%d" % i)[1]
    assert np.abs(np.sort(np.diag(S))[::-1] - lam_ref).max() > 1e3 * C.TOL * np.linalg.norm(S)
