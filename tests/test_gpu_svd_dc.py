"""Divide & conquer SVD on the device: la / dev .bidiag_svd(d, e) and .svd_decomp(A, algo='dc') against oracle.svd_dc, the C
restatement of the reference's svd_dc.js. Inputs, references and bounds: tests/svd_dc_common.py."""
import re

import numpy as np
import pytest

import oracle
import svd_dc_common as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def la():
    from nd4js_amd import la as _la
    return _la


@pytest.fixture(scope="module")
def dev():
    from nd4js_amd import dev as _dev
    return _dev


def _on_device(dev, fn, *arrays, **kw):
    import torch
    out = fn(*[torch.from_numpy(np.array(a)).cuda() for a in arrays], **kw)
    return tuple(o.cpu().numpy() for o in out)


def _svd_both(la, dev, a, **kw):
    """the case through la (host arrays) and through dev (device arrays)"""
    return [la.svd_decomp(a, **kw), _on_device(dev, dev.svd_decomp, a, **kw)]


def _bidiag_both(la, dev, d, e):
    return [la.bidiag_svd(d, e), _on_device(dev, dev.bidiag_svd, d, e)]


# ---- the solver alone ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(C.BIDIAG_CASES))
def test_bidiag_svd_against_the_oracle(la, dev, name):
    d, e = C.BIDIAG_CASES[name]
    B, _, ref, _ = C.bidiag_reference(name)
    K, J = B.shape
    for u2, sv, v2 in _bidiag_both(la, dev, d, e):
        assert u2.shape == (K, K) and sv.shape == (K,) and v2.shape == (J, J)
        C.check_values(sv, ref)
        C.check_properties(B, u2, sv, v2[:K])                       # B = U2 diag(sv) V2[:K]
        assert np.abs(v2 @ v2.T - np.eye(J)).max() <= 4 * C.EPS * J   # all J rows of V2 are orthonormal


def test_bidiag_svd_vectors_of_a_dense_spectrum(la, dev):
    """distinct singular values: the vectors are the oracle's up to sign and rounding"""
    for name in ("rand_17_18", "rand_65_65", "rand_129_130"):
        d, e = C.BIDIAG_CASES[name]
        B, ur, ref, vr = C.bidiag_reference(name)
        K = B.shape[0]
        for u2, sv, v2 in _bidiag_both(la, dev, d, e):
            C.check_vectors(u2, v2[:K], ur, vr, ref)


def test_bidiag_svd_members_are_independent_at_any_scale(la):
    """one member scaled by 1e+150 and one by 1e-150 (n = 17): every member's result has the bits of its own single run"""
    d = np.stack([C._u(7101, 17, -1, 1), 1e150 * C._u(7102, 17, -1, 1), 1e-150 * C._u(7103, 17, -1, 1)])
    e = np.stack([C._u(7104, 17, -1, 1), 1e150 * C._u(7105, 17, -1, 1), 1e-150 * C._u(7106, 17, -1, 1)])
    U, S, V = la.bidiag_svd(d, e)
    for b in range(3):
        u, s, v = la.bidiag_svd(d[b], e[b])
        assert u.tobytes() == U[b].tobytes() and s.tobytes() == S[b].tobytes() and v.tobytes() == V[b].tobytes()
        B = C.bidiag_dense(d[b], e[b])
        _, ref, _ = oracle.svd_dc(B)
        C.check_values(s, ref)
        C.check_properties(B, u, s, v[:17])


def test_bidiag_svd_batch_beyond_one_chunk(dev):
    """the merges of a level times the members of a chunk share one grid dimension and one GEMM batch (<= 65535): at K = 33
    (one GEMM level) a chunk holds 3640 members, so 3700 members take two. Members on both sides of the cut have the bits of
    their own single run."""
    import torch
    K, batch = 33, 3700
    g = np.random.default_rng(7200)
    d, e = g.uniform(-1, 1, (batch, K)), g.uniform(-1, 1, (batch, K))
    U, S, V = (x.cpu().numpy() for x in dev.bidiag_svd(torch.from_numpy(d).cuda(), torch.from_numpy(e).cuda()))
    for b in (0, 3639, 3640, 3699):
        u, s, v = _on_device(dev, dev.bidiag_svd, d[b], e[b])
        assert u.tobytes() == U[b].tobytes() and s.tobytes() == S[b].tobytes() and v.tobytes() == V[b].tobytes()
        B = C.bidiag_dense(d[b], e[b])
        C.check_values(s, oracle.svd_dc(B)[1])
        C.check_properties(B, u, s, v[:K])


# ---- svd_decomp(A, algo='dc') ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(C.DENSE_CASES))
def test_svd_decomp_dc_dense(la, dev, name):
    a, ur, ref, vr = C.dense_reference(name)
    for u, sv, v in _svd_both(la, dev, np.asarray(a), algo="dc"):
        C.check_values(sv, ref)
        C.check_properties(a, u, sv, v)
        C.check_vectors(u, v, ur, vr, ref)


@pytest.mark.parametrize("name", list(C.STRUCTURED_CASES))
def test_svd_decomp_dc_structured(la, dev, name):
    a, _, ref, _ = C.dense_reference(name)
    for u, sv, v in _svd_both(la, dev, np.asarray(a), algo="dc"):
        C.check_values(sv, ref)
        C.check_properties(a, u, sv, v)
        if name in C.RANKS:
            assert np.all(sv[C.RANKS[name]:] <= 1e-10 * sv[0])


def test_default_route_is_untouched(la, dev):
    """algo=None and algo='jacobi' are today's path: the bits of a call without the argument; anything else is refused"""
    a = np.asarray(C.DENSE_CASES["sq_33"])
    base = la.svd_decomp(a)
    for kw in ({"algo": None}, {"algo": "jacobi"}):
        for got in _svd_both(la, dev, a, **kw):
            assert all(x.tobytes() == y.tobytes() for x, y in zip(got, base))
    dc = la.svd_decomp(a, algo="dc")
    assert dc[0].tobytes() != base[0].tobytes()                     # ... and 'dc' is another algorithm
    assert la.svd_dc is la.svd_decomp
    import torch
    for fn, arg in ((la.svd_decomp, a), (dev.svd_decomp, torch.from_numpy(np.array(a)).cuda())):
        with pytest.raises(ValueError):
            fn(arg, algo="qr")


def test_nan_input_ends_and_leaves_the_handle_usable(la):
    """bounded loops: a NaN ends in the reference's assertion (dense input: or in NaN outputs), never in a hang; the errors
    themselves are pinned in test_gpu_svd_dc_paths.py"""
    from nd4js_amd import _lib
    a = np.array(C.DENSE_CASES["sq_33"])
    a[5, 7] = np.nan
    try:
        u, sv, v = la.svd_decomp(a, algo="dc")
        assert np.isnan(sv).any() or np.isnan(u).any() or np.isnan(v).any()
    except _lib.Nd4HipError as ex:
        assert ex.code == -3 and re.search(r"svd_dc: Assertion failed\. \(svd_dc\.js:\d+\)", str(ex))
    d, e = np.ones(20), np.ones(20)                     # the reference always asserts here (test_svd_dc_paths_host.py): so must we
    d[3] = np.nan
    with pytest.raises(_lib.Nd4HipError, match=r"svd_dc: Assertion failed\. \(svd_dc\.js:\d+\)") as ex:
        la.bidiag_svd(d, e)
    assert ex.value.code == -3
    a, _, ref, _ = C.dense_reference("sq_33")
    u, sv, v = la.svd_decomp(np.asarray(a), algo="dc")
    C.check_values(sv, ref)
    C.check_properties(a, u, sv, v)


def test_profile_record(dev):
    import torch
    from nd4js_amd import _lib
    h = _lib.handle(0)
    h.profile_enable(True)
    try:
        A = torch.from_numpy(np.array(C.DENSE_CASES["sq_130"])).cuda()
        dev.svd_decomp(A, algo="dc")
        p = h.profile_last()
        assert p[0]["valid"] and p[0]["op"] == "svd_dc" and p[0]["kernel_ms"] > 0.0
        assert p[0]["flops"] == 21.0 * 130 ** 3 and p[0]["bytes"] == 8.0 * (130 * 130 + 261 * 130)
    finally:
        h.profile_enable(False)
