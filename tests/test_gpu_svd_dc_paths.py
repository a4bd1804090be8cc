"""Every path of the divide & conquer SVD on the device (csrc/svd_dc.hip), selected by inputs named for it.

What a merge does there depends on two counts the data decide (n0 values deflated because z = 0, n1 - n0 deflated by a
rotation); tests/svd_dc_common.py holds inputs built so that a given count meets a given size, and
tests/test_svd_dc_paths_host.py asserts on the CPU, from the reference restatement's own records, that each input reaches what
it is named for and that the restatement itself stays inside the bounds used here. The device's own counts are not exposed:
the oracle's records plus exactly structured inputs are the evidence that a path is taken.

Bounds are the project's: check_values and check_properties (slack 1) against oracle.bidiag_svd_dc / oracle.svd_dc, and all J
rows of V2 orthonormal. Each test prints the share of every bound it used before it asserts (pytest -s shows them)."""
import re

import numpy as np
import pytest

import oracle
import svd_dc_common as C

pytestmark = pytest.mark.gpu

# the lines of svd_dc.js whose assertions the device restates (csrc/svd_dc.hip: dc_fail)
ASSERT_LINES = {202, 206, 393, 405, 429, 486, 507, 583}


@pytest.fixture(scope="module")
def la():
    from nd4js_amd import la as _la
    return _la


@pytest.fixture(scope="module")
def dev():
    from nd4js_amd import dev as _dev
    return _dev


def _on_device(fn, *arrays, **kw):
    import torch
    out = fn(*[torch.from_numpy(np.array(a)).cuda() for a in arrays], **kw)
    return tuple(o.cpu().numpy() for o in out)


def _bidiag_both(la, dev, d, e):
    return [la.bidiag_svd(d, e), _on_device(dev.bidiag_svd, d, e)]


def _same_bytes(x, y):
    return all(a.tobytes() == b.tobytes() for a, b in zip(x, y))


def _checked(label, d, e, got, ref):
    """print the shares of the bounds, then hold the result to them"""
    u2, sv, v2 = got
    if np.all(np.isfinite(sv)) and sv.shape == ref.shape:
        print("%s: share of the bounds (values, reconstruction, U, V) = %s"
              % (label, " ".join("%.3f" % x for x in C.used(C.bidiag_dense(d, e), u2, sv, v2, ref))))
    C.check_bidiag(d, e, u2, sv, v2, ref)


# ---- the catalogue ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(C.PATH_CASES))
def test_bidiag_svd_path(la, dev, name):
    d, e = C.PATH_CASES[name]
    ref = C.path_reference(name)[2]
    for got in _bidiag_both(la, dev, d, e):
        _checked(name, d, e, got, ref)


@pytest.mark.parametrize("K,J", C.TINY_SHAPES)
def test_bidiag_svd_every_tiny_problem(la, dev, K, J):
    """every (d, e) over (-1.5, 0, 0.75) in one batched call per shape: one leaf each, every zero and sign branch of dc_leaves
    (b4 = 0; b4 != 0 with b2 = 0; the |x| < |y| swap; x < 0; sgn; norm 0 in the 1 x 2 leaf)"""
    D, E = C.tiny_problems(K, J)
    worst = np.zeros(4)
    for U2, S, V2 in _bidiag_both(la, dev, D, E):
        assert U2.shape == D.shape[:1] + (K, K) and S.shape == D.shape and V2.shape == D.shape[:1] + (J, J)
        for b in range(D.shape[0]):
            ref = oracle.bidiag_svd_dc(D[b], E[b])[1]
            worst = np.maximum(worst, C.used(C.bidiag_dense(D[b], E[b]), U2[b], S[b], V2[b], ref))
            C.check_bidiag(D[b], E[b], U2[b], S[b], V2[b], ref)
    print("tiny %d x %d: largest share of the bounds = %s" % (K, J, " ".join("%.3f" % x for x in worst)))


# ---- members that take different paths in one launch ------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mixed_67_68", "mixed_69_69"])
def test_members_differ_at_a_gemm_level(la, dev, name):
    """dc_gather / dc_scatter take the member from blockIdx.z / nm and the merge from blockIdx.z % nm, and every member has its
    own outer and inner order and its own (n0, n1): members with different counts take different early returns in one launch.
    Every member has the bits of its own single run and meets the bounds."""
    members = C.mixed_members(name)
    D, E = np.stack([d for d, _ in members]), np.stack([e for _, e in members])
    for batched, single in ((la.bidiag_svd, la.bidiag_svd),
                            (lambda d, e: _on_device(dev.bidiag_svd, d, e), lambda d, e: _on_device(dev.bidiag_svd, d, e))):
        U2, S, V2 = batched(D, E)
        for b, (d, e) in enumerate(members):
            assert _same_bytes(single(d, e), (U2[b], S[b], V2[b])), "member %d is not its single run" % b
            _checked("%s[%d]" % (name, b), d, e, (U2[b], S[b], V2[b]), oracle.bidiag_svd_dc(d, e)[1])


def test_no_state_survives_a_call(la, dev):
    """the workspace is reused from call to call: a call with other counts in between changes nothing"""
    r, s = C.PATH_CASES["rand_70_71"], C.PATH_CASES["quad_16_singular"]
    for run in (la.bidiag_svd, lambda d, e: _on_device(dev.bidiag_svd, d, e)):
        first = run(*r)
        _checked("quad_16_singular between", s[0], s[1], run(*s), C.path_reference("quad_16_singular")[2])
        assert _same_bytes(first, run(*r))
        _checked("rand_70_71", r[0], r[1], first, C.path_reference("rand_70_71")[2])


@pytest.mark.parametrize("K,batch,chunk", [(1, 32770, 32767), (3, 16400, 16383)])
def test_leaf_only_batch_beyond_one_chunk(dev, K, batch, chunk):
    """K = 1 (one leaf, no merge level): a chunk holds 32767 members, so blockIdx.y of dc_leaves reaches its top; K = 3 (one
    merge of m = 3): a chunk holds 16383 and dc_wrot runs with 2 * 16383 in z. Members on both sides of the cut have the bits of
    their own single run."""
    import torch
    g = np.random.default_rng(7300 + K)
    d, e = g.uniform(-1, 1, (batch, K)), g.uniform(-1, 1, (batch, K))
    U, S, V = (x.cpu().numpy() for x in dev.bidiag_svd(torch.from_numpy(d).cuda(), torch.from_numpy(e).cuda()))
    for b in (0, chunk - 1, chunk, batch - 1):
        got = _on_device(dev.bidiag_svd, d[b], e[b])
        assert _same_bytes(got, (U[b], S[b], V[b])), "member %d is not its single run" % b
        C.check_bidiag(d[b], e[b], *got, oracle.bidiag_svd_dc(d[b], e[b])[1])
    for b in range(0, batch, 997):                                          # ... and a sample of all of them has the right values
        C.check_values(S[b], oracle.bidiag_svd_dc(d[b], e[b])[1])


# ---- svd_decomp(A, algo='dc') ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(C.PATH_DENSE_CASES))
def test_svd_decomp_dc_path(la, dev, name):
    a, _, ref, _ = C.dense_reference(name)
    for u, sv, v in (la.svd_decomp(np.asarray(a), algo="dc"), _on_device(dev.svd_decomp, a, algo="dc")):
        if sv.shape == ref.shape and np.all(np.isfinite(sv)):
            M, N = a.shape[-2:]
            shares = [C.used(*x) for x in zip(a.reshape(-1, M, N), u.reshape(-1, M, min(M, N)), sv.reshape(-1, min(M, N)),
                                              v.reshape(-1, min(M, N), N), ref.reshape(-1, min(M, N)))]
            print("%s: share of the bounds (values, reconstruction, U, V) = %s"
                  % (name, " ".join("%.3f" % x for x in np.max(shares, axis=0))))
        C.check_values(sv, ref)
        C.check_properties(a, u, sv, v)
        if name in C.RANKS:
            assert np.all(sv[C.RANKS[name]:] <= 1e-10 * sv[0])


# ---- errors ------------------------------------------------------------------------------------------------------------------
def _assert_raises_an_assertion(fn, *args):
    from nd4js_amd import _lib
    with pytest.raises(_lib.Nd4HipError) as ex:
        fn(*args)
    found = re.search(r"svd_dc: Assertion failed\. \(svd_dc\.js:(\d+)\)", str(ex.value))
    assert ex.value.code == -3 and found and int(found.group(1)) in ASSERT_LINES, str(ex.value)
    return int(found.group(1))


def test_nan_and_inf_raise_the_assertion_of_the_reference(la, dev):
    """Inputs for which the reference always asserts (line 429, pinned in test_svd_dc_paths_host.py): the device must raise
    too, never return NaN. The line need not be 429: the roots of a merge run in parallel, each meets its own first failing
    check, and the first writer of the flag word wins."""
    for d, e in C.error_inputs():
        for run in (la.bidiag_svd, lambda d, e: _on_device(dev.bidiag_svd, d, e)):
            print("line", _assert_raises_an_assertion(run, d, e))


def test_nan_in_a_leaf_only_problem_is_no_error(la, dev):
    """K = 1 and K = 2 have no merge and so no assertion: NaN goes through the closed forms into the outputs, in the outputs
    where the oracle has some and in no other"""
    for K, J in C.TINY_SHAPES:
        for pos in range(K + J - 1):
            x = np.array([0.75, -1.5, 0.5, 1.25][:K + J - 1])
            x[pos] = np.nan
            d, e = x[:K].copy(), x[K:].copy()
            want = oracle.bidiag_svd_dc(d, e)
            assert any(np.isnan(w).any() for w in want)
            for got in _bidiag_both(la, dev, d, e):
                assert [bool(np.isnan(g).any()) for g in got] == [bool(np.isnan(w).any()) for w in want], (K, J, pos)


def test_a_failed_member_fails_the_call_and_the_handle_stays_usable(la, dev):
    d, e = C.PATH_CASES["rand_70_71"]
    D, E = np.stack([d, d, d]), np.stack([e, e, e])
    D[1, 40] = np.nan
    for run in (la.bidiag_svd, lambda d, e: _on_device(dev.bidiag_svd, d, e)):
        before = run(d, e)
        _assert_raises_an_assertion(run, D, E)
        assert _same_bytes(before, run(d, e))
        _checked("rand_70_71 after a failed call", d, e, before, C.path_reference("rand_70_71")[2])


def test_sizes_beyond_the_largest_are_refused(la, dev):
    """K = 2049 does not fit the LDS copies of a merge (DC_MAXM = 2048): an argument error before any kernel runs"""
    import torch
    from nd4js_amd import _lib
    d, e = C.PATH_CASES["rand_70_71"]
    before = la.bidiag_svd(d, e)
    big = np.ones(2049)
    zero = np.zeros((2049, 2049))
    for fn, args, kw in ((la.bidiag_svd, (big, big), {}), (dev.bidiag_svd, (torch.from_numpy(big).cuda(),) * 2, {}),
                         (la.svd_decomp, (zero,), {"algo": "dc"}), (dev.svd_decomp, (torch.from_numpy(zero).cuda(),), {"algo": "dc"})):
        with pytest.raises(_lib.Nd4HipError, match=r"svd_dc: the divide & conquer solver takes (1 <= )?min\(M, N\) <= 2048") as ex:
            fn(*args, **kw)
        assert ex.value.code == -1
        assert _same_bytes(before, la.bidiag_svd(d, e))
