"""pldlp_* without a device: the reference's validation messages, pldlp_l / pldlp_d / pldlp_p (host-side numpy) against the
fixtures of tests/golden/pldlp, the ABI's argument refusals, and the numpy restatement of tests/pldlp_common.py against EVERY
decomposition and solve fixture bit for bit, which is what entitles tests/test_gpu_pldlp.py to use it where no full fixture
exists."""
import ctypes
import os

import numpy as np
import pytest

import pldlp_common as pc
from conftest import ROOT
from nd4js_amd import _lib, la

NAMES = ["pldlp_decomp", "pldlp_solve", "pldlp_l", "pldlp_d", "pldlp_p"]
ABI = ["nd4hip_dsytrf_bk_batched", "nd4hip_dsytrf_bk_batched_ex", "nd4hip_dsytrs_bk_batched"]


def _members(name):
    """(b, LD, P) of every member of a fixture that factorises, with the complete LD"""
    c = pc.CASES[name]
    N = c["N"]
    if "LD" not in c["files"]:
        return
    LD, P = pc.load(c, "LD").reshape(-1, N, N), pc.load(c, "P").reshape(-1, N)
    for b, r in enumerate(pc.reference(name)):
        if not isinstance(r, pc.Singular):
            yield b, LD[b], P[b]


# ------------------------------------------------------------------------------------------------ the fixtures themselves
def test_manifest_is_complete_and_small():
    for entry in list(pc.CASES.values()) + list(pc.SOLVES.values()):
        for key, fn in entry["files"].items():
            path = os.path.join(pc.DIR, fn)
            assert os.path.getsize(path) <= pc.SIZE_LIMIT, fn
            assert pc.sha256(entry, key) == entry["sha256"][key], fn
    fams = {f for c in pc.CASES.values() for f in c["families"]}
    assert fams >= {"dense", "zero_diag", "kkt", "diag_dominant", "antidiag", "identity", "ties", "scaled_up", "scaled_down", "subnormal",
                    "inf_entry", "nan_last", "zero_col_first", "nan_col"}
    sizes = {c["N"] for c in pc.CASES.values()}
    lim = la.pldlp_limits()["lds_max_n"]
    assert sizes >= {1, 2, 3, 17, 33, lim, lim + 1, 130}
    assert {pc.SOLVES[k]["J"] for k in pc.SOLVES} >= {1, 2, 33}


def test_fixtures_reach_every_branch():
    dense = [pc.CASES[k] for k in pc.SINGLE if pc.CASES[k]["family"] == "dense" and pc.CASES[k]["N"] >= 33]
    assert all(c["pivots_2x2"] >= 0.15 * c["N"] and c["moved_rows"] >= 0.4 * c["N"] for c in dense)
    for k in pc.SINGLE:
        c = pc.CASES[k]
        if c["family"] == "diag_dominant":
            assert c["pivots_2x2"] == 0 and c["moved_rows"] == 0          # no interchange, no 2x2
        if c["family"] == "antidiag":
            assert c["pivots_2x2"] == c["N"] // 2                          # only 2x2 (and the middle element of an odd size)
        if c["family"] in ("zero_col_first", "nan_col") and c["N"] > 1:
            assert c["error"] == pc.SINGULAR
    assert pc.CASES["zero_1"]["error"] is None                             # the last step is not checked: [[0]] factorises
    assert pc.CASES["batch_singular_5x17"]["error_member"] == 3


# ------------------------------------------------------------------------------------------------ restatement against fixtures
@pytest.mark.parametrize("name", pc.ALL)
def test_restatement_reproduces_the_fixture(name):
    c = pc.CASES[name]
    N = c["N"]
    ref = pc.reference(name)
    failing = [b for b, r in enumerate(ref) if isinstance(r, pc.Singular)]
    assert (failing[0] if failing else None) == c["error_member"]
    if failing:
        assert str(ref[failing[0]]) == c["error"] == pc.SINGULAR
    if not c["lead"] and failing:
        assert "LD" not in c["files"]
        return
    P = pc.load(c, "P").reshape(-1, N)
    for b, r in enumerate(ref):
        if isinstance(r, pc.Singular):
            continue
        LD_ref, P_ref = r
        assert np.array_equal(P[b], P_ref), (name, b)
        assert not np.triu(LD_ref, 1).any()
        if "LD" in c["files"]:
            LD = pc.load(c, "LD").reshape(-1, N, N)[b]
            assert np.array_equal(np.isnan(LD), np.isnan(LD_ref)) and pc.same_bits(LD, LD_ref), (name, b)
        else:
            assert pc.same_bits(LD_ref.reshape(-1)[pc.load(c, "LDidx")], pc.load(c, "LDval")), name


def test_nan_at_the_last_diagonal_element_is_no_error():
    for name in pc.SINGLE:
        c = pc.CASES[name]
        if c["family"] == "nan_last":
            LD = pc.load(c, "LD")
            nan = np.isnan(LD)
            assert c["error"] is None and nan[-1, -1] and nan.sum() == 1


def test_ties_keep_the_first_maximum(monkeypatch):
    # column 0 below the diagonal is (3, -3, 3): r = 1. A_kk = 1 < alpha 3 and 1 < alpha 3 (3 / 3), A_rr = 0 < alpha 3: a 2x2 step on
    # rows (0, 1), nothing interchanged. Had the last maximum won (r = 3, A_rr = 0 as well), rows 1 and 3 would have been interchanged
    S = np.array([[1.0, 3, -3, 3], [3, 0, 3, 1], [-3, 3, 2, 1], [3, 1, 1, 0]])
    assert pc.decomp_ref(S)[1].tolist()[:2] == [0, ~1]
    # rows / columns 1 and 2 exchanged: the first maximum is again r = 1, now with A_rr = 2 >= alpha 3: a 1x1 step with rows 0 and 1
    # interchanged. The last maximum (r = 3, A_rr = 0) would have given a 2x2 step
    S2 = S[[0, 2, 1, 3]][:, [0, 2, 1, 3]]
    assert pc.decomp_ref(S2)[1].tolist()[:2] == [1, 0]
    # the 33 x 33 small-integer fixture depends on the rule: with the LAST maximum the restatement leaves the reference's P
    def last_max(x):
        if np.isnan(x).any():
            return len(x) - 1, x[-1]
        i = len(x) - 1 - int(np.argmax(x[::-1]))
        return i, x[i]
    monkeypatch.setattr(pc, "_argmax_seq", last_max)
    for name in ("ties_33",):
        assert not np.array_equal(pc.decomp_ref(pc.input_matrix(name))[1], pc.load(pc.CASES[name], "P"))


@pytest.mark.parametrize("name", sorted(pc.SOLVES))
def test_solve_restatement_reproduces_the_fixture(name):
    sv = pc.SOLVES[name]
    c = pc.CASES[sv["decomp"]]
    N, J = sv["N"], sv["J"]
    LD, P = pc.load(c, "LD").reshape(-1, N, N), pc.load(c, "P").reshape(-1, N)
    S = pc.input_matrix(sv["decomp"]).reshape(-1, N, N)
    if not sv["ld_lead"]:
        LD, P, S = LD[:1], P[:1], S[:1]
    X, y = pc.load(sv, "X").reshape(-1, N, J), pc.rhs(sv).reshape(-1, N, J)
    worst = 0.0
    for b in range(X.shape[0]):
        bl, by = b % len(LD), b % len(y)
        x = pc.solve_ref(LD[bl], P[bl], y[by])
        assert pc.same_bits(x, X[b]), (name, b)
        worst = max(worst, pc.backward_error(S[bl], x, y[by]))
    assert worst <= 4.0 * max(sv["ref_backward_error"], N * pc.EPS)
    assert sv["ref_backward_error"] <= 1e-13


# ------------------------------------------------------------------------------------------------ pldlp_l / pldlp_d / pldlp_p
@pytest.mark.parametrize("name", [k for k in pc.ALL if "LD" in pc.CASES[k]["files"] and pc.CASES[k]["N"] <= 65])
def test_l_d_p_rebuild_the_matrix(name):
    N = pc.CASES[name]["N"]
    S = pc.input_matrix(name).reshape(-1, N, N)
    for b, LD, P in _members(name):
        L, D, p = la.pldlp_l(LD, P), la.pldlp_d(LD, P), la.pldlp_p(LD, P)
        assert L.shape == D.shape == (N, N) and p.shape == (N,) and p.dtype == np.int32
        assert np.array_equal(np.diag(L), np.ones(N)) and not np.triu(L, 1).any()
        assert pc.same_bits(D, D.T) and sorted(p.tolist()) == list(range(N))
        for i in range(N):
            inner = P[i] < 0
            assert np.array_equal(L[i, :i - inner], LD[i, :i - inner]) and (not inner or (L[i, i - 1] == 0 and D[i, i - 1] == LD[i, i - 1]))
        assert pc.same_bits(np.diag(D), np.diag(LD))
        if np.isfinite(S[b]).all() and np.isfinite(LD).all():
            A = S[b][p][:, p]
            assert np.linalg.norm(L @ D @ L.T - A) <= 64 * N * pc.EPS * np.linalg.norm(np.abs(L) @ np.abs(D) @ np.abs(L.T))
        assert all(pc.same_bits(x, y) for x, y in zip((L, D, p), (la.pldlp_l([LD, P]), la.pldlp_d([LD, P]), la.pldlp_p([LD, P]))))


def test_l_d_p_broadcast_like_the_reference():
    c = pc.CASES["batch_2x3x17"]
    LD, P = pc.load(c, "LD"), pc.load(c, "P")
    L = la.pldlp_l(LD, P)
    assert L.shape == (2, 3, 17, 17) and pc.same_bits(L[1, 2], la.pldlp_l(LD[1, 2], P[1, 2]))
    # LD [3, 17, 17] against P [2, 1, 17]
    L = la.pldlp_l(LD[0], P[:, :1])
    D = la.pldlp_d(LD[0], P[:, :1])
    assert L.shape == D.shape == (2, 3, 17, 17)
    assert pc.same_bits(L[1, 2], la.pldlp_l(LD[0, 2], P[1, 0])) and pc.same_bits(D[1, 2], la.pldlp_d(LD[0, 2], P[1, 0]))
    assert la.pldlp_p(LD[0], P[:, :1]).shape == (2, 1, 17)                 # pldlp_p returns P's own shape
    for fn in (la.pldlp_l, la.pldlp_d, la.pldlp_p):
        with pytest.raises(ValueError, match="Shapes are not broadcast-compatible."):
            fn(LD, P[:, :2])


def test_invalid_p_messages():
    LD = np.eye(4)
    ok = np.array([0, 1, ~2, 3], dtype=np.int32)
    with pytest.raises(ValueError, match=r"pldlp_solve\(LD,P,y\): P is invalid\."):
        la.pldlp_p(LD, np.array([~0, 1, 2, 3], dtype=np.int32))                  # a second row at i = 0
    with pytest.raises(ValueError, match=r"pldlp_solve\(LD,P,y\): P is invalid\."):
        la.pldlp_p(LD, np.array([0, ~1, ~2, 3], dtype=np.int32))                 # two second rows in a row
    with pytest.raises(ValueError, match=r"pldlp_solve\(LD,P,y\): P contains out-of-bounds indices\."):
        la.pldlp_p(LD, np.array([0, 1, 2, 4], dtype=np.int32))
    with pytest.raises(ValueError, match=r"pldlp_solve\(LD,P,y\): P contains out-of-bounds indices\."):
        la.pldlp_p(LD, np.array([0, 1, ~7, 3], dtype=np.int32))
    with pytest.raises(ValueError, match=r"pldlp_solve\(LD,P,y\): P contains duplicate indices\."):
        la.pldlp_p(LD, np.array([0, 1, ~1, 3], dtype=np.int32))
    assert la.pldlp_p(LD, ok).tolist() == [0, 1, 2, 3]
    # pldlp_solve checks P on the host, before any device work: these raise with no device present
    for bad, msg in (([~0, 1, 2, 3], "P is invalid."), ([0, 1, 2, 9], "out-of-bounds"), ([0, 1, 1, 3], "duplicate")):
        with pytest.raises(ValueError, match=msg):
            la.pldlp_solve(LD, np.array(bad, dtype=np.int32), np.ones((4, 1)))
        with pytest.raises(ValueError, match=msg):
            la.pldlp_solve([LD, np.array(bad, dtype=np.int32)], np.ones((4, 1)))


# ------------------------------------------------------------------------------------------------ validation messages
def test_validation_messages_need_no_device():
    with pytest.raises(ValueError, match="Last two dimensions must be quadratic."):
        la.pldlp_decomp(np.ones((2, 3)))
    with pytest.raises(ValueError, match="Last two dimensions must be quadratic."):
        la.pldlp_decomp(np.ones(3))
    with pytest.raises(TypeError):
        la.pldlp_decomp(np.ones((2, 2), dtype=np.float32))
    with pytest.raises(TypeError):
        la.pldlp_decomp(np.ones((2, 2), dtype=np.complex128))
    with pytest.raises(ValueError, match="unknown tier"):
        la.pldlp_decomp(np.eye(2), tier="mfma")
    P = np.arange(3, dtype=np.int32)
    for fn, extra in ((la.pldlp_l, ()), (la.pldlp_d, ()), (la.pldlp_p, ()), (la.pldlp_solve, (np.ones((3, 1)),))):
        with pytest.raises(ValueError, match=r"pldlp_solve\(LD,P,y\): LD must be at least 2D\."):
            fn(np.ones(3), P, *extra)
        with pytest.raises(ValueError, match=r"pldlp_solve\(LD,P,y\): P must be at least 1D\."):
            fn(np.eye(3), np.int32(0), *extra)
        with pytest.raises(ValueError, match=r"pldlp_solve\(LD,P,y\): LD must be square\."):
            fn(np.ones((3, 2)), P, *extra)
        with pytest.raises(ValueError, match=r"pldlp_solve\(LD,P,y\): LD and P shape mismatch\."):
            fn(np.eye(3), P[:2], *extra)
    with pytest.raises(ValueError, match=r"pldlp_solve\(LD,P,y\): y must be at least 2D\."):
        la.pldlp_solve(np.eye(3), P, np.ones(3))
    with pytest.raises(ValueError, match=r"pldlp_solve\(LD,P,y\): LD and y shape mismatch\."):
        la.pldlp_solve(np.eye(3), P, np.ones((2, 1)))
    with pytest.raises(ValueError, match="Shapes are not broadcast-compatible."):
        la.pldlp_solve(np.ones((2, 3, 3)), np.zeros((2, 3), dtype=np.int32), np.ones((3, 3, 1)))
    with pytest.raises(ValueError, match="Assertion failed."):
        la.pldlp_solve(np.eye(3), None)
    with pytest.raises(TypeError):
        la.pldlp_solve(np.eye(3, dtype=np.float32), P, np.ones((3, 1)))
    with pytest.raises(TypeError):
        la.pldlp_solve(np.eye(3), P, np.ones((3, 1), dtype=np.complex128))


# ------------------------------------------------------------------------------------------------ the C ABI
def test_abi_exports_and_header():
    lib = _lib.load()
    assert all(callable(getattr(la, n)) for n in NAMES)
    src = open(os.path.join(ROOT, "include", "nd4hip.h")).read()
    for n in ABI:
        for suffix in ("", "_dev"):
            assert hasattr(lib, n + suffix) and n + suffix in _lib.SIGNATURES and n + suffix in src
    for t, v in (("AUTO", 0), ("LDS", 1), ("GLOBAL", 2), ("GRID", 3)):
        assert "#define ND4HIP_PLDLP_TIER_%s" % t in src and la.PLDLP_TIERS[t.lower()] == v
    lim = la.pldlp_limits()
    assert lim["lds_max_n"] >= 64 and lim["lds_max_n"] * (lim["lds_max_n"] + 1) * 8 <= 160 * 1024
    assert lim["global_max_n"] == 2048 and lim["grid_tile"] >= 16


def test_abi_argument_refusals_need_no_device():
    lib = _lib.load()
    lim = la.pldlp_limits()
    buf = (ctypes.c_double * 16)()
    ip = (ctypes.c_int32 * 4)()
    p, q = ctypes.cast(buf, ctypes.c_void_p), ctypes.cast(ip, ctypes.c_void_p)

    def refused(rc, text):
        assert rc == -1 and text in lib.nd4hip_last_error().decode()
    for fn in (lib.nd4hip_dsytrf_bk_batched_ex, lib.nd4hip_dsytrf_bk_batched_ex_dev):
        refused(fn(None, -1, 2, p, p, q, 0), "negative extent")
        refused(fn(None, 1, 2, p, p, q, 4), "unknown tier 4")
        refused(fn(None, 1, 2, p, p, q, -1), "unknown tier -1")
        refused(fn(None, 1, lim["lds_max_n"] + 1, p, p, q, 1), "tier 1 is not available at N = %d" % (lim["lds_max_n"] + 1))
        refused(fn(None, 1, lim["global_max_n"] + 1, p, p, q, 2), "tier 2 is not available")
        refused(fn(None, 1, 2, p, p, q, 0), "NULL handle")
    for fn in (lib.nd4hip_dsytrf_bk_batched, lib.nd4hip_dsytrf_bk_batched_dev):
        refused(fn(None, 1, -2, p, p, q), "negative extent")
        refused(fn(None, 1, 2, p, p, q), "NULL handle")
    for fn in (lib.nd4hip_dsytrs_bk_batched, lib.nd4hip_dsytrs_bk_batched_dev):
        refused(fn(None, 1, 2, -1, p, 4, q, 2, p, 2, p), "negative extent")
        refused(fn(None, 2, 2, 1, p, 3, q, 2, p, 2, p), "a stride must be 0 or at least the size of one operand")
        refused(fn(None, 2, 2, 1, p, 4, q, 1, p, 2, p), "a stride must be 0")
        refused(fn(None, 2, 2, 1, p, 4, q, 2, p, 1, p), "a stride must be 0")
    # the host-pointer solve looks at P completely before it needs a device
    for bad, msg in (([-1, 1], "P is invalid."), ([0, 2], "out-of-bounds"), ([1, 1], "duplicate"), ([0, -4], "out-of-bounds")):
        ip[0], ip[1] = bad
        refused(lib.nd4hip_dsytrs_bk_batched(None, 1, 2, 1, p, 0, q, 0, p, 0, p), msg)
    ip[0], ip[1] = 0, 1
    refused(lib.nd4hip_dsytrs_bk_batched(None, 1, 2, 1, p, 0, q, 0, p, 0, p), "NULL handle")
    refused(lib.nd4hip_dsytrf_bk_tier(None, 1, 2, 0), "NULL handle")


@pytest.mark.skipif(_lib.load().nd4hip_device_count() > 0, reason="GPU present")
def test_no_cpu_fallback_without_gpu():
    with pytest.raises(_lib.Nd4HipError):
        la.pldlp_decomp(np.eye(3))
    with pytest.raises(_lib.Nd4HipError):
        la.pldlp_solve(np.eye(3), np.arange(3, dtype=np.int32), np.ones((3, 1)))
