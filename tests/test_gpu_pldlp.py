"""pldlp_decomp and pldlp_solve on the device (csrc/pldlp.hip) against the reference's recorded results (tests/golden/pldlp,
tools/gen_golden_pldlp.js).

LD and P are compared with the reference bit for bit, on every fixture and on every tier that can hold it (the 'global' and 'grid'
tiers hold every size, so the small special matrices run through all three). A fixture above 130 rows holds P and 4096 sampled
entries of LD; it is checked on those and in full against the numpy restatement of tests/pldlp_common.py, which
tests/test_pldlp_host.py holds to every fixture bit for bit.

The solve's substitutions (csrc/trsm.hip) sum in another order than the reference's, so x is held to
  * ||x - x_ref|| <= 1e-10 ||x_ref|| on the diagonally dominant fixtures (the project's parity gate), and
  * a backward error ||S x - y|| / (||S|| ||x|| + ||y||) of at most max(N eps, 4 x the reference's own value on that input) on all.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import pldlp_common as pc
from nd4js_amd import _lib, dev, la

pytestmark = pytest.mark.gpu
LIM = la.pldlp_limits()
LDS_MAX, TILE = LIM["lds_max_n"], LIM["grid_tile"]
TIER_ID = la.PLDLP_TIERS


def tiers(N):
    return (["lds"] if N <= LDS_MAX else []) + ["global", "grid"]


@functools.lru_cache(maxsize=None)
def cu_count():
    """the batch from which AUTO prefers 'global' to 'grid' above the LDS limit: the device's CU count"""
    lo, hi = 1, 1 << 16
    while lo < hi:
        mid = (lo + hi) // 2
        if la.pldlp_tier(mid, LDS_MAX + 1) == "global":
            hi = mid
        else:
            lo = mid + 1
    return lo


def raw_decomp(S, tier):
    """the host-pointer entry point as it is: (rc, message, LD, P), so that the members beside a singular one can be read"""
    S = np.ascontiguousarray(S, dtype=np.float64)
    N = S.shape[-1]
    LD, P = np.full_like(S, 7.0), np.full(S.shape[:-1], -99, dtype=np.int32)
    h = _lib.handle()
    rc = h.lib.nd4hip_dsytrf_bk_batched_ex(h.ptr, int(np.prod(S.shape[:-2], dtype=np.int64)), N, la._ptr(S), la._ptr(LD), la._ptr(P),
                                           TIER_ID[tier])
    return rc, h.lib.nd4hip_last_error().decode() if rc else "", LD, P


def check_against_fixture(name, LD, P, skip=()):
    """LD, P of the device against the fixture (complete or sampled) and against the restatement, member by member"""
    c = pc.CASES[name]
    N = c["N"]
    LD, P = LD.reshape(-1, N, N), P.reshape(-1, N)
    Pf = pc.load(c, "P").reshape(-1, N)
    for b, r in enumerate(pc.reference(name)):
        if b in skip:
            continue
        assert np.array_equal(P[b], Pf[b]), (name, b)
        if "LD" in c["files"]:
            assert pc.same_bits(LD[b], pc.load(c, "LD").reshape(-1, N, N)[b]), (name, b)
        else:
            assert pc.same_bits(LD[b].reshape(-1)[pc.load(c, "LDidx")], pc.load(c, "LDval")), name
        assert pc.same_bits(LD[b], r[0]) and np.array_equal(P[b], r[1]), (name, b)
        assert not np.triu(LD[b], 1).any() and not np.signbit(np.triu(LD[b], 1)).any()       # exact (positive) zeros above the diagonal


OK_SINGLE = [k for k in pc.SINGLE if pc.CASES[k]["error"] is None]
BAD_SINGLE = [k for k in pc.SINGLE if pc.CASES[k]["error"] is not None]
OK_BATCH = [k for k in pc.BATCHES if pc.CASES[k]["error"] is None]
BAD_BATCH = [k for k in pc.BATCHES if pc.CASES[k]["error"] is not None]


# ------------------------------------------------------------------------------------------------ tier against fixture
@pytest.mark.parametrize("name,tier", [(k, t) for k in OK_SINGLE + OK_BATCH for t in tiers(pc.CASES[k]["N"])])
def test_tier_reproduces_the_fixture_bit_for_bit(name, tier):
    LD, P = la.pldlp_decomp(pc.input_matrix(name), tier=tier)
    assert P.dtype == np.int32 and LD.shape == tuple(pc.CASES[name]["lead"]) + (pc.CASES[name]["N"],) * 2
    check_against_fixture(name, LD, P)


def test_sizes_cover_every_kernel_path():
    """the sizes the parametrised test above runs, named from the kernels' constants"""
    sizes = {pc.CASES[k]["N"] for k in OK_SINGLE}
    assert {1, 2, 3, 17, LDS_MAX - 1, LDS_MAX} <= sizes                        # lds: tiny, odd, the limit and the limit - 1
    assert {64, 65} <= sizes                                                    # lds: both sides of its small instance (N <= 64)
    assert {LDS_MAX + 1, 130} <= sizes                                          # global: the first size beyond LDS, 130
    assert {TILE - 1, TILE + 1, 4 * TILE + 37} <= sizes                        # grid: below one update tile, straddling, several + odd rest
    assert max(sizes) <= 520


@pytest.mark.parametrize("name", ["dense_3", "dense_65", "kkt_129", "dense_293", "batch_2x3x17"])
def test_tiers_agree_with_each_other_and_with_auto(name):
    S = pc.input_matrix(name)
    N = pc.CASES[name]["N"]
    got = {t: la.pldlp_decomp(S, tier=t) for t in tiers(N) + ["auto"]}
    for t in got:
        assert pc.same_bits(got[t][0], got["global"][0]) and np.array_equal(got[t][1], got["global"][1]), (name, t)


@pytest.mark.parametrize("name", BAD_SINGLE)
def test_zero_column_or_nan_is_the_reference_error(name):
    S = pc.input_matrix(name)
    for tier in tiers(pc.CASES[name]["N"]):
        with pytest.raises(ValueError) as e:
            la.pldlp_decomp(S, tier=tier)
        assert str(e.value) == pc.SINGULAR + " (matrix 0)", (name, tier)


# ------------------------------------------------------------------------------------------------ special members
@pytest.mark.parametrize("name", BAD_BATCH)
def test_singular_member_is_named_and_isolated(name):
    c = pc.CASES[name]
    S = pc.input_matrix(name)
    bad = {b for b, r in enumerate(pc.reference(name)) if isinstance(r, pc.Singular)}
    assert min(bad) == c["error_member"]
    for tier in tiers(c["N"]):
        with pytest.raises(ValueError) as e:
            la.pldlp_decomp(S, tier=tier)
        assert str(e.value) == pc.SINGULAR + " (matrix %d)" % c["error_member"], (name, tier)
        rc, msg, LD, P = raw_decomp(S, tier)
        assert rc == -5 and msg == pc.SINGULAR + " (matrix %d)" % c["error_member"]
        check_against_fixture(name, LD, P, skip=bad)


def test_singular_member_behind_the_first_chunk_keeps_its_index():
    """a batch long enough for the host-pointer form to cut it: the member's index counts from the start of the caller's batch"""
    good, badm = pc.input_matrix("dense_17"), pc.input_matrix("zero_col_first_17")
    S = np.broadcast_to(good, (40000, 17, 17)).copy()
    S[39990] = badm
    rc, msg, LD, P = raw_decomp(S, "auto")
    assert rc == -5 and msg == pc.SINGULAR + " (matrix 39990)"
    c = pc.CASES["dense_17"]
    for b in (0, 32767, 32768, 39989, 39991, 39999):
        assert pc.same_bits(LD[b], pc.load(c, "LD")) and np.array_equal(P[b], pc.load(c, "P"))


def test_last_diagonal_nan_factorises():
    for name in [k for k in OK_SINGLE if pc.CASES[k]["family"] == "nan_last"]:
        for tier in tiers(pc.CASES[name]["N"]):
            LD, P = la.pldlp_decomp(pc.input_matrix(name), tier=tier)
            nan = np.isnan(LD)
            assert nan[-1, -1] and nan.sum() == 1, (name, tier)
    for tier in ("lds", "global", "grid"):
        LD, P = la.pldlp_decomp(np.zeros((1, 1)), tier=tier)               # the last step is not checked: [[0]] factorises
        assert LD.tolist() == [[0.0]] and P.tolist() == [0]


def test_ties_take_the_first_maximum():
    S = np.array([[1.0, 3, -3, 3], [3, 0, 3, 1], [-3, 3, 2, 1], [3, 1, 1, 0]])
    S2 = np.ascontiguousarray(S[[0, 2, 1, 3]][:, [0, 2, 1, 3]])
    for tier in ("lds", "global", "grid"):
        for A, head in ((S, [0, ~1]), (S2, [1, 0])):
            LD, P = la.pldlp_decomp(A, tier=tier)
            ref = pc.decomp_ref(A)
            assert P.tolist()[:2] == head and np.array_equal(P, ref[1]) and pc.same_bits(LD, ref[0]), tier
    # a NaN below the diagonal of column 0: every later element replaces, so the last row is taken and step 0 is no error; the
    # NaN then spreads through the update and a later step refuses it, on the device as in the restatement
    A = pc.symmetric(777, 9, 9)
    A[4, 0] = A[0, 4] = np.nan
    with pytest.raises(pc.Singular):
        pc.decomp_ref(A)
    for tier in ("lds", "global", "grid"):
        with pytest.raises(ValueError) as e:
            la.pldlp_decomp(A, tier=tier)
        assert str(e.value) == pc.SINGULAR + " (matrix 0)", tier


def test_extreme_scales_keep_the_bits():
    for name in [k for k in OK_SINGLE if pc.CASES[k]["family"] in ("scaled_up", "scaled_down", "subnormal")]:
        S = pc.input_matrix(name)
        assert (np.abs(S).max() > 2.0 ** 390) or (np.abs(S).max() < 2.0 ** -390)
        for tier in tiers(pc.CASES[name]["N"]):
            check_against_fixture(name, *la.pldlp_decomp(S, tier=tier))


# ------------------------------------------------------------------------------------------------ batches and AUTO
def test_global_tier_on_a_batch_larger_than_the_chip():
    names = ["dense_17", "zero_diag_17", "kkt_17", "ties_17", "antidiag_17", "diag_dominant_17", "subnormal_17"]
    batch = cu_count() + 5
    S = np.stack([pc.input_matrix(names[b % len(names)]) for b in range(batch)])
    LD, P = la.pldlp_decomp(S, tier="global")
    for b in range(batch):
        c = pc.CASES[names[b % len(names)]]
        assert pc.same_bits(LD[b], pc.load(c, "LD")) and np.array_equal(P[b], pc.load(c, "P")), b


def test_auto_takes_the_documented_tier():
    cu = cu_count()
    assert cu == torch.cuda.get_device_properties(0).multi_processor_count
    assert la.pldlp_tier(1, 1) == la.pldlp_tier(1, LDS_MAX) == la.pldlp_tier(10 * cu, LDS_MAX) == "lds"
    assert la.pldlp_tier(1, LDS_MAX + 1) == la.pldlp_tier(cu - 1, LDS_MAX + 1) == "grid"
    assert la.pldlp_tier(cu, LDS_MAX + 1) == la.pldlp_tier(cu, LIM["global_max_n"]) == "global"
    assert la.pldlp_tier(cu, LIM["global_max_n"] + 1) == "grid"
    for t in ("lds", "global", "grid"):
        assert la.pldlp_tier(3, 17, tier=t) == t
    with pytest.raises(ValueError, match="tier 1 is not available at N = %d" % (LDS_MAX + 1)):
        la.pldlp_tier(1, LDS_MAX + 1, tier="lds")
    with pytest.raises(ValueError, match="tier 1 is not available"):
        la.pldlp_decomp(pc.input_matrix("dense_%d" % (LDS_MAX + 1)), tier="lds")
    with pytest.raises(ValueError, match="tier 2 is not available"):
        la.pldlp_decomp(np.eye(LIM["global_max_n"] + 1), tier="global")
    # AUTO on each side of the boundaries gives the fixture's bits (the tier it took is what the query above says)
    for name in ("dense_%d" % LDS_MAX, "dense_%d" % (LDS_MAX + 1)):
        check_against_fixture(name, *la.pldlp_decomp(pc.input_matrix(name)))
    S = np.broadcast_to(pc.input_matrix("kkt_129"), (cu, 129, 129)).copy()
    h = _lib.handle()
    h.profile_enable(True)
    try:
        LD, P = la.pldlp_decomp(S)
        rec = h.profile_last()[0]
    finally:
        h.profile_enable(False)
    assert rec["op"] == "dsytrf_bk_batched" and rec["valid"]
    c = pc.CASES["kkt_129"]
    for b in (0, 1, cu // 2, cu - 1):
        assert pc.same_bits(LD[b], pc.load(c, "LD")) and np.array_equal(P[b], pc.load(c, "P"))


def test_device_arrays_and_in_place():
    for name in ("dense_33", "batch_3x129", "dense_130"):
        S = torch.from_numpy(pc.input_matrix(name)).cuda()
        LD, P = dev.pldlp_decomp(S)
        check_against_fixture(name, LD.cpu().numpy(), P.cpu().numpy())
        LD2, P2 = dev.pldlp_decomp(S, out=S)                               # S may be LD
        assert LD2.data_ptr() == S.data_ptr()
        check_against_fixture(name, LD2.cpu().numpy(), P2.cpu().numpy())
    with pytest.raises(ValueError) as e:
        dev.pldlp_decomp(torch.from_numpy(pc.input_matrix("batch_singular_5x17")).cuda())
    assert str(e.value) == pc.SINGULAR + " (matrix 3)"


# ------------------------------------------------------------------------------------------------ solve
def solve_case(name):
    sv = pc.SOLVES[name]
    c = pc.CASES[sv["decomp"]]
    N = sv["N"]
    LD, P, S = pc.load(c, "LD"), pc.load(c, "P"), pc.input_matrix(sv["decomp"])
    if not sv["ld_lead"] and c["lead"]:
        LD, P, S = LD.reshape(-1, N, N)[0], P.reshape(-1, N)[0], S.reshape(-1, N, N)[0]
    return sv, LD, P, S, pc.rhs(sv), pc.load(sv, "X")


def check_backward(S, x, y, ref_value, N, what):
    lead = np.broadcast_shapes(S.shape[:-2], y.shape[:-2])
    Sb, yb = np.broadcast_to(S, lead + S.shape[-2:]).reshape(-1, N, N), np.broadcast_to(y, lead + y.shape[-2:]).reshape((-1,) + y.shape[-2:])
    xb = x.reshape((-1,) + x.shape[-2:])
    worst = max(pc.backward_error(Sb[b], xb[b], yb[b]) for b in range(len(xb)))
    print("%s: backward error %.3e, reference %.3e, ratio %.2f" % (what, worst, ref_value, worst / ref_value if ref_value else float("nan")))
    assert worst <= pc.backward_bound(ref_value, N), what
    return worst


@pytest.mark.parametrize("name", sorted(pc.SOLVES))
def test_solve_against_the_fixture(name):
    sv, LD, P, S, y, X = solve_case(name)
    x = la.pldlp_solve(LD, P, y)
    assert x.shape == X.shape and np.isfinite(x).all()
    if pc.CASES[sv["decomp"]]["family"] == "diag_dominant":
        assert np.linalg.norm(x - X) <= pc.GATE * np.linalg.norm(X)
    check_backward(S, x, y, sv["ref_backward_error"], sv["N"], name)
    assert pc.same_bits(x, la.pldlp_solve([LD, P], y))                     # the ([LD, P], y) form


def test_solve_beyond_the_full_fixtures():
    """293 rows: LD, P from the device (the restatement's bits), the reference's own error from the restatement's solve"""
    S = pc.input_matrix("dense_293")
    LD, P = la.pldlp_decomp(S)
    y = pc.symmetric(4242, 293, 293)[:, :3].copy()
    x = la.pldlp_solve(LD, P, y)
    ref = pc.backward_error(S, pc.solve_ref(LD, P, y), y)
    assert ref <= 1e-13
    check_backward(S, x, y, ref, 293, "dense_293 J=3")


def test_solve_layouts():
    sv, LD, P, S, y, X = solve_case("solve_batch_2x3x17_j33")
    # general broadcasting of the leading axes: LD, P [3, ...] against y [2, 1, ...]
    x = la.pldlp_solve(LD[0], P[0], y[:, :1])
    for a in range(2):
        for b in range(3):
            assert pc.same_bits(x[a, b], la.pldlp_solve(LD[0, b], P[0, b], y[a, 0]))
    # one column, and device arrays with y aliasing X
    x1 = la.pldlp_solve(LD, P, y[..., :1])
    check_backward(S, x1, y[..., :1], sv["ref_backward_error"], 17, "J = 1")
    dLD, dP, dY = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (LD, P, y))
    dX = dev.pldlp_solve(dLD, dP, dY)
    assert pc.same_bits(dX.cpu().numpy(), la.pldlp_solve(LD, P, y))
    keep = dX.cpu().numpy()
    out = dev.pldlp_solve(dLD, dP, dY, out=dY)                            # X may be Y
    assert out.data_ptr() == dY.data_ptr() and pc.same_bits(out.cpu().numpy(), keep)
    # one LD, P for a batch of y on the device
    dY = torch.from_numpy(y).cuda()
    one = dev.pldlp_solve(dLD[0, 0], dP[0, 0], dY).cpu().numpy()
    assert pc.same_bits(one[1, 2], la.pldlp_solve(LD[0, 0], P[0, 0], y[1, 2]))


def test_invalid_p_is_refused():
    c = pc.CASES["dense_17"]
    LD, P, y = pc.load(c, "LD"), pc.load(c, "P").copy(), np.ones((17, 2))
    h = _lib.handle()
    h.profile_enable(True)
    try:
        la.pldlp_solve(LD, P, y)
        assert h.profile_last()[0]["op"] == "dsytrs_bk_batched"
        la.matmul2(np.eye(2), np.eye(2))
        bad = P.copy()
        bad[5] = 17
        with pytest.raises(ValueError, match="out-of-bounds"):
            la.pldlp_solve(LD, bad, y)
        # the host-pointer entry point itself refuses before any launch: the last profiled call is still the matmul
        x = np.empty((17, 2))
        rc = h.lib.nd4hip_dsytrs_bk_batched(h.ptr, 1, 17, 2, la._ptr(LD), 0, la._ptr(bad), 0, la._ptr(y), 0, la._ptr(x))
        assert rc == -1 and "out-of-bounds" in h.lib.nd4hip_last_error().decode()
        assert h.profile_last()[0]["op"] == "dgemm_batched"
    finally:
        h.profile_enable(False)
    # the device form cannot look at P on the host: its kernels range-check every index, flag the call and stay in bounds
    guard = torch.full((3, 17, 2), 5.0, dtype=torch.float64, device="cuda")
    dLD, dY = torch.from_numpy(LD).cuda(), torch.from_numpy(y).cuda()
    for i, v in ((5, 17), (0, ~3), (16, 1 << 30), (3, -(1 << 31))):
        bad = P.copy()
        bad[i] = v
        with pytest.raises(ValueError, match=r"pldlp_solve\(LD,P,y\): P contains out-of-bounds indices\."):
            dev.pldlp_solve(dLD, torch.from_numpy(bad).cuda(), dY, out=guard[1])
        assert (guard[0] == 5.0).all() and (guard[2] == 5.0).all()
    assert pc.same_bits(dev.pldlp_solve(dLD, torch.from_numpy(P).cuda(), dY).cpu().numpy(), la.pldlp_solve(LD, P, y))
