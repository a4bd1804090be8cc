"""Every kernel path of lu.hip through nd4hip_dgetrf_batched_dev (the batch reaches the kernels as it is), against the oracle on the
same inputs: generic matrices, and inputs whose pivots are decided by exact ties, zeros, NaN and Inf (lu_common.py; each is proved
against the oracle on the CPU in test_lu_ref_host.py). Every case asserts through lu_common.regime(), the Python twin of the regime
choice of getrf_impl / lu_la_range / lu_outer_block, that it takes the path it is there for.

Gates of every member with a reference: P bit-identical to the oracle's; the same isfinite pattern (and the same infinities); on
the finite part relerr <= 1e-12 (N <= 2048; 1e-11 beyond, the gates of test_gpu_lu.py) and max |L| <= 1; LU, P and nothing else written
(GUARD sentinels either side of both, the input unchanged); omega_gpu <= G * omega_oracle with omega = max |L U - A[P]| / (|L||U|),
the product in np.longdouble, over all rows (N <= 600) or 48 rows at the regime boundaries (lu_common.sample_rows).

Case -> path -> condition in the source (lu.hip: getrf_impl; NB = 16)

  single matrix, N = 48, 63 (both structured)    lu_panel_global + lu_laswp + rank-16 nd4_gemm             N < 64
  64, 79                                         lu_panel_row<1> (no look-ahead), global tail              64 <= N < 80
  80 160 512 514 600 1026 1100 1600 2048         lu_panel_row_la<1|2|4> + lu_narrow_fused (staged panel)   N >= 80, batch <= 12, N even
                                                 + lu_update_blocks; the range's last panel and the        R by the panel's height:
                                                 tail: lu_narrow_top/_gemm, lu_panel_global                <= 512 | <= 1024 | <= 2048
  81 161 513 515 1027 1101                       the same with lu_narrow_top + lu_narrow_gemm between      N odd (scalar loads and stores)
                                                 every two panels
  (12,160) (3,600) (12,512)                      the look-ahead form over grid.y, one stage per member     2 <= batch <= 12
  (13,130) (13,511) (40,256)                     lu_panel_row<R> + lu_laswp + rank-16 product, one level   batch > 12, N < 512
  (13,512) (13,600) (13,1100) (20,640)           the same in outer blocks of 128 + lu_outer_far            batch > 12, 512 <= N <= 2048
  12 | 13 members of 512^2                       either side of LU_LA_MAX_BATCH, the same members
  2100, 2101, (2,2100)                           lu_panel_mw_la<1,2> (5 workgroups) with the fold prologue N > 2048, batch * P <= 64
                                                 (2101: lu_narrow_top/_gemm instead), outer block 512,
                                                 lu_outer_far, then lu_panel_row_la<4|2|1> below 2048 rows
  2100 with ND4HIP_LU_MW_R = 2 | 4               lu_panel_mw_la<2,1> | <4,1>: slots t + 512 i in one workgroup, lu_narrow_fused between
  4200                                           lu_panel_mw_la<1,4> (9 workgroups: P > 8)                 analytic P[c], no oracle
  (13,2100)                                      <4,8,1024> split panels + lu_laswp + lu_outer_far         13 x 5 workgroups > 64
  2100 | 4200 with ND4HIP_LU_MW_R = 0            <4,8,1024> | <8,4,1024> then <4,8,1024>                   the switch back to the split panels
  (13,2100) with ND4HIP_LU_MW_R = 4              lu_panel_mw<4,1> WITHOUT look-ahead                        batch > 12 and batch * P <= 64:
                                                 unreachable with the default rows per workgroup (test_lu_ref_host.py)

Inputs per regime (lu_common.structured_keys): generic; planted ties in every placement the kernel's layout has (two rows of one
wave; of two waves, the lower row in the later one; one thread's two register slots; a high slot-0 thread against a low slot-1
thread; three rows with mixed signs; for the multi-workgroup panel rows of different workgroups, of the last, partly filled one,
and astride a workgroup boundary) at panel columns 0, 7 and 15 of the first, a middle and the last panel, either side of an
outer-block end and of the hand-over at 2048 rows; a zero column in the second panel and at N - 3; a NaN in the last row.
Beyond 2048 rows every panel kernel gets all of these at 2100: the default multi-workgroup panel, ND4HIP_LU_MW_R = 2 | 4 | 0, and as
members of the batch of 13 the split panels and lu_panel_mw<4,1> without look-ahead; the planted input of the R = 4 runs has its ties
astride row j0 + 2048, where the two workgroups meet. 2048 has a planted input of its own (register slots 2 and 3 of one thread).
Inf below the diagonal, with and without a NaN start row, once per panel kernel: 160, 600, (13,512), 2100 (there with every
ND4HIP_LU_MW_R and in the batch of 13). The four pivot-sequence
patterns of test_gpu_lu.test_lookahead_pivot_patterns at 161, (13,512) and 2100. Member isolation, the in-place form LU == A
(bit-identical to out of place) and repeatability of the exchange (bit-identical twice) at the end.

Measured on the MI355X, every figure from one run (252 cases, about 105 s in all; the two batches of 13 x 2100^2 take 6.4 s each, every other case at most 3.6 s): omega_gpu / omega_oracle, the worst
member of each group; the oracle's omega is 1.6e-16 ... 3.4e-16 on generic and planted inputs (up to 5.0e-15 on a zero column). The
worst of all is 1.62, so G = 4: the power of two at or above twice that. It leaves room for the other summation order of the rank-16
/ 128 / 512 MFMA products and for FMA contraction, and for nothing else. Nothing failed: no kernel was changed.

  group                                              cases   ratio                                     worst relerr
  single generic, 19 sizes up to 2048                  19    <= 1.36 (513)                             9.7e-14
  single structured 48 63 79 160 161 515 600 1027 1100 44    <= 1.62 (79, zero column at N - 3)        4.1e-14
  2048 planted                                          1    0.92                                      5.0e-14
  (12,160) | (3,600) | (12,512) look-ahead             18    1.21 | 1.10 | 1.06                        2.1e-14
  (13,130) | (13,511) | (40,256) one level             20    1.24 | 1.24 | 1.24                        1.7e-14
  (13,512) | (13,600) | (13,1100) | (20,640) two       22    1.15 | 0.98 | 1.31 | 1.10                 4.6e-14
  2100 generic, ND4HIP_LU_MW_R unset | 2 | 4 | 0        4    1.55 each (the same bits of LU on the 48 sampled rows)   9.5e-14
  2100 structured (11); planted and the five zero /    29    <= 1.08; <= 1.50 (planted, R = 2)         9.8e-14
    NaN / Inf inputs with R = 2 | 4 | 0 (6 each)
  2101 generic                                          1    0.93                                      1.0e-13
  (13,2100) split panels | lu_panel_mw<4,1>, 8 members 16    1.55 | 1.55 (member 0 is the 2100 generic input)  9.8e-14

Mutations of lu.hip tried one at a time against this file and against test_gpu_lu.py as it was before this file existed (without
its 6000 / 8300 / 4096 cases), none committed:
  lu_panel_row_body prefers the higher row on equal magnitude (slots, wave and block)   first caught by test_single_structured[79-planted] (P)
  the winner over the exchange slots of lu_panel_mw_body prefers the higher row          test_tall[planted-2100] (P)
  pivot_mag gives a NaN start row -1                                                     test_single_inf_pivots[nan_diag_inf_below-160] (P)
  `fast` forced true in lu_panel_mw_body                                                 test_tall[inf_below-2100] (NaN where the reference has 0)
  the outer blocks of a batch end one panel early (phase 3 of getrf_impl)                test_batch_member[two_level_13x512-0]
Each run stopped at its first failure; the earlier test_gpu_lu.py passed under all five. `fast` forced true was not tried in
lu_panel_row_body: there the earlier test_denormal_and_huge_pivots_take_the_true_division fails too (it runs that kernel), and
the inf_below cases at 160, 600 and (13,512) take the same branch.

Oracle factorisations beyond 2048 rows: 16 (2100: generic, four planted layouts, five with zero, NaN and Inf pivots, four pivot
patterns; 2101; 2048 planted not counted). The four pivot patterns at 2100 are the generic constructions of
test_lookahead_pivot_patterns with an oracle run each, not built from `planted`: a reversal or a cyclic shift of every pivot cannot be
planted with rows r > c only.
"""
import functools

import numpy as np
import pytest

import oracle
from lu_common import (KEY_PLANTED_2048, LARGE_STRUCT, PATTERNS, SMALL_STRUCT, SPECIALS, call_getrf_dev, make_input, omega_lu, planted, planted_plants, regime, relerr,
                       rows_for_layout, sample_rows, structured_keys)
pytestmark = pytest.mark.gpu
G = 4.0              # see "Measured" above: twice the worst ratio (1.62), rounded up to a power of two (never more than 16)


def _gate(N):
    return 1e-12 if N <= 2048 else 1e-11


@functools.lru_cache(maxsize=None)
def _input(key):
    a = make_input(key)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def _ref(key):
    """(input, oracle LU, oracle P): one oracle factorisation per input and module"""
    a = _input(key)
    with np.errstate(all="ignore"):
        rlu, rp = oracle.lu_decomp(a)
    rlu.setflags(write=False)
    rp.setflags(write=False)
    return a, rlu, rp


@functools.lru_cache(maxsize=None)
def _omega_ref(key):
    """(rows of the omega sample, omega of the oracle's factors on them)"""
    a, rlu, rp = _ref(key)
    extra = [r for c, rs, _ in planted_plants(key)[0] for r in rs + [c]] if key[0] == "planted" else list(key[3:])
    rows = sample_rows(key[2], extra=extra)
    return rows, omega_lu(a, rlu, rp, rows)


def _tag(key):
    return "-".join(str(k) for k in key)


def check_member(tag, key, lu, p, with_omega=True):
    a, rlu, rp = _ref(key)
    N = key[2]
    assert np.array_equal(p, rp), tag
    fin = np.isfinite(rlu)
    assert np.array_equal(np.isfinite(lu), fin), tag
    assert np.array_equal(np.isinf(lu), np.isinf(rlu)) and np.array_equal(lu[np.isinf(rlu)], rlu[np.isinf(rlu)]), tag
    err = relerr(lu[fin], rlu[fin])
    lmax = np.abs(lu[np.tril(fin, -1)]).max(initial=0.0)
    assert err <= _gate(N) and lmax <= 1.0, (tag, err, lmax)
    if with_omega:
        rows, wo = _omega_ref(key)
        wg = omega_lu(a, lu, p, rows, ref=rlu)
        print("RATIO %-44s relerr %.2e omega_gpu %.3g omega_oracle %.3g ratio %.2f" % (tag, err, wg, wo, wg / wo))
        assert wg <= G * wo, tag


def check_properties(a, lu, p):
    """test_gpu_lu.check_properties: L U == A[P] norm-wise, max |L| <= 1, P a permutation"""
    N = a.shape[-1]
    L, U = np.tril(lu, -1) + np.eye(N), np.triu(lu)
    assert relerr(L @ U, a[p.astype(np.int64)]) <= 1e-13 * max(N, 8)
    assert np.abs(np.tril(lu, -1)).max(initial=0.0) <= 1.0
    assert np.array_equal(np.sort(p), np.arange(N))


def run(a, expect, mw=None, inplace=False, absent=()):
    """the factorisation of a [batch, N, N] through the device form, after the proof that it takes the paths `expect`"""
    a = np.asarray(a)
    a3 = a.reshape((-1,) + a.shape[-2:])
    got = regime(a3.shape[0], a3.shape[-1], mw)
    assert set(expect) <= got and not set(absent) & got, (sorted(got), expect, absent)
    lu, p, intact = call_getrf_dev(a3, inplace=inplace, mw_env=mw)
    assert intact, "a guard region or the input was written"
    return lu, p


def run_keys(keys, expect, mw=None, absent=()):
    return run(np.stack([_input(k) for k in keys]), expect, mw, absent=absent)


# -------------------------------------------------------------------------------------------------- 1. one matrix, N <= 2048
SINGLE = [(48, {"global", "laswp", "rank16"}, {"row1"}), (63, {"global"}, {"row1"}),
          (64, {"row1", "global"}, {"row_la1"}), (79, {"row1", "global"}, {"row_la1"}),
          (80, {"row_la1", "narrow_fused", "update_blocks"}, {"row1"}), (160, {"row_la1", "narrow_fused"}, ()),
          (512, {"row_la1", "narrow_fused"}, {"row_la2"}), (514, {"row_la2", "row_la1", "narrow_fused"}, {"row_la4"}),
          (600, {"row_la2", "narrow_fused"}, ()), (1026, {"row_la4", "row_la2", "row_la1", "narrow_fused"}, ()),
          (1100, {"row_la4", "narrow_fused"}, ()), (1600, {"row_la4", "narrow_fused"}, ()), (2048, {"row_la4", "narrow_fused"}, {"outer512"}),
          (81, {"row_la1", "narrow_split"}, {"narrow_fused"}), (161, {"row_la1", "narrow_split"}, {"narrow_fused"}),
          (513, {"row_la2", "narrow_split"}, {"narrow_fused"}), (515, {"row_la2", "narrow_split"}, {"narrow_fused"}),
          (1027, {"row_la4", "narrow_split"}, {"narrow_fused"}), (1101, {"row_la4", "narrow_split"}, {"narrow_fused"})]


def _paths_of(N):
    return next((e, x) for n, e, x in SINGLE if n == N)


@pytest.mark.parametrize("N", [n for n, _, _ in SINGLE])
def test_single_generic(N):
    key = ("generic", 32000 + N, N)
    expect, absent = _paths_of(N)
    lu, p = run_keys([key], expect, absent=absent)
    check_member(_tag(key), key, lu[0], p[0])


SINGLE_STRUCT = [s for s in SMALL_STRUCT + LARGE_STRUCT[:2] if s[2] is None]


@pytest.mark.parametrize("i", range(1, 5), ids=["planted", "zero_col_panel2", "zero_col_N-3", "nan_last_row"])
@pytest.mark.parametrize("N,seed", [(s[0], s[1]) for s in SINGLE_STRUCT])
def test_single_structured(N, seed, i):
    """ties, zero and NaN pivots on each single-matrix regime up to 2048 rows: 48 (global), 79 (register panel without look-ahead),
    160 / 600 / 1100 (staged look-ahead, R = 1 / 2 / 4), 161 / 515 / 1027 (the in-place narrow update of odd N)"""
    key = structured_keys(N, seed)[i]
    expect, absent = _paths_of(N)
    lu, p = run_keys([key], expect, absent=absent)
    check_member(_tag(key), key, lu[0], p[0])


def test_single_planted_2048():
    """four register slots per thread with room for every placement: ties in slots 2 and 3 of one thread (c3) in lu_panel_row_la<4>"""
    assert "row4:c3" in planted_plants(KEY_PLANTED_2048)[1]
    lu, p = run_keys([KEY_PLANTED_2048], {"row_la4", "row_la2", "row_la1", "narrow_fused"})
    check_member(_tag(KEY_PLANTED_2048), KEY_PLANTED_2048, lu[0], p[0])


@pytest.mark.parametrize("key", [k for k in SPECIALS if k[2] in (160, 600)], ids=_tag)
def test_single_inf_pivots(key):
    """+Inf below the diagonal wins (multipliers x / Inf = 0 through the IEEE division, not the reciprocal: no NaN anywhere); against a
    NaN start row it does not (pivot_mag: NaN wins only as the start row, and then also against Inf)"""
    lu, p = run_keys([key], _paths_of(key[2])[0])
    check_member(_tag(key), key, lu[0], p[0])


@pytest.mark.parametrize("fam", PATTERNS)
def test_single_pivot_patterns_odd(fam):
    """no interchange, full reversal, cyclic shift, the same far rows again and again: through lu_colblock_update's one gather/scatter
    and the in-place narrow update (N = 161)"""
    key = (fam, 32500, 161)
    lu, p = run_keys([key], {"row_la1", "narrow_split"}, absent={"narrow_fused"})
    check_member(_tag(key), key, lu[0], p[0])


# ---------------------------------------------------------------------------------------------------------------- 2. batches
def _generic_keys(batch, N, seed):
    return [("generic", seed + m, N) for m in range(batch)]


def _pad(keys, batch, N, seed):
    return keys + _generic_keys(batch - len(keys), N, seed)


BATCHES = {
    # name: (member keys, paths, paths it must not take, members with an oracle comparison, of which with omega)
    "la_12x160": (_pad(structured_keys(160, 31020) + [k for k in SPECIALS if k[2] == 160], 12, 160, 33000),
                  {"row_la1", "narrow_fused", "update_blocks"}, {"row1"}, range(12), range(12)),
    "la_3x600": (_pad(structured_keys(600, 31040)[1:3], 3, 600, 33020), {"row_la2", "row_la1", "narrow_fused"}, {"row2"}, range(3), range(3)),
    "la_12x512": (_generic_keys(12, 512, 33040), {"row_la1", "narrow_fused"}, {"batch_outer128", "row1"}, range(12), (0, 5, 11)),
    "one_level_13x130": (_pad(structured_keys(130, 31060, "batch"), 13, 130, 33060), {"row1", "global", "laswp", "rank16"},
                         {"row_la1", "batch_outer128"}, range(13), range(13)),
    "one_level_13x511": (_generic_keys(13, 511, 33080), {"row1", "rank16"}, {"row_la1", "batch_outer128"}, range(13), (0, 6, 12)),
    "one_level_40x256": (_generic_keys(40, 256, 33100), {"row1", "rank16"}, {"row_la1", "batch_outer128"}, range(40), (0, 13, 26, 39)),
    "two_level_13x512": (structured_keys(512, 31070, "batch") + [k for k in SPECIALS if k[2] == 512] + [(f, 33150, 512) for f in PATTERNS]
                         + _generic_keys(2, 512, 33160), {"row1", "batch_outer128", "laswp", "rank16"}, {"row_la1"}, range(13), range(13)),
    "two_level_13x600": (_generic_keys(13, 600, 33180), {"row2", "row1", "batch_outer128"}, {"row_la2"}, range(13), (0, 6, 12)),
    "two_level_13x1100": (_generic_keys(13, 1100, 33200), {"row4", "row2", "row1", "batch_outer128"}, {"row_la4"}, (0, 6, 12), (0, 6, 12)),
    "two_level_20x640": (_generic_keys(20, 640, 33220), {"row2", "row1", "batch_outer128"}, {"row_la2"}, range(20), (0, 9, 19)),
}


@functools.lru_cache(maxsize=1)
def _batch_result(name):
    keys, expect, absent = BATCHES[name][:3]
    assert len(set(keys)) == len(keys)
    return run_keys(keys, expect, absent=absent)


@pytest.mark.parametrize("name,m", [(n, m) for n, c in BATCHES.items() for m in c[3]], ids=lambda v: str(v))
def test_batch_member(name, m):
    """one member of a batch (the batch itself is factorised once): all gates against the oracle on that member; every member's P
    differs from its neighbour's"""
    keys, _, _, _, with_omega = BATCHES[name]
    lu, p = _batch_result(name)
    check_member(name + ":" + _tag(keys[m]), keys[m], lu[m], p[m], with_omega=m in with_omega)
    assert not np.array_equal(p[m], p[(m + 1) % len(keys)])


@pytest.mark.parametrize("name", [n for n, c in BATCHES.items() if len(c[3]) < len(c[0])])
def test_batch_members_without_oracle(name):
    keys = BATCHES[name][0]
    lu, p = _batch_result(name)
    for m, k in enumerate(keys):
        check_properties(_input(k), lu[m], p[m])


def test_batch_12_and_13_agree():
    """LU_LA_MAX_BATCH: 12 members take the look-ahead form, the same 12 with a thirteenth the throughput form in outer blocks of
    128: identical P, factors within rounding of each other and of the oracle"""
    keys = _generic_keys(13, 512, 33040)                                      # the first 12: la_12x512
    lu12, p12 = run_keys(keys[:12], {"row_la1", "narrow_fused"}, absent={"batch_outer128"})
    lu13, p13 = run_keys(keys, {"row1", "batch_outer128"}, absent={"row_la1"})
    assert np.array_equal(p12, p13[:12])
    for m in range(12):
        assert relerr(lu12[m], lu13[m]) <= 1e-12
    for m in (0, 11, 12):
        check_member("13x512:" + _tag(keys[m]), keys[m], lu13[m], p13[m], with_omega=m == 12)


# ---------------------------------------------------------------------------------------------------- 3. beyond 2048 rows
N_TALL = 2100
SEED_TALL = LARGE_STRUCT[2][1]
MW_DEFAULT = {"mw_la<1,2>", "fold", "narrow_fused", "outer512", "row_la4", "row_la2", "row_la1", "update_blocks", "global"}
TALL = [(k, None, MW_DEFAULT, {"tall8"}) for k in structured_keys(N_TALL, SEED_TALL)]
TALL += [(k, None, MW_DEFAULT, {"tall8"}) for k in SPECIALS if k[2] == N_TALL]
TALL += [((f, 34000, N_TALL), None, MW_DEFAULT, {"tall8"}) for f in PATTERNS]
TALL += [(("generic", 34010, 2101), None, {"mw_la<1,2>", "fold", "narrow_split", "outer512", "row_la4"}, {"narrow_fused", "tall8"})]
KEY_MW2 = ("planted", SEED_TALL + 5, N_TALL, "mw2")
KEY_TALL8 = ("planted", SEED_TALL + 6, N_TALL, "tall8")
KEY_MW4 = ("planted", SEED_TALL + 7, N_TALL, "mw4")        # ties astride row j0 + 2048: the two workgroups of R = 4
# zero column in the second panel and at N - 3, NaN in the last row, Inf below the diagonal without and with a NaN start row
NONFINITE_TALL = [k for k, _, _, _ in TALL[2:7]]
MW_PATHS = {2: ({"mw_la<2,1>", "narrow_fused", "outer512"}, {"fold", "mw_la<1,2>"}),
            4: ({"mw_la<4,1>", "narrow_fused", "outer512"}, {"fold", "mw_la<1,2>"}),
            0: ({"tall8", "row4", "laswp", "rank16", "outer512", "row_la4"}, {"mw_la<1,2>"})}
for _mw, _planted in ((2, KEY_MW2), (4, KEY_MW4), (0, KEY_TALL8)):         # every other panel kernel beyond 2048 rows: the same inputs again
    TALL += [(k, _mw) + MW_PATHS[_mw] for k in [TALL[0][0], _planted] + NONFINITE_TALL]


@pytest.mark.parametrize("key,mw,expect,absent", TALL, ids=["%s-mw%s" % (_tag(k), m) for k, m, _, _ in TALL])
def test_tall(key, mw, expect, absent):
    """one matrix of 2100 (2101) rows: the multi-workgroup panel with the in-kernel exchange (default: one row per thread, 5 workgroups,
    the previous panel's narrow update folded into the prologue; ND4HIP_LU_MW_R = 2 | 4: 3 | 2 workgroups with 2 | 4 register slots per
    thread), or the split panels (ND4HIP_LU_MW_R = 0); then the outer block's far update and the register panels below 2048 rows"""
    lu, p = run_keys([key], expect, mw, absent=absent)
    check_member(_tag(key) + "-mw%s" % mw, key, lu[0], p[0])


def _tall_batch():
    """13 members of 2100^2: a generic one, the planted ones of the 1024-thread layout and of two workgroups of 2048 rows, the five
    with zero, NaN and Inf pivots, generic ones with other seeds"""
    return [TALL[0][0], KEY_TALL8, KEY_MW4] + NONFINITE_TALL + _generic_keys(5, N_TALL, 34100)


@pytest.mark.parametrize("mw,expect,absent", [(None, {"tall8", "row4", "row2", "row1", "global", "laswp", "rank16", "outer512"}, {"mw<1,2>", "row_la4"}),
                                              (4, {"mw<4,1>", "row4", "laswp", "rank16", "outer512"}, {"tall8", "mw_la<4,1>", "row_la4"})],
                         ids=["split_panels", "mw_without_lookahead"])
def test_tall_batch_of_13(mw, expect, absent):
    """13 x 5 workgroups are not co-resident: the batch keeps the 8-column panels on 1024 threads. With ND4HIP_LU_MW_R = 4 (2 workgroups
    per matrix, 26 in all) it is the one shape that takes lu_panel_mw without look-ahead. Members 0 to 7 (generic, planted, zero, NaN
    and Inf pivots) against the oracle, whose factorisations test_tall shares; the properties on the five other generic members."""
    keys = _tall_batch()
    assert {"row4:c", "row4:e_last"} <= set(planted_plants(KEY_TALL8)[1]) and {"mw4:f_wg", "mw4:f_last", "mw4:f_astride"} <= set(planted_plants(KEY_MW4)[1])
    a = np.stack([_input(k) if m < 8 else make_input(k) for m, k in enumerate(keys)])
    lu, p = run(a, expect, mw, absent=absent)
    for m in range(8):
        check_member("13x2100-mw%s:%s" % (mw, _tag(keys[m])), keys[m], lu[m], p[m])
    for m in range(13):
        if m >= 8:
            check_properties(a[m], lu[m], p[m])
        assert not np.array_equal(p[m], p[(m + 1) % 13])


def _first_panel_plants(kind, N, cols, names, R, T):
    """column cols[i] gets the placement names[i] of the layout"""
    plants = []
    for c, name in zip(cols, names):
        rows, signs = next((r, s) for n, r, s in rows_for_layout(kind, 0, N, k=c, R=R, T=T) if n == name)
        plants.append((c, rows, signs))
    return plants


@pytest.mark.parametrize("mw,expect,kind,R,T,cols,names", [
    (None, {"mw_la<1,4>", "mw_la<1,2>", "fold", "outer512"}, "mw", 1, 512, (0, 1, 7, 15), ("f_three", "f_astride", "f_last", "f_wg")),
    (0, {"tall4", "tall8", "outer512"}, "row", 8, 1024, (0, 1, 2, 3, 4, 7), ("c3", "d", "c", "b", "a", "e"))],
    ids=["mw_9_workgroups", "tall4"])
def test_4200_planted_first_panel(mw, expect, kind, R, T, cols, names):
    """4200 rows: 9 workgroups per panel (PQ = 4: the poll reads four groups of slots), or <8, 4, 1024> (rows t + 1024 i, 4-column
    panels). No oracle at this size: ties planted in the first columns only, where the outcome is known without one: P[c] is the
    lowest planted row and the losers' multipliers are exactly +-1; L U = A[P] and max |L| <= 1 on the whole matrix."""
    N = 4200
    plants = _first_panel_plants(kind, N, cols, names, R, T)
    a = planted(34200, N, plants)
    lu, p = run(a[None], expect, mw)
    lu, p = lu[0], p[0]
    pos = np.argsort(p)
    for c, rows, signs in plants:
        assert p[c] == min(rows), (c, rows, p[c])
        win = signs[rows.index(min(rows))]
        assert lu[c, c] == win * 4096.0
        for r, s in zip(rows, signs):
            if r != min(rows):
                assert lu[pos[r], c] == s * win, (c, r)
    check_properties(a, lu, p)


# ------------------------------------------------------------------------------ 4. isolation, in place, twice the same
@pytest.mark.parametrize("batch,N,expect", [(12, 160, {"row_la1"}), (13, 600, {"row2", "batch_outer128"}), (2, N_TALL, {"mw_la<1,2>", "fold"})])
def test_member_isolation(batch, N, expect):
    """member 1 has a zero column (NaN from its second panel on), the others are clean: each of them is finite, passes every gate
    and equals, with identical P and to relerr <= 1e-12, the same matrix factorised alone (not bit for bit: alone it may take another form)"""
    zc = ("zero_column", 35001, N, 21) if N != N_TALL else TALL[2][0]
    keys = _generic_keys(batch, N, 35010 + N) if N != N_TALL else [TALL[0][0], zc]
    keys[1] = zc
    lu, p = run_keys(keys, expect)
    check_member("isolation %dx%d:%s" % (batch, N, _tag(zc)), zc, lu[1], p[1], with_omega=False)
    omega_on = (0, 2, batch - 1)
    for m in [m for m in range(batch) if m != 1]:
        assert np.isfinite(lu[m]).all()
        check_member("isolation %dx%d:%s" % (batch, N, _tag(keys[m])), keys[m], lu[m], p[m], with_omega=m in omega_on)
        solo, psolo = run_keys([keys[m]], ())
        assert np.array_equal(psolo[0], p[m]) and relerr(lu[m], solo[0]) <= 1e-12
        assert not np.array_equal(p[m], p[(m + 1) % batch])


@pytest.mark.parametrize("batch,N,expect", [(1, 160, {"row_la1", "narrow_fused"}), (1, 513, {"row_la2", "narrow_split"}),
                                            (13, 512, {"row1", "batch_outer128"}), (1, N_TALL, {"mw_la<1,2>", "fold", "outer512"})])
def test_in_place_and_repeatable(batch, N, expect):
    """the ABI's in-place form LU == A gives bit for bit what the out-of-place call gives, and the same call twice in one process gives
    the same bits (2100: the exchange slots are cleared per call and the tags restart)"""
    a = np.stack([_input(k) for k in (_generic_keys(batch, N, 33040) if N == 512 else [TALL[0][0]] if N == N_TALL else [("generic", 32000 + N, N)])])
    lu, p = run(a, expect)
    lu2, p2 = run(a, expect)
    lui, pi = run(a, expect, inplace=True)
    bits = lambda x: x.view(np.int64)
    assert np.array_equal(bits(lu), bits(lu2)) and np.array_equal(p, p2)
    assert np.array_equal(bits(lu), bits(lui)) and np.array_equal(p, pi)
