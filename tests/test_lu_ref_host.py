"""CPU checks of what test_gpu_lu_paths.py rests on: every structured input does to the REFERENCE what its docstring says (the planted
ties are live when their column is reached, the lowest planted row wins, the losers' multipliers are exactly +-1; the zero, NaN and
Inf inputs leave exactly the predicted non-finite pattern), `regime()` returns the documented paths on both sides of every boundary
of lu.hip's regime choice, `omega_lu` is small on the oracle's factors and large on a wrong one, and the host form's chunking is what
the edits to test_gpu_lu.py say it is.

Measured here: omega_lu of the oracle 2.4e-16 (N = 160), 3.3e-16 (600), 2.6e-16 (2100 planted, 48 rows); the largest term of one
entry left out: 0.033 to 0.056; LU[N-1, N-1] changed by 1e-9 relative: 1.9e-12 to 6.1e-11."""
import functools

import numpy as np
import pytest

import oracle
from lu_common import (EPS, KEY_PLANTED_2048, LARGE_STRUCT, SMALL_STRUCT, SPECIALS, V, make_input, omega_lu, planted_plants, regime, rows_for_layout, sample_rows,
                       structured_keys)
from test_gpu_batched_paths import _host_chunk


@functools.lru_cache(maxsize=None)
def _ref(key):
    a = make_input(key)
    with np.errstate(all="ignore"):
        lu, p = oracle.lu_decomp(a)
    return a, lu, p


def _nonfinite(lu):
    return ~np.isfinite(lu)


def _region(N, c, with_diag=False):
    want = np.zeros((N, N), dtype=bool)
    want[c + 1:, c:] = True
    want[c, c] = with_diag
    return want


def check_family(key):
    """the reference's outcome on the input `key`, as the family's docstring predicts it"""
    a, lu, p = _ref(key)
    fam, N = key[0], key[2]
    assert np.array_equal(np.sort(p), np.arange(N))
    if fam == "planted":
        plants, used = planted_plants(key)
        assert len(plants) >= 2
        assert np.isfinite(lu).all() and np.abs(np.triu(lu)).max() == V and np.abs(np.tril(lu, -1)).max() <= 1.0
        pos = np.argsort(p)                                                      # where each original row ended up
        for c, rows, signs in plants:
            assert p[c] == min(rows), (c, rows, p[c])
            win = signs[rows.index(min(rows))]
            assert lu[c, c] == win * V
            for r, s in zip(rows, signs):
                if r != min(rows):
                    assert lu[pos[r], c] == s * win, (c, r)                      # exactly +-1: the tie was live
    elif fam == "zero_column":
        assert np.array_equal(_nonfinite(lu), _region(N, key[3]))
    elif fam == "nan_last_row":
        want = np.zeros((N, N), dtype=bool)
        want[N - 1, key[3]:] = True
        assert np.array_equal(_nonfinite(lu), want) and p[N - 1] == N - 1
    elif fam == "inf_below":
        c, r = key[3:]
        want = np.zeros((N, N), dtype=bool)
        want[c, c] = True
        assert p[c] == r and np.array_equal(_nonfinite(lu), want) and lu[c, c] == np.inf and not lu[c + 1:, c].any()
    elif fam == "nan_diag_inf_below":
        c, r = key[3:]
        assert p[c] == c and np.array_equal(_nonfinite(lu), _region(N, c, with_diag=True))
    else:
        assert np.isfinite(lu).all()


@pytest.mark.parametrize("N,seed,variant", SMALL_STRUCT + LARGE_STRUCT[:2])
def test_structured_inputs_do_what_they_say(N, seed, variant):
    for key in structured_keys(N, seed, variant):
        check_family(key)


@pytest.mark.parametrize("key", [k for k in SPECIALS if k[2] <= 600] + [("zero_column", 35001, 160, 21), ("zero_column", 35001, 600, 21)],   # (the last two: test_member_isolation)
                         ids=lambda k: "%s-%d" % (k[0], k[2]))
def test_inf_and_nan_pivots_do_what_they_say(key):
    check_family(key)


def test_every_placement_of_a_layout_is_planted_somewhere():
    """the placement names each regime's planted input uses (no oracle needed): every placement rows_for_layout has for a layout is
    planted in at least one of the inputs that reach the kernel with that layout"""
    used = lambda N, *variant: set(planted_plants(("planted", 0, N) + variant)[1])
    assert used(63) == {"global1:a", "global1:e"}
    assert {"row1:a", "row1:b0"} <= used(79) and {"row1:a", "row1:b0", "row1:b", "row1:e", "row1:e_last"} <= used(160) | used(512, "batch")
    assert {"row2:a", "row2:b", "row2:c", "row2:d", "row2:e"} <= used(600) and "row2:e_last" in used(1027)
    assert {"row4:a", "row4:b", "row4:c", "row4:d", "row4:c3", "row4:e"} <= used(2048) and "row4:e_last" in used(1100)
    assert {"mw1:f_wg", "mw1:f_last", "mw1:f_astride", "mw1:f_three", "mw1:a", "mw1:b0", "mw1:b", "mw1:e", "mw1:e_last"} <= used(2100)
    assert {"mw2:f_wg", "mw2:f_last", "mw2:f_astride", "mw2:f_three", "mw2:a", "mw2:b", "mw2:c", "mw2:d", "mw2:e"} <= used(2100, "mw2")
    assert {"mw4:f_wg", "mw4:f_last", "mw4:f_astride", "mw4:a", "mw4:b", "mw4:c", "mw4:d", "mw4:c3", "mw4:e", "mw4:e_last"} <= used(2100, "mw4")
    assert {"row4:a", "row4:b", "row4:c", "row4:d", "row4:e", "row4:e_last"} <= used(2100, "tall8")        # 1024 threads; slot 2 is partly filled
    for c, rows, _ in planted_plants(("planted", 0, 2100, "mw4"))[0][:3]:                     # the two workgroups of R = 4 meet at row j0 + 2048
        assert min(rows) < 2048 <= max(rows)


def test_planted_2048_does_what_it_says():
    check_family(KEY_PLANTED_2048)


def test_planted_2100_and_omega_sensitivity():
    """the N = 2100 instance (plants in the multi-workgroup panels, either side of the hand-over to the register panels at 2048 rows
    and of the outer-block end), and omega_lu at the three sizes: clean <= 4 eps, one dropped term > 1e-3, one entry off by 1e-9
    relative > 1e3 x the clean value"""
    key = structured_keys(*LARGE_STRUCT[2])[1]
    check_family(key)
    plants, used = planted_plants(key)
    assert {"mw1:f_wg", "mw1:f_last", "mw1:f_astride"} <= set(used) and any(u.startswith("row4") for u in used)
    for k in (("generic", 31300, 160), ("generic", 31301, 600), key):
        a, lu, p = _ref(k)
        N = k[2]
        rows = sample_rows(N, extra=[r for c, rs, _ in plants for r in rs + [c]] if k is key else ())
        assert len(rows) == (N if N <= 600 else 48)
        clean = omega_lu(a, lu, p, rows)
        # entry (i, i + 1) of a row in the middle of the sample that is not a planted one (whose terms are exact zeros)
        i = next(int(r) for r in rows[len(rows) // 2:] if r + 1 < N and np.abs(lu[r, :r] * lu[:r, r + 1]).max() > 1e-3)
        j = i + 1
        k = int(np.argmax(np.abs(lu[i, :i] * lu[:i, j])))                          # its largest term: one term of one rank-16 update
        dropped = lu.copy()
        dropped[i, j] += lu[i, k] * lu[k, j]                                       # ... left out
        bumped = lu.copy()
        bumped[N - 1, N - 1] *= 1.0 + 1e-9
        wd, wb = omega_lu(a, dropped, p, rows), omega_lu(a, bumped, p, rows)
        print("N %d omega clean %.3g dropped term %.3g bumped entry %.3g" % (N, clean, wd, wb))
        assert clean <= 4 * EPS and wd > 1e-3 and wb > 1e3 * clean


def test_omega_excludes_what_the_reference_lost():
    """zero column: LU[c+1:, c:] is excluded and the finite part is as clean as a generic factorisation; a non-finite entry where the
    reference is finite gives NaN (fails every gate)"""
    for key in (("zero_column", 31310, 96, 21), ("nan_last_row", 31311, 96, 21), ("inf_below", 31312, 96, 21, 80)):
        a, lu, p = _ref(key)
        assert omega_lu(a, lu, p) <= 4 * EPS
        bad = lu.copy()
        bad[3, 5] = np.nan
        assert not omega_lu(a, bad, p, ref=lu) <= 1.0
        off = lu.copy()
        off[10, 12] *= 1.0 + 1e-6
        assert omega_lu(a, off, p, ref=lu) > 1e-9


def test_rows_for_layout_placements():
    """each placement sits where its name says, in the kernel's (workgroup, wave, thread, slot) coordinates"""
    by = {n: (r, s) for n, r, s in rows_for_layout("row", 32, 1100, k=7, R=4, T=512)}
    t = lambda r: (r - 32) % 512
    slot = lambda r: (r - 32) // 512
    a, b, c, d, e = (by[n][0] for n in "abcde")
    assert t(a[0]) // 64 == t(a[1]) // 64 and slot(a[0]) == slot(a[1]) == 0
    assert b[0] < b[1] and slot(b[0]) == 0 and slot(b[1]) == 1 and t(b[0]) // 64 > t(b[1]) // 64     # the lower row in the later wave
    assert t(c[0]) == t(c[1]) and slot(c[1]) == slot(c[0]) + 1
    assert d[0] < d[1] and slot(d[0]) == 0 and slot(d[1]) == 1 and t(d[0]) > t(d[1])
    assert len(e) == 3 and len({t(r) // 64 for r in e}) == 3 and set(by["e"][1]) == {1, -1}
    assert all(r > 39 for rows, _ in by.values() for r in rows)                    # never the start row j0 + k or a finished row
    mw = {n: (r, s) for n, r, s in rows_for_layout("mw", 16, 2100, k=15, R=1)}
    wg = lambda r: (r - 16) // 512
    assert wg(mw["f_wg"][0][0]) != wg(mw["f_wg"][0][1])
    assert wg(mw["f_last"][0][1]) == (2100 - 16 - 1) // 512 and wg(mw["f_last"][0][0]) == 1
    assert wg(mw["f_astride"][0][0]) + 1 == wg(mw["f_astride"][0][1]) and mw["f_astride"][0][0] + 1 == mw["f_astride"][0][1]
    assert len({wg(r) for r in mw["f_three"][0]}) == 3
    assert "c" not in {n for n, _, _ in rows_for_layout("row", 0, 160, R=1)}       # one slot: no two-slot placement


@pytest.mark.parametrize("batch,N,mw,has,has_not", [
    (1, 63, None, {"global"}, {"row1", "row_la1"}),
    (1, 64, None, {"row1", "global", "laswp"}, {"row_la1"}),                       # 64 rows: the register panel, not yet the look-ahead form
    (1, 79, None, {"row1", "global"}, {"row_la1"}),
    (1, 80, None, {"row_la1", "update_blocks", "narrow_fused", "narrow_split", "global"}, {"row1"}),   # two look-ahead panels of 80 and 64 rows
    (1, 96, None, {"row_la1", "narrow_fused", "narrow_split"}, {"row1"}),         # (the range's last panel always takes the in-place pair)
    (1, 97, None, {"row_la1", "narrow_split"}, {"narrow_fused"}),                 # odd N: lu_narrow_top + lu_narrow_gemm
    (1, 512, None, {"row_la1"}, {"row_la2"}),
    (1, 513, None, {"row_la2", "row_la1", "narrow_split"}, {"row_la4", "narrow_fused"}),
    (1, 1024, None, {"row_la2"}, {"row_la4"}),
    (1, 1025, None, {"row_la4", "row_la2"}, set()),
    (1, 2048, None, {"row_la4", "narrow_fused"}, {"outer512", "mw_la<1,2>", "tall8"}),
    (1, 2049, None, {"mw_la<1,2>", "outer512", "row_la4", "narrow_split"}, {"fold", "tall8"}),   # one tall panel: nothing to fold into
    (1, 2100, None, {"mw_la<1,2>", "fold", "narrow_fused", "outer512", "row_la4", "row_la2", "row_la1", "global"}, {"tall8", "mw<1,2>"}),
    (1, 2101, None, {"mw_la<1,2>", "fold", "narrow_split", "outer512"}, {"narrow_fused"}),
    (1, 2100, 2, {"mw_la<2,1>", "narrow_fused", "outer512"}, {"fold", "mw_la<1,2>"}),
    (1, 2100, 4, {"mw_la<4,1>", "narrow_fused"}, {"fold"}),
    (1, 2100, 0, {"tall8", "row4", "outer512", "row_la4"}, {"mw_la<1,2>", "tall4"}),
    (1, 4200, None, {"mw_la<1,4>", "mw_la<1,2>", "fold", "outer512"}, {"tall8", "tall4"}),             # 9 workgroups: PQ = 4
    (1, 4200, 0, {"tall4", "tall8", "outer512"}, {"mw_la<1,4>"}),
    (2, 2100, None, {"mw_la<1,2>", "fold"}, {"tall8"}),
    (12, 2100, None, {"mw_la<1,2>"}, {"tall8"}),                                   # 12 x 5 workgroups <= 64
    (13, 2100, None, {"tall8", "outer512", "row4", "row2", "row1", "global", "rank16"}, {"mw<1,2>", "mw_la<1,2>", "row_la4"}),   # 13 x 5 > 64
    (13, 2100, 4, {"mw<4,1>", "outer512", "row4"}, {"tall8", "mw_la<4,1>"}),      # the only way to lu_panel_mw without look-ahead
    (32, 2100, 4, {"mw<4,1>"}, {"tall8"}),
    (33, 2100, 4, {"tall8"}, {"mw<4,1>"}),                                         # 33 x 2 > 64
    (12, 160, None, {"row_la1", "narrow_fused"}, {"row1"}),
    (13, 160, None, {"row1", "laswp", "rank16", "global"}, {"row_la1", "batch_outer128"}),
    (12, 512, None, {"row_la1"}, {"batch_outer128", "row1"}),
    (13, 511, None, {"row1"}, {"batch_outer128"}),
    (13, 512, None, {"row1", "batch_outer128"}, {"row_la1"}),
    (13, 600, None, {"row2", "row1", "batch_outer128", "global"}, {"row_la2"}),
    (13, 1100, None, {"row4", "row2", "row1", "batch_outer128"}, set()),
    (13, 2048, None, {"row4", "batch_outer128"}, {"outer512"}),
    (13, 130, None, {"row1", "global"}, {"batch_outer128"}),
    (40, 256, None, {"row1"}, {"batch_outer128"}),
])
def test_regime_at_every_boundary(batch, N, mw, has, has_not):
    got = regime(batch, N, mw)
    assert has <= got, (has - got, got)
    assert not (has_not & got), (has_not & got)


def test_no_default_shape_reaches_the_plain_multi_workgroup_panel():
    """lu_panel_mw without look-ahead needs batch > 12 together with batch * ceil(N / mw_rt) <= 64: with the default rows per
    workgroup (N <= 8192: 512, so at least 5 workgroups beyond 2048 rows; <= 16384: 1024, at least 9; above: 2048, at least 9) that
    is impossible; only ND4HIP_LU_MW_R=4 with 13 <= batch <= 32 gets there"""
    for N in (2049, 2100, 4096, 8192, 8193, 16384, 16385, 32768):
        for batch in (1, 12, 13, 14, 32, 64):
            assert not any(p.startswith("mw<") for p in regime(batch, N)), (batch, N)
    for batch in (13, 32):
        assert "mw<4,1>" in regime(batch, 2100, 4)
    assert not any(p.startswith("mw<") for p in regime(12, 2100, 4) | regime(33, 2100, 4))


def test_what_the_host_form_makes_of_the_old_batch_shapes():
    """la.lu_decomp cuts a batch into chunks of about 64 MB, at most 8: the shapes test_gpu_lu.py used for the throughput form and for
    the split panels reached the kernels as batches of 8, 7 and 2, all of which take the look-ahead form. Those tests now go
    through the device form."""
    assert _host_chunk(16, 16 * 512 ** 2 + 4 * 512) == 8
    assert _host_chunk(14, 16 * 600 ** 2 + 4 * 600) == 7
    assert _host_chunk(14, 16 * 2100 ** 2 + 4 * 2100) == 2
    for batch, N in ((8, 512), (7, 600)):
        assert "row_la1" in regime(batch, N) and "batch_outer128" not in regime(batch, N)
    assert "tall8" not in regime(2, 2100) and "tall8" in regime(14, 2100) and "batch_outer128" in regime(16, 512) | regime(14, 600)
