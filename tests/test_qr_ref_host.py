"""CPU side of the QR path tests: the dispatch twins of qr_common.py pinned on both sides of every boundary of the QR drivers (qr.hip) and panel launchers (qr_house.hip, qr_rowsplit.hip, qr_batched_panel.hip), the
structured input families proved to do to the oracle and to the panels what they claim, and the oracle's invariance under
power-of-two column scaling (what lets test_gpu_qr_paths.py demand bit-identical factors for `graded`). No GPU."""
import numpy as np
import pytest

import oracle
import qr_common as qc
from qr_common import CASES, EPS, form, panel_plan

# the oracle's own column-wise backward error and orthogonality over every case of test_gpu_qr_paths.py of at most 1100 rows, all five
# families, and the 2064 x 272 full case, in units of eps: measured 6.4 ... 130 (colbe; 34 without la_300x130 dense, the one tall input
# whose reference branch leaves 130) and 7 ... 64 (orth; 34 up to 1100 rows). The bounds below are those with a little room.
ORACLE_COLBE_EPS = (4.0, 160.0)
ORACLE_ORTH_EPS = (5.0, 80.0)


# ------------------------------------------------------------------------------------------------------------------ form()
@pytest.mark.parametrize("args,want", [
    ((1, 63, 63, False), "blocked"), ((1, 64, 64, False), "lookahead"),                      # m: 63 | 64
    ((1, 2048, 2048, False), "lookahead"), ((1, 2049, 2049, False), "tall"),                 # 2048 | 2049
    ((24, 320, 320, False), "lookahead"), ((25, 320, 320, False), "batched"),                # batch: 24 | 25
    ((8, 2100, 1100, False), "tall"), ((9, 2100, 1100, False), "blocked"),                   # 8 | 9 beyond 2048 rows
    ((1, 2100, 255, True), "blocked"), ((1, 2100, 256, True), "tall"),                       # L: 255 | 256
    ((1, 16384, 16384, False), "tall"), ((1, 16385, 16385, False), "blocked"),
    ((1, 2310, 280, True), "tall"), ((1, 2330, 280, True), "blocked"),                       # a ragged last panel must fit 2048 rows
    ((25, 128, 128, False), "batched"), ((25, 112, 112, False), "blocked"),                  # panels: 8 | 7 (two outer blocks of 64)
    ((25, 256, 256, False), "batched"), ((25, 240, 240, False), "batched"),                  # 16 | 15: blocks of 128 | 64
    ((25, 100, 100, False), "blocked"), ((25, 128, 131, False), "batched"),                  # L % 16; an odd ld stays batched
    ((2, 40, 40, False), "blocked"), ((30, 40, 40, False), "blocked"),
    ((1, 2049, 3, False), "tsqr"), ((1, 2049, 3, True), "blocked"),                          # TSQR: never for the full form
    ((1, 4096, 1024, False), "tsqr"), ((1, 4096, 1040, False), "tall"),                      # the stacked R fits 2048 rows ...
    ((1, 8320, 832, False), "tsqr"), ((1, 8319, 832, False), "tall") ,                      # ... or is at most half as tall as A
    ((1, 70000, 64, False), "tsqr"), ((16385, 4096, 16, False), "blocked"),                  # batch * nblk <= 32768
])
def test_form_on_both_sides_of_every_boundary(args, want):
    assert form(*args) == want


def test_batched_form_needs_more_than_24_matrices():
    """M <= 2048 with 2 <= batch <= 24 is the look-ahead form from 64 rows on; below 64 rows there are at most 3 panels, fewer than
    two outer blocks: qr_choose's `batch > 1` never decides, and form_q = compact_wy is unreachable in the batched form"""
    for batch in (2, 24):
        for M in (16, 48, 63, 64, 100, 2048):
            for N in (M, 2 * M, max(M // 2, 1)):
                assert form(batch, M, N, False) != "batched"


# -------------------------------------------------------------------------------------------------------------- panel_plan()
@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_every_gpu_case_takes_the_path_it_names(case):
    qc.check_plan(case)


def _kernels(*args):
    return panel_plan(*args)["panels"]


def test_panel_kernels_by_height_and_batch():
    # row-split launch: batch 8 | 9; R by height 512 | 513, 1024 | 1025; stops below 64 rows and at a ragged panel
    assert _kernels(8, 96, 96, False) == ["qrh_bc<1>"] * 3 + ["qr_panel_row_la<1>"] * 3
    assert _kernels(9, 96, 96, False) == ["qr_panel_row_la<1>"] * 6
    assert _kernels(1, 528, 32, False) == ["qrh_bc<2>", "qrh_bc<1>"] and _kernels(1, 1040, 32, False) == ["qrh_bc<4>", "qrh_bc<2>"]
    assert _kernels(1, 300, 130, False) == ["qrh_bc<1>"] * 8 + ["qr_panel_row_la<1>"]
    assert _kernels(9, 528, 32, False) == ["qr_panel_row_la<2>", "qr_panel_row_la<1>"]
    assert _kernels(9, 1040, 32, False) == ["qr_panel_row_la<4>", "qr_panel_row_la<2>"]
    assert [qc.rowsplit_workgroups(m) for m in (64, 496, 497, 600, 1100, 2048)] == [1, 1, 2, 2, 3, 5]
    # batched panels: batch 63 | 64 picks the few-wave variants up to 1024 rows; 256 | 257, 512 | 513, 1024 | 1025
    assert _kernels(63, 256, 128, False)[0] == "qrb_panel<1,8>" and _kernels(64, 256, 128, False)[0] == "qrb_panel<4,1>"
    assert _kernels(64, 272, 128, False)[:2] == ["qrb_panel<4,2>", "qrb_panel<4,1>"]
    assert _kernels(64, 528, 128, False)[:2] == ["qrb_panel<4,4>", "qrb_panel<4,2>"]
    assert _kernels(64, 1040, 128, False)[:2] == ["qrb_panel<4,8>", "qrb_panel<4,4>"]
    assert _kernels(25, 528, 128, False)[:2] == ["qrb_panel<2,8>", "qrb_panel<1,8>"]
    assert _kernels(25, 1040, 128, False)[:2] == ["qrb_panel<4,8>", "qrb_panel<2,8>"]
    # an odd leading dimension, a ragged panel and fewer than 64 rows keep the thread-per-row kernel
    assert set(_kernels(25, 128, 131, False)) == {"qr_panel_row<1,8>"} and set(_kernels(64, 128, 131, False)) == {"qr_panel_row<4,1>"}
    assert _kernels(25, 100, 100, False) == ["qrb_panel<1,8>"] * 3 + ["qr_panel_row<1,8>"] * 4
    # beyond 2048 rows without the row-split launch: 2048 | 2049, 4096 | 4097, 8192 | 8193
    assert _kernels(9, 2064, 32, True) == ["qr_panel_part<4,8>", "qrb_panel<4,8>"]
    assert _kernels(1, 4112, 32, True) == ["qr_panel_part<8,4>", "qr_panel_part<4,8>"]
    assert _kernels(1, 8208, 32, True) == ["qr_panel<1,false>", "qr_panel_part<8,4>"]


def test_outer_blocks_qt_and_form_q():
    p = panel_plan
    assert p(25, 128, 128, False)["outer"] == (64, False) and p(25, 144, 144, False)["outer"] == (64, True)
    assert p(25, 240, 240, False)["outer"] == (64, True) and not p(25, 240, 240, False)["coupling"]          # 15 panels
    assert p(25, 256, 256, False)["outer"] == (128, False) and p(25, 256, 256, False)["coupling"]            # 16 panels
    assert p(25, 272, 272, False)["outer"] == (128, True)
    assert p(9, 2100, 1100, False)["outer"] == (128, True) and p(25, 112, 112, False)["outer"] is None
    # Q^T accumulator: batch 4 | 5, L 255 | 256
    assert p(4, 320, 320, False)["qt"] and not p(5, 320, 320, False)["qt"]
    assert p(1, 256, 256, False)["qt"] and not p(1, 255, 255, False)["qt"] and p(1, 257, 257, False)["form_q"] == "qt_transpose"
    assert p(1, 255, 255, False)["form_q"] == "panel_backward" and p(25, 128, 128, False)["form_q"] == "batched_backward"
    assert p(1, 2064, 272, True)["form_q"] == "tall_blocks" and p(2, 2064, 272, True)["form_q"] == "tall_blocks_rebuild"
    # compact_wy (form_q_compact_wy): only the blocked form beyond 2048 rows with at most 4 matrices and 256 columns, e.g. a
    # ragged last panel taller than 2048 rows; the oracle costs M N^2 there, so no GPU case names it
    assert p(1, 5000, 2900, False)["form"] == "blocked" and p(1, 5000, 2900, False)["form_q"] == "compact_wy"
    # the wide tail of the last thread-per-row reflector
    assert p(1, 272, 600, False)["update_blocks"] and not p(1, 300, 130, False)["update_blocks"]


def test_tall_form_blocks_and_the_ragged_last_panel():
    t = panel_plan(1, 2100, 256, True)
    assert t["panels"] == ["qrh_bc<0>"] * 4 + ["qrh_bc<4>"] * 12 and t["tall_blocks"] == 1 and t["far"]
    # the ragged last panel sits in an outer block that starts above 2048 rows: the whole block is factorised with one level
    r = panel_plan(1, 2310, 280, True)
    assert r["tall_blocks"] == 2 and r["panels"] == ["qrh_bc<0>"] * 17 + ["qr_panel_row_la<4>"]
    # ... and when it is the first panel of its block nothing changes
    assert panel_plan(1, 2200, 264, True)["panels"] == ["qrh_bc<0>"] * 10 + ["qrh_bc<4>"] * 6 + ["qr_panel_row_la<4>"]


def test_tsqr_split():
    for case in CASES:
        if case["id"] in qc.TSQR_EXPECT:
            qc.check_plan(case)
    t = panel_plan(1, 70000, 64, False)["tsqr"]
    assert t["blocks"]["form"] == "blocked" and t["blocks"]["panels"] == ["qrb_panel<4,8>"] * 4 and t["stacked"]["form"] == "tsqr" and t["stacked"]["tsqr"]["nblk"] == 2
    assert panel_plan(1, 2049, 3, False)["tsqr"]["blocks"]["form"] == "lookahead"


def test_panel_entry_point():
    assert [qc.panel_entry(b, M) for b, M in ((1, 64), (8, 600), (1, 1100), (8, 2048))] == [("qrh_bc<1>", 1), ("qrh_bc<2>", 2), ("qrh_bc<4>", 3), ("qrh_bc<4>", 5)]
    assert [qc.panel_entry(9, M)[0] for M in (300, 600, 1100)] == ["qrb_panel<1,8>", "qrb_panel<2,8>", "qrb_panel<4,8>"]
    assert [qc.panel_entry(64, M)[0] for M in (200, 400, 900, 1100)] == ["qrb_panel<4,1>", "qrb_panel<4,2>", "qrb_panel<4,4>", "qrb_panel<4,8>"]
    assert qc.panel_entry(8, 63)[0] == "qr_panel_row<1,8>" and qc.panel_entry(70, 48)[0] == "qr_panel_row<4,1>"


# ---------------------------------------------------------------------------------------------------------------- the families
def test_adv_and_kahan_blocks_do_what_they_claim():
    """The model on the exact diagonal blocks. adv: the first three pairs pass the pivot test with ADV_SPARE to spare; the first is hot by
    the series, the second by the elimination chain (max |E| = 4.5e-4), the third is flagged after the first pass (max |E| = 0.46
    against HR_PASS1_MAX = 1e-2). The fourth, cond(K) = 3.3e11, claims nothing: cond(K^T K) eps = 2.5e7, so fp64 cannot tell its
    Gram matrix from an indefinite one and rounding decides between breakdown in phase B and the flag after the first pass. kahan: s = 0.9 and 0.8
    are hot by the series; s = 0.7 has its smallest pivot ratio at 0.7^30 = 2.25e-5, 2.25 times the criterion, and claims nothing."""
    for (c, d), claim in zip(qc.ADV_PAIRS[:3], qc.ADV_CLAIMS[:3]):
        m = qc.gram_model(qc.adv_block(c, d))
        assert qc.classify(m, spare=qc.ADV_SPARE) == claim, (c, d, m)
        assert abs(m["ratio"] / (d * d / (c * c * (1 + 14 * d * d) + d * d)) - 1) <= 0.01
    assert [round(np.log10(qc.gram_model(qc.adv_block(c, d))["cond"])) for c, d in qc.ADV_PAIRS] == [4, 7, 10, 12]
    k4 = qc.adv_block(*qc.ADV_PAIRS[3])
    assert np.linalg.cond(k4) ** 2 * EPS >= 1e6
    for s, claim in zip(qc.KAHAN_S, ("hot, series", "hot, series", None)):
        assert qc.classify(qc.gram_model(qc.kahan_block(s))) == claim
    assert abs(qc.gram_model(qc.kahan_block(0.7))["ratio"] / 0.7 ** 30 - 1) <= 0.01


GRAM_CASES = [c for c in CASES if "cond" in qc.families_of(c, panel_plan(c["batch"], c["M"], c["N"], c["full"]))]


@pytest.mark.parametrize("case", GRAM_CASES, ids=[c["id"] for c in GRAM_CASES])
def test_cond_panels_are_clear_of_the_criterion(case):
    """every full panel of at least 64 rows of every cond input is hot by the series or flagged, with SPARE to spare; both kinds occur"""
    a, other = qc.batch_input(case, "cond")
    seen = set()
    for member in ([a[0]] if other is None else [a[0], a[other]]):
        for p, K in enumerate(qc.panel_blocks(member)):
            if case["M"] - 16 * p < qc.HR_MIN_ROWS:                        # (shorter panels take the thread-per-row kernels)
                break
            cl = qc.classify(qc.gram_model(K))
            want = "hot, series" if qc.COND_DELTAS[p % 6] >= 3e-2 else "flagged"
            assert cl == want, (case["id"], p, cl)
            seen.add(cl)
    assert seen == {"hot, series", "flagged"} or case["M"] - 32 < qc.HR_MIN_ROWS or min(case["M"], case["N"]) < 48          # (fewer than three such panels)


def _oracle(a, full):
    with np.errstate(all="ignore"):
        return (oracle.qr_decomp_full if full else oracle.qr_decomp)(a)


ORACLE_CASES = [c for c in CASES if c["M"] <= 1100] + [c for c in CASES if c["id"] == "tall_272"]


@pytest.mark.parametrize("case", ORACLE_CASES, ids=[c["id"] for c in ORACLE_CASES])
def test_oracle_metrics_on_every_family(case):
    plan = panel_plan(case["batch"], case["M"], case["N"], case["full"])
    for fam in qc.families_of(case, plan):
        a = qc.batch_input(case, fam)[0][0]
        q, r = _oracle(a, case["full"])
        assert qc.is_triu(r)
        cb, ob = qc.colbe(a, q, r) / EPS, qc.orth(q, both=case["full"] or case["M"] <= case["N"]) / EPS
        assert ORACLE_COLBE_EPS[0] <= cb <= ORACLE_COLBE_EPS[1] and ORACLE_ORTH_EPS[0] <= ob <= ORACLE_ORTH_EPS[1], (case["id"], fam, cb, ob)


@pytest.mark.parametrize("shape,full", [((300, 130), False), ((272, 600), False), ((257, 257), False), ((300, 130), True), ((130, 300), True)])
def test_oracle_commutes_with_power_of_two_column_scaling(shape, full):
    """oracle(A D) == (Q, R D) bit for bit, D = diag(2^k_j), k_j = ((37 j) mod 201) - 100"""
    a = qc.make_input("dense", 62000 + shape[0], *shape)
    d = np.ldexp(1.0, qc.graded_exponents(shape[1]))
    q, r = _oracle(a, full)
    qg, rg = _oracle(a * d, full)
    assert np.array_equal(qg, q) and np.array_equal(rg, r * d)
    assert np.array_equal(qc.make_input("graded", 62000 + shape[0], *shape), a * d)


def test_special_inputs_against_the_oracle():
    """triangular input: Q = I and R = A exactly; zero columns stay exactly zero in R and do not disturb the oracle's other columns
    beyond rounding; one NaN shows in R"""
    t = qc.make_input("triu", 62100, 300, 130)
    q, r = _oracle(t, False)
    assert np.array_equal(q, np.eye(300)[:, :130]) and np.array_equal(r, t[:130])
    z = qc.make_input("zero", 62101, 300, 130)
    q, r = _oracle(z, False)
    assert not r[:, [3, 21, 129]].any() and qc.colbe(z, q, r) <= ORACLE_COLBE_EPS[1] * EPS
    n = qc.make_input("nan", 62102, 300, 130)
    assert np.isnan(_oracle(n, False)[1]).any()
