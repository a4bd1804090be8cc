"""The catalogue of tests/svd_dc_common.py is what it claims, checked on the CPU: for every input that test_gpu_svd_dc_paths.py
sends to the device, the reference restatement (oracle.bidiag_svd_dc, stats=True) reports the path the case is named for, and
its own result stays inside the bounds the device is held to. Without this a case could stop reaching its path (another seed,
another split) and the device test would go on passing for the wrong reason.

The conditions are asserted, not the exact counts: the counts belong to the reference's arithmetic, the conditions to the
device code (which kernel, which branch, which workgroup)."""
import numpy as np
import pytest

import oracle
import svd_dc_common as C


def _merge(rec, off, n):
    hit = [r for r in rec if (r["off"], r["n"]) == (off, n)]
    assert len(hit) == 1
    return hit[0]


def _roots(r):
    return r["n"] - 1 - r["n1"]


def test_records_are_the_recursion():
    """one record per merge, children before their parent, with 0 <= n0 <= n1 <= m and no more upper shifts than roots"""
    for name in C.PATH_CASES:
        B, _, _, _, rec = C.path_reference(name)
        want = [(off, n) for off, n, leaf in C.recursion_nodes(B.shape[0] + 1) if not leaf]
        assert [(r["off"], r["n"]) for r in rec] == want
        for r in rec:
            assert 0 <= r["n0"] <= r["n1"] <= r["n"] - 1
            assert 0 <= r["shift_hi"] <= max(_roots(r) - 1, 0)
            assert 0 <= r["rot_chain"] <= max(r["n1"] - r["n0"] - 1, 0) and 0 <= r["rot_last"] <= r["n1"] - r["n0"]


def test_quad_16_rotates_at_a_gemm_level_and_fills_all_three_lists():
    rec = C.path_reference("quad_16")[4]
    for off in (0, 34):                                   # two merges of m = 33 in one level: gather, GEMM, scatter with nm = 2
        r = _merge(rec, off, 34)
        assert r["n1"] > r["n0"] and _roots(r) >= 2
    top = _merge(rec, 0, 68)
    assert top["n0"] >= 1 and top["n1"] - top["n0"] >= 2 and _roots(top) >= 2


def test_quad_16_weak_chains_rotations():
    """three or more equal values with z of order 1: rotations that share their partner, where the order matters"""
    rec = C.path_reference("quad_16_weak")[4]
    top = _merge(rec, 0, 68)
    assert top["rot_chain"] >= 2 and top["n0"] >= 1 and _roots(top) >= 2
    assert all(_merge(rec, off, 34)["n1"] > _merge(rec, off, 34)["n0"] for off in (0, 34))
    assert all(r["rot_chain"] == 0 for r in C.path_reference("quad_16")[4])      # ... which quad_16 does not do


@pytest.mark.parametrize("name,inner", [("quad_16_singular", (34, 34)), ("sing_69", (35, 35))])
def test_singular_cases_rotate_into_the_last_index(name, inner):
    B, _, _, _, rec = C.path_reference(name)
    assert B.shape[0] == B.shape[1]                       # J = K
    assert _merge(rec, *inner)["hh_zero"]
    top = rec[-1]
    assert top["n"] - 1 > 32 and top["hh_zero"] and top["rot_last"] >= 1 and top["n0"] >= 1 and _roots(top) >= 2


def test_twin_130_rotates_beyond_column_256():
    top = C.path_reference("twin_130")[4][-1]
    m = top["n"] - 1
    assert m > 256 and top["n1"] - top["n0"] >= 2 and top["n1"] < 256 < m        # columns c >= 256 hold roots: every rotation
    assert top["n0"] >= 1                                                        # changes them


def test_twin_34_zeros_deflate_by_z_at_every_gemm_level():
    rec = C.path_reference("twin_34_zeros")[4]
    for off, n in ((0, 35), (35, 35), (0, 70)):
        r = _merge(rec, off, n)
        assert r["n0"] >= 2 and _roots(r) >= 2
    rec2 = C.path_reference("twin_34_zeros_b2")[4]
    assert rec2[-1]["n0"] > rec[-1]["n0"] and _roots(rec2[-1]) >= 2              # b2 = 0: more of the right child deflates
    assert not rec2[-1]["hh_zero"]


def test_zero_middle_69_leaves_one_root():
    top = C.path_reference("zero_middle_69")[4][-1]
    m = top["n"] - 1
    assert m == 69 and top["hh_zero"] and top["n0"] == top["n1"] == m - 1


def test_rand_70_71_pads_the_smaller_merge():
    rec = C.path_reference("rand_70_71")[4]
    assert {(r["off"], r["n"]) for r in rec if r["n"] - 1 > 32} == {(0, 35), (35, 36), (0, 71)}
    assert rec[-1]["n0"] >= 1 and rec[-1]["n1"] == rec[-1]["n0"]


def test_graded_40_shifts_to_the_upper_pole():
    top = C.path_reference("graded_40")[4][-1]
    m = top["n"] - 1
    assert m == 40 and top["n0"] >= m // 4 and top["shift_hi"] >= 3 * (_roots(top) - 1) // 4


def test_max_2048_is_the_largest_size():
    top = C.path_reference("max_2048")[4][-1]
    assert top["n"] - 1 == 2048 and _roots(top) >= 2 and top["n0"] >= 1


def test_mixed_batches_differ_in_their_counts_at_a_gemm_level():
    for name, shape in (("mixed_67_68", (67, 67)), ("mixed_69_69", (69, 68))):
        tops, inner = set(), set()
        for d, e in C.mixed_members(name):
            assert (d.shape[0], e.shape[0]) == shape
            rec = oracle.bidiag_svd_dc(d, e, stats=True)[3]
            assert rec[-1]["n"] - 1 > 32 and rec[-2]["n"] - 1 > 32
            tops.add((rec[-1]["n0"], rec[-1]["n1"], rec[-1]["hh_zero"]))
            inner.add((rec[-2]["n0"], rec[-2]["n1"]))
        assert len(tops) == len(C.mixed_members(name)) and len(inner) >= 2
    assert any(hh for _, _, hh in tops)


@pytest.mark.parametrize("name", list(C.PATH_CASES))
def test_the_oracle_meets_the_bounds_of_the_device(name):
    d, e = C.PATH_CASES[name]
    B, u2, sv, v2, _ = C.path_reference(name)
    C.check_bidiag(d, e, u2, sv, v2, np.linalg.svd(B, compute_uv=False))
    got = oracle.bidiag_svd_dc(d, e)                      # the records change nothing
    assert all(x.tobytes() == y.tobytes() for x, y in zip(got, (u2, sv, v2)))


def test_the_oracle_meets_the_bounds_on_the_mixed_members():
    for name in ("mixed_67_68", "mixed_69_69"):
        for d, e in C.mixed_members(name):
            u2, sv, v2 = oracle.bidiag_svd_dc(d, e)
            C.check_bidiag(d, e, u2, sv, v2, np.linalg.svd(C.bidiag_dense(d, e), compute_uv=False))


@pytest.mark.parametrize("K,J", C.TINY_SHAPES)
def test_the_oracle_on_every_tiny_problem(K, J):
    """3^(K + J - 1) problems of one leaf each; among them every zero and sign branch of the closed forms"""
    D, E = C.tiny_problems(K, J)
    assert D.shape == (3 ** (K + J - 1), K) and E.shape == (3 ** (K + J - 1), J - 1)
    assert len({tuple(x) for x in np.hstack([D, E])}) == D.shape[0]
    for d, e in zip(D, E):
        u2, sv, v2, rec = oracle.bidiag_svd_dc(d, e, stats=True)
        assert rec == []
        C.check_bidiag(d, e, u2, sv, v2, np.linalg.svd(C.bidiag_dense(d, e), compute_uv=False))


def test_the_oracle_agrees_with_its_dense_entry():
    """(d, e) directly and the dense bidiagonal through oracle.svd_dc (bidiagonalisation in front) give the same values"""
    for name in ("rand_70_71", "sing_69", "quad_16_weak"):
        B, _, sv, _, _ = C.path_reference(name)
        C.check_values(sv, oracle.svd_dc(np.array(B))[1])


@pytest.mark.parametrize("name", list(C.PATH_DENSE_CASES))
def test_the_oracle_meets_the_bounds_on_the_dense_cases(name):
    a, u, sv, v = C.dense_reference(name)
    C.check_values(sv, np.linalg.svd(a, compute_uv=False))
    C.check_properties(a, u, sv, v)
    if name in C.RANKS:
        assert np.all(sv[C.RANKS[name]:] <= 1e-10 * sv[0])


def test_the_oracle_raises_line_429_for_the_four_error_inputs():
    for d, e in C.error_inputs():
        with pytest.raises(RuntimeError, match=r"svd_dc: 'Assertion failed\.' \(svd_dc\.js:429\)"):
            oracle.bidiag_svd_dc(d, e)
        with pytest.raises(RuntimeError, match=r"svd_dc: 'Assertion failed\.' \(svd_dc\.js:\d+\)"):
            oracle.svd_dc(C.bidiag_dense(d, e))


def test_wrapper_arguments():
    with pytest.raises(ValueError):
        oracle.bidiag_svd_dc(np.ones(4), np.ones(2))
    with pytest.raises(ValueError):
        oracle.bidiag_svd_dc(np.ones((2, 4)), np.ones((2, 4)))
