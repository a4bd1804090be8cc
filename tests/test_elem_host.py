"""Elementwise arithmetic and axis reductions without a device: the fixtures of tests/golden/elem against their manifest, the numpy
model of tests/elem_common.py against EVERY fixture (bit for bit where the reference's value is not a NaN), the planners of
nd4js_amd.la against the recorded shapes and every recorded refusal, and the two entry points in the ctypes table."""
import os

import numpy as np
import pytest

import elem_common as ec
from nd4js_amd import _lib, la


# ------------------------------------------------------------------------------------------------ the fixtures themselves
def test_manifest_matches_the_files():
    entries = list(ec.INPUTS.values()) + [c["out"] for c in ec.CASES.values()]
    assert len({e["file"] for e in entries}) == len(entries)
    for e in entries:
        assert os.path.getsize(os.path.join(ec.DIR, e["file"])) <= ec.SIZE_LIMIT, e["file"]
        assert ec.sha256(e) == e["sha256"], e["file"]
        a = ec.load(e)
        assert list(a.shape) == e["shape"] and a.dtype == np.float64, e["file"]
    on_disk = {f for f in os.listdir(ec.DIR) if f.endswith(".npy")}
    assert on_disk == {e["file"] for e in entries}


def test_fixtures_cover_every_operator_and_the_hard_values():
    assert len(ec.CASES) >= 120
    assert {c["op"] for c in ec.CASES.values() if c["fn"] == "zip"} == set(ec.BINARY)
    assert {c["op"] for c in ec.CASES.values() if c["fn"] == "map"} == set(ec.UNARY) | {None}
    assert {c["op"] for c in ec.CASES.values() if c["fn"] == "reduce"} == set(ec.REDUCERS)
    a = ec.load(ec.INPUTS["Sa_64x65"])
    assert np.isnan(a).any() and np.isposinf(a).any() and np.isneginf(a).any()
    assert ((a == 0) & np.signbit(a)).any() and ((a == 0) & ~np.signbit(a)).any()
    tiny = (a != 0) & (np.abs(a) < 2.0 ** -1022)
    assert (tiny & (a > 0)).any() and (tiny & (a < 0)).any()
    mag = np.abs(a[np.isfinite(a) & ~tiny & (a != 0)])
    assert mag.min() < 2.0 ** -30 and mag.max() > 2.0 ** 30
    texts = {e["message"] for e in ec.ERRORS}
    for t in ("Shapes are not broadcast-compatible.", "Reduction axis 2 out of bounds.", "Reduction axis -1 out of bounds.",
              "Only 1D nd.Array allowed for axes.", "Invalid dtype float64 for axes."):
        assert t in texts, t


def test_sum_fixtures_tell_fold_orders_apart():
    """what the generator asserted when it wrote them: a reversed fold of the same data has other bits somewhere"""
    seen = 0
    for name in ec.ALL:
        c = ec.CASES[name]
        if c["fn"] != "reduce" or c["op"] not in ("add", "mul"):
            continue
        x = ec.inputs_of(c)[0]
        red = la._reduce_axes(x.ndim, ec.axes_of(c))
        if int(np.prod([x.shape[d] for d in red], dtype=np.int64)) < 3:
            continue
        flipped = np.flip(x, axis=tuple(sorted(red)))
        assert not ec.same(ec.fold_model(c["op"], flipped, ec.axes_of(c)), ec.load(c["out"])), name
        seen += 1
    assert seen >= 20


# ------------------------------------------------------------------------------------------------ the model against fixtures
@pytest.mark.parametrize("name", ec.ALL)
def test_model_reproduces_the_fixture(name):
    c = ec.CASES[name]
    want = ec.load(c["out"])
    got = ec.model_of(c)
    assert np.shape(got) == want.shape, (name, np.shape(got), want.shape)
    assert ec.same(got, want), name


def test_min_max_follow_the_engine_not_the_hardware():
    z, n = 0.0, float("nan")
    for a, b, lo, hi in [(z, -z, -z, z), (-z, z, -z, z), (1.0, n, n, n), (n, 1.0, n, n), (-np.inf, n, n, n), (2.0, 3.0, 2.0, 3.0)]:
        assert ec.same(ec.zip_model("min", a, b), np.float64(lo)) and ec.same(ec.zip_model("max", a, b), np.float64(hi)), (a, b)
    assert ec.same(ec.zip_model("neg", 0.0), np.float64(-0.0)) and ec.same(ec.zip_model("abs", -0.0), np.float64(0.0))
    assert ec.same(ec.fold_model("add", np.full((2, 5), -0.0), 1), np.full(2, -0.0))      # the first element is copied: -0 survives
    assert ec.same(ec.fold_model("add", [1e16, 1.0, -1e16, 1.0], 0), np.float64(1.0))     # ((1 + 1e16) - 1e16) + 1, in this order
    x = ec.special(5, 9, 33)
    for op in ("min", "max"):
        assert ec.same(ec.fold_model(op, x, 1, halves=True), ec.fold_model(op, x, 1)), op


# ------------------------------------------------------------------------------------------------ the planners
@pytest.mark.parametrize("name", ec.ALL)
def test_planner_gives_the_recorded_shape(name):
    c = ec.CASES[name]
    ins = ec.inputs_of(c)
    if c["fn"] == "reduce":
        out_shape, bshape, flags, loop = la._reduce_plan(ins[0].shape, ec.axes_of(c))
        assert len(bshape) <= la.EW_MAX_ND and all(n > 1 for n in bshape)
        assert all(f != g for f, g in zip(flags, flags[1:])), "kept and reduced axes alternate"
        assert int(np.prod(bshape, dtype=np.int64)) * len(loop) == ins[0].size
    else:
        out_shape, strides, (bshape, bstrides, loop) = la._zip_plan([a.shape for a in ins])
        assert len(bshape) <= la.EW_MAX_ND and int(np.prod(bshape, dtype=np.int64)) * len(loop) == int(np.prod(out_shape, dtype=np.int64))
        # the box, evaluated on the host, addresses what broadcasting addresses
        res = np.arange(int(np.prod(out_shape, dtype=np.int64))).reshape(out_shape)
        for k, a in enumerate(ins):
            want = np.broadcast_to(np.arange(a.size).reshape(a.shape), out_shape).reshape(-1)
            got = np.empty(res.size, dtype=np.int64)
            for offs in loop:
                idx = np.full(tuple(bshape), offs[k], dtype=np.int64)
                cdx = np.full(tuple(bshape), offs[-1], dtype=np.int64)
                cs = la._c_strides(bshape)
                for d, n in enumerate(bshape):
                    step = np.arange(n, dtype=np.int64).reshape([-1 if j == d else 1 for j in range(len(bshape))])
                    idx = idx + step * bstrides[k][d]
                    cdx = cdx + step * cs[d]
                got[cdx.reshape(-1)] = idx.reshape(-1)
            assert np.array_equal(got, want), (name, k)
    assert list(out_shape) == c["out"]["shape"], name


def test_the_table_of_the_planners():
    assert la._zip_plan([[70, 1], [1, 130]])[2] == ([70, 130], [[1, 0], [0, 1]], [(0, 0, 0)])
    assert la._zip_plan([[3, 5], [3, 5]])[2] == ([15], [[1], [1]], [(0, 0, 0)])
    assert la._zip_plan([[], [3, 5]])[2] == ([15], [[0], [1]], [(0, 0, 0)])
    assert la._zip_plan([[], []])[:2] == ([], [[], []])
    shape, _, (bshape, _, loop) = la._zip_plan([[2, 1] * 5, [1, 2] * 5])
    assert shape == [2] * 10 and bshape == [2] * 8 and len(loop) == 4 and loop[1] == (0, 16, 256)
    assert la._reduce_plan([2, 3, 4], [0, 2]) == ([3], [2, 3, 4], [1, 0, 1], [(0, 0)])
    assert la._reduce_plan([2, 3, 4], -1) == ([2, 3], [6, 4], [0, 1], [(0, 0)])
    assert la._reduce_plan([2, 3, 4], []) == ([2, 3, 4], [24], [0], [(0, 0)])
    assert la._reduce_plan([2, 3, 4], [1, -2, 1])[0] == [2, 4]
    assert la._reduce_plan([2, 3, 4], np.array([0, 1, 2], dtype=np.int32)) == ([], [24], [1], [(0, 0)])
    assert la._reduce_plan([2, 1, 1, 4], [1]) == ([2, 1, 4], [8], [0], [(0, 0)])
    out, bshape, flags, loop = la._reduce_plan([2] * 9, [1, 3, 5, 7])         # K R K R K R K R K: the outer kept axis is a loop
    assert out == [2] * 5 and bshape == [2] * 8 and flags == [1, 0] * 4 and loop == [(0, 0), (256, 16)]
    with pytest.raises(ValueError, match="alternating"):
        la._reduce_plan([2] * 9, [0, 2, 4, 6, 8])


@pytest.mark.parametrize("i", range(len(ec.ERRORS)))
def test_refusal_has_the_recorded_text(i):
    e = ec.ERRORS[i]
    plan, args = ec.refused_call(e)
    with pytest.raises(ValueError) as info:
        plan(*args)
    assert str(info.value) == e["message"], e


# ------------------------------------------------------------------------------------------------ the C ABI table
def test_the_two_entry_points_are_bound_without_host_pointer_twins():
    for n in ("nd4hip_dzip_nd_dev", "nd4hip_dreduce_nd_dev"):
        assert n in _lib.SIGNATURES and hasattr(_lib.load(), n), n
        assert n[:-4] not in _lib.SIGNATURES and not hasattr(_lib.load(), n[:-4]), n
    assert la.EW_OPS == {"add": 0, "sub": 1, "mul": 2, "div": 3, "min": 4, "max": 5, "neg": 16, "abs": 17}
