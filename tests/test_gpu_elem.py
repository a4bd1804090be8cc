"""Elementwise arithmetic and ordered axis reductions on the device (csrc/elem.hip) through dev.* and the raw C ABI: every fixture
of tests/golden/elem against the reference's recorded result and, on shapes that have no fixture, against the numpy model of
tests/elem_common.py. Both are exact: uint64 views where the expected value is not a NaN, NaN-ness where it is. No tolerance.

Shapes are the smallest that reach each path of elem.hip. zip: the dense kernel with 16-byte accesses, with its 8-byte tail and
stepped down to 8-byte accesses by an odd offset; the rows kernel with whole short rows per work item and with pieces of long
rows; the elems kernel for small boxes, an innermost stride of 2, 8 axes that cannot be merged, and a loop of launches for 10.
reduce: the tile kernel with every number of outputs per workgroup over one and over several chunks, along rows and down columns;
one lane per output down columns; the split min / max with its second pass; the walk of a reduced multi-index."""
import ctypes

import numpy as np
import pytest
import torch

import elem_common as ec
from nd4js_amd import _lib, dev, la

pytestmark = pytest.mark.gpu
ERR_ARG = -1
SENTINEL = 0x7ff8a5a5a5a5a5a5


def to_dev(a):
    return torch.from_numpy(np.array(a, dtype=np.float64)).cuda()


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def check(got, want, what):
    got = host(got)
    assert got.shape == np.shape(want), (what, got.shape, np.shape(want))
    assert ec.same(got, want), what


# ------------------------------------------------------------------------------------------------ every fixture
@pytest.mark.parametrize("name", ec.ALL)
def test_fixture_on_the_device(name):
    c = ec.CASES[name]
    ins = ec.inputs_of(c)
    ts = [to_dev(a) for a in ins]
    before = [t.clone() for t in ts]
    if c["fn"] == "zip":
        got = dev.zip_elems(ts, c["op"])
    elif c["fn"] == "map":
        got = dev.map_elems(ts[0], c["op"])
    else:
        got = dev.reduce_elems(ts[0], ec.axes_of(c), c["op"])
    check(got, ec.load(c["out"]), name)
    assert all(t.data_ptr() != got.data_ptr() for t in ts), "a fresh tensor"
    for t, b in zip(ts, before):
        assert torch.equal(t.view(torch.int64), b.view(torch.int64)), "an input was modified"


# ------------------------------------------------------------------------------------------------ zip against the model
MAT = ec.special(11, 70, 130)
ROW = ec.special(12, 130)
COL = ec.special(13, 70, 1)
BIG_A = ec.special(14, 1024, 1030)
BIG_COL = ec.special(15, 1024, 1)
LONG = ec.special(16, 2, 4100)


@pytest.mark.parametrize("op", ec.BINARY)
def test_zip_broadcasts_of_every_operator(op):
    for a, b in ((ROW, MAT), (MAT, ROW), (np.float64(-0.0), MAT), (MAT, np.array(np.nan)), (COL, MAT), (MAT, COL), (COL, ROW),
                 (LONG, LONG[:1]), (LONG[:1], LONG)):          # (rows of 4100: pieces of 2048 per work item)
        check(dev.zip_elems([to_dev(a), to_dev(b)], op), ec.zip_model(op, a, b), (op, np.shape(a), np.shape(b)))


@pytest.mark.parametrize("op", ["add", "div", "min"])
def test_zip_1024_x_1030(op):
    check(dev.zip_elems([to_dev(BIG_A), to_dev(BIG_COL)], op), ec.zip_model(op, BIG_A, BIG_COL), op)
    check(dev.zip_elems([to_dev(BIG_A), to_dev(BIG_A[::-1].copy())], op), ec.zip_model(op, BIG_A, BIG_A[::-1]), op)


@pytest.mark.parametrize("op", ec.UNARY)
def test_map_of_every_shape(op):
    for a in (ROW, MAT, BIG_A[:3], np.float64(-0.0), np.array([np.nan])):
        check(dev.map_elems(to_dev(a), op), ec.zip_model(op, a), (op, np.shape(a)))
    got = dev.map_elems(to_dev(MAT))
    assert np.array_equal(host(got).view(np.uint64), MAT.view(np.uint64)), "a copy keeps every bit, NaN payloads too"


def raw_zip(op, shape, A, a_off, a_strides, B, b_off, b_strides, n_out=None):
    """nd4hip_dzip_nd_dev as it is, into a sentinel-filled C: (return code, C as uint64)"""
    h = dev._h(A)
    count = int(np.prod(shape, dtype=np.int64)) if n_out is None else n_out
    C = torch.full((count,), SENTINEL, dtype=torch.int64, device="cuda")
    arr = lambda v: (ctypes.c_int64 * max(len(v), 1))(*v)
    rc = h.lib.nd4hip_dzip_nd_dev(h.ptr, la.EW_OPS[op], len(shape), arr(shape), dev._p(A), A.numel(), a_off, arr(a_strides),
                                  dev._p(B) if B is not None else None, B.numel() if B is not None else 0, b_off,
                                  arr(b_strides) if B is not None else None, dev._p(C), count)
    torch.cuda.synchronize()
    return rc, C.cpu().numpy().view(np.uint64)


@pytest.mark.parametrize("op", ec.BINARY + ec.UNARY)
def test_raw_boxes_odd_offsets_and_an_inner_stride_of_two(op):
    a, b = ec.special(21, 9000), ec.special(22, 9000)
    A, B = to_dev(a), to_dev(b)
    unary = op in ec.UNARY
    # dense, each operand in turn one element off a 16-byte boundary: the kernel steps down to 8-byte accesses
    for n, ao, bo in ((4097, 1, 0), (4097, 0, 1), (4097, 1, 1), (4096, 0, 0), (4097, 2, 4)):
        rc, got = raw_zip(op, [n], A, ao, [1], None if unary else B, bo, [1])
        want = ec.zip_model(op, a[ao:ao + n], None if unary else b[bo:bo + n])
        assert rc == 0 and ec.same(got.view(np.float64), want), (op, n, ao, bo)
    # an innermost stride of 2 (and 3 on the other operand): one thread per element
    rc, got = raw_zip(op, [30, 100], A, 3, [200, 2], None if unary else B, 1, [0, 3])
    av = np.lib.stride_tricks.as_strided(a[3:], shape=(30, 100), strides=(1600, 16))
    bv = np.broadcast_to(b[1:1 + 300:3], (30, 100))
    assert rc == 0 and ec.same(got.view(np.float64).reshape(30, 100), ec.zip_model(op, av, None if unary else bv)), op
    # rows with an offset, a broadcast row and a broadcast column
    rc, got = raw_zip(op, [60, 130], A, 7, [0, 1], None if unary else B, 5, [1, 0])
    want = ec.zip_model(op, np.broadcast_to(a[7:137], (60, 130)), None if unary else np.broadcast_to(b[5:65, None], (60, 130)))
    assert rc == 0 and ec.same(got.view(np.float64).reshape(60, 130), want), op


# ------------------------------------------------------------------------------------------------ reduce against the model
def data_for(op, seed, *shape):
    return {"add": ec.finite, "mul": ec.near_one}.get(op, ec.special)(seed, *shape)


# (shape, axes): paths that no fixture reaches
REDUCE_PATHS = [((33000, 70), 1),             # rows, 64 outputs per workgroup, two chunks of 64
                ((16400, 300), 1),            # rows, 16 outputs per workgroup, two chunks of 256
                ((20, 2500), 1),              # rows, 8 outputs per workgroup, five chunks of 512; min / max: one workgroup per row
                ((2, 9000), 1),               # min / max: every row split in pieces, second pass over [2, S]
                ((2100, 1100), 1),            # min / max: enough rows, no split
                ((70, 40000), 0),             # columns through tiles of 64 outputs, two chunks of 64
                ((300, 20000), 0),            # columns through tiles of 16 outputs, two chunks of 256
                ((1100, 130), 0),             # the same with few outputs, five chunks
                ((40, 66000), 0),             # columns, one lane per output
                ((3, 17, 66000), 1),          # the same with an outer kept axis
                ((3, 5, 7, 4, 3, 2), [1, 3, 5])]   # K R K R K R: the walk of a reduced multi-index


@pytest.mark.parametrize("op", ec.REDUCERS)
@pytest.mark.parametrize("case", range(len(REDUCE_PATHS)))
def test_reduce_paths(op, case):
    shape, axes = REDUCE_PATHS[case]
    x = data_for(op, 100 + case, *shape)
    check(dev.reduce_elems(to_dev(x), axes, op), ec.fold_model(op, x, axes), (op, shape, axes))


MILLION = ec.special(31, 1000, 1000)
MILLION_CLEAN = ec.special(32, 1000, 1000, specials=False)


@pytest.mark.parametrize("op", ["min", "max"])
def test_min_max_of_a_million_through_the_tree(op):
    for x in (MILLION, MILLION_CLEAN):
        want = ec.fold_model(op, x, [0, 1], halves=True)
        check(dev.reduce_elems(to_dev(x), [0, 1], op), want, op)
        check(dev.reduce_elems(to_dev(x.reshape(4, 250000)), 1, op), ec.fold_model(op, x.reshape(4, 250000), 1, halves=True), op)
    assert np.isnan(ec.fold_model(op, MILLION, [0, 1], halves=True)) and np.isfinite(ec.fold_model(op, MILLION_CLEAN, [0, 1], halves=True))
    z = np.zeros((3, 5000))
    z[1, 4321] = -0.0
    z[2, :] = -0.0
    check(dev.reduce_elems(to_dev(z), 1, op), ec.fold_model(op, z, 1, halves=True), "zeros of both signs")


def test_a_row_of_negative_zeros_sums_to_negative_zero():
    x = ec.finite(41, 6, 300)
    x[2, :] = -0.0
    x[4, :] = 0.0
    x[5, :7] = -0.0
    got = host(dev.reduce_elems(to_dev(x), 1, "add"))
    assert got[2] == 0 and np.signbit(got[2]) and got[4] == 0 and not np.signbit(got[4])
    assert ec.same(got, ec.fold_model("add", x, 1))
    col = host(dev.reduce_elems(to_dev(np.full((300, 6), -0.0)), 0, "add"))
    assert (col == 0).all() and np.signbit(col).all()
    assert ec.same(host(dev.reduce_elems(to_dev([1e16, 1.0, -1e16, 1.0]), 0, "add")), np.float64(1.0))


def test_axes_forms_and_refusals_of_the_planner():
    x = ec.finite(42, 4, 5, 6)
    X = to_dev(x)
    for axes in (1, [1], [-2], [1, 1, -2], np.array([1], dtype=np.int32)):
        check(dev.reduce_elems(X, axes, "add"), ec.fold_model("add", x, 1), axes)
    check(dev.reduce_elems(X, [], "mul"), x, "no axes: a copy")
    check(dev.reduce_elems(X, [0, 1, 2], "add"), ec.fold_model("add", x, [0, 1, 2]), "0-d")
    with pytest.raises(ValueError, match="Reduction axis 3 out of bounds."):
        dev.reduce_elems(X, 3, "add")
    with pytest.raises(ValueError, match="Invalid dtype float64 for axes."):
        dev.reduce_elems(X, np.array([1.0]), "add")
    with pytest.raises(ValueError, match="Shapes are not broadcast-compatible."):
        dev.zip_elems([X, to_dev(np.zeros((4, 6)))], "add")
    for bad in (lambda: dev.reduce_elems(X, 1, "sub"), lambda: dev.reduce_elems(X, 1, "div"), lambda: dev.zip_elems([X, X], "neg"),
                lambda: dev.map_elems(X, "add"), lambda: dev.zip_elems([X], "add"), lambda: dev.zip_elems([X, X], "hypot")):
        with pytest.raises(ValueError):
            bad()
    for bad in (lambda: dev.zip_elems([X, X.cpu()], "add"), lambda: dev.map_elems(X.to(torch.float32), "neg"),
                lambda: dev.reduce_elems(X.transpose(0, 1), 1, "add")):
        with pytest.raises(TypeError):
            bad()


# ------------------------------------------------------------------------------------------------ refusals of the C ABI
def test_refusals_write_nothing_and_leave_the_handle_usable():
    a = ec.special(51, 48)
    A, B = to_dev(a), to_dev(ec.special(52, 48))
    h = dev._h(A)
    C = torch.full((24,), SENTINEL, dtype=torch.int64, device="cuda")
    arr = lambda v: (ctypes.c_int64 * max(len(v), 1))(*v)
    flags = lambda v: (ctypes.c_int32 * max(len(v), 1))(*v)
    ap, bp, cp = A.data_ptr(), B.data_ptr(), C.data_ptr()
    P = ctypes.c_void_p

    def z(op, shape, a, a_len, a_off, a_st, b, b_len, b_off, b_st, c, c_len):
        return h.lib.nd4hip_dzip_nd_dev(h.ptr, op, len(shape), arr(shape), P(a), a_len, a_off, arr(a_st), P(b) if b else None, b_len, b_off,
                                        arr(b_st), P(c), c_len)

    def r(op, shape, red, a, a_len, c, c_len):
        return h.lib.nd4hip_dreduce_nd_dev(h.ptr, op, len(shape), arr(shape), flags(red), P(a), a_len, P(c), c_len)
    ok = ([4, 6], ap, 48, 0, [6, 1], bp, 48, 0, [6, 1], cp, 24)
    assert z(6, *ok) == ERR_ARG and z(-1, *ok) == ERR_ARG and z(15, *ok) == ERR_ARG and z(18, *ok) == ERR_ARG     # unknown operators
    assert z(16, *ok) == ERR_ARG                                                       # B given with a unary operator
    assert z(0, [4, 6], ap, 48, 0, [6, 1], None, 0, 0, [6, 1], cp, 24) == ERR_ARG       # B missing with a binary one
    assert z(0, [1] * 9, ap, 48, 0, [0] * 9, bp, 48, 0, [0] * 9, cp, 1) == ERR_ARG      # ndim 9
    assert z(0, [4, 0], ap, 48, 0, [6, 1], bp, 48, 0, [6, 1], cp, 24) == ERR_ARG        # an extent below 1
    assert z(0, [4, 6], ap, 48, 0, [6, -1], bp, 48, 0, [6, 1], cp, 24) == ERR_ARG       # a negative stride
    assert z(0, [4, 6], ap, 48, 0, [6, 1], bp, 48, 5, [6, -1], cp, 24) == ERR_ARG
    assert z(0, [4, 6], ap, 48, 25, [6, 1], bp, 48, 0, [6, 1], cp, 24) == ERR_ARG       # A left by one element
    assert z(0, [4, 6], ap, 48, -1, [6, 1], bp, 48, 0, [6, 1], cp, 24) == ERR_ARG
    assert z(0, [4, 6], ap, 48, 0, [6, 1], bp, 23, 0, [6, 1], cp, 24) == ERR_ARG        # B left by one element
    assert z(0, [4, 6], ap, 48, 0, [6, 1], bp, 48, 0, [6, 1], cp, 23) == ERR_ARG        # c_len is not the count
    assert z(0, [4, 6], ap, 48, 0, [6, 1], bp, 48, 0, [6, 1], cp, 25) == ERR_ARG
    assert z(0, [4, 6], ap, 48, 0, [6, 1], bp, 48, 0, [6, 1], ap + 8 * 23, 24) == ERR_ARG      # C over the last element read of A
    assert z(0, [4, 6], ap, 48, 0, [0, 0], bp, 48, 24, [6, 1], bp + 8 * 1, 24) == ERR_ARG      # C over what is read of B
    assert z(17, [4, 6], ap, 48, 0, [6, 1], None, 0, 0, [6, 1], ap, 24) == ERR_ARG              # in place
    assert r(1, [4, 6], [0, 1], ap, 24, cp, 4) == ERR_ARG and r(3, [4, 6], [0, 1], ap, 24, cp, 4) == ERR_ARG      # sub, div
    assert r(16, [4, 6], [0, 1], ap, 24, cp, 4) == ERR_ARG and r(7, [4, 6], [0, 1], ap, 24, cp, 4) == ERR_ARG
    assert r(0, [1] * 9, [0] * 9, ap, 24, cp, 1) == ERR_ARG                             # ndim 9
    assert r(0, [4, 0], [0, 1], ap, 24, cp, 4) == ERR_ARG                               # an extent below 1
    assert r(0, [4, 6], [0, 1], ap, 23, cp, 4) == ERR_ARG                               # A shorter than the box
    assert r(0, [4, 6], [0, 1], ap, 24, cp, 6) == ERR_ARG and r(0, [4, 6], [0, 1], ap, 24, cp, 24) == ERR_ARG     # c_len
    assert r(0, [4, 6], [0, 1], ap, 24, ap + 8 * 23, 4) == ERR_ARG                      # C over A's last element
    assert r(0, [4, 6], [0, 0], ap, 24, ap, 24) == ERR_ARG                              # the copy in place
    assert b"nd4hip_dreduce_nd" in h.lib.nd4hip_last_error()
    torch.cuda.synchronize()
    assert (C == SENTINEL).all(), "a refused call wrote"
    assert z(0, [4, 6], ap, 48, 24, [6, 1], bp, 48, 0, [6, 1], cp, 24) == 0             # the next calls on the handle succeed
    torch.cuda.synchronize()
    assert ec.same(C.cpu().numpy().view(np.float64).reshape(4, 6), ec.zip_model("add", a[24:].reshape(4, 6), host(B)[:24].reshape(4, 6)))
    assert r(5, [4, 6], [0, 1], ap, 48, cp, 4) == 0
    torch.cuda.synchronize()
    assert ec.same(C.cpu().numpy().view(np.float64)[:4], ec.fold_model("max", a[:24].reshape(4, 6), 1))
    # C may sit right behind what is read, and an operand may be read beyond the part that another call wrote
    assert z(0, [4, 6], ap, 48, 0, [6, 1], ap, 48, 0, [6, 1], ap + 8 * 24, 24) == 0
    torch.cuda.synchronize()
    assert ec.same(host(A)[24:].reshape(4, 6), ec.zip_model("add", a[:24].reshape(4, 6), a[:24].reshape(4, 6)))


# ------------------------------------------------------------------------------------------------ profile records
def test_profile_names_and_bytes():
    A, r = to_dev(MAT), to_dev(ROW)
    h = dev._h(A)
    h.profile_enable(True)
    try:
        dev.zip_elems([A, r], "add")
        torch.cuda.synchronize()
        p = h.profile_last()[0]
        assert p["op"] == "zip_nd" and p["flops"] == 0 and p["bytes"] == 8 * (9100 + 9100 + 130), p
        dev.map_elems(A, "abs")
        torch.cuda.synchronize()
        p = h.profile_last()[0]
        assert p["op"] == "zip_nd" and p["bytes"] == 8 * (9100 + 9100), p
        dev.zip_elems([A, to_dev(2.0)], "mul")
        torch.cuda.synchronize()
        assert h.profile_last()[0]["bytes"] == 8 * (9100 + 9100 + 1)
        dev.reduce_elems(A, 1, "add")
        torch.cuda.synchronize()
        p = h.profile_last()[0]
        assert p["op"] == "reduce_nd" and p["flops"] == 0 and p["bytes"] == 8 * (9100 + 70), p
        dev.reduce_elems(A, [0, 1], "max")
        torch.cuda.synchronize()
        assert h.profile_last()[0]["bytes"] == 8 * (9100 + 1)
    finally:
        h.profile_enable(False)
