"""Slices, axis permutations, reshape, concat and stack on the device (csrc/gather.hip) through dev.*: every fixture of
tests/golden/slice against the reference's recorded result, and, on shapes that have no fixture, against numpy's own indexing of
the same words. Nothing is computed, so every comparison is of unsigned integer views (uint64 / uint32) and exact.

Shapes are the smallest that reach each path of gather.hip: the rows kernel in 16-byte, 8-byte and 4-byte words, with whole
short rows per work item and with pieces of long rows; the tiles kernel with and without 16-byte accesses at the tile edges 63,
64, 65 and 129 and in 32 x 32 tiles of complex pairs; the elems kernel for small boxes, for 8 axes that cannot be merged, and in
a loop of launches for 10. Every dst handed to dev.strided_copy is filled with a sentinel first: no sentinel is left inside the
box and every word outside it still is one."""
import numpy as np
import pytest
import torch

import slice_common as sc
from nd4js_amd import _lib, dev, la

pytestmark = pytest.mark.gpu
ERR_ARG = -1
SENTINEL = {torch.float64: 0x7ff8a5a5a5a5a5a5, torch.int32: 0x5a5a5a5a}     # as int64 / int32 bit patterns


def to_dev(a):
    """a numpy array on the device; complex128 as float64 [..., 2]"""
    a = np.ascontiguousarray(a) if np.ndim(a) else np.asarray(a)
    if a.dtype == np.complex128:
        a = a.reshape(a.shape + (1,)).view(np.float64)
    return torch.from_numpy(np.array(a)).cuda()


def dev_words(t):
    """the words of a device tensor as slice_common.words gives them for the matching numpy array"""
    a = t.cpu().numpy()
    return np.asarray(a, order="C").view({8: np.uint64, 4: np.uint32}[a.dtype.itemsize])


def int_view(t):
    return t.view(torch.int64) if t.dtype == torch.float64 else t


def run(fn, ins):
    """fn(tensors, pairs) on device copies of `ins`, as words; the inputs are not modified"""
    ts = [to_dev(a) for a in ins]
    before = [t.clone() for t in ts]
    pairs = ins[0].dtype == np.complex128
    out = fn(ts, pairs)
    torch.cuda.synchronize()
    for t, b in zip(ts, before):
        assert torch.equal(int_view(t), int_view(b))
    return dev_words(out)


def call_of(c):
    fn = c["fn"]
    if fn == "sliceElems":
        return lambda ts, pairs: dev.slice_elems(ts[0], *sc.py_slices(c["slices"]), pairs=pairs)
    if fn == "transpose":
        return lambda ts, pairs: dev.transpose(ts[0], *c["axes"], pairs=pairs)
    if fn == "reshape":
        return lambda ts, pairs: dev.reshape(ts[0], *c["shape"], pairs=pairs)
    return lambda ts, pairs: getattr(dev, fn)(c["axis"], ts, pairs=pairs)


# ------------------------------------------------------------------------------------------------ every fixture
@pytest.mark.parametrize("name", sc.ALL)
def test_fixture_on_the_device(name):
    c = sc.CASES[name]
    ins = sc.inputs_of(c)
    if c["fn"] == "transpose" and not c["axes"] and ins[0].dtype == np.int32:
        with pytest.raises(TypeError):                       # transpose() without axes is today's call: float64 only
            dev.transpose(to_dev(ins[0]))
        return
    got = run(call_of(c), ins)
    want = sc.words(sc.load(c["out"]))
    assert got.shape == want.shape and got.dtype == want.dtype, (name, got.shape, want.shape)
    assert np.array_equal(got, want), name


# ------------------------------------------------------------------------------------------------ helpers for shapes without fixture
def np_index(slices):
    """numpy's index for a slice list of the reference"""
    out = []
    for s in slices:
        if s == "...":
            out.append(Ellipsis)
        elif s == "new":
            out.append(None)
        elif isinstance(s, (list, tuple)):
            out.append(slice(*s))
        else:
            out.append(s)
    return tuple(out)


def check_slice(A, *slices):
    """dev.slice_elems against numpy's indexing of the same words"""
    idx = np_index(slices)
    if A.dtype == np.complex128 and Ellipsis in idx:
        idx = idx + (slice(None),)                           # the axis of the pair
    want = sc.words(A)[idx]
    got = run(lambda ts, pairs: dev.slice_elems(ts[0], *slices, pairs=pairs), [A])
    assert got.shape == want.shape, (slices, got.shape, want.shape)
    assert np.array_equal(got, want), slices


def check_transpose(A, *axes):
    nd = A.ndim
    order = list(axes) + [i for i in range(nd) if i not in axes]
    w = sc.words(A)
    want = np.ascontiguousarray(w.transpose(order + list(range(nd, w.ndim))))
    got = run(lambda ts, pairs: dev.transpose(ts[0], *axes, pairs=pairs), [A])
    assert got.shape == want.shape, (axes, got.shape, want.shape)
    assert np.array_equal(got, want), axes


def raw_copy(dst_shape, dtype, dst_off, dst_strides, src, src_off, src_strides, shape):
    """dev.strided_copy into a sentinel-filled dst; checks the sentinel rule and returns the box as words"""
    tdtype = torch.int32 if dtype == np.int32 else torch.float64
    S = to_dev(src)
    n = int(np.prod(dst_shape, dtype=np.int64))
    D = torch.full((n,), SENTINEL[tdtype], dtype=torch.int64 if tdtype == torch.float64 else torch.int32, device="cuda").view(tdtype)
    dev.strided_copy(D, dst_off, dst_strides, S.reshape(-1), src_off, src_strides, shape)
    torch.cuda.synchronize()
    d = dev_words(D)
    sent = np.array(SENTINEL[tdtype]).astype(np.int64 if tdtype == torch.float64 else np.int32).view(d.dtype)
    inside = np.zeros(n, dtype=bool)
    idx = np.full(tuple(shape), dst_off, dtype=np.int64)
    for k, (m, s) in enumerate(zip(shape, dst_strides)):
        idx = idx + (np.arange(m, dtype=np.int64) * s).reshape([-1 if j == k else 1 for j in range(len(shape))])
    inside[idx.reshape(-1)] = True
    assert (d[~inside] == sent).all(), "a word outside the box was written"
    want = sc.view(sc.words(src).reshape(-1), shape, src_off, src_strides)
    assert not (want == sent).any()
    assert np.array_equal(d[idx], want), "the box"
    return d[idx]


# ------------------------------------------------------------------------------------------------ rows
ROWS = [((3, 60), (2, 130)),                   # even length, even offset: 16-byte words
        ((3, 60), (2, 129)),                   # odd length
        ((3, 60), (3, 129)),                   # even length, base only 8-byte aligned
        ("...", (5, 6)),                       # rows of one word
        ((None, None, 3),),                    # outer step, whole rows
        ((None, None, -1),)]                   # outer reversal


@pytest.mark.parametrize("dtype", [np.float64, np.int32])
@pytest.mark.parametrize("slices", ROWS)
def test_rows_every_width(dtype, slices):
    check_slice(sc.special(11, 67, 130, dtype=dtype), *slices)


@pytest.mark.parametrize("dtype", [np.float64, np.int32])
def test_rows_in_a_batch(dtype):
    check_slice(sc.special(12, 3, 2, 67, 130, dtype=dtype), "...", 1, (3, 60), (2, 130))


def test_rows_int32_odd_length_allows_4_bytes_only_and_even_length_8():
    A = sc.special(13, 67, 130, dtype=np.int32)
    check_slice(A, (3, 60), (1, 130))            # 129 words from an odd offset
    check_slice(A, (3, 60), (2, 128))            # 126 words: 8-byte words, not 16
    check_slice(A, (3, 60), (4, 128))            # 124 words from a 16-byte boundary, pitch 130: 8-byte words
    check_slice(sc.special(18, 67, 132, dtype=np.int32), (3, 60), (4, 132))      # 128 words, pitch 132, 16-byte base: 16-byte words


def test_rows_complex_pairs():
    Z = sc.special(14, 33, 37, dtype=np.complex128)
    check_slice(Z, (3, 30), (1, 36))
    check_slice(Z, "...", (5, 6))
    check_slice(Z, (None, None, -1))


def test_rows_longer_than_a_work_item_are_cut():
    A = sc.special(15, 3, 5000)
    check_slice(A, "...", (1, 4998))             # 4997 single words: pieces of 2048, 2048 and 901
    check_slice(A, "...", (2, 4998))             # 2498 16-byte words: 2048 and 450


def test_rows_through_strided_copy_with_the_sentinel():
    A = sc.special(16, 67, 130)
    raw_copy((57 * 128 + 7,), np.float64, 4, [128, 1], A, 3 * 130 + 2, [130, 1], [57, 128])
    raw_copy((57 * 127 + 7,), np.float64, 3, [127, 1], A, 3 * 130 + 2, [130, 1], [57, 127])
    I = sc.special(17, 67, 130, dtype=np.int32)
    raw_copy((57 * 127 + 7,), np.int32, 5, [127, 1], I, 3 * 130 + 3, [130, 1], [57, 127])
    # into a strided dst: a column block of a wider matrix (what concat along the last axis does)
    raw_copy((67 * 200,), np.float64, 64, [200, 1], A, 0, [130, 1], [67, 130])


# ------------------------------------------------------------------------------------------------ tiles
@pytest.mark.parametrize("shape", [(5, 65, 130), (3, 63, 64), (2, 129, 65)])
@pytest.mark.parametrize("axes", [(2, 0, 1), (1, 2, 0)])
def test_tiles_axis_permutations(shape, axes):
    check_transpose(sc.special(21, *shape), *axes)


@pytest.mark.parametrize("axes", [(2, 0, 1), (1, 2, 0), (1, 0)])
def test_tiles_int32_and_complex(axes):
    check_transpose(sc.special(22, 3, 65, 67, dtype=np.int32), *axes)
    check_transpose(sc.special(23, 3, 33, 34, dtype=np.complex128), *axes)


def test_rows_of_four_words_under_an_axis_permutation():
    check_transpose(sc.special(24, 65, 63, 4), 1, 0, 2)


def test_tiles_permutation_of_a_slice_with_an_odd_base_offset():
    A = sc.special(25, 4, 66, 132)
    shape, off, strides = la._slice_plan(A.shape, [(1, 4), (0, 66), (1, 131)])
    assert off % 2 == 1 and shape == [3, 66, 130] and strides == [66 * 132, 132, 1]
    # out[k, i, j] = A[1 + i, j, 1 + k]: the box in dst order (130, 3, 66)
    got = raw_copy((130 * 3 * 66,), np.float64, 0, la._c_strides([130, 3, 66]), A, off, [strides[2], strides[0], strides[1]], [130, 3, 66])
    assert np.array_equal(got, np.ascontiguousarray(sc.words(A)[1:4, :, 1:131].transpose(2, 0, 1)))
    # an even base, even extents and even strides: the 16-byte tile form
    raw_copy((128 * 3 * 66,), np.float64, 0, la._c_strides([128, 3, 66]), A, off + 1, [1, 66 * 132, 132], [128, 3, 66])


# ------------------------------------------------------------------------------------------------ elems and stepped inner axes
@pytest.mark.parametrize("dtype", [np.float64, np.int32, np.complex128])
@pytest.mark.parametrize("slices", [("...", (None, None, 2)), ("...", (None, None, -1)), ("...", (129, 0, -3)), ((None, None, -2), (None, None, -1))])
def test_stepped_and_reversed_inner_axis(dtype, slices):
    check_slice(sc.special(31, 67, 130, dtype=dtype), *slices)


def test_eight_axes_that_cannot_be_merged():
    A = sc.special(32, 2, 3, 2, 3, 2, 3, 2, 5)
    shape, off, strides = la._slice_plan(A.shape, [(None, None, 2)] * 8)
    assert len(la._reduce_box(shape, strides, la._c_strides(shape))[0]) == 4      # four of the results' axes have extent 1 and go
    check_slice(A, *[(None, None, 2)] * 8)
    B = sc.special(33, 3, 4, 3, 4, 3, 4, 3, 5)
    shape, off, strides = la._slice_plan(B.shape, [(None, None, 2)] * 8)
    ks, kss, kds, loop = la._reduce_box(shape, strides, la._c_strides(shape))
    assert len(ks) == 8 and len(loop) == 1
    check_slice(B, *[(None, None, 2)] * 8)


def test_ten_axes_take_a_loop_of_launches():
    A = sc.special(34, *([4] * 10), dtype=np.int32)
    shape, off, strides = la._slice_plan(A.shape, [(None, None, 2)] * 10)
    ks, kss, kds, loop = la._reduce_box(shape, strides, la._c_strides(shape))
    assert len(ks) == 8 and len(loop) == 4
    check_slice(A, *[(None, None, 2)] * 10)


@pytest.mark.parametrize("dtype", [np.float64, np.int32, np.complex128])
def test_zero_d_results_and_new_axes(dtype):
    A = sc.special(35, 4, 6, dtype=dtype)
    check_slice(A, 1, 2)
    check_slice(A, "new", 1, "new")
    check_slice(A, "...", "new")
    check_slice(A, -1)


# ------------------------------------------------------------------------------------------------ concat / stack
def check_list(fn, axis, arrays):
    ws = [sc.words(a) for a in arrays]
    nd = arrays[0].ndim
    ax = axis if axis >= 0 else axis + nd + (1 if fn == "stack" else 0)
    want = (np.concatenate if fn == "concat" else np.stack)(ws, axis=ax)
    got = run(lambda ts, pairs: getattr(dev, fn)(axis, ts, pairs=pairs), arrays)
    assert got.shape == want.shape, (fn, axis, got.shape, want.shape)
    assert np.array_equal(got, want), (fn, axis)


@pytest.mark.parametrize("dtype", [np.float64, np.int32, np.complex128])
def test_concat(dtype):
    mk = lambda k, *shape: sc.special(40 + k, *shape, dtype=dtype)
    check_list("concat", 0, [mk(0, 65, 130)])
    check_list("concat", 0, [mk(0, 65, 130), mk(1, 3, 130)])
    check_list("concat", 0, [mk(k, 1 + 7 * k, 33) for k in range(5)])
    check_list("concat", -1, [mk(0, 67, 3), mk(1, 67, 64), mk(2, 67, 1)])
    check_list("concat", 2, [mk(0, 2, 3, 4, 35), mk(1, 2, 3, 1, 35), mk(2, 2, 3, 30, 35)])


@pytest.mark.parametrize("dtype", [np.float64, np.int32, np.complex128])
def test_stack(dtype):
    mk = lambda k: sc.special(50 + k, 5, 33, 34, dtype=dtype)
    for axis in (0, 1, 3, -1):
        check_list("stack", axis, [mk(0), mk(1)])
    check_list("stack", 2, [mk(k) for k in range(5)])
    check_list("stack", 0, [mk(0)])


def test_lists_of_mixed_dtype_are_refused():
    with pytest.raises(TypeError):
        dev.concat(0, [to_dev(np.zeros((2, 2))), to_dev(np.zeros((2, 2), dtype=np.int32))])
    with pytest.raises(ValueError, match="Shape along all axes but the concatentation axis must match."):
        dev.concat(0, [to_dev(np.zeros((2, 2))), to_dev(np.zeros((2, 3)))])


# ------------------------------------------------------------------------------------------------ offsets beyond 2^31 bytes
def test_offsets_beyond_two_to_the_31_bytes():
    from nd4js_amd import rng
    N = 16400
    A = dev.fill_uniform(77, (N, N))
    assert A.numel() * 8 > 2 ** 31
    try:
        flat = np.arange(N, dtype=np.int64)[:, None] * N + np.arange(N, dtype=np.int64)[None, :]
        for slices, idx in ((((-3, None), (-5, None)), (slice(-3, None), slice(-5, None))),
                            (((None, None, 4100), (None, None, -4099)), (slice(None, None, 4100), slice(None, None, -4099)))):
            got = dev.slice_elems(A, *slices)
            torch.cuda.synchronize()
            at = flat[idx]
            want = np.array([rng.fill_uniform(77, 1, offset=int(i))[0] for i in at.reshape(-1)]).reshape(at.shape)
            assert np.array_equal(got.cpu().numpy().view(np.uint64), want.view(np.uint64)), slices
    finally:
        del A
        torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_write_nothing_and_leave_the_handle_usable():
    S = to_dev(sc.special(61, 48))
    sent = SENTINEL[torch.float64]
    D = torch.full((24,), sent, dtype=torch.int64, device="cuda").view(torch.float64)
    h = _lib.handle(S.device.index)
    arr = lambda v: (_lib.c_i64 * max(len(v), 1))(*v)
    import ctypes

    def rc(shape, src, src_len, src_off, ss, dst, dst_len, dst_off, ds):
        return h.lib.nd4hip_gather_nd_dev(h.ptr, 8, len(shape), arr(shape), ctypes.c_void_p(src), src_len, src_off, arr(ss),
                                          ctypes.c_void_p(dst), dst_len, dst_off, arr(ds))
    sp, dp = S.data_ptr(), D.data_ptr()
    assert rc([4, 6], sp, 48, 25, [6, 1], dp, 24, 0, [6, 1]) == ERR_ARG            # leaves src by one element
    assert rc([4, 6], sp, 48, 0, [6, 1], dp, 24, 1, [6, 1]) == ERR_ARG             # leaves dst by one element
    assert rc([4, 6], sp, 48, 0, [6, 1], sp + 8 * 12, 24, 0, [6, 1]) == ERR_ARG    # dst inside src
    assert rc([1] * 9, sp, 48, 0, [0] * 9, dp, 24, 0, [0] * 9) == ERR_ARG          # ndim 9
    assert rc([4, 0], sp, 48, 0, [6, 1], dp, 24, 0, [6, 1]) == ERR_ARG             # an extent below 1
    for bad in ((D, 1, [6, 1], S, 0, [6, 1], [4, 6]), (D, 0, [6, 1], S, 25, [6, 1], [4, 6]), (D, 0, [0] * 9, S, 0, [0] * 9, [1] * 9)):
        with pytest.raises(ValueError):
            dev.strided_copy(*bad)
    with pytest.raises(ValueError):
        dev.strided_copy(S[12:36], 0, [6, 1], S, 0, [6, 1], [4, 6])
    torch.cuda.synchronize()
    assert (D.view(torch.int64) == sent).all(), "a refused call wrote"
    dev.strided_copy(D, 0, [6, 1], S, 24, [6, 1], [4, 6])                          # the next call on the handle succeeds
    torch.cuda.synchronize()
    assert torch.equal(D.view(torch.int64), S[24:].view(torch.int64))


# ------------------------------------------------------------------------------------------------ reshape
def test_reshape_is_a_view_and_runs_no_kernel():
    A = to_dev(sc.special(62, 4, 6))
    h = _lib.handle(A.device.index)
    h.profile_enable(True)
    try:
        B = dev.slice_elems(A, (1, 3))
        torch.cuda.synchronize()
        before = h.profile_last()
        assert before[0]["op"] == "gather_nd" and before[0]["bytes"] == 2 * 8 * 12
        R = dev.reshape(A, -1, 3)
        assert tuple(R.shape) == (8, 3) and R.data_ptr() == A.data_ptr()
        assert dev.reshape(A, 2, 3, 4).data_ptr() == A.data_ptr()
        Z = to_dev(sc.special(63, 4, 6, dtype=np.complex128))
        assert tuple(dev.reshape(Z, 3, -1, pairs=True).shape) == (3, 8, 2)
        assert h.profile_last() == before
    finally:
        h.profile_enable(False)
    with pytest.raises(ValueError, match="Shape cannot be inferred."):
        dev.reshape(A, 5, -1)
    assert tuple(B.shape) == (2, 6)
