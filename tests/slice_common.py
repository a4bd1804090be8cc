"""Shared by the slice tests: the golden manifest of tests/golden/slice (tools/gen_golden_slice.js), the planners of nd4js_amd.la
evaluated on the host with numpy's as_strided over an integer view, and a restatement of the bounds rule of nd4hip_gather_nd_dev.

Everything here moves words and never computes, so every comparison is made on unsigned integer views: float64 as uint64,
int32 as uint32, complex128 as pairs of uint64. There is no tolerance anywhere."""
import hashlib
import json
import os

import numpy as np
from numpy.lib.stride_tricks import as_strided

from conftest import GOLDEN
from nd4js_amd import la

DIR = os.path.join(GOLDEN, "slice")
SIZE_LIMIT = 100 * 1000
FNS = ["sliceElems", "transpose", "reshape", "concat", "stack"]

with open(os.path.join(DIR, "manifest.json")) as _f:
    _M = json.load(_f)
INPUTS = _M["inputs"]
CASES = _M["cases"]
ERRORS = _M["errors"]
ALL = sorted(CASES)

_cache = {}


def load(entry):
    """a fixture file, read once and never written"""
    a = _cache.get(entry["file"])
    if a is None:
        a = np.load(os.path.join(DIR, entry["file"]))
        a.setflags(write=False)
        _cache[entry["file"]] = a
    return a


def sha256(entry):
    with open(os.path.join(DIR, entry["file"]), "rb") as f:
        return hashlib.sha256(f.read()).hexdigest()


def words(a):
    """the words the device moves: uint64 for float64, uint32 for int32, [..., 2] uint64 for complex128"""
    a = np.asarray(a, order="C")                             # (ascontiguousarray would turn a 0-d result into [1])
    if a.dtype == np.complex128:
        return a.reshape(a.shape + (1,)).view(np.uint64)
    return a.view({8: np.uint64, 4: np.uint32}[a.dtype.itemsize])


def same_words(a, b):
    a, b = words(a), words(b)
    return a.shape == b.shape and a.dtype == b.dtype and bool(np.array_equal(a, b))


def py_slices(slices):
    """a recorded slice list as the planners take it (JSON null is None already)"""
    return [tuple(s) if isinstance(s, list) else s for s in slices]


def inputs_of(c):
    return [load(INPUTS[n]) for n in (c["arrays"] if "arrays" in c else [c["A"]])]


# ------------------------------------------------------------------------------------------------ plans evaluated with numpy
def view(flat, shape, off, strides):
    """flat[off + sum i_d strides[d]] for the box `shape`, as a copy; flat is 1-d, or [n, 2] for complex pairs"""
    lo, hi = la._box_reach(shape, strides, off)
    assert 0 <= lo and hi < flat.shape[0], "the plan leaves the operand"
    item = flat.strides[0]
    tail_shape, tail_strides = tuple(flat.shape[1:]), tuple(flat.strides[1:])
    v = as_strided(flat[off:], shape=tuple(shape) + tail_shape, strides=tuple(s * item for s in strides) + tail_strides, writeable=False)
    return np.array(v)


def flat_words(a):
    w = words(a)
    return w.reshape((-1, 2)) if a.dtype == np.complex128 else w.reshape(-1)


def scatter(out_flat, off, strides, shape, piece):
    """out_flat[off + sum i_d strides[d]] = piece[i], the dst side of a plan"""
    idx = np.full(tuple(shape), off, dtype=np.int64)
    for d, (n, s) in enumerate(zip(shape, strides)):
        idx = idx + (np.arange(n, dtype=np.int64) * s).reshape([-1 if k == d else 1 for k in range(len(shape))])
    out_flat[idx.reshape(-1)] = piece.reshape((-1,) + piece.shape[len(shape):])


def planned(c):
    """the result of one recorded call from the planners of la.py alone, as words"""
    ins = inputs_of(c)
    fn = c["fn"]
    if fn == "sliceElems":
        shape, off, strides = la._slice_plan(ins[0].shape, py_slices(c["slices"]))
        return view(flat_words(ins[0]), shape, off, strides)
    if fn == "transpose":
        shape, strides = la._transpose_plan(ins[0].shape, c["axes"])
        return view(flat_words(ins[0]), shape, 0, strides)
    if fn == "reshape":
        shape = la._reshape_shape(ins[0].shape, ins[0].size, c["shape"])
        w = flat_words(ins[0])
        return w.reshape(tuple(shape) + w.shape[1:])
    shapes = [list(a.shape) for a in ins]
    if fn == "concat":
        out_shape, strides, offs = la._concat_plan(c["axis"], shapes)
    else:
        ax, out_shape, strides, offs = la._stack_plan(c["axis"], shapes)
        shapes = [s[:ax] + [1] + s[ax:] for s in shapes]
    w0 = flat_words(ins[0])
    out = np.zeros((int(np.prod(out_shape, dtype=np.int64)),) + w0.shape[1:], dtype=w0.dtype)
    for a, sh, off in zip(ins, shapes, offs):
        w = flat_words(a)
        scatter(out, off, strides, sh, w.reshape(tuple(sh) + w.shape[1:]))
    return out.reshape(tuple(out_shape) + w0.shape[1:])


def refused_call(e):
    """(planner, arguments) of a refused call recorded in the manifest"""
    fn = e["fn"]
    if fn == "sliceElems":
        return la._slice_plan, (e["a_shape"], py_slices(e["slices"]))
    if fn == "transpose":
        return la._transpose_plan, (e["a_shape"], e["axes"])
    if fn == "reshape":
        n = int(np.prod(e["a_shape"], dtype=np.int64))
        return la._reshape_shape, (e["a_shape"], n, e["shape"])
    return {"concat": la._concat_plan, "stack": la._stack_plan}[fn], (e["axis"], e["shapes"])


# ------------------------------------------------------------------------------------------------ the bounds rule of the C ABI
GATHER_MAX_ND = 8


def abi_refuses(elem_bytes, shape, src_ptr, src_len, src_off, src_strides, dst_ptr, dst_len, dst_off, dst_strides):
    """include/nd4hip.h on nd4hip_gather_nd_dev: the reason the entry point returns ND4HIP_ERR_ARG, or None"""
    if len(shape) > GATHER_MAX_ND:
        return "ndim"
    if any(n < 1 for n in shape):
        return "extent"
    slo, shi = la._box_reach(shape, src_strides, src_off)
    dlo, dhi = la._box_reach(shape, dst_strides, dst_off)
    if slo < 0 or shi >= src_len:
        return "src"
    if dlo < 0 or dhi >= dst_len:
        return "dst"
    s0, s1 = src_ptr + slo * elem_bytes, src_ptr + (shi + 1) * elem_bytes
    d0, d1 = dst_ptr + dlo * elem_bytes, dst_ptr + (dhi + 1) * elem_bytes
    if s0 < d1 and d0 < s1:
        return "overlap"
    return None


# ------------------------------------------------------------------------------------------------ inputs for shapes without fixture
SPECIAL_BITS = np.array([0x7ff8dead0000beef, 0xfff0000000000000, 0x7ff0000000000000, 0x8000000000000000, 0x0000000000000001,
                         0x800123456789abcd, 0x7ff4000000000001], dtype=np.uint64)      # NaN payloads, infinities, -0, denormals, a signalling NaN


def special(seed, *shape, dtype=np.float64):
    """distinct values, so that a misplaced element cannot pass, with the hard bit patterns planted"""
    rng = np.random.default_rng(seed)
    if dtype == np.int32:
        n = int(np.prod(shape, dtype=np.int64))
        a = rng.permutation(np.arange(-(n // 2), n - n // 2, dtype=np.int64) * 7919 % (2 ** 31 - 1)).astype(np.int32).reshape(shape)
        if n >= 4:
            a.reshape(-1)[rng.choice(n, 2, replace=False)] = [-2 ** 31, 2 ** 31 - 1]
        return a
    full = tuple(shape) + ((2,) if dtype == np.complex128 else ())
    a = rng.uniform(-1.0, 1.0, size=full)
    flat = a.reshape(-1).view(np.uint64)
    if flat.size >= 16:
        pos = rng.choice(flat.size, size=min(flat.size // 2, 3 * SPECIAL_BITS.size), replace=False)
        flat[pos] = np.resize(SPECIAL_BITS, pos.size)
    return a.view(np.complex128).reshape(shape) if dtype == np.complex128 else a
