"""Shared by the elementwise tests: the golden manifest of tests/golden/elem (tools/gen_golden_elem.js) and a numpy model of what
csrc/elem.hip computes.

The operators are single IEEE operations on float64, which numpy performs with the same rounding, so the model is exact: every
comparison is of uint64 views where the expected value is not a NaN, and of NaN-ness where it is (which operand's payload
survives in a computed NaN is the host CPU's rule, not IEEE's). There is no tolerance anywhere.

  zip_model   op on broadcast operands; min and max are written out with the sign bit and NaN (Math.min / Math.max: a NaN operand
              gives NaN, -0 is below +0), not with numpy's own minimum / maximum
  fold_model  reduceElems: acc = x[first], then acc = op(x, acc) over the reduced index in row-major order of the reduced axes,
              vectorised over the outputs"""
import hashlib
import json
import os

import numpy as np

from conftest import GOLDEN
from nd4js_amd import la

DIR = os.path.join(GOLDEN, "elem")
SIZE_LIMIT = 100 * 1000
BINARY = ["add", "sub", "mul", "div", "min", "max"]
UNARY = ["neg", "abs"]
REDUCERS = ["add", "mul", "min", "max"]

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


def inputs_of(c):
    return [load(INPUTS[n]) for n in (c["arrays"] if "arrays" in c else [c["A"]])]


def same(got, want):
    """equal shapes; equal bits where `want` is not a NaN, a NaN where it is"""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape or got.dtype != np.float64 or want.dtype != np.float64:
        return False
    nan = np.isnan(want)
    g, w = np.asarray(got, order="C").view(np.uint64), np.asarray(want, order="C").view(np.uint64)
    return bool(np.array_equal(np.isnan(got), nan) and np.array_equal(g[~nan], w[~nan]))


# ------------------------------------------------------------------------------------------------ the model
def _js_min(a, b):
    a, b = np.broadcast_arrays(a, b)
    out = np.where(a < b, a, b)                              # a < b: a; b < a or equal: b
    tie = a == b
    out = np.where(tie & np.signbit(a), a, out)              # equal (the two zeros): the negative one if there is one
    out = np.where(np.isnan(b), b, out)
    return np.where(np.isnan(a), a, out)


def _js_max(a, b):
    a, b = np.broadcast_arrays(a, b)
    out = np.where(a > b, a, b)
    tie = a == b
    out = np.where(tie, np.where(np.signbit(a), b, a), out)  # equal (the two zeros): the positive one if there is one
    out = np.where(np.isnan(b), b, out)
    return np.where(np.isnan(a), a, out)


def zip_model(op, a, b=None):
    a = np.asarray(a, dtype=np.float64)
    if b is not None:
        b = np.asarray(b, dtype=np.float64)
    with np.errstate(all="ignore"):
        if op == "add":
            return a + b
        if op == "sub":
            return a - b
        if op == "mul":
            return a * b
        if op == "div":
            return a / b
        if op == "min":
            return _js_min(a, b)
        if op == "max":
            return _js_max(a, b)
        if op == "neg":
            return np.negative(a)                           # flips the sign bit, of zeros and NaNs too
        if op == "abs":
            return np.abs(a)
    raise KeyError(op)


def fold_model(op, x, axes, halves=False):
    """reduceElems(axes, 'float64', op) of x. halves=True (min and max only, for which the order is immaterial: a NaN anywhere gives
    NaN and -0 is below +0 whatever the order) folds halves against each other instead of element by element."""
    x = np.asarray(x, dtype=np.float64)
    red = sorted(la._reduce_axes(x.ndim, axes))
    keep = [d for d in range(x.ndim) if d not in red]
    out_shape = tuple(x.shape[d] for d in keep)
    if not red:
        return x.copy()
    rows = np.ascontiguousarray(x.transpose(keep + red)).reshape(int(np.prod(out_shape, dtype=np.int64)), -1)
    if halves:
        assert op in ("min", "max")
        while rows.shape[1] > 1:
            h = rows.shape[1] // 2
            rest = rows[:, 2 * h:]
            rows = np.concatenate([zip_model(op, rows[:, :h], rows[:, h:2 * h]), rest], axis=1)
        return rows[:, 0].reshape(out_shape)
    acc = rows[:, 0].copy()
    for j in range(1, rows.shape[1]):
        acc = zip_model(op, rows[:, j], acc)
    return acc.reshape(out_shape)


def model_of(c):
    """the model's result of one recorded case"""
    ins = inputs_of(c)
    if c["fn"] == "zip":
        return zip_model(c["op"], ins[0], ins[1])
    if c["fn"] == "map":
        return ins[0].copy() if c["op"] is None else zip_model(c["op"], ins[0])
    return fold_model(c["op"], ins[0], axes_of(c))


def axes_of(c):
    return np.array(c["axes"], dtype=np.int32) if c.get("axes_int32") else c["axes"]


def refused_call(e):
    """(planner, arguments) of a refused call recorded in the manifest"""
    if e["fn"] == "zip":
        return la._zip_plan, (e["shapes"],)
    if "axes_array" in e:
        a = e["axes_array"]
        return la._reduce_plan, (e["a_shape"], np.array(a["data"], dtype=a["dtype"]).reshape(a["shape"]))
    return la._reduce_plan, (e["a_shape"], e["axes"])


# ------------------------------------------------------------------------------------------------ inputs for shapes without fixture
SPECIAL_BITS = np.array([0x7ff8000000000000, 0xfff0000000000000, 0x7ff0000000000000, 0x8000000000000000, 0x0000000000000000,
                         0x0000000000000001, 0x800123456789abcd], dtype=np.uint64)      # NaN, the infinities, both zeros, denormals


def special(seed, *shape, specials=True):
    """values spread over 2^-40 .. 2^40, with the hard bit patterns planted"""
    rng = np.random.default_rng(seed)
    a = rng.uniform(-1.0, 1.0, size=shape) * np.exp2(rng.integers(-40, 41, size=shape))
    a = np.asarray(a, dtype=np.float64)
    flat = a.reshape(-1).view(np.uint64)
    if specials and flat.size >= 16:
        pos = rng.choice(flat.size, size=min(flat.size // 4, 3 * SPECIAL_BITS.size), replace=False)
        flat[pos] = np.resize(SPECIAL_BITS, pos.size)
    return a


def finite(seed, *shape):
    """comparable magnitudes with a few large ones: sums that round differently in different orders"""
    rng = np.random.default_rng(seed)
    a = rng.uniform(-1.0, 1.0, size=shape)
    big = rng.random(size=shape) < 0.1
    return np.where(big, a * np.exp2(rng.integers(-40, 41, size=shape)), a)


def near_one(seed, *shape):
    """magnitudes in [0.5, 1.5) with random signs: long products stay finite"""
    rng = np.random.default_rng(seed)
    return (1.0 + rng.uniform(-0.5, 0.5, size=shape)) * rng.choice([-1.0, 1.0], size=shape)
