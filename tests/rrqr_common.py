"""Shared helpers of the column-pivoted QR tests: the golden fixtures of tests/golden/rrqr/ (tools/gen_golden_rrqr.js) and
their inputs, regenerated from the seed with the repo's generator and the families of tests/families.py."""
import json
import os

import numpy as np

from families import apply_family
from nd4js_amd.rng import fill_uniform

GOLDEN_RRQR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rrqr")
EPS = 2.0 ** -52


def manifest():
    with open(os.path.join(GOLDEN_RRQR, "manifest.json")) as f:
        return json.load(f)["cases"]


def load(meta, key):
    return np.load(os.path.join(GOLDEN_RRQR, meta["files"][key]))


def _special(fam, a):
    M, N = a.shape
    if fam == "identity":
        a[...] = np.eye(M, N)
    elif fam == "zero":
        a[...] = 0.0
    elif fam == "dupcols":
        a[:, 1::2] = a[:, 0:N - 1:2][:, :a[:, 1::2].shape[1]]
    else:
        apply_family(fam, a, 0)
    return a


def make(seed, shape, fam):
    """the generator's input(): nd4_uniform(seed, i) then the family on each batch member with seed + b"""
    shape = tuple(shape)
    a = fill_uniform(seed, int(np.prod(shape))).reshape((-1,) + shape[-2:])
    for b in range(a.shape[0]):
        if fam in ("identity", "zero", "dupcols"):
            _special(fam, a[b])
        else:
            apply_family(fam, a[b], seed + b)
    return a.reshape(shape)


def y_of(meta):
    N = meta["shape"][-2]
    return fill_uniform(meta["y_seed"], N * meta["J"]).reshape(N, meta["J"])


def separated_prefix(R, rank):
    """first step i where the winning trailing norm c_i = ||R[i:, i]|| is within 1e-10 (relative) of a later candidate
    c_k = ||R[i:, k]||, or at / below the rank threshold; K if neither happens (the rows >= i of the reference's R are the
    trailing matrix at step i up to an orthogonal transformation)"""
    M, N = R.shape
    K = min(M, N)
    T = 2 * EPS * max(M, N) * np.linalg.norm(np.triu(R))
    for i in range(K):
        c = np.linalg.norm(R[i:, i:], axis=0)
        if i >= rank or c[0] <= T:
            return i
        if c.size > 1 and (c[0] - c[1:].max()) / c[0] < 1e-10:
            return i
    return K
