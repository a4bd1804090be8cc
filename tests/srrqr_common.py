"""Shared helpers of the strong RRQR tests: the fixtures of tests/golden/srrqr/ (tools/gen_golden_srrqr.js) and their inputs,
regenerated with the repo's generator."""
import json
import os

import numpy as np

from nd4js_amd.rng import fill_uniform
from rrqr_common import make

GOLDEN_SRRQR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "srrqr")
EPS = 2.0 ** -52


def manifest():
    with open(os.path.join(GOLDEN_SRRQR, "manifest.json")) as f:
        return json.load(f)["cases"]


def load(meta, key):
    return np.load(os.path.join(GOLDEN_SRRQR, meta["files"][key]))


def lowrank(seed, M, N, r):
    """B [M, r] C [r, N], accumulated over k in the generator's order"""
    B = fill_uniform(seed, M * r).reshape(M, r)
    C = fill_uniform(seed + 1, r * N).reshape(r, N)
    a = np.zeros((M, N))
    for k in range(r):
        a += B[:, k:k + 1] * C[k:k + 1, :]
    return a


def kahan(n, theta):
    s, c = np.sin(theta), np.cos(theta)
    a = np.zeros((n, n))
    for i in range(n):
        a[i, i:] = s ** i * -c * (1 - 25 * EPS * i)
        a[i, i] = s ** i * 1 * (1 - 25 * EPS * i)
    return a


def input_of(meta):
    fam, shape = meta["family"], tuple(meta["shape"])
    if fam == "lowrank":
        return lowrank(meta["seed"], shape[0], shape[1], meta["lowrank"])
    if fam == "kahan":
        return kahan(shape[0], meta["theta"])
    if "seed" not in meta:
        return np.eye(*shape)
    return make(meta["seed"], shape, fam)


def y_of(meta):
    N = meta["shape"][-2]
    return fill_uniform(meta["y_seed"], N * meta["J"]).reshape(N, meta["J"])


def strong_F(R, r):
    """max over i < r <= j of hypot((A^-1 B)_ij, ||row i of A^-1|| ||column j of C||) for A = R[:r, :r], B = R[:r, r:],
    C = R[r:, r:] (Gu-Eisenstat's bound that srrqr keeps below dtol); -inf when there is no such pair"""
    M, N = R.shape
    if r == 0 or r >= N:
        return -np.inf
    Ai = np.linalg.inv(R[:r, :r])
    AB = Ai @ R[:r, r:]
    rn = np.linalg.norm(Ai, axis=1)
    cn = np.linalg.norm(R[r:, r:], axis=0) if r < M else np.zeros(N - r)
    return float(np.hypot(AB, rn[:, None] * cn[None, :]).max())


# ---- test_gpu_srrqr_paths.py ------------------------------------------------------------------------------------------------
def urvls_factors(seed, n, r):
    """synthetic U R V of order n and rank r for urv_lstsq: U, V orthogonal (numpy's QR of uniform matrices), R = [[T, 0],
    [0, 0]] with exact zeros outside the r x r triangle T = D + E (cond <= ~5, rrqr_common.ls_factors), Y [n, 3] uniform"""
    from nd4js_amd import rng
    from rrqr_common import ls_factors
    U, R, _, Y = ls_factors(seed, n, n, n, 3, r)
    R[r:] = 0.0
    R[:, r:] = 0.0
    V = np.linalg.qr(rng.matrix(seed + 5, n, n))[0]
    return U, R, V, Y


def urvls_ref(U, R, V, r, Y, dtype=np.longdouble):
    """urv_lstsq (urv.js:138-323): x = V[:r]^T T^-1 (U^T Y)[:r] with T = R[:r, :r], in `dtype`"""
    T = np.asarray(R)[:r, :r].astype(dtype)
    z = np.asarray(U)[:, :r].astype(dtype).T @ np.asarray(Y).astype(dtype)
    for i in range(r - 1, -1, -1):
        z[i] = (z[i] - T[i, i + 1:] @ z[i + 1:]) / T[i, i]
    return np.asarray(V)[:r].astype(dtype).T @ z
