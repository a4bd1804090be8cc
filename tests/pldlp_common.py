"""Shared by the pivoted-LDL^T tests: the golden manifest of tests/golden/pldlp (tools/gen_golden_pldlp.js) and a plain numpy
float64 statement of the algorithm, written from Bunch-Kaufman partial pivoting as LAPACK's DSYTF2 does it on the lower
triangle, in the operation order the device contract fixes (include/nd4hip.h, csrc/pldlp.hip):

  * alpha = (sqrt(17) + 1) / 8;
  * both searches keep the FIRST maximum, and once a NaN has been met every later element replaces, so with a NaN anywhere the
    last element of the scan is taken;
  * a step before the last whose max(A_rk, A_kk) is not > 0 (NaN included) is an error; the last step is not checked;
  * A_kk < alpha A_rk, then A_kk < (alpha A_rk) (A_rk / A_sr), then A_rr < alpha A_sr;
  * a 2x2 step complements P[r] before rows / columns k+1 and r are interchanged;
  * 1x1: t_i = a_ik / d, a_ij -= t_i a_jk with a_jk unscaled, then a_ik = t_i;
  * 2x2: D10 = (1 / (D00 D11 - 1)) / tmp, a_ij -= (a_ik s0_j + a_i,k+1 s1_j) from the old columns, then the columns become s0, s1.

Every step is vectorised over the trailing triangle with elementwise numpy operations only, so each multiplication, addition and
division is rounded once. tests/test_pldlp_host.py holds this statement to every fixture bit for bit, which is what entitles the
GPU tests to use it where no full fixture exists."""
import hashlib
import json
import math
import os

import numpy as np

from conftest import GOLDEN

DIR = os.path.join(GOLDEN, "pldlp")
EPS = 2.0 ** -52
SIZE_LIMIT = 1 << 20
GATE = 1e-10                                   # the project's parity gate
ALPHA = (math.sqrt(17.0) + 1.0) / 8.0
SINGULAR = "_pldlp_decomp(M,N, LD,LD_off, P,P_off): Zero column or NaN encountered."

with open(os.path.join(DIR, "manifest.json")) as _f:
    _M = json.load(_f)
CASES = _M["cases"]                            # decompositions
SOLVES = _M["solves"]                          # solves, each on the LD, P of one decomposition case
ALL = sorted(CASES)
SINGLE = [k for k in ALL if not CASES[k]["lead"]]
BATCHES = [k for k in ALL if CASES[k]["lead"]]


def load(entry, key):
    return np.load(os.path.join(DIR, entry["files"][key]))


def sha256(entry, key):
    with open(os.path.join(DIR, entry["files"][key]), "rb") as f:
        return hashlib.sha256(f.read()).hexdigest()


def same_bits(a, b):
    """equal in every bit, where NaN equals any NaN"""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    if a.shape != b.shape:
        return False
    return bool(np.all((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))))


def symmetric(seed, *shape):
    """the lower triangle of the repo's seeded generator, mirrored (twin of `symmetric` in tools/gen_golden_pldlp.js)"""
    from nd4js_amd import rng
    G = rng.matrix(seed, *shape)
    L = np.tril(G)
    return L + np.swapaxes(np.tril(G, -1), -1, -2)


def input_matrix(name):
    """S [lead..., N, N] of a decomposition case: from its file, or regenerated from the seed"""
    c = CASES[name]
    N, inp = c["N"], c["input"]
    if inp["kind"] == "file":
        return load(c, "S")
    S = symmetric(inp["seed"], N, N)
    if inp["kind"] == "zero_diag":
        S[np.arange(N), np.arange(N)] = 0.0
    elif inp["kind"] == "kkt":
        S[inp["m"]:, inp["m"]:] = 0.0
    else:
        assert inp["kind"] == "dense", inp
    return np.ascontiguousarray(S)


def rhs(entry):
    """y [lead..., N, J] of a solve case, from its seed"""
    from nd4js_amd import rng
    return rng.matrix(entry["y_seed"], *entry["y_shape"])


# ------------------------------------------------------------------------------------------------ the factorisation
class Singular(ValueError):
    pass


def _argmax_seq(x):
    """(index, value) that `best = -inf; for x_i: if not (best >= x_i): best, idx = x_i, i` ends with, for x >= 0 or NaN"""
    if np.isnan(x).any():
        return len(x) - 1, x[-1]
    i = int(np.argmax(x))                        # the first maximum
    return i, x[i]


def _swap(LD, P, k, l):
    """rows / columns k < l of the symmetric matrix whose lower triangle LD holds"""
    P[[k, l]] = P[[l, k]]
    LD[[k, l], :k] = LD[[l, k], :k]
    t = LD[k + 1:l, k].copy()
    LD[k + 1:l, k] = LD[l, k + 1:l]
    LD[l, k + 1:l] = t
    LD[k, k], LD[l, l] = LD[l, l], LD[k, k]
    LD[l + 1:, [k, l]] = LD[l + 1:, [l, k]]


def decomp_ref(S):
    """(LD, P) of one matrix S [N, N] (lower triangle read); Singular with the reference's text for a zero column or NaN"""
    S = np.asarray(S, dtype=np.float64)
    N = S.shape[0]
    LD = np.tril(S).copy()
    LD[np.triu_indices(N, 1)] = 0.0
    P = np.arange(N, dtype=np.int32)
    alpha = np.float64(ALPHA)
    k = 0
    with np.errstate(all="ignore"):
        while k < N:
            two = False
            if k < N - 1:
                q, A_rk = _argmax_seq(np.abs(LD[k + 1:, k]))
                r = k + 1 + q
                A_kk = np.abs(LD[k, k])
                if np.isnan(A_rk) or np.isnan(A_kk) or not (A_rk > 0 or A_kk > 0):
                    raise Singular(SINGULAR)
                if A_kk < alpha * A_rk:
                    _, A_sr = _argmax_seq(np.abs(np.concatenate([LD[r, k:r], LD[r + 1:, r]])))
                    if A_kk < (alpha * A_rk) * (A_rk / A_sr):
                        A_rr = np.abs(LD[r, r])
                        if A_rr < alpha * A_sr:
                            two = True
                            P[r] ^= -1
                            k += 1
                        if k != r:
                            _swap(LD, P, k, r)
            n0 = k + 1                                        # the trailing matrix starts here
            T = LD[n0:, n0:]
            low = np.tril(np.ones(T.shape, dtype=bool))
            if not two:
                d = LD[k, k]
                c = LD[n0:, k].copy()
                t = c / d
                upd = t[:, None] * c[None, :]
                T[low] = T[low] - upd[low]
                LD[n0:, k] = t
            else:
                tmp = LD[k, k - 1]
                D00 = LD[k, k] / tmp
                D11 = LD[k - 1, k - 1] / tmp
                D10 = (np.float64(1.0) / (D00 * D11 - np.float64(1.0))) / tmp
                c0, c1 = LD[n0:, k - 1].copy(), LD[n0:, k].copy()
                s0 = D10 * (D00 * c0 - c1)
                s1 = D10 * (D11 * c1 - c0)
                upd = c0[:, None] * s0[None, :] + c1[:, None] * s1[None, :]
                T[low] = T[low] - upd[low]
                LD[n0:, k - 1] = s0
                LD[n0:, k] = s1
            k += 1
    return LD, P


_REF = {}


def reference(name):
    """the restatement's per-member results of a decomposition case, computed once: a list of (LD, P) or Singular"""
    if name not in _REF:
        N = CASES[name]["N"]
        out = []
        for s in input_matrix(name).reshape(-1, N, N):
            try:
                out.append(decomp_ref(s))
            except Singular as e:
                out.append(e)
        _REF[name] = out
    return _REF[name]


# ------------------------------------------------------------------------------------------------ the solve
def solve_ref(LD, P, y):
    """x [N, J] with S x = y [N, J] in the reference's operation order (permute, forward substitution that skips the entry inside
    a 2x2 block, block scaling, transposed backward substitution, scatter)"""
    LD, y = np.asarray(LD, dtype=np.float64), np.asarray(y, dtype=np.float64)
    N = LD.shape[0]
    I = np.where(P < 0, ~P, P)
    neg = P < 0
    with np.errstate(all="ignore"):
        t = y[I].copy()
        for i in range(1, N):
            for k in range(i - int(neg[i])):
                t[i] = t[i] - LD[i, k] * t[k]
        i = 0
        while i < N:
            if i < N - 1 and neg[i + 1]:
                s = LD[i + 1, i]
                D00, D11 = LD[i + 1, i + 1] / s, LD[i, i] / s
                D10 = (np.float64(1.0) / (D00 * D11 - np.float64(1.0))) / s
                y0, y1 = t[i].copy(), t[i + 1].copy()
                t[i] = D10 * (D00 * y0 - y1)
                t[i + 1] = D10 * (D11 * y1 - y0)
                i += 2
            else:
                t[i] = t[i] / LD[i, i]
                i += 1
        for k in range(N - 1, 0, -1):
            for i in range(k - int(neg[k]) - 1, -1, -1):
                t[i] = t[i] - LD[k, i] * t[k]
        x = np.empty_like(t)
        x[I] = t
    return x


def backward_error(S, x, y):
    """||S x - y||_F / (||S||_F ||x||_F + ||y||_F) of one system"""
    with np.errstate(all="ignore"):
        return float(np.linalg.norm(S @ x - y) / (np.linalg.norm(S) * np.linalg.norm(x) + np.linalg.norm(y)))


def backward_bound(ref_value, N):
    """the larger of N eps and four times the reference's own value on that input"""
    return max(N * EPS, 4.0 * ref_value)
