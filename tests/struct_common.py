"""Shared by the structure-function tests: the golden manifest of tests/golden/struct (tools/gen_golden_struct.js) and a plain
numpy statement of the nine functions (include/nd4hip.h, csrc/struct.hip):

  * transpose swaps the last two axes;
  * tril keeps x where i >= j - k, triu where i <= j - k, every other element is +0.0;
  * diag takes A[i + max(0, -offset), i + max(0, offset)] for i < L = min(M, M + offset, N, N - offset);
  * diag_mat writes d on the diagonal of a matrix of +0.0;
  * permute_* / unpermute_* broadcast the leading axes of A and of P against each other (the result has max(A.ndim, P.ndim + 1)
    axes); permute gathers through P; unpermute starts from +0.0 and stores row / column i at P[i] in ascending i, so a later i
    overwrites an earlier one and what no i names stays zero.

Values are only moved (through uint64 views), so every bit of a copied element survives. tests/test_struct_host.py holds this
statement to every fixture bit for bit, which is what entitles the GPU tests to use it on shapes that have no fixture."""
import hashlib
import json
import os

import numpy as np

from conftest import GOLDEN

DIR = os.path.join(GOLDEN, "struct")
SIZE_LIMIT = 1 << 20
GATE = 1e-10                                   # the project's parity gate
PERM = ["permute_rows", "permute_cols", "unpermute_rows", "unpermute_cols"]
NAMES = ["transpose", "tril", "triu", "diag", "diag_mat"] + PERM

with open(os.path.join(DIR, "manifest.json")) as _f:
    _M = json.load(_f)
INPUTS = _M["inputs"]
CASES = _M["cases"]
ERRORS = _M["errors"]
ALL = sorted(CASES)


def _path(entry):
    return os.path.join(DIR, entry["file"])


def load(entry):
    return np.load(_path(entry))


def sha256(entry):
    with open(_path(entry), "rb") as f:
        return hashlib.sha256(f.read()).hexdigest()


def case(name):
    """(fn, positional arguments as numpy arrays / ints, expected result) of one fixture"""
    c = CASES[name]
    a = c["args"]
    args = [load(INPUTS[a["A"]])]
    if "P" in a:
        args.append(load(INPUTS[a["P"]]))
    for key in ("k", "offset"):
        if key in a:
            args.append(int(a[key]))
    return c["fn"], args, load(c["out"])


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(a, b):
    """equal in every bit, where NaN equals any NaN"""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    if a.shape != b.shape:
        return False
    return bool(np.all((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))))


def exact_bits(a, b):
    """equal in every bit, NaN payloads included"""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.array_equal(a.view(np.uint64), b.view(np.uint64)))


# ------------------------------------------------------------------------------------------------ inputs for shapes without fixture
SPECIAL_BITS = np.array([0x7ff8dead0000beef, 0xfff0000000000000, 0x7ff0000000000000, 0x8000000000000000, 0x0000000000000001,
                         0x800123456789abcd, 0x7ff4000000000001], dtype=np.uint64)      # quiet NaN with a payload, -Inf, +Inf, -0, denormals, a signalling NaN


def special(seed, *shape):
    """uniform values with NaN payloads, infinities, -0 and denormals planted; distinct values elsewhere, so that a misplaced
    element cannot pass"""
    rng = np.random.default_rng(seed)
    a = rng.uniform(-1.0, 1.0, size=shape)
    flat = a.reshape(-1).view(np.uint64)
    if flat.size:
        pos = rng.choice(flat.size, size=min(flat.size, 3 * SPECIAL_BITS.size), replace=False)
        flat[pos] = np.resize(SPECIAL_BITS, pos.size)
    return a


def index_vector(kind, seed, lead, L):
    rng = np.random.default_rng(seed)
    n = int(np.prod(lead, dtype=np.int64)) if lead else 1
    if kind == "identity":
        P = np.tile(np.arange(L), (n, 1))
    elif kind == "dup":
        P = rng.integers(0, L, size=(n, L))
    else:
        P = np.stack([rng.permutation(L) for _ in range(n)])
    return np.ascontiguousarray(P.reshape(tuple(lead) + (L,)), dtype=np.int32)


# ------------------------------------------------------------------------------------------------ the restatement
def _u(a):
    a = np.ascontiguousarray(a, dtype=np.float64)
    return a.view(np.uint64)


def transpose(A):
    A = np.asarray(A, dtype=np.float64)
    if A.ndim < 2:
        return A
    return np.ascontiguousarray(np.swapaxes(_u(A), -1, -2)).view(np.float64)


def _tri(A, k, upper):
    U = _u(A)
    M, N = U.shape[-2:]
    i, j = np.arange(M, dtype=object)[:, None], np.arange(N, dtype=object)[None, :]      # exact for any int64 k
    zero = np.array((i > j - k) if upper else (i < j - k), dtype=bool)
    return np.where(zero, np.uint64(0), U).view(np.float64)


def tril(A, k=0):
    return _tri(A, k, False)


def triu(A, k=0):
    return _tri(A, k, True)


def diag(A, offset=0):
    U = _u(A)
    M, N = U.shape[-2:]
    assert -M < offset < N
    L = min(M, M + offset, N, N - offset)
    i = np.arange(L)
    return np.ascontiguousarray(U[..., i + max(0, -offset), i + max(0, offset)]).view(np.float64)


def diag_mat(d):
    U = _u(d)
    N = U.shape[-1]
    D = np.zeros(U.shape + (N,), dtype=np.uint64)
    i = np.arange(N)
    D[..., i, i] = U
    return D.view(np.float64)


def _permute(A, P, cols, inverse):
    U, P = _u(A), np.asarray(P)
    assert P.dtype == np.int32 and U.ndim >= 2 and P.ndim >= 1
    M, N = U.shape[-2:]
    L = N if cols else M
    assert P.shape[-1] == L
    lead = np.broadcast_shapes(U.shape[:-2], P.shape[:-1])          # the result has max(A.ndim, P.ndim + 1) axes
    Ub = np.broadcast_to(U, lead + (M, N)).reshape(-1, M, N)
    Pb = np.broadcast_to(P, lead + (L,)).reshape(-1, L)
    B = np.zeros(Ub.shape, dtype=np.uint64)
    if ((Pb < 0) | (Pb >= L)).any():
        raise ValueError("P.contains invalid indices.")
    members = np.arange(Ub.shape[0])
    if not inverse:
        B = np.take_along_axis(Ub, Pb[:, None, :] if cols else Pb[:, :, None], axis=2 if cols else 1)
    else:
        for i in range(L):                                          # ascending i: the last writer wins
            if cols:
                B[members, :, Pb[:, i]] = Ub[:, :, i]
            else:
                B[members, Pb[:, i], :] = Ub[:, i, :]
    return B.reshape(lead + (M, N)).view(np.float64)


def permute_rows(A, P):
    return _permute(A, P, False, False)


def permute_cols(A, P):
    return _permute(A, P, True, False)


def unpermute_rows(A, P):
    return _permute(A, P, False, True)


def unpermute_cols(A, P):
    return _permute(A, P, True, True)


RESTATED = {"transpose": transpose, "tril": tril, "triu": triu, "diag": diag, "diag_mat": diag_mat, "permute_rows": permute_rows,
            "permute_cols": permute_cols, "unpermute_rows": unpermute_rows, "unpermute_cols": unpermute_cols}


def refused_call(e):
    """the arguments of a refused call recorded in the manifest, as la.* takes them"""
    A = np.zeros(e["a_shape"])
    if e["fn"] in PERM:
        P = np.zeros(e["p_shape"], dtype=e["p_dtype"])
        if "p_values" in e:
            P = np.array(e["p_values"], dtype=np.int32).reshape(e["p_shape"])
        elif e["p_dtype"] == "int32" and P.ndim:
            P = (np.arange(P.size, dtype=np.int32) % P.shape[-1]).reshape(P.shape)
        return (A, P)
    if e["fn"] == "diag":
        return (A, e["offset"])
    return (A,)
