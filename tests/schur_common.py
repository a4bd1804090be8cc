"""Shared by the Schur tests: the golden manifest of tests/golden/schur and a restatement in Python of the reference's
schur_qrfrancis_inplace (schur.js:388-683) in its operation order: the Francis iteration with its nested calls (`recurse`), the
exceptional shift's draws from AleaRNG('nd.la.schur_qrfrancis_inplace') (alea_rng.js:37-90, :135-142), node 12's Math.hypot and
the pass that resolves real-eigenvalued 2x2 blocks. Every scalar decision is taken on Python floats; the plane rotations and the
products of `recurse` are element by element (numpy float64 slices, one multiply-multiply-add per element and sums in ascending
j), so the result has the reference's bits. The one deviation is the sweep budget of the device form (include/nd4hip.h): a call
at size n raises NoConvergence after 30 max(10, n) sweeps instead of the reference's 1e9 stuck iterations."""
import hashlib
import json
import math
import os

import numpy as np

from conftest import GOLDEN

DIR = os.path.join(GOLDEN, "schur")
EPS = 2.0 ** -52
SIZE_LIMIT = 1 << 20
GATE = 1e-10                                   # the project's gate on residuals

with open(os.path.join(DIR, "manifest.json")) as _f:
    CASES = json.load(_f)["cases"]
ALL = sorted(CASES)
SINGLE = [k for k in ALL if not CASES[k]["lead"]]
FINITE = [k for k in SINGLE if "ref_residual" in CASES[k]]
EIGEN = [k for k in SINGLE if "Lam" in CASES[k]["files"]]


def load(name, key):
    return np.load(os.path.join(DIR, CASES[name]["files"][key]))


def sha256(name, key):
    with open(os.path.join(DIR, CASES[name]["files"][key]), "rb") as f:
        return hashlib.sha256(f.read()).hexdigest()


def input_matrix(name):
    """A [lead..., N, N] of a case: from its file, or regenerated from the seed"""
    from nd4js_amd import rng
    c = CASES[name]
    N, lead, inp = c["N"], c["lead"], c["input"]
    if inp["kind"] == "file":
        return load(name, "A")
    A = rng.matrix(inp["seed"], *lead, N, N)
    if inp["kind"] == "hessenberg":
        A = np.triu(A, -1)
        for i in inp["zeros"]:
            A[..., i, i - 1] = 0.0
    return np.ascontiguousarray(A)


def hessenberg_pair(name):
    """(U, H): the reference's hessenberg_decomp of the case's input; (I, A) for a Hessenberg input"""
    c = CASES[name]
    if c["input"]["kind"] == "hessenberg":
        A = input_matrix(name)
        return np.broadcast_to(np.eye(c["N"]), A.shape).copy(), A
    return load(name, "U"), load(name, "H")


def same_bits(a, b):
    """equal in every bit, where NaN equals any NaN"""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    if a.shape != b.shape:
        return False
    return bool(np.all((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))))


def budget(n):
    """sweeps allowed to one francis_qr call at size n (LAPACK's dlahqr: 30 per eigenvalue, at least 300)"""
    return 30 * max(10, n)


class NoConvergence(Exception):
    pass


# ------------------------------------------------------------------------------------------------ alea_rng.js
def _u32(x):
    return float(int(x) % 4294967296)


def _mash(text, seed):
    for ch in text:
        seed += ord(ch)
        temp = 0.02519603282416938 * seed
        seed = _u32(temp)
        temp -= seed
        temp *= seed
        seed = _u32(temp)
        temp -= seed
        seed += temp * 4294967296.0
    return seed


def alea_seed(text="nd.la.schur_qrfrancis_inplace"):
    """(s0, s1, s2, c) of a fresh AleaRNG(text) (alea_rng.js:64-82)"""
    s0 = _mash(" ", float(0xefc8249d))
    s1 = _mash(" ", s0)
    s2 = _mash(" ", s1)
    t0 = _mash(text, s2)
    t1 = _mash(text, t0)
    t2 = _mash(text, t1)
    out = []
    for s, t in ((s0, t0), (s1, t1), (s2, t2)):
        s = _u32(s)
        s -= _u32(t)
        s *= 2.0 ** -32
        s += 1.0 if s < 0 else 0.0
        out.append(s)
    return (out[0], out[1], out[2], 1.0)


ALEA_SEED = alea_seed()


class Alea:
    def __init__(self):
        self.s0, self.s1, self.s2, self.c = ALEA_SEED

    def _next(self):
        t = 2091639 * self.s0 + self.c * 2.0 ** -32
        self.s0, self.s1 = self.s1, self.s2
        self.c = float(int(t))
        self.s2 = t - self.c
        return self.s2

    def uniform(self, lo, hi):
        a = self._next()
        s = a + float(int(self._next() * 0x200000)) * 2.0 ** -53
        return lo * (1 - s) + s * hi


# ------------------------------------------------------------------------------------------------ scalar helpers
def _div(a, b):
    if b == 0:
        return math.nan if (a == 0 or a != a) else math.copysign(math.inf, a) * math.copysign(1.0, b)
    return a / b


def _jsmax(a, b):
    if a != a or b != b:
        return math.nan
    return a if a > b else b


def _sqrt(x):
    return math.sqrt(x) if x >= 0 else math.nan


def giv_rot_qr(a, b):
    """_giv_rot.js:22-37"""
    mx = _jsmax(abs(a), abs(b))
    if mx == 0:
        return 1.0, 0.0, 0.0
    a, b = _div(a, mx), _div(b, mx)
    norm = _sqrt(a * a + b * b)
    return _div(a, norm), _div(b, norm), norm * mx


def hypot_node12(a, b):
    """node 12's Math.hypot of two numbers: an infinity wins, then NaN, else max * sqrt(sum (x / max)^2)"""
    a, b = abs(a), abs(b)
    if a == math.inf or b == math.inf:
        return math.inf
    if a != a or b != b:
        return math.nan
    mx = a if a > b else b
    if mx == 0:
        return 0.0
    x, y = a / mx, b / mx
    return _sqrt(x * x + y * y) * mx


# ------------------------------------------------------------------------------------------------ schur_qrfrancis_inplace
class Stats:
    def __init__(self, budget_fn=budget):
        self.budget = budget_fn
        self.calls = []            # (n, sweeps) per francis_qr call
        self.draws = 0
        self.rec_interior = 0      # recursions through the interior scan (schur.js:515-521)
        self.rec_small = 0         # recursions through the >>>4 rule (:507)
        self.depth = 0             # deepest nesting of recurse

    @property
    def max_sweeps(self):
        return max((s for _, s in self.calls), default=0)

    @property
    def worst_budget_share(self):
        return max((s / self.budget(n) for n, s in self.calls), default=0.0)


def _rot(X, i, j, c, s, axis):
    if axis == 0:
        a, b = X[i].copy(), X[j].copy()
        X[i] = s * b + c * a
        X[j] = c * b - s * a
    else:
        a, b = X[:, i].copy(), X[:, j].copy()
        X[:, i] = s * b + c * a
        X[:, j] = c * b - s * a


def _francis(Q, H, st, depth):
    """francis_qr (schur.js:415-591) on the n x n views Q (rows of Q^T) and H"""
    n = H.shape[0]
    st.depth = max(st.depth, depth)
    slot = len(st.calls)
    st.calls.append((n, 0))
    limit = st.budget(n)
    h = lambda i, j: float(H[i, j])

    def is_zero(i):
        if abs(h(i, i - 1)) > EPS * (abs(h(i - 1, i - 1)) + abs(h(i, i))):
            return False
        H[i, i - 1] *= 0.0
        return True

    def giv(i, j, c, s):
        assert j > i
        _rot(H[:, max(0, i - 1):], i, j, c, s, 0)
        _rot(H[:min(n, j + 2)], i, j, c, s, 1)
        _rot(Q, i, j, c, s, 0)

    def recurse(s, e):
        m = e - s
        assert m <= n >> 1 and m >= 3
        q = np.eye(m)
        _francis(q, H[s:e, s:e], st, depth + 1)
        qt = np.ascontiguousarray(q.T)                    # q[n*j+k] of the reference after its transposition
        def left(X):                                       # X [m, cols] -> sum over ascending j of qt[j, k] X[j, i]
            acc = np.zeros(X.shape)
            for j in range(m):
                acc += qt[j][:, None] * X[j][None, :]
            return acc
        Q[s:e, :] = left(Q[s:e, :].copy())
        H[s:e, e:] = left(H[s:e, e:].copy())
        X = H[:s, s:e].copy()
        acc = np.zeros(X.shape)
        for j in range(m):
            acc += qt[j][None, :] * X[:, j][:, None]
        H[:s, s:e] = acc

    rng = Alea()
    stuck, start, end, sweeps = 0, 0, n, 0
    while True:
        done = False
        while not done:
            if end - start < 3:
                return
            if end - start < n >> 4:
                st.rec_small += 1
                recurse(start, end)
                return
            if is_zero(start + 1):
                start += 1
            elif is_zero(end - 1):
                end -= 1
            elif is_zero(start + 2):
                start += 2
            elif is_zero(end - 2):
                end -= 2
            else:
                done = True
            mid = (start + end) >> 1
            i = start + 2
            while done:
                i += 1
                if not i < end - 2:
                    break
                if is_zero(i):
                    done = False
                    st.rec_interior += 1
                    if i > mid:
                        recurse(i, end)
                        end = i
                    else:
                        recurse(start, i)
                        start = i
            if not done:
                stuck = 0
        if sweeps >= limit:
            raise NoConvergence("nd4hip_dhseqr_batched: no convergence after %d sweeps (the budget of 30 max(10, n) at n = %d)." % (limit, n))
        stuck += 1
        sweeps += 1
        st.calls[slot] = (n, sweeps)

        i, j = end - 2, end - 1
        tr = h(i, i) + h(j, j)
        det = h(i, i) * h(j, j) - h(i, j) * h(j, i)
        if tr * tr > 4 * det:
            sign = 1.0 if tr >= 0 else -1.0
            den = tr + sign * _sqrt(tr * tr - 4 * det)
            ev1 = 0.5 * den
            ev2 = _div(det * 2.0, den)
            if abs(h(j, j) - ev1) > abs(h(j, j) - ev2):
                ev1 = ev2
            tr = ev1 * 2
            det = ev1 * ev1
        if stuck % 16 == 0:
            tr = abs(h(j, i)) + abs(h(i, end - 3))
            det = tr * tr
            st.draws += 1
            tr *= rng.uniform(1.25, 1.75)

        i, j, k = start, start + 1, start + 2
        a1 = h(i, i) * h(i, i) + h(i, j) * h(j, i) - tr * h(i, i) + det
        a2 = h(j, i) * (h(i, i) + h(j, j) - tr)
        a3 = h(j, i) * h(k, j)
        for _ in range(2):
            if a2 != 0:
                c, s, norm = giv_rot_qr(a1, a2)
                giv(i, j, c, s)
                a1 = norm
            j, a2 = k, a3

        for col in range(start, end - 2):
            i = col + 1
            for j in range(col + 2, min(end, col + 4)):
                Hi, Hj = h(i, col), h(j, col)
                if Hj == 0:
                    continue
                c, s, _ = giv_rot_qr(Hi, Hj)
                giv(i, j, c, s)
                H[j, col] *= 0.0


def resolve_2x2(Q, H):
    """schur.js:603-676 on Q (rows of Q^T) and H"""
    N = H.shape[0]
    for j in range(1, N):
        i = j - 1
        if float(H[j, i]) == 0:
            continue
        Hii, Hij, Hji, Hjj = float(H[i, i]), float(H[i, j]), float(H[j, i]), float(H[j, j])
        A = Hjj - Hii
        ABC = A * A + 4 * Hij * Hji
        if ABC < 0:
            continue
        if Hij == 0:
            c, s = 0.0, 1.0
        else:
            T = A + (-1.0 if A < 0 else 1.0) * _sqrt(ABC)
            R = Hij * 2
            TR = hypot_node12(T, R)
            s = _div(-T if R < 0 else T, TR)
            c = _div(abs(R), TR)
        _rot(H[:, i:], i, j, c, s, 0)
        _rot(H[:j + 1], i, j, c, s, 1)
        _rot(Q, i, j, c, s, 0)
        H[j, i] *= 0.0


def qrfrancis_ref(U, H, budget_fn=budget):
    """schur_qrfrancis_inplace on one matrix: (Q, T, Stats) from a Hessenberg decomposition (U, H)"""
    st = Stats(budget_fn)
    Qt = np.ascontiguousarray(np.asarray(U, dtype=np.float64).T)
    T = np.array(H, dtype=np.float64)
    with np.errstate(all="ignore"):
        _francis(Qt, T, st, 0)
        resolve_2x2(Qt, T)
    return np.ascontiguousarray(Qt.T), T, st


_REF = {}


def reference(name):
    """the restatement's (Q, T, [Stats per member]) of a fixture, computed once"""
    if name not in _REF:
        U, H = hessenberg_pair(name)
        N = CASES[name]["N"]
        Qs, Ts, sts = [], [], []
        for u, h in zip(U.reshape(-1, N, N), H.reshape(-1, N, N)):
            q, t, st = qrfrancis_ref(u, h)
            Qs.append(q), Ts.append(t), sts.append(st)
        _REF[name] = (np.array(Qs).reshape(U.shape), np.array(Ts).reshape(U.shape), sts)
    return _REF[name]


# ------------------------------------------------------------------------------------------------ measures
def schur_errors(A, Q, T):
    """(||Q T Q^T - A||_F / ||A||_F, ||Q^T Q - I||_F) of one matrix"""
    na = np.linalg.norm(A)
    r = np.linalg.norm(Q @ T @ Q.T - A)
    return float(r / na if na > 0 else r), float(np.linalg.norm(Q.T @ Q - np.eye(A.shape[0])))


def eig_errors(A, lam, V):
    """(largest column residual ||A v - lambda v||_2 / (||A||_F ||v||_2), largest | scaled 2-norm of a column - 1 |)"""
    na = np.linalg.norm(A)
    R = A @ V - V * lam[None, :]
    res = float((np.linalg.norm(R, axis=0) / ((na if na > 0 else 1.0) * np.linalg.norm(V, axis=0))).max())
    P = np.abs(np.concatenate([V.real, V.imag], axis=0))
    m = P.max(axis=0)
    return res, float(np.abs(np.sqrt(((P / m) ** 2).sum(axis=0)) * m - 1.0).max())


def bound(ref_value, N):
    """four times the reference's own value (N 2^-52 in place of a zero), never above the gate"""
    return min(4.0 * (ref_value if ref_value > 0 else N * EPS), GATE)
