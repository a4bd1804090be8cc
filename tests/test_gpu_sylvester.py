"""schur_sylvester, sylvester_solve and lyapunov_solve on the device (csrc/trsyl.hip) through la and dev, which must give the same bits and
leave their operands untouched. Every operand lies on the grid of multiples of 2^-10, so C = A X + X B is exact in float64 and X_true is
the exact solution. The gates are 8 x the largest forward error and residual of scipy.linalg.solve_sylvester (LAPACK's trsyl) on these
same inputs, measured outside the suite: DESIGN.md 4.31."""
import numpy as np
import pytest

from nd4js_amd import _lib, la

pytestmark = pytest.mark.gpu

LD, EPS = np.longdouble, np.finfo(np.float64).eps
FWD_GATE, RES_GATE = 8 * 40.86, 8 * 5.51           # in eps: 8 x scipy's largest over all cases below
# one tile up to 64, tile starts at 63 k; 127 with a 2x2 block at its end leaves its third tile empty
SHAPES = [(1, 1), (2, 3), (3, 2), (16, 17), (33, 31), (64, 65), (65, 64), (96, 40), (127, 66), (129, 130), (200, 257)]


def grid(x):
    return np.round(x * 1024) / 1024


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def quasi(rng, lead, n):
    """upper quasi-triangular, diagonal in [1.5, 2.5], 2x2 blocks [[a, b], [-c, a]] at 0, 2, n - 2 and across every tile start 63 k"""
    T = np.triu(grid(rng.standard_normal(lead + (n, n)) / np.sqrt(n)), 1) + grid(1.5 + rng.random(lead + (n,)))[..., None] * np.eye(n)
    last = -2
    for i in sorted({0, 2, n - 2} | set(range(62, n - 1, 63))):
        if last + 1 < i < n - 1:
            T[..., i + 1, i + 1] = T[..., i, i]
            T[..., i, i + 1], T[..., i + 1, i] = grid(0.25 + rng.random(lead) / 2), -grid(0.25 + rng.random(lead) / 2)
            last = i
    return T


def dense(rng, lead, n):
    return grid(rng.standard_normal(lead + (n, n)) / np.sqrt(n)) + 2 * np.eye(n)


def case(kind, M, N, trans=False, nb=3):
    """(A, B, C, X_true): A shared by the nb members of B and C; kind: quasi (with op(B) = B^T if trans) or dense"""
    rng = np.random.default_rng(1000 * M + N)
    A, B = (quasi if kind == "quasi" else dense)(rng, (), M), (quasi if kind == "quasi" else dense)(rng, (nb,), N)
    X = grid(rng.standard_normal((nb, M, N)))
    return A, B, A @ X + X @ (np.swapaxes(B, -1, -2) if trans else B), X


def errors(A, B, C, X, Xt):
    """(forward error, residual) in eps, the largest over the members; B already transposed where the equation has B^T"""
    R = C.astype(LD) - A.astype(LD) @ X.astype(LD) - X.astype(LD) @ B.astype(LD)
    scale = np.abs(A).sum(-1).max() + np.abs(B).sum(-2).max(-1)
    return (float((np.abs(X - Xt).max((-1, -2)) / np.abs(Xt).max((-1, -2))).max() / EPS),
            float((np.abs(R).max((-1, -2)) / (scale * np.abs(X).max((-1, -2)))).max() / EPS))


def both(name, *ops, **kw):
    """la.<name> and dev.<name> on the same operands: the same bits and flags, the operands untouched; la's result"""
    import torch
    from nd4js_amd import dev
    keep, up, ih, idv = [o.copy() for o in ops], [torch.from_numpy(o.copy()).cuda() for o in ops], {}, {}
    info = kw.pop("info", False)
    X = getattr(la, name)(*ops, **kw, **({"info": ih} if info else {}))
    Xd = getattr(dev, name)(*up, **kw, **({"info": idv} if info else {}))
    assert all(same_bits(o, k) and same_bits(u.cpu().numpy(), k) for o, u, k in zip(ops, up, keep)), name + ": an operand was written"
    assert same_bits(X, Xd.cpu().numpy()), name + ": la and dev differ"
    if info:
        assert np.array_equal(ih["singular"], idv["singular"].cpu().numpy()) and ih["singular"].dtype == np.int32
        return X, ih["singular"]
    return X


def gate(what, A, B, C, X, Xt):
    fwd, res = errors(A, B, C, X, Xt)
    print("%s: forward %.2f eps, residual %.2f eps" % (what, fwd, res))
    assert np.isfinite(X).all() and fwd <= FWD_GATE and res <= RES_GATE, (fwd, res)


@pytest.mark.parametrize("trans", [False, True])
@pytest.mark.parametrize("M,N", SHAPES)
def test_schur_sylvester(M, N, trans):
    TA, TB, C, Xt = case("quasi", M, N, trans)
    below = np.tri(M, k=-2, dtype=bool)
    TA = np.where(below, np.nan, TA)                            # below the first subdiagonal nothing is read
    X = both("schur_sylvester", TA, TB, C, trans_b=trans)
    gate("schur_sylvester %dx%d" % (M, N), np.where(below, 0.0, TA), np.swapaxes(TB, -1, -2) if trans else TB, C, X, Xt)
    if (M, N) in ((33, 31), (129, 130)):                        # one shape per tier: a member has the bits it has alone
        assert all(same_bits(X[m], la.schur_sylvester(TA, TB[m], C[m], trans_b=trans)) for m in range(3))


@pytest.mark.parametrize("M,N", SHAPES)
def test_sylvester_solve(M, N):
    A, B, C, Xt = case("dense", M, N)
    X = both("sylvester_solve", A, B, C)
    gate("sylvester_solve %dx%d" % (M, N), A, B, C, X, Xt)
    if (M, N) == (33, 31):
        assert all(same_bits(X[m], la.sylvester_solve(A, B[m], C[m])) for m in range(3))


@pytest.mark.parametrize("N", [33, 130])
def test_lyapunov_solve(N):
    """equal to sylvester_solve(A, A^T, Q) within the gate; symmetric to the same gate for a symmetric Q, without being symmetrised"""
    rng = np.random.default_rng(N)
    A, Xt = dense(rng, (), N), grid(rng.standard_normal((N, N)))
    Xt = Xt + Xt.T
    Q = A @ Xt + Xt @ A.T
    X = both("lyapunov_solve", A, Q)
    gate("lyapunov_solve %d" % N, A, A.T, Q, X, Xt)
    top = np.abs(Xt).max() * EPS
    assert np.abs(X - la.sylvester_solve(A, A.T.copy(), Q)).max() / top <= FWD_GATE and np.abs(X - X.T).max() / top <= FWD_GATE


def test_singular_member():
    """TA = [[1]], TB = [[-1]] as member 1 of 3: flagged and NaN with info, the others as alone; without info a raise that names it"""
    import torch
    from nd4js_amd import dev
    TA, TB, C = np.array([[[2.0]], [[1.0]], [[3.0]]]), np.array([[[1.0]], [[-1.0]], [[0.5]]]), np.ones((3, 1, 1))
    for name in ("schur_sylvester", "sylvester_solve"):
        X, flags = both(name, TA, TB, C, info=True)
        assert flags[0] == 0 and flags[1] != 0 and flags[2] == 0 and np.isnan(X[1]).all()
        assert all(same_bits(X[m], getattr(la, name)(TA[m], TB[m], C[m])) for m in (0, 2))
        with pytest.raises(_lib.Nd4HipError, match=r"%s\(\w+,\w+,C\): the equation is singular\. \(matrix 1\)" % name) as err:
            getattr(la, name)(TA, TB, C)
        assert err.value.code == -5
        with pytest.raises(_lib.Nd4HipError, match=r"\(matrix 1\)"):
            getattr(dev, name)(*(torch.from_numpy(o).cuda() for o in (TA, TB, C)))
        assert same_bits(getattr(la, name)(TA[0], TB[0], C[0]), np.array([[1.0 / 3.0]]))     # the handle stays usable
