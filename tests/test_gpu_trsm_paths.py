"""Every kernel path of trsm.hip (the solver under tril_solve, triu_solve, lu_solve, cholesky_solve, ldl_solve, qr_lstsq, rrqr / urv
solves and the far-column update of the tall LU), against the oracle's substitution on the same inputs.

Gate of every accuracy case: omega_gpu <= 16 * omega_oracle, omega = max |T X - Y| / (|T||X| + |Y|) with the residual in np.longdouble
(trsm_common.omega; two-stage forms for Cholesky / LDL^T / LU). omega needs no reference solution and does not grow with the condition
number; the oracle reaches <= 4 eps on every family (test_trsm_ref_host.py), a dropped or misplaced operand gives omega > 1e-3. The
factor 16 leaves the algorithm itself a margin of more than 4: a numpy model of the one-launch algorithm (trsm_common.model_one_launch,
measured in test_trsm_ref_host.py) stays within 2.8 x the oracle on every family, 3.5 x over other right-hand sides and sizes.

Case -> path -> condition in the source (nd4_trsm_ld / nd4_trsm_t_ex: trsm_cols_ok)

  one launch: tri_inv_blocks + trsm_cols per panel of 1024 rows (+ nd4_gemm between panels)
                                                          M >= 256, M % 32 == 0, J * batch >= 32, T 16-byte aligned, ldT and sT even
    grid M in {256, 288, 544, 1024, 1056, 2080} x (J, batch) in {(32,1), (33,1), (17,2), (1,32), (3,11)}, 4 (upper, unit) modes,
    strided and shared T                                  288 / 544: second / third accumulator slot; 1056, 2080: 2 and 3 panels
    cholesky_solve / ldl_solve N in {288, 1056, 2080}     trsm_cols<false,false> then trsm_cols<true,true>; N > 1024: nd4_gemm(trans);
                                                          (J, batch) = (7, 6) with a strided factor at every N
    families at M = 256, 1056; scales at M = 256, 1056; isolation at (288, 11, 3)
    zero pivot at the ends of the 32-row blocks and of the 8-row sub-blocks, Inf pivot, a diagonal spanning 2^1100 in one block: M = 256
  blocked: tri_block_solve + nd4_gemm per 32 rows         otherwise
    (256, 31, 1)   J * batch < 32          (224, 64, 1)  M < 256          (255 | 257, 40, 1)  M % 32 != 0
    T offset by one double (not 16-byte aligned), strideT = M*M + 1 (odd)   the host-side guard of trsm_cols_ok
    tails M in {1, 31, 32, 33, 95} x J in {1, 257}, 4 modes; families at M = 257, 1057; scales at 257; pivots at M = 64; isolation at 95

Measured on the MI355X with the kernels as they are now (8 x 8 sub-blocks, guarded normalisation), every row from one run:
omega_gpu / omega_oracle, worst case of each group; the oracle's omega is 1.0e-16 ... 4.7e-16 for one triangle, up to 3.5e-15 for the
two-stage N = 2080 solves.

  case                                                     path        ratio
  grid, 6 x 5 shapes x 4 modes, strided / shared T         one launch  <= 1.68 (M=2080, J=3, batch=11, upper unit, shared)
  cholesky_solve N = 288 | 1056 | 2080                     one launch  1.68 | 1.18 | 0.74
  ldl_solve      N = 288 | 1056 | 2080                     one launch  1.50 | 0.95 | 0.72
  families M = 256 | 1056 (one launch) | 257 | 1057 (blocked)
    well_lower 0.91 | 0.86 | 1.34 | 0.86    well_upper 0.82 | 1.09 | 1.00 | 1.20    qr_r_1e6   0.86 | 0.84 | 1.00 | 0.89
    qr_r_1e13  0.84 | 1.01 | 1.10 | 1.08    lu_u       1.84 | 1.08 | 0.91 | 1.20    lu_l       0.93 | 1.22 | 0.82 | 0.83
    unit_dense_upper 1.79 | 2.30 | 1.81 | 1.93          unit_dense_lower 2.08 | 1.20 | 0.99 | 0.96
    row_graded 0.94 | 0.82 | 0.79 | 0.99    col_graded 0.81 | 0.90 | 1.20 | 0.87
    kahan_1.2  2.93 | 3.49 | 2.64 | 3.11
  a diagonal of 2^600 and 2^-500 in one block, M = 256     one launch  1.30 (lower), 0.96 (upper)
  dispatch edges (7 cases x lower / upper)                 see above   <= 1.27; (256, 32, 1), the one-launch side: 0.95 / 1.03
  blocked tails M in {1, 31, 32, 33, 95}, 4 modes          blocked     <= 1.97 (M=32, J=1, upper unit)
  scales 2^-1000, 2^600, 2^1000 (identical per case: the normalisation makes the solve scale invariant)
    triangles M = 256 | 1056 (one launch) | 257 (blocked), lower / upper    0.87 / 0.95 | 0.94 / 1.05 | 1.02 / 0.91
    lu_solve 1.07    cholesky_solve 0.81 (2^-1000), 1.09    qr_lstsq 0.77   (one launch)
  scale 2^-1030: error against the np.longdouble substitution, GPU / oracle (gate: 8 x)
    triangles M = 256 lower 5.6e-13 / 6.2e-13, upper 6.1e-13 / 7.9e-13; M = 1056 lower 7.1e-13 / 7.4e-13, upper 7.3e-13 / 6.3e-13;
    M = 257 (blocked) lower 5.9e-13 / 5.9e-13, upper 5.2e-13 / 5.2e-13
    lu_solve 3.0e-12 / 1.5e-12    cholesky_solve 7.7e-07 / 9.0e-07 (a right-hand side of 2^-1050: few bits left)    qr_lstsq 2.9e-12 / 2.9e-12

What the test found in the kernels it was written against, both on the one-launch path:
  - without a normalisation of blocks of extreme scale in tri_inv_blocks, the seven 2^-1030 cases (test_scaled_triangles at 256 and
    1056, test_scaled_factor_solves) returned Inf / NaN where the reference is finite;
  - with the whole 32 x 32 diagonal block inverted explicitly, kahan_1.2 measured 39.9 (M = 256) and 82.1 (M = 1056), omega 6.5e-15 /
    1.3e-14 against 1.6e-16, and test_families[kahan_1.2-256 | 1056] failed: that algorithm is not componentwise backward stable
    where a diagonal block has a large inverse (entries up to 1.4e4 there; its numpy model gave 5 to 240), and unit_dense reached 4.0.
    The kernel now inverts 8 x 8 sub-blocks and couples them by substitution (trsm.hip: tri_inv_blocks).
"""
import ctypes
import functools

import numpy as np
import pytest

import oracle
from families import triangle
from nd4js_amd import rng
from trsm_common import (FAMILIES, LD, call_dtrsm_dev, colerr, effective, family, grid20, omega, omega_cholesky, omega_factored, omega_ldl,
                         subst, triangle20)

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -52
GATE = 16.0

@pytest.fixture(scope="module")
def la():
    from nd4js_amd import la as _la
    return _la


def relerr(x, ref):
    return np.linalg.norm((x - ref).ravel()) / max(np.linalg.norm(ref.ravel()), 1e-300)


def _osolve(T, Y, upper):
    return (oracle.triu_solve if upper else oracle.tril_solve)(T, Y)


def _gate(tag, wg, wo):
    print("RATIO %-60s omega_gpu %.3g omega_oracle %.3g ratio %.2f" % (tag, wg, wo, wg / wo if wo > 0 else np.inf))
    assert wg <= GATE * wo, tag


@functools.lru_cache(maxsize=4)
def _well(M, upper):
    t = triangle(22000 + M + int(upper), (M, M), upper)
    t.setflags(write=False)
    return t


# ---------------------------------------------------------------------------------------------- 1. one-launch path: the shape grid
GRID_M = [256, 288, 544, 1024, 1056, 2080]
GRID_JB = [(32, 1), (33, 1), (17, 2), (1, 32), (3, 11)]
MODES = [(False, False), (True, False), (False, True), (True, True)]      # (upper, unit)


def _members(T0, batch, unit):
    """a strided batch from one triangle: member b is T0 (1 + b / 64), every member different from every other; unit: NaN on the
    diagonal, which must not be read"""
    T = T0[None] * (1.0 + np.arange(batch) / 64.0)[:, None, None]
    if unit:
        T[:, np.arange(T0.shape[0]), np.arange(T0.shape[0])] = np.nan
    return T


def _check_members(tag, T, Y, X, upper, unit):
    """T [batch or 1, M, M], X, Y [batch, M, J]: the gate per member (shared T: all members' columns in one solve)"""
    batch, M, J = Y.shape
    if T.shape[0] == 1:
        E = effective(T[0], upper, unit)
        Yc, Xc = (np.ascontiguousarray(a.transpose(1, 0, 2).reshape(M, batch * J)) for a in (Y, X))
        _gate(tag, omega(E, Xc, Yc, upper), omega(E, _osolve(E, Yc, upper), Yc, upper))
        return
    wg = wo = 0.0
    for b in range(batch):
        E = effective(T[b], upper, unit)
        wg, wo = max(wg, omega(E, X[b], Y[b], upper)), max(wo, omega(E, _osolve(E, Y[b], upper), Y[b], upper))
    _gate(tag, wg, wo)


@pytest.mark.parametrize("upper,unit", MODES)
@pytest.mark.parametrize("M,J,batch", [(M, J, b) for M in GRID_M for J, b in GRID_JB if (M, b) != (2080, 32)])
def test_one_launch_grid(la, M, J, batch, upper, unit):
    """every mode through the ABI between guard regions, batch > 1 with a strided and with a shared T; the non-unit modes through
    la.tril_solve / la.triu_solve as well. (2080, 1, 32) is left out: 32 triangles of 2080^2 are a gigabyte, (1056, 1, 32) has the same batch
    over two panels."""
    T0 = _well(M, upper)
    Y = rng.matrix(22100 + M + J, batch, M, J)
    tag = "grid M=%d J=%d batch=%d %s%s" % (M, J, batch, "upper" if upper else "lower", " unit" if unit else "")
    for shared in ((True,) if batch == 1 else (False, True)):
        T = _members(T0, 1 if shared else batch, unit)
        X, intact = call_dtrsm_dev(upper, unit, T, Y, shared_T=shared)
        assert intact, tag
        _check_members(tag + (" shared" if shared else " strided") + " abi", T, Y, X, upper, unit)
        if shared and not unit:                          # (the host form cuts a strided batch into chunks, each with its own J * batch)
            Xh = (la.triu_solve if upper else la.tril_solve)(T[0] if shared else T, Y)
            _check_members(tag + (" shared" if shared else " strided") + " la", T, Y, Xh, upper, unit)


# ------------------------------------------------------------------------------------------------- 2. transposed instantiations
def _two_stage_dev(name, F, Y, shared):
    """nd4hip_dpotrs / dldltrs_batched_dev on device copies; shared: one factor for all members (stride 0)"""
    import torch
    from nd4js_amd import _lib
    batch, N, J = Y.shape
    Fd, Yd = torch.from_numpy(np.ascontiguousarray(F)).cuda(), torch.from_numpy(np.ascontiguousarray(Y)).cuda()
    Xd = torch.empty_like(Yd)
    h = _lib.handle(0)
    h.set_stream(torch.cuda.current_stream().cuda_stream)
    fn = getattr(h.lib, name)
    _lib.check(fn(h.ptr, batch, N, J, ctypes.c_void_p(Fd.data_ptr()), 0 if shared else N * N, ctypes.c_void_p(Yd.data_ptr()), N * J,
                  ctypes.c_void_p(Xd.data_ptr())))
    torch.cuda.synchronize()
    return Xd.cpu().numpy()


def _chol_factor(seed, N):
    B = rng.matrix(seed, N, N)
    S = B @ B.T
    S[np.arange(N), np.arange(N)] += N
    return np.linalg.cholesky(S)


def _ldl_packed(seed, N):
    """test_ldl_sizes's factors, packed: unit-lower L0 (entries / 4, or 2 / N beyond 512) below the diagonal, D0 = +-(1 + |u|) on it"""
    r = rng.matrix(seed, N, N)
    d0 = np.where(np.diag(r) >= 0, 1 + np.diag(r), -1 + np.diag(r))
    return np.tril(r * (0.25 if N <= 512 else 2.0 / N), -1) + np.diag(d0)


@pytest.mark.parametrize("J,batch", [(32, 1), (7, 6)])
@pytest.mark.parametrize("N", [288, 1056, 2080])
@pytest.mark.parametrize("op", ["cholesky", "ldl"])
def test_two_stage_solves(op, N, J, batch):
    """forward with L, backward with L^T (trsm_cols<true, true>; N > 1024: the transposed panel update). A batch has its own factor
    per member (strided T) up to 1056; at 2080 (three panels) member b is the first factor times 1 + b / 64, itself the factor of
    another matrix and just as strided, which spares five factorisations of 2080^2."""
    shared = batch == 1
    make = _chol_factor if op == "cholesky" else _ldl_packed
    if N == 2080 and batch > 1:
        F = make(23000 + N, N)[None] * (1.0 + np.arange(batch) / 64.0)[:, None, None]
    else:
        F = np.stack([make(23000 + N + 7 * b, N) for b in range(1 if shared else batch)])
    Y = rng.matrix(23100 + N + J, batch, N, J)
    X = _two_stage_dev("nd4hip_dpotrs_batched_dev" if op == "cholesky" else "nd4hip_dldltrs_batched_dev", F, Y, shared)
    osolve, om, tol = (oracle.cholesky_solve, omega_cholesky, 1e-14) if op == "cholesky" else (oracle.ldl_solve, omega_ldl, 1e-13)
    wg = wo = 0.0
    for b in range(batch):
        Fb = F[0 if shared else b]
        ref = osolve(Fb, Y[b])
        wg, wo = max(wg, om(Fb, X[b], Y[b])), max(wo, om(Fb, ref, Y[b]))
        if N <= 1056:
            assert relerr(X[b], ref) <= tol, (op, N, b)
    _gate("two-stage %s N=%d J=%d batch=%d" % (op, N, J, batch), wg, wo)


# ------------------------------------------------------------------------------------------------------- 3. accuracy families
@pytest.mark.parametrize("M", [256, 1056, 257, 1057])
@pytest.mark.parametrize("name", list(FAMILIES))
def test_families(la, name, M):
    """R of an ill-conditioned A, the factors of an LU, unit, graded and Kahan triangles: one launch at 256 / 1056, blocked at 257 / 1057"""
    T, upper = family(name, 24000 + M, M)
    Y = rng.matrix(24100 + M, M, 32)
    X = (la.triu_solve if upper else la.tril_solve)(T, Y)
    _gate("family %s M=%d" % (name, M), omega(T, X, Y, upper), omega(T, _osolve(T, Y, upper), Y, upper))


# ----------------------------------------------------------------------------------------------------------- 4. dispatch edges
@pytest.mark.parametrize("upper", [False, True])
@pytest.mark.parametrize("M,J,batch,t_offset,odd", [(256, 31, 1, 0, False), (256, 32, 1, 0, False), (224, 64, 1, 0, False), (255, 40, 1, 0, False),
                                                    (257, 40, 1, 0, False), (256, 32, 1, 1, False), (256, 16, 2, 0, True)])
def test_dispatch_edges(M, J, batch, t_offset, odd, upper):
    """either side of every term of trsm_cols_ok; a T that is not 16-byte aligned or has an odd batch stride must take the blocked
    path (the one-launch kernel reads T with 16-byte loads)"""
    T = _members(_well(M, upper), batch, False)
    Y = rng.matrix(25000 + M + J, batch, M, J)
    X, intact = call_dtrsm_dev(upper, False, T, Y, t_offset=t_offset, stride_t=M * M + 1 if odd else None)
    assert intact
    _check_members("edge M=%d J=%d batch=%d off=%d odd=%d %s" % (M, J, batch, t_offset, odd, "upper" if upper else "lower"), T, Y, X, upper, False)


@pytest.mark.parametrize("upper,unit", MODES)
@pytest.mark.parametrize("J", [1, 257])
@pytest.mark.parametrize("M", [1, 31, 32, 33, 95])
def test_blocked_tails(M, J, upper, unit):
    """a last block of 1, 31, 32 rows, one and two 256-column workgroups"""
    T = _members(_well(M, upper), 1, unit)
    Y = rng.matrix(25100 + M + J, 1, M, J)
    X, intact = call_dtrsm_dev(upper, unit, T, Y, shared_T=True)
    assert intact
    _check_members("tail M=%d J=%d %s%s" % (M, J, "upper" if upper else "lower", " unit" if unit else ""), T, Y, X, upper, unit)


# ------------------------------------------------------------------------------------------------------------- 6. isolation
@pytest.mark.parametrize("upper", [False, True])
@pytest.mark.parametrize("M", [288, 95])
def test_members_and_columns_are_isolated(M, upper):
    """(M, 11, 3): one launch at 288 (J * batch = 33), blocked at 95. A singular member leaves the other members bit-identical, a NaN
    in one column of one member every other column of every member. (Not against a solo run: J * batch < 32 takes the other path.)"""
    J, batch = 11, 3
    T = np.stack([triangle(26000 + M + b, (M, M), upper) for b in range(batch)])
    Y = rng.matrix(26100 + M, batch, M, J)
    X, intact = call_dtrsm_dev(upper, False, T, Y)
    assert intact and np.isfinite(X).all()
    Tz = T.copy()
    Tz[1, 40, 40] = 0.0
    Xz, intact = call_dtrsm_dev(upper, False, Tz, Y)
    assert intact and np.array_equal(Xz[[0, 2]], X[[0, 2]]) and not np.isfinite(Xz[1]).all()
    Yn = Y.copy()
    Yn[0, M // 2, 5] = np.nan
    Xn, intact = call_dtrsm_dev(upper, False, T, Yn)
    others = [c for c in range(J) if c != 5]
    assert intact and np.array_equal(Xn[1:], X[1:]) and np.array_equal(Xn[0][:, others], X[0][:, others])
    assert np.isnan(Xn[0][:, 5]).any()


# -------------------------------------------------------------------------------------------- 7. non-finite like the reference
@pytest.mark.parametrize("upper", [False, True])
@pytest.mark.parametrize("M", [64, 256])
def test_zero_and_inf_pivots_like_the_reference(la, M, upper):
    """a zero pivot: non-finite exactly where the reference's substitution is (the rows solved before it stay finite), the finite
    entries to 1e-12 of the column's largest; an Inf pivot: finite everywhere, its row exactly 0"""
    solve = la.triu_solve if upper else la.tril_solve
    Y = rng.matrix(27000 + M, M, 32)
    for p in (0, 7, 8, 23, 24, 31, 32, M - 1):     # the ends of the 32-row blocks and of the 8-row sub-blocks of the one-launch path
        T = _well(M, upper).copy()
        T[p, p] = 0.0
        with np.errstate(all="ignore"):
            x, ref = solve(T, Y), _osolve(T, Y, upper)
            fin = np.isfinite(ref)
            assert np.array_equal(np.isfinite(x), fin), (M, upper, p)
            assert fin.any() == (p != (M - 1 if upper else 0))
            big = np.where(fin, np.abs(ref), 0.0).max(axis=0)
            assert (np.abs(np.where(fin, x - ref, 0.0)) <= 1e-12 * big).all(), (M, upper, p)
    T = _well(M, upper).copy()
    T[5, 5] = np.inf
    x, ref = solve(T, Y), _osolve(T, Y, upper)
    assert np.isfinite(x).all() and np.isfinite(ref).all() and np.array_equal(x[5], np.zeros(32)) and np.array_equal(ref[5], np.zeros(32))
    assert np.abs(x - ref).max() <= 1e-12 * np.abs(ref).max()


@pytest.mark.parametrize("upper", [False, True])
def test_diagonal_spanning_more_than_the_normalisation_can_hold(la, upper):
    """one 32-row block with pivots of 2^600 and 2^-500: every plain reciprocal is finite, but scaled by the largest diagonal the small
    pivot would flush to 0, so tri_inv_blocks must leave such a block unscaled. Finite like the reference, and the omega gate."""
    M = 256
    T = _well(M, upper).copy()
    T[3, 3] *= 2.0 ** 600
    T[10, 10] *= 2.0 ** -500
    Y = rng.matrix(27500 + int(upper), M, 32)
    x, ref = (la.triu_solve if upper else la.tril_solve)(T, Y), _osolve(T, Y, upper)
    assert np.isfinite(ref).all() and np.isfinite(x).all()
    _gate("wide diagonal M=%d %s" % (M, "upper" if upper else "lower"), omega(T, x, Y, upper), omega(T, ref, Y, upper))


# ------------------------------------------------------------------------------------------------------- 8. extreme scales
SCALES = [-1030, -1000, 600, 1000]


def _scale_check(tag, e, xg, xo, om, truth):
    """finite wherever the oracle is; the omega gate for 2^-1000 ... 2^1000; at 2^-1030 (denormal products: the reference loses bits
    itself) the error against the np.longdouble substitution within 8 x the oracle's"""
    assert np.isfinite(xg)[np.isfinite(xo)].all(), tag
    if e >= -1000:
        _gate(tag, om(xg), om(xo))
        return
    t = truth()
    eg, eo = colerr(xg, t), colerr(xo, t)
    print("TRUTH %-60s err_gpu %.3g err_oracle %.3g ratio %.2f" % (tag, eg, eo, eg / eo if eo > 0 else np.inf))
    assert eg <= 8 * eo, tag


@pytest.mark.parametrize("e", SCALES)
@pytest.mark.parametrize("upper", [False, True])
@pytest.mark.parametrize("M", [256, 1056, 257])
def test_scaled_triangles(la, M, upper, e):
    """T and Y on the 2^-20 grid times 2^e (exact, denormals included): the solution is that of the unscaled system. One launch at
    256 and 1056 (tri_inv_blocks must not go through an overflowing reciprocal), blocked at 257."""
    s = 2.0 ** e
    T, Y = triangle20(28000 + M + int(upper), M, upper) * s, grid20(28100 + M, M, 32) * s
    with np.errstate(all="ignore"):
        xg, xo = (la.triu_solve if upper else la.tril_solve)(T, Y), _osolve(T, Y, upper)
        _scale_check("scale 2^%d tri M=%d %s" % (e, M, "upper" if upper else "lower"), e, xg, xo, lambda x: omega(T, x, Y, upper),
                     lambda: subst(T.astype(LD), Y.astype(LD), upper))


@pytest.mark.parametrize("e", SCALES)
@pytest.mark.parametrize("op", ["lu_solve", "cholesky_solve", "qr_lstsq"])
def test_scaled_factor_solves(la, op, e):
    """the consumers at M = 256, 32 columns, their triangular factor (on the 2^-20 grid) times 2^e. lu_solve: U scaled, the unit L not;
    qr_lstsq: R scaled, Q not; right-hand sides times 2^e, so the solution is O(1). cholesky_solve: L times 2^e solves with L L^T, the
    solution is O(2^-e) times the right-hand side's scale, which is 2^e for e > 0 and 2^(e - 20) for e < 0 to keep it representable."""
    M, J, s = 256, 32, 2.0 ** e
    g20 = lambda a: np.round(a * 2.0 ** 20) * 2.0 ** -20
    with np.errstate(all="ignore"):
        if op == "lu_solve":
            lu, p = oracle.lu_decomp(rng.matrix(28200, M, M))
            lu = g20(lu)
            assert (np.diag(lu) != 0).all()
            L, U = effective(lu, False, unit=True), np.triu(lu) * s
            LU, Y = np.tril(lu, -1) + U, grid20(28201, M, J) * s
            xg, xo = la.lu_solve(LU, p, Y), oracle.lu_solve(LU, p, Y)
            om = lambda x: omega_factored([(L, "lower"), (U, "upper")], x, Y[p])
            truth = lambda: subst(U.astype(LD), subst(L.astype(LD), Y[p].astype(LD), False), True)
        elif op == "cholesky_solve":
            L = g20(_chol_factor(28210, M)) * s
            Y = grid20(28211, M, J) * (s if e > 0 else s * 2.0 ** -20)
            xg, xo = la.cholesky_solve(L, Y), oracle.cholesky_solve(L, Y)
            om = lambda x: omega_cholesky(L, x, Y)
            truth = lambda: subst(L.T.astype(LD), subst(L.astype(LD), Y.astype(LD), False), True)
        else:
            Q, R = np.linalg.qr(rng.matrix(28220, M, M))
            R, Y = np.triu(g20(R)) * s, grid20(28221, M, J) * s
            xg, xo = la.qr_lstsq(Q, R, Y), oracle.qr_lstsq(Q, R, Y)
            qty = Q.T.astype(LD) @ Y.astype(LD)
            om = lambda x: omega_factored([(R, "upper")], x, (qty, np.abs(Q.T) @ np.abs(Y)))
            truth = lambda: subst(R.astype(LD), qty, True)
        _scale_check("scale 2^%d %s M=%d" % (e, op, M), e, xg, xo, om, truth)
