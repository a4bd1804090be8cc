"""Helpers of the LU path tests (test_lu_ref_host.py, test_gpu_lu_paths.py, test_gpu_lu.py); nothing here needs a GPU to import.

  regime           Python twin of the regime choice of lu.hip (getrf_impl, lu_la_range, lu_outer_block): the set of kernel paths a call
                   takes. Every GPU case asserts that the path it is there for is in that set.
  call_getrf_dev   nd4hip_dgetrf_batched_dev on LU and P carved out of sentinel-filled device buffers
  planted, zero_column, nan_last_row, inf_below, nan_diag_inf_below
                   inputs whose pivots are decided by exact ties, zeros, NaN and Inf; each says why the outcome is exact
  rows_for_layout  where to plant tied rows so that a kernel's reduction can go wrong
  omega_lu         componentwise backward error max |L U - A[P]| / (|L||U|), the product in np.longdouble
  make_input, structured_keys, SMALL_STRUCT, LARGE_STRUCT, SPECIALS
                   the structured inputs the GPU test uses, by name, shared with the CPU test that proves them against the oracle
"""
import ctypes
import os

import numpy as np

from nd4js_amd import rng

LD = np.longdouble
EPS = 2.0 ** -52

# ---- the constants of the regime choice, each with its place in nd4js_amd/csrc/lu.hip -------------------------------------------
NB = 16                    # lu.hip:29    panel width
LU_OUTER = 512             # lu.hip:995   outer block of a matrix taller than 2048 rows
LU_LA_MAX_BATCH = 12       # lu.hip:1000  the largest batch that takes the look-ahead form
LU_BATCH_OUTER = 128       # lu.hip:1004  outer block of a batch that fills the chip (N >= 4 * LU_BATCH_OUTER)
MW_MAXP = 16               # lu.hip:432   most workgroups per multi-workgroup panel
MW_CORESIDENT = 64         # lu.hip:1191  batch * workgroups per panel must not exceed this
ROWS_GLOBAL = 64           # lu.hip:1076, 1116  panels shorter than this take lu_panel_global; the look-ahead form stops there
ROWS_R1 = 512              # lu.hip:1077, 1128  one row per thread up to here
ROWS_R2 = 1024             # lu.hip:1078, 1129  two rows per thread up to here
ROWS_R4 = 2048             # lu.hip:1076, 1124, 1212  four rows per thread up to here; above: multi-workgroup or split panels
ROWS_TALL8 = 4096          # lu.hip:1065  <4, 8, 1024> up to here
ROWS_TALL4 = 8192          # lu.hip:1066  <8, 4, 1024> up to here
MW_T = 512                 # lu.hip:462   threads per workgroup of the multi-workgroup panel


def _mw(N, batch, mw_env):
    """(mw_on, mw_rt) of getrf_impl (lu.hip:1188-1191); mw_env: the value of ND4HIP_LU_MW_R, None when unset"""
    mw_r = mw_env if mw_env is not None and mw_env >= 0 else (1 if N <= MW_MAXP * 512 else (2 if N <= MW_MAXP * 1024 else 4))
    mw_rt = (1 if mw_r == 1 else 2 if mw_r == 2 else 4) * 512
    mw_on = mw_r != 0 and N > ROWS_R4 and batch * (-(-N // mw_rt)) <= MW_CORESIDENT and N <= MW_MAXP * mw_rt
    return mw_on, mw_rt


def _mw_name(prefix, m, mw_rt):
    Pw = -(-m // mw_rt)
    return "%s<%d,%d>" % (prefix, mw_rt // 512, 1 if Pw <= 4 else 2 if Pw <= 8 else 4)


def _row_name(prefix, m):
    return prefix + ("1" if m <= ROWS_R1 else "2" if m <= ROWS_R2 else "4")


def _la_range(paths, N, mw_rt, j_from, j_to, full_end):
    """lu_la_range (lu.hip:1105-1157); returns the first column it did not factorise"""
    fused = N % 2 == 0
    pj0, j0, folded = -1, j_from, False
    while j0 < j_to and N - j0 >= ROWS_GLOBAL:
        m = N - j0
        if m > ROWS_R4:
            paths.add(_mw_name("mw_la", m, mw_rt))
            if folded:
                paths.add("fold")
        else:
            paths.add(_row_name("row_la", m))
        c0 = j0 + NB
        more = c0 < j_to and N - c0 >= ROWS_GLOBAL
        folded = False
        if more and mw_rt == 512 and m - NB > ROWS_R4:
            folded = True
        elif fused and more:
            paths.add("narrow_fused")
        elif c0 < full_end and c0 < N:
            paths.add("narrow_split")
        pj0 = j0
        j0 += NB
    if pj0 >= 0:
        paths.add("update_blocks")
    return j0


def _outer_block(paths, N, mw_on, mw_rt, J, bend, two_level):
    """lu_outer_block (lu.hip:1056-1098)"""
    j0 = J
    while j0 < bend:
        m = N - j0
        tall8, tall4 = ROWS_R4 < m <= ROWS_TALL8, ROWS_TALL8 < m <= ROWS_TALL4
        mw = mw_on and m > ROWS_R4 and bend - j0 >= NB
        step = NB if mw else 8 if tall8 else 4 if tall4 else NB
        nb = min(bend - j0, step)
        if mw:
            paths.add(_mw_name("mw", m, mw_rt))
        elif tall8:
            paths.add("tall8")
        elif tall4:
            paths.add("tall4")
        elif ROWS_GLOBAL <= m <= ROWS_R4:
            paths.add(_row_name("row", m))
        else:
            paths.add("global")
        if N > nb:
            paths.add("laswp")
        if N - j0 - nb > 0 and bend - j0 - nb > 0:
            paths.add("rank16")
        j0 += step
    if two_level and N - bend > 0:
        paths.add("outer512" if N > ROWS_R4 else "batch_outer128")


def regime(batch, N, mw_env=None):
    """the kernel paths of one nd4hip_dgetrf_batched_dev call (getrf_impl, lu.hip:1161-1240):
      global | row1 row2 row4 | tall8 tall4 | mw<R,PQ>      the panel kernels of the throughput form (lu_outer_block), with laswp, rank16
      row_la1 row_la2 row_la4 | mw_la<R,PQ> (+ fold)         the panels of the look-ahead form (lu_la_range), with update_blocks and
      narrow_fused | narrow_split                            what stages the next panel's columns between two of them
      outer512 | batch_outer128                              lu_outer_far after an outer block of 512 (N > 2048) or 128 columns (a batch)"""
    paths = set()
    la_on = N >= ROWS_GLOBAL + NB and batch <= LU_LA_MAX_BATCH
    batch_two_level = batch > LU_LA_MAX_BATCH and N <= ROWS_R4 and N >= 4 * LU_BATCH_OUTER
    NBO = LU_OUTER if N > ROWS_R4 else (LU_BATCH_OUTER if batch_two_level else N)
    mw_on, mw_rt = _mw(N, batch, mw_env)
    j = 0
    while N - j > ROWS_R4:                                                       # phase 1
        if la_on and mw_on:
            _la_range(paths, N, mw_rt, j, j + LU_OUTER, j + LU_OUTER)
            paths.add("outer512")
        else:
            _outer_block(paths, N, mw_on, mw_rt, j, j + LU_OUTER, True)
        j += LU_OUTER
    if la_on and N - j >= ROWS_GLOBAL + NB:                                      # phase 2
        j = _la_range(paths, N, mw_rt, j, N, N)
    if batch_two_level:                                                          # phase 3
        while j < N:
            bend = min(j + NBO, N)
            _outer_block(paths, N, mw_on, mw_rt, j, bend, bend < N)
            j += NBO
    elif j < N:
        _outer_block(paths, N, mw_on, mw_rt, j, N, False)
    return paths


# ------------------------------------------------------------------------------------------------------------------ guarded call
GUARD = 4096                                           # elements before and after LU and P
SENTINEL = -6.02214076e23                              # no factorisation of these inputs produces it
PSENTINEL = -0x5A5A5A5B                                # outside [0, N)


class mw_env_set:
    """ND4HIP_LU_MW_R for the calls inside (getrf_impl reads it per call); None: unset"""

    def __init__(self, value):
        self.value = value

    def __enter__(self):
        self.old = os.environ.pop("ND4HIP_LU_MW_R", None)
        if self.value is not None:
            os.environ["ND4HIP_LU_MW_R"] = str(self.value)

    def __exit__(self, *exc):
        os.environ.pop("ND4HIP_LU_MW_R", None)
        if self.old is not None:
            os.environ["ND4HIP_LU_MW_R"] = self.old


def call_getrf_dev(a, inplace=False, mw_env=None):
    """(LU, P, intact) of nd4hip_dgetrf_batched_dev on a [batch, N, N] (or [N, N]): the batch reaches the kernels as it is. LU and
    P lie inside larger device tensors, GUARD elements of SENTINEL / PSENTINEL on either side; intact: both guards are bit-unchanged
    after the call and (out of place) so is the input. inplace: the input is copied into the LU region and passed as A == LU."""
    import torch
    from nd4js_amd import _lib
    a3 = np.ascontiguousarray(a, dtype=np.float64).reshape((-1,) + a.shape[-2:])
    batch, N = a3.shape[0], a3.shape[-1]
    n = batch * N * N
    lbuf = torch.full((2 * GUARD + n,), SENTINEL, dtype=torch.float64, device="cuda")
    pbuf = torch.full((2 * GUARD + batch * N,), PSENTINEL, dtype=torch.int32, device="cuda")
    lu_d, p_d = lbuf[GUARD:GUARD + n], pbuf[GUARD:GUARD + batch * N]
    if inplace:
        lu_d.copy_(torch.from_numpy(a3.reshape(-1)))
        a_d = lu_d
    else:
        a_d = torch.from_numpy(a3.reshape(-1)).cuda()
    h = _lib.handle(0)
    h.set_stream(torch.cuda.current_stream().cuda_stream)
    with mw_env_set(mw_env):
        _lib.check(h.lib.nd4hip_dgetrf_batched_dev(h.ptr, batch, N, ctypes.c_void_p(a_d.data_ptr()), ctypes.c_void_p(lu_d.data_ptr()),
                                                   ctypes.c_void_p(p_d.data_ptr())))
        torch.cuda.synchronize()
    intact = all(bool((g == s).all()) for g, s in ((lbuf[:GUARD], SENTINEL), (lbuf[GUARD + n:], SENTINEL),
                                                   (pbuf[:GUARD], PSENTINEL), (pbuf[GUARD + batch * N:], PSENTINEL)))
    if not inplace:
        intact = intact and bool(torch.equal(a_d.view(torch.int64).cpu(), torch.from_numpy(a3.reshape(-1)).view(torch.int64)))
    lu = lu_d.cpu().numpy().reshape(a3.shape).copy()
    p = p_d.cpu().numpy().reshape(batch, N).copy()
    if np.ndim(a) == 2:
        lu, p = lu[0], p[0]
    return lu, p, intact


# --------------------------------------------------------------------------------------------------------------------- families
V = 4096.0


def planted(seed, N, plants, V=V):
    """rng.matrix(seed, N, N) with exact pivot ties planted: plants = [(c, rows, signs), ...]; every listed row r > c gets
    a[r, :c] = 0 and a[r, c] = sign * V; rows are distinct across plants.
    Why the ties are live when column c is reached: a zero prefix makes every earlier multiplier of row r exactly 0 (0 / pivot), so
    every earlier update subtracts 0 * u and leaves the row bit-unchanged; a zero never wins the strict '>' scan of an earlier column,
    and no earlier column j < c < r has r as its start row, so the row is neither chosen nor displaced. At column c the planted rows
    tie at V, above anything elimination leaves in a uniform (-1, 1) matrix (test_lu_ref_host.py: max |U| == V). The reference picks
    the lowest planted row (first strict maximum); the losers' multipliers are +-V / +-V = +-1 exactly.
    A planted row cannot be the start row j0 + k of its own column (r > c): the start row wins a tie by position in the reference,
    with no comparison between equals, so it would say nothing about the tie-break."""
    a = rng.matrix(seed, N, N)
    seen = set()
    for c, rows, signs in plants:
        assert len(rows) == len(signs) and len(rows) >= 2
        for r, s in zip(rows, signs):
            assert c < r < N and r not in seen, (c, r)
            seen.add(r)
            a[r, :c] = 0.0
            a[r, c] = s * V
    return a


def zero_column(seed, N, c):
    """column c exactly zero. Every update of it is 0 - l * 0 = 0, so at column c no candidate beats the start row (no strict
    maximum: P[c] is what the earlier interchanges left at c), every multiplier below is 0 / 0 = NaN and so is all of LU[c+1:, c:];
    from there on every start row is NaN, which no later row beats: no further interchange. Rows 0..c of LU stay finite."""
    a = rng.matrix(seed, N, N)
    a[:, c] = 0.0
    return a


def nan_last_row(seed, N, c):
    """row N-1: zero prefix and NaN at column c. The prefix keeps the row untouched up to column c (see planted); fabs(NaN) > x is
    false, so the NaN never wins a pivot and the row stays last; its multiplier NaN / pivot spreads NaN over LU[N-1, c:] only."""
    a = rng.matrix(seed, N, N)
    a[N - 1, :c] = 0.0
    a[N - 1, c] = np.nan
    return a


def inf_below(seed, N, c, r):
    """row r > c: zero prefix and +Inf at column c: it wins column c (P[c] = r), every multiplier is x / Inf = 0 exactly, so the
    only non-finite entry of LU is U[c, c] = Inf."""
    assert c < r < N
    a = rng.matrix(seed, N, N)
    a[r, :c] = 0.0
    a[r, c] = np.inf
    return a


def nan_diag_inf_below(seed, N, c, r):
    """inf_below, and row c has a zero prefix and NaN at (c, c): fabs(Inf) > fabs(NaN) is false, so the NaN start row keeps the pivot
    (P[c] = c) against an infinite candidate, and LU[c+1:, c:] and LU[c, c] are NaN."""
    a = inf_below(seed, N, c, r)
    a[c, :c] = 0.0
    a[c, c] = np.nan
    return a


def rows_for_layout(kind, j0, N, k=0, R=1, T=512):
    """Planted-row placements [(name, rows, signs), ...] for column j0 + k of a panel at j0 whose kernel keeps row j0 + t + T * i in
    (thread t, register slot i), i < R (kind "row": lu_panel_row_body, T = 512 or 1024), or row j0 + w * R * 512 + t + 512 * i in
    (workgroup w, thread t, slot i) (kind "mw": lu_panel_mw_body), or strides over the rows with T threads (kind "global"). Only the
    placements that fit (rows below N, slots below R) are returned; offsets carry k so that the plants of one panel stay distinct.
      a  two rows in one wave                          b  two waves (R >= 2: the lower row in the LATER wave, against slot 1 of wave 0)
      c  one thread, two register slots: r, r + T      d  the lower row in a high slot-0 thread, the higher in a low slot-1 thread
      e  three rows, mixed signs, three waves          f* (mw) different workgroups; the last, partly filled one; a pair astride a
                                                          workgroup boundary; three workgroups with mixed signs
    g: a planted row equal to j0 + k itself is impossible (see planted)."""
    c = j0 + k
    out = []

    def add(name, rows, signs):
        if all(c < r < N for r in rows) and len(set(rows)) == len(rows):
            out.append((name, list(rows), list(signs)))

    if kind == "global":
        add("a", [c + 2, c + 9], [1, -1])
        add("e", [c + 3, c + 20, c + 21], [-1, 1, 1])
        return out
    Tw = T if kind == "row" else MW_T
    if kind == "mw":                                   # first what only this kernel has
        RT = R * MW_T
        nwg = -(-(N - j0) // RT)
        add("f_wg", [j0 + 100 + k, j0 + RT + (100 + k) % max(N - j0 - RT, 1)], [1, -1])       # (a short last workgroup: wrapped into it)
        add("f_last", [j0 + RT + 7 + k if nwg > 2 else j0 + 40 + k + 16, N - 2 - k - 16], [-1, 1])
        add("f_astride", [j0 + RT - 1, j0 + RT], [1, 1] if k % 2 else [-1, 1])
        if nwg >= 3:
            add("f_three", [j0 + (nwg - 1) * RT + 2 + k, j0 + RT + 300 + k, j0 + 72 + k], [1, -1, 1])
    add("a", [j0 + 20 + k, j0 + 45 + k], [-1, 1])
    if R >= 2:
        add("b", [j0 + 300 + k, j0 + Tw + 5 + k], [1, -1])
        add("c", [j0 + 60 + k, j0 + 60 + k + Tw], [1, 1])
        add("d", [j0 + Tw - 12 + k - 16, j0 + Tw + 3 + k + 16], [-1, -1])
    else:
        add("b0", [j0 + 30 + k, j0 + 66 + k], [-1, -1])
        add("b", [j0 + 70 + k, j0 + 200 + k], [1, -1])
    if R >= 4:
        add("c3", [j0 + 77 + k + 2 * Tw, j0 + 77 + k + 3 * Tw], [-1, 1])
    add("e", [j0 + 17 + k + 16, j0 + 66 + k + 16, j0 + 150 + k], [-1, 1, 1])
    if N - c > 80:
        add("e_last", [N - 70 - k, N - 40 - k, N - 2 - k], [1, -1, -1])      # the last rows the kernel holds
    return out


def plants_for(layouts, N):
    """one plant per (kind, j0, k, R, T) of `layouts`, the placements taken in turn (the first whose rows are still free), so that
    every placement the layout has is used when there are enough plant columns"""
    taken, plants, turn, used = set(), [], {}, []
    for kind, j0, k, R, T in layouts:
        opts = rows_for_layout(kind, j0, N, k, R, T)
        key = (kind, R, T)
        for s in range(len(opts)):
            name, rows, signs = opts[(turn.get(key, 0) + s) % len(opts)]
            if not taken & set(rows):
                taken |= set(rows)
                plants.append((j0 + k, rows, signs))
                used.append("%s%d:%s" % (kind, R, name))
                turn[key] = turn.get(key, 0) + s + 1
                break
    return plants, used


# ------------------------------------------------------------------------------------------------------------------------ omega
def sample_rows(N, extra=(), seed=1, cap=48):
    """all rows for N <= 600; else at most `cap`: the first and the last row, the rows either side of every regime boundary (64, 512,
    1024, 2048 rows from the bottom, ends of the outer blocks of 512 beyond 2048 rows), `extra` (planted rows, plant columns), and seeded others"""
    if N <= 600:
        return np.arange(N)
    rows = [0, N - 1]
    for b in (ROWS_GLOBAL, ROWS_R1, ROWS_R2, ROWS_R4):
        rows += [N - b - 1, N - b]
    if N > ROWS_R4:
        for e in range(LU_OUTER, N, LU_OUTER):
            rows += [e - 1, e]
    rows = [r for r in rows if 0 <= r < N]
    rows = list(dict.fromkeys(rows + [int(r) for r in extra if 0 <= r < N]))[:cap]
    i = 0
    while len(rows) < cap:
        r = int(rng.hash_idx(seed, i, N))
        i += 1
        if r not in rows:
            rows.append(r)
    return np.array(sorted(rows))


def omega_lu(a, lu, p, rows=None, ref=None):
    """max over the given rows i (all by default) and all columns j of |L U - A[P]|_ij / (|L||U|)_ij: the product in np.longdouble,
    the denominator (no cancellation) in fp64. Excluded: every entry whose sum holds a term with a non-finite factor of `ref` (the
    reference's LU; default lu itself), which is where the reference is non-finite and, for an infinite pivot U[c, c], the column
    below it (the multipliers x / Inf = 0 have forgotten x). A non-finite entry of lu where ref is finite gives NaN, which fails
    every `<=` gate."""
    N = a.shape[-1]
    rows = np.arange(N) if rows is None else np.asarray(rows)
    nf = ~np.isfinite(lu if ref is None else ref)
    bad = (np.cumsum(np.tril(nf, -1)[rows], axis=1) > 0) | (np.cumsum(np.triu(nf), axis=0)[rows] > 0)
    ap = a[p[rows].astype(np.int64)]
    bad |= ~np.isfinite(ap)
    clean = np.where(nf, 0.0, lu)
    L = np.tril(clean, -1)[rows]
    L[np.arange(len(rows)), rows] = 1.0
    U = np.triu(clean)
    with np.errstate(all="ignore"):
        prod = np.empty(L.shape, dtype=LD)
        order = np.argsort(rows)
        Ul = U.astype(LD)
        for s in range(0, len(rows), 64):                                        # a row i only has terms k <= i
            idx = order[s:s + 64]
            kmax = int(rows[idx].max()) + 1
            prod[idx] = L[idx, :kmax].astype(LD) @ Ul[:kmax]
        num = np.abs(prod - np.where(bad, 0.0, ap).astype(LD))
        den = (np.abs(L) @ np.abs(U)).astype(LD)
        q = np.where(den > 0, num / np.where(den > 0, den, 1), np.where(num == 0, 0, np.inf))
        q = np.where(bad, 0, q)
        return float(q.max())


def relerr(x, ref):
    return np.linalg.norm((x - ref).ravel()) / max(np.linalg.norm(ref.ravel()), 1e-300)


# ------------------------------------------------------------------------------------------------ the structured inputs, by name
def _panel_layouts(kind, j0s, R_of, T=512, ks=(0, 7, 15)):
    return [(kind, j0, k, R_of(j0), T) for j0 in j0s for k in ks]


def _R(N):
    return lambda j0: 1 if N - j0 <= ROWS_R1 else 2 if N - j0 <= ROWS_R2 else 4


def _planted_spec(N, variant=None):
    """the plant layouts of the regime that a single matrix of N rows takes (variant: "batch" for batch > 12, "tall8" / "mw2" / "mw4"
    for the other panel kernels beyond 2048 rows): panel columns 0, 7 and 15 of the first, a middle and the last full panel of the
    regime; either side of an outer-block end; either side of the panel where the height crosses 2048 rows"""
    if N < ROWS_GLOBAL:
        return [("global", 0, 0, 1, 512), ("global", 0, 15, 1, 512)] + ([("global", 16, 5, 1, 512)] if N > 40 else [])
    if N < ROWS_GLOBAL + NB:
        return _panel_layouts("row", [0], _R(N))
    if N <= ROWS_R4:
        last = ((N - ROWS_GLOBAL) // NB) * NB                                     # the last panel of >= 64 rows
        j0s = sorted({0, min(NB, last), (last // 2 // NB) * NB, last})
        lay = _panel_layouts("row", j0s, _R(N))
        if variant == "batch" and N >= 4 * LU_BATCH_OUTER:                       # either side of the first outer-block end
            lay += [("row", LU_BATCH_OUTER - NB, 15, _R(N)(LU_BATCH_OUTER - NB), 512), ("row", LU_BATCH_OUTER, 0, _R(N)(LU_BATCH_OUTER), 512)]
        return lay
    if variant == "tall8":                                                       # 8-column panels: columns 0, 7 | 8, 15 are two panels
        return [("row", 0, 0, 4, 1024), ("row", 0, 7, 4, 1024), ("row", 8, 0, 4, 1024), ("row", 8, 7, 4, 1024),
                ("row", 16, 0, 4, 1024), ("row", 24, 5, 4, 1024), ("row", 48, 3, 4, 1024), ("row", 56, 0, 4, 512)]                  # (N = 2100: the panel at 56 is the first of <= 2048 rows)
    Rm = 2 if variant == "mw2" else 4 if variant == "mw4" else 1
    cross = ((N - ROWS_R4 - 1) // NB) * NB                                       # the last panel taller than 2048 rows
    lay = _panel_layouts("mw", range(0, cross, NB), lambda j0: Rm) + [("mw", cross, 15, Rm, 512), ("row", cross + NB, 0, 4, 512)]
    lay += [("row", LU_OUTER - NB, 15, _R(N)(LU_OUTER - NB), 512), ("row", LU_OUTER, 0, _R(N)(LU_OUTER), 512)]
    last = ((N - ROWS_GLOBAL) // NB) * NB
    return lay + _panel_layouts("row", [last], _R(N), ks=(7,))


def make_input(key):
    """key = (family, seed, N, *args): the input matrix of that name. Families: generic, planted [variant], zero_column c,
    nan_last_row c, inf_below c r, nan_diag_inf_below c r, nopiv | reverse | cyclic | far (the pivot-sequence patterns of
    test_gpu_lu.test_lookahead_pivot_patterns at any N)."""
    fam, seed, N = key[:3]
    args = key[3:]
    if fam == "generic":
        return rng.matrix(seed, N, N)
    if fam == "planted":
        return planted(seed, N, plants_for(_planted_spec(N, *args), N)[0])
    if fam in ("zero_column", "nan_last_row", "inf_below", "nan_diag_inf_below"):
        return globals()[fam](seed, N, *args)
    base = rng.matrix(seed, N, N)
    i = np.arange(N)
    if fam == "nopiv":                                   # diagonally dominant: no interchange anywhere
        base[i, i] += 100.0
        return base
    if fam == "reverse":                                 # the pivot of column j is row N-1-j: every row moves twice
        a = base[::-1].copy()
        a[i, N - 1 - i] += 100.0
        return a
    if fam == "cyclic":                                  # each pivot is the next row (inside the top block)
        base[i, (i + 1) % N] += 100.0
        return base
    if fam == "far":                                     # the same far rows win again and again in one panel
        base[N // 2 - 10, :16] *= 1e3
        base[N // 2 - 9, :16] *= 1e2
        return base
    raise KeyError(fam)


def planted_plants(key):
    """(plants, placement names) of a planted key"""
    return plants_for(_planted_spec(key[2], *key[3:]), key[2])


def structured_keys(N, seed, variant=None):
    """the five inputs every regime gets: generic, planted, zero_column at the sixth column of the regime's second panel (one clean
    panel, then NaN through every later kernel) and at column N - 3, nan_last_row"""
    pl = ("planted", seed + 1, N) + ((variant,) if variant else ())
    c2 = NB + 5 if N >= 2 * NB + 6 else N // 2
    return [("generic", seed, N), pl, ("zero_column", seed + 2, N, c2), ("zero_column", seed + 3, N, N - 3), ("nan_last_row", seed + 4, N, c2)]


PATTERNS = ("nopiv", "reverse", "cyclic", "far")

# every structured input of test_gpu_lu_paths.py with N <= 600 (the CPU test proves each against the oracle), and one at N = 2100
SMALL_STRUCT = [(48, 31000, None), (63, 31005, None), (79, 31010, None), (160, 31020, None), (161, 31030, None), (600, 31040, None), (515, 31050, None),
                (130, 31060, "batch"), (512, 31070, "batch")]
LARGE_STRUCT = [(1100, 31100, None), (1027, 31110, None), (2100, 31120, None)]
KEY_PLANTED_2048 = ("planted", 31131, 2048)          # four register slots per thread with room for every placement (c3: slots 2 and 3)
SPECIALS = [("inf_below", 31200, 160, 21, 150), ("nan_diag_inf_below", 31201, 160, 21, 150),
            ("inf_below", 31202, 600, 21, 590), ("nan_diag_inf_below", 31203, 600, 21, 590),
            ("inf_below", 31204, 512, 21, 300), ("nan_diag_inf_below", 31205, 512, 21, 300),
            ("inf_below", 31206, 2100, 21, 1500), ("nan_diag_inf_below", 31207, 2100, 21, 1500)]
