"""Helpers of the QR path tests (test_qr_ref_host.py, test_gpu_qr_paths.py); nothing here needs a GPU to import.

  form, panel_plan      Python twins of qr_choose and of the drivers of qr.hip (qr_factor_lookahead, qr_factor_tall, qr_block_panels,
                        qr_factor_batched, qr_factor_blocked, qr_rows_lookahead, qr_form_q, geqrf_tsqr) and of the panel units'
                        launchers (nd4_qr_panel_shape in qr_house.hip, QrhHost::panel in qr_rowsplit.hip): which kernel factorises every 16-column panel of a call, the outer blocks, how Q is formed.
                        Every GPU case asserts through them that it takes the path it is there for.
  panel_entry           the same for nd4hip_dgeqr2_panel_batched_dev (nd4_geqr2_panel)
  dense, graded, cond, kahan, adv, zero_columns, triangular, one_nan (make_input), bare_panel
                        the input families, all seeded through nd4js_amd.rng
  gram_model            numpy model of phase B and of the first CholeskyQR pass of the row-split and batched panels: the Cholesky pivots
                        with the d^2 >= thr G_ii test, Q1 = C R1^-1, max |Q1^T Q1 - I|; classify() turns it into the claim of a panel
  colbe, orth, is_triu  the metrics
  call_qr, call_panel   the device entry points on inputs and outputs carved out of sentinel-filled device buffers
"""
import ctypes

import numpy as np

from nd4js_amd import rng

EPS = 2.0 ** -52

# ---- the constants of the dispatch (nd4js_amd/csrc/qr_internal.h where no file is named) ------------------------------------------------
NB = 16                        # panel width
HR_PIVOT_THR = 1e-5            # a Cholesky pivot below this fraction of its diagonal entry flags the panel
HR_SERIES_MAX = 1e-5           # max |Q1^T Q1 - I| up to which R2 comes from the series, beyond it from the elimination chain
HR_PASS1_MAX = 1e-2            # max |Q1^T Q1 - I| beyond which the panel is flagged after the first pass
HR_MIN_ROWS = 64               # shorter panels take the thread-per-row kernels
QR_SMALL_WG_BATCH = 64         # batches from here on take the few-wave panel variants
QR_LA_MAX_BATCH = 24           # qr.hip
QR_ROWSPLIT_MAX_BATCH = 8      # qr.hip
QR_QT_MAX_BATCH = 4            # qr.hip
QR_TALL_MAX_ROWS = 16384       # qr.hip
QR_OUTER = 128                 # qr.hip
QR_BATCH_OUTER_NARROW = 64     # qr.hip
ROWS_REG = 2048                # the register-resident panels; TSQR's row blocks
ROWS_HALVES = 4096             # qr_panel_part<4,8> up to here
ROWS_QUARTERS = 8192           # qr_panel_part<8,4> up to here; beyond: the global-memory qr_panel<1,false>


def _cdiv(a, b):
    return -(-a // b)


def _batch_outer(npanels):                                                       # qr_batch_outer
    return QR_OUTER if npanels >= 16 else QR_BATCH_OUTER_NARROW


def form(batch, M, N, full):
    """qr_choose: tsqr | lookahead | tall | batched | blocked"""
    L = min(M, N)
    npanels = _cdiv(L, NB)
    nblk = _cdiv(M, ROWS_REG)
    if (not full and M > ROWS_REG and N <= ROWS_REG and batch * nblk <= 32768 and M // nblk >= N
            and (nblk * N <= ROWS_REG or 2 * nblk * N <= M)):
        return "tsqr"
    if 64 <= M <= ROWS_REG and batch <= QR_LA_MAX_BATCH:
        return "lookahead"
    if batch <= QR_ROWSPLIT_MAX_BATCH and ROWS_REG < M <= QR_TALL_MAX_ROWS and L >= 256 and (L % NB == 0 or M - (L // NB) * NB <= ROWS_REG):
        return "tall"
    if M <= ROWS_REG and batch > 1 and L % NB == 0 and npanels >= 2 * (_batch_outer(npanels) // NB):
        return "batched"
    return "blocked"


def _rsel(m):
    return 1 if m <= 512 else 2 if m <= 1024 else 4


def _few(batch, m):
    """<R,NWV> of nd4_qr_panel_shape (qr_house.hip): qrb_panel and qr_panel_row share it"""
    if batch >= QR_SMALL_WG_BATCH and m <= 1024:
        return "<4,%d>" % (1 if m <= 256 else 2 if m <= 512 else 4)
    return "<%d,8>" % _rsel(m)


def _rowsplit(m):
    """QrhHost::panel: qrh_bc<R>, R = 0 beyond the register-resident height"""
    return "qrh_bc<%d>" % (_rsel(m) if m <= ROWS_REG else 0)


def rowsplit_workgroups(m):
    """row workgroups of one qrh_bc launch on a panel of m rows"""
    return (m + NB + 511) // 512


def _rows_lookahead(plan, M, L, N, pnl):
    """qr_rows_lookahead from panel pnl on"""
    npanels = _cdiv(L, NB)
    for p in range(pnl, npanels):
        plan["panels"].append("qr_panel_row_la<%d>" % _rsel(M - p * NB))
    if pnl < npanels:
        j0 = (npanels - 1) * NB
        nb = min(L - j0, NB)
        plan["update_blocks"] = j0 + nb + NB < N                              # the last reflector on the columns the narrow launch left


def _block_panels(plan, batch, M, N, L, P0, pend):
    """qr_block_panels"""
    ldv = _cdiv(L, NB) * NB
    for p in range(P0, pend):
        j0 = p * NB
        nb, m = min(L - j0, NB), M - j0
        if ROWS_REG < m <= ROWS_QUARTERS:
            w = 8 if m <= ROWS_HALVES else 4
            plan["panels"].append("qr_panel_part<4,8>" if w == 8 else "qr_panel_part<8,4>")
            plan["t_assemble"] = plan["t_assemble"] or nb > w
        elif m <= ROWS_REG:
            if batch > QR_ROWSPLIT_MAX_BATCH and nb == NB and m >= HR_MIN_ROWS and N % 2 == 0 and ldv % 2 == 0:
                plan["panels"].append("qrb_panel" + _few(batch, m))
            else:
                plan["panels"].append("qr_panel_row" + _few(batch, m))
        else:
            plan["panels"].append("qr_panel<1,false>")


def panel_plan(batch, M, N, full):
    """One nd4_geqrf_q_ex call with a Q as a dict:
      form          form(batch, M, N, full)
      panels        the kernel that factorises each 16-column panel, left to right: qrh_bc<R> (the row-split launch; R = 0 beyond 2048
                    rows), qrb_panel<R,NWV>, qr_panel_row<R,NWV>, qr_panel_row_la<R>, qr_panel_part<4,8> | <8,4>, qr_panel<1,false>
      outer         (columns per outer block, the last one ragged) of the two-level forms, None for one level
      coupling      the two-half wy_t_small coupling runs (batched form, a block wider than 64 columns)
      far           a block's reflectors reach columns right of the block at once (nd4_qr_block_update / wy_block_update)
      t_assemble    qr_t_assemble joins the parts of a panel factorised in halves or quarters
      update_blocks the last thread-per-row reflector reaches a wide tail through qr_update_blocks
      qt            Q^T is accumulated in the shadow of the panels
      form_q        qt_transpose | compact_wy | tall_blocks | tall_blocks_rebuild | batched_backward | panel_backward (qr_form_q)
      tsqr          for the tsqr form: nblk, mb, padded, recurses, and the plans of the two inner calls (blocks, stacked)"""
    L = min(M, N)
    npanels = _cdiv(L, NB)
    f = form(batch, M, N, full)
    plan = dict(form=f, panels=[], outer=None, coupling=False, far=False, t_assemble=False, update_blocks=False, qt=False, form_q=None, tsqr=None)
    if f == "tsqr":                                                               # geqrf_tsqr
        nblk = _cdiv(M, ROWS_REG)
        mb = (_cdiv(M, nblk) + 1) & ~1
        plan["tsqr"] = dict(nblk=nblk, mb=mb, padded=nblk * mb != M, recurses=form(batch, nblk * N, N, False) == "tsqr",
                            blocks=panel_plan(batch * nblk, mb, N, False), stacked=panel_plan(batch, nblk * N, N, False))
        plan["panels"] = plan["tsqr"]["blocks"]["panels"] + plan["tsqr"]["stacked"]["panels"]
        return plan
    use_hr = (f == "lookahead" and batch <= QR_ROWSPLIT_MAX_BATCH) or f == "tall"
    plan["qt"] = f == "lookahead" and batch <= QR_QT_MAX_BATCH and L >= 256

    def rowsplit_run(pnl):                                                        # row-split panels while they are full and tall enough
        while pnl < npanels and L - pnl * NB >= NB and M - pnl * NB >= HR_MIN_ROWS:
            plan["panels"].append(_rowsplit(M - pnl * NB))
            pnl += 1
        return pnl

    first_low = npanels
    if f == "lookahead":                                                          # qr_factor_lookahead
        _rows_lookahead(plan, M, L, N, rowsplit_run(0) if use_hr else 0)
    elif f == "tall":                                                             # qr_factor_tall
        ppb = QR_OUTER // NB
        P0 = 0
        while P0 < npanels and M - P0 * NB > ROWS_REG:
            pend = min(P0 + ppb, npanels)
            if pend == npanels and L % NB != 0:                                   # a block with the ragged last panel: one level, below
                break
            plan["panels"] += [_rowsplit(M - p * NB) for p in range(P0, pend)]
            first_low = pend
            plan["far"] = plan["far"] or (pend * NB if pend < npanels else N) < N
            P0 += ppb
        plan["outer"] = (QR_OUTER, npanels % ppb != 0 or L % NB != 0)
        plan["tall_blocks"] = first_low // ppb + (first_low % ppb != 0)           # outer blocks factorised with two levels
        _rows_lookahead(plan, M, L, N, rowsplit_run(first_low))
    elif f == "batched":                                                          # qr_factor_batched
        ppb = _batch_outer(npanels) // NB
        plan["outer"] = (ppb * NB, npanels % ppb != 0)
        for P0 in range(0, npanels, ppb):
            pend = min(P0 + ppb, npanels)
            _block_panels(plan, batch, M, N, L, P0, pend)
            plan["coupling"] = plan["coupling"] or (pend - P0) * NB > 64
            plan["far"] = plan["far"] or (pend * NB if pend < npanels else N) < N
    else:                                                                         # qr_factor_blocked
        ppb = QR_OUTER // NB if M > ROWS_REG else npanels
        if ppb < npanels:
            plan["outer"] = (QR_OUTER, npanels % ppb != 0 or L % NB != 0)
        for P0 in range(0, npanels, ppb):
            pend = min(P0 + ppb, npanels)
            _block_panels(plan, batch, M, N, L, P0, pend)
            plan["far"] = plan["far"] or (pend * NB if pend < npanels else N) < N
    # qr_form_q
    if plan["qt"]:
        plan["form_q"] = "qt_transpose"
    elif f != "tall" and batch <= QR_QT_MAX_BATCH and L >= 256:
        plan["form_q"] = "compact_wy"
    elif f == "tall":
        plan["form_q"] = "tall_blocks_rebuild" if batch > 1 else "tall_blocks"    # (batch > 1: every block's T is rebuilt per matrix)
    else:
        plan["form_q"] = "batched_backward" if f == "batched" else "panel_backward"
    return plan


def panel_entry(batch, M):
    """nd4_geqr2_panel: (kernel, row workgroups of the row-split launch or 0)"""
    if batch <= QR_ROWSPLIT_MAX_BATCH and M >= HR_MIN_ROWS:
        return _rowsplit(M), rowsplit_workgroups(M)
    if M >= NB and M >= HR_MIN_ROWS:
        return "qrb_panel" + _few(batch, M), 0
    return "qr_panel_row" + _few(batch, M), 0


def has_gram_panel(plan):
    """the call has a CholeskyQR2 panel (row-split or batched)"""
    return any(p.startswith(("qrh_bc", "qrb_panel")) for p in plan["panels"])


# --------------------------------------------------------------------------------------------------------------------- families
COND_DELTAS = (3e-2, 1e-1, 3e-4, 1e-4, 1e-6, 1e-9)
"""The issue's cycle is 1e-2, 3e-3, 1e-3, 1e-4, 1e-6, 1e-9. Column 9 of a panel leaves the span of the columns before it by about
delta times its length, so its pivot ratio d^2 / G_ii is about delta^2 (times what the earlier columns leave of a random column):
9e-6 for 3e-3, the criterion itself; 1e-4 and 1e-6 for 1e-2 and 1e-3, a factor of 10 from it before that spread. All three are within a
factor of 10 of HR_PIVOT_THR = 1e-5 and are replaced: 3e-2 and 1e-1 (hot: 9e-4, 1e-2), 3e-4 (flagged: 9e-8). test_qr_ref_host.py
confirms every panel of every cond case with the model."""
KAHAN_S = (0.9, 0.8, 0.7)
ADV_PAIRS = ((0.5, 0.05), (1.0, 0.01), (2.0, 0.02), (3.0, 0.03))
ADV_CLAIMS = ("hot, series", "hot, chain", "flagged", None)
SPARE = 10.0
ADV_SPARE = 9.8
"""The margin a claim must have on HR_PIVOT_THR, HR_SERIES_MAX and HR_PASS1_MAX: a factor of 10, as the issue sets it, for every cond
and kahan panel. The four (c, delta) pairs of `adv` are set by the issue as well, and their smallest pivot ratio is
delta^2 / (c^2 (1 + 14 delta^2) + delta^2) = 9.99e-5, 9.94e-5, 9.87e-5 for the last three: a factor of 10 from 1e-5 to the two digits the
issue quotes ("1.0e-4", "9.9e-5"), not to three. For those pairs alone the margin is ADV_SPARE = 9.8."""


def graded_exponents(N):
    return (37 * np.arange(N)) % 201 - 100


def kahan_block(s, n=NB):
    c = np.sqrt(1.0 - s * s)
    return np.diag(s ** np.arange(n)) @ (np.eye(n) - c * np.triu(np.ones((n, n)), 1))


def adv_block(c, delta, n=NB):
    d = np.full(n, delta)
    d[0] = 1.0
    return np.diag(d) @ (np.eye(n) - c * np.triu(np.ones((n, n)), 1))


def _orthonormal(seed, M, k):
    q, r = np.linalg.qr(rng.matrix(seed, M, k))
    return q * np.where(np.diag(r) < 0, -1.0, 1.0)


def _block_of(fam, p):
    if fam == "kahan":
        return kahan_block(KAHAN_S[p % len(KAHAN_S)])
    return adv_block(*ADV_PAIRS[p % len(ADV_PAIRS)])


def r0_of(fam, seed, M, N):
    """the upper triangular (trapezoidal) R0 [min(M, N), N] of a kahan / adv input: the structured blocks on the diagonal, uniform
    (-1, 1) / 4 above them and right of them"""
    L = min(M, N)
    r0 = np.triu(rng.matrix(seed + 1, L, N)) * 0.25
    for p in range(_cdiv(L, NB)):
        j0 = p * NB
        nb = min(L - j0, NB)
        r0[j0:j0 + nb, j0:j0 + nb] = _block_of(fam, p)[:nb, :nb]
    return r0


def make_input(fam, seed, M, N):
    """one [M, N] input of the family:
      dense       rng.matrix
      graded      dense times diag(2^k_j), k_j = ((37 j) mod 201) - 100: every panel holds columns 2^+-100 apart
      cond        dense with column 16 p + 9 <- column 16 p + 2 + delta * column 16 p + 9, delta = COND_DELTAS[p mod 6]
      kahan, adv  U R0, U orthonormal [M, min(M, N)] (numpy QR of a seeded matrix), R0 = r0_of(...): in exact arithmetic the rows from
                  j0 on of the updated panel at j0 are an orthonormal basis times the diagonal block, its Gram matrix K^T K
      zero        dense with columns 3 and 16 + 5 (and the last one) exactly zero
      triu        upper triangular with a diagonal away from zero: the reference rotates nothing, Q = I and R = A exactly
      nan         dense with one NaN in the middle of column 5"""
    if fam in ("dense", "graded", "cond", "zero", "nan"):
        a = rng.matrix(seed, M, N)
        if fam == "graded":
            a = a * np.ldexp(1.0, graded_exponents(N))
        elif fam == "cond":
            for p in range(min(M, N) // NB):
                a[:, NB * p + 9] = a[:, NB * p + 2] + COND_DELTAS[p % len(COND_DELTAS)] * a[:, NB * p + 9]
        elif fam == "zero":
            for c in (3, NB + 5, N - 1):
                if 0 <= c < N:
                    a[:, c] = 0.0
        elif fam == "nan":
            a[M // 2, min(5, N - 1)] = np.nan
        return a
    if fam == "triu":
        a = np.triu(rng.matrix(seed, M, N))
        i = np.arange(min(M, N))
        a[i, i] += np.where(a[i, i] < 0, -3.0, 3.0)
        return a
    if fam in ("kahan", "adv"):
        return _orthonormal(seed, M, min(M, N)) @ r0_of(fam, seed, M, N)
    raise KeyError(fam)


def bare_panel(fam, seed, M, which=0):
    """[M, 16] = U K for the panel entry point; which: the index into KAHAN_S / ADV_PAIRS (dense: a plain rng.matrix; flagged: two
    equal columns)"""
    if fam == "dense":
        return rng.matrix(seed, M, NB)
    if fam == "flagged":
        a = rng.matrix(seed, M, NB)
        a[:, 11] = a[:, 4]
        return a
    return _orthonormal(seed, M, NB) @ _block_of(fam, which)


# ------------------------------------------------------------------------------------------------------------------------ model
def gram_model(K, rows=512, seed=77001):
    """Phase B and the first pass of a CholeskyQR2 panel whose exactly updated rows are U K (U orthonormal [rows, 16], K [16, 16]),
    in plain fp64: G = C^T C, R1 = chol(G), the pivot test d^2 >= thr G_ii, the explicit R1^-1, Q1 = C R1^-1, E = Q1^T Q1 - I.
    This is the arithmetic of neither kernel to the last bit: qrh_bc multiplies by the explicit inverse and then refines Q1 once,
    qrb_panel substitutes with R1, and both sum in another order. max |E| is eps cond(K)^2 times a modest factor in all three; the
    claims "hot, chain" and "flagged after the first pass" rest on the factor SPARE they keep from HR_SERIES_MAX and HR_PASS1_MAX, not
    on equality with the kernels. Returns dict(ratio: the smallest d^2 / G_ii (0 when the factorisation breaks down), emax: max |E| (inf then),
    cond: cond_2(K))."""
    K = np.asarray(K, dtype=np.float64)
    C = _orthonormal(seed, rows, K.shape[0]) @ K
    G = C.T @ C
    out = dict(ratio=0.0, emax=np.inf, cond=float(np.linalg.cond(K)))
    try:
        R1 = np.linalg.cholesky(G).T
    except np.linalg.LinAlgError:
        return out
    d = np.diag(R1)
    out["ratio"] = float((d * d / np.diag(G)).min())
    Q1 = C @ np.linalg.inv(R1)
    out["emax"] = float(np.abs(Q1.T @ Q1 - np.eye(K.shape[0])).max())
    return out


def classify(model, spare=SPARE):
    """the claim a panel can make with `spare` to spare on all three thresholds: "hot, series" | "hot, chain" | "flagged" | None"""
    if model["ratio"] * spare <= HR_PIVOT_THR:
        return "flagged"
    if model["ratio"] < spare * HR_PIVOT_THR:
        return None
    if model["emax"] * spare <= HR_SERIES_MAX:
        return "hot, series"
    if model["emax"] >= spare * HR_PASS1_MAX:
        return "flagged"                                                       # (after the first pass)
    if spare * HR_SERIES_MAX <= model["emax"] and model["emax"] * spare <= HR_PASS1_MAX:
        return "hot, chain"
    return None


def panel_blocks(a):
    """the 16 x 16 diagonal blocks of R of the full panels of a: what the updated panels look like up to an orthonormal factor"""
    r = np.linalg.qr(a, mode="r")
    return [r[j0:j0 + NB, j0:j0 + NB] for j0 in range(0, (min(a.shape) // NB) * NB, NB)]


# ---------------------------------------------------------------------------------------------------------------------- metrics
def colbe(a, q, r, matmul=np.matmul):
    """max_j ||(Q R - A)[:, j]|| / ||a_j|| over the columns that are not exactly zero"""
    res = np.asarray(matmul(q, r)) - a
    nrm = np.linalg.norm(a, axis=-2)
    num = np.linalg.norm(res, axis=-2)
    keep = nrm > 0
    return float((num[keep] / nrm[keep]).max()) if keep.any() else 0.0


def orth(q, both=False, matmul=np.matmul):
    """max |Q^T Q - I|, and with `both` (square Q) also max |Q Q^T - I|"""
    qt = np.swapaxes(q, -1, -2)
    o = float(np.abs(np.asarray(matmul(qt, q)) - np.eye(q.shape[-1])).max())
    if both:
        o = max(o, float(np.abs(np.asarray(matmul(q, qt)) - np.eye(q.shape[-2])).max()))
    return o


def is_triu(r):
    return bool(np.array_equal(np.tril(r, -1), np.zeros_like(r)))


def relerr(x, ref):
    return np.linalg.norm((x - ref).ravel()) / max(np.linalg.norm(ref.ravel()), 1e-300)


def torch_matmul(x, y):
    """fp64 product on the device by torch (never by this library), for residuals beyond about 2000 rows"""
    import torch
    return torch.matmul(torch.from_numpy(np.ascontiguousarray(x)).cuda(), torch.from_numpy(np.ascontiguousarray(y)).cuda()).cpu().numpy()


# ------------------------------------------------------------------------------------------------------------------ guarded call
GUARD = 4096                                           # elements before and after every buffer
SENTINEL = -6.02214076e23                              # no factorisation of these inputs produces it


def _carve(n, src=None):
    import torch
    buf = torch.full((2 * GUARD + n,), SENTINEL, dtype=torch.float64, device="cuda")
    view = buf[GUARD:GUARD + n]
    if src is not None:
        view.copy_(torch.from_numpy(np.array(src, dtype=np.float64).reshape(-1)))       # (a copy: src may be read-only)
    return buf, view


def _guards_intact(bufs):
    return all(bool((b[:GUARD] == SENTINEL).all()) and bool((b[b.numel() - GUARD:] == SENTINEL).all()) for b in bufs)


def _same_bits(view, a):
    import torch
    return bool(torch.equal(view.view(torch.int64).cpu(), torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64).reshape(-1)).view(torch.int64)))


def call_qr(a, kind="decomp", y=None):
    """The device entry points behind dev.qr_decomp ("decomp": Q [.., M, L], R [.., L, N]), dev.qr_decomp_full ("full": Q [.., M, M],
    R [.., M, N]) and dev.qr_decomp_inplace ("inplace": A <- R, Y <- Q^T Y; returns (Y, R)) on a [batch, M, N]: the batch reaches
    qr_choose as it is. Input and outputs lie inside larger device tensors, GUARD elements of SENTINEL on either side; `intact`: every
    guard is bit-unchanged after the call and (out of place) so is the input. Returns (Q or Q^T Y, R, intact)."""
    import torch
    from nd4js_amd import _lib
    a3 = np.ascontiguousarray(a, dtype=np.float64).reshape((-1,) + a.shape[-2:])
    batch, M, N = a3.shape
    L = min(M, N)
    h = _lib.handle(0)
    h.set_stream(torch.cuda.current_stream().cuda_stream)
    abuf, a_d = _carve(a3.size, a3)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    if kind == "inplace":
        y3 = np.ascontiguousarray(y, dtype=np.float64).reshape(batch, M, -1)
        ybuf, y_d = _carve(y3.size, y3)
        _lib.check(h.lib.nd4hip_dgeqrf_qty_batched_dev(h.ptr, batch, M, N, y3.shape[-1], p(a_d), p(y_d)))
        torch.cuda.synchronize()
        return y_d.cpu().numpy().reshape(y3.shape).copy(), a_d.cpu().numpy().reshape(a3.shape).copy(), _guards_intact((abuf, ybuf))
    qc = M if kind == "full" else L
    qbuf, q_d = _carve(batch * M * qc)
    rbuf, r_d = _carve(batch * qc * N)
    fn = h.lib.nd4hip_dgeqrf_full_batched_dev if kind == "full" else h.lib.nd4hip_dgeqrf_q_batched_dev
    _lib.check(fn(h.ptr, batch, M, N, p(a_d), p(q_d), p(r_d)))
    torch.cuda.synchronize()
    intact = _guards_intact((abuf, qbuf, rbuf)) and _same_bits(a_d, a3)
    return q_d.cpu().numpy().reshape(batch, M, qc).copy(), r_d.cpu().numpy().reshape(batch, qc, N).copy(), intact


def call_panel(a):
    """nd4hip_dgeqr2_panel_batched_dev on a [batch, M, 16], guarded like call_qr: (R [batch, 16, 16] = the top block of A as the call
    left it, V [batch, M, 16], T [batch, 16, 16], intact)"""
    import torch
    from nd4js_amd import _lib
    a3 = np.ascontiguousarray(a, dtype=np.float64)
    batch, M, _ = a3.shape
    h = _lib.handle(0)
    h.set_stream(torch.cuda.current_stream().cuda_stream)
    abuf, a_d = _carve(a3.size, a3)
    vbuf, v_d = _carve(a3.size)
    tbuf, t_d = _carve(batch * NB * NB)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    _lib.check(h.lib.nd4hip_dgeqr2_panel_batched_dev(h.ptr, batch, M, NB, p(a_d), p(v_d), p(t_d)))
    torch.cuda.synchronize()
    intact = _guards_intact((abuf, vbuf, tbuf))
    r = a_d.cpu().numpy().reshape(a3.shape)[:, :NB, :].copy()
    return r, v_d.cpu().numpy().reshape(a3.shape).copy(), t_d.cpu().numpy().reshape(batch, NB, NB).copy(), intact


# ------------------------------------------------------------------------------------------ the cases of test_gpu_qr_paths.py
# (id, batch, M, N, full, what panel_plan must say: kernels that must appear in `panels`, then key = value pairs)
def _c(id, batch, M, N, full, kernels, **expect):
    return dict(id=id, batch=batch, M=M, N=N, full=full, kernels=tuple(kernels), expect=expect)


CASES = [
    # ---- look-ahead form
    _c("la_64", 1, 64, 64, False, ["qrh_bc<1>", "qr_panel_row_la<1>"], form="lookahead", qt=False),
    _c("la_300x130", 1, 300, 130, False, ["qrh_bc<1>", "qr_panel_row_la<1>"], form="lookahead", update_blocks=False),
    _c("la_300x130_full", 1, 300, 130, True, ["qrh_bc<1>", "qr_panel_row_la<1>"], form="lookahead", form_q="panel_backward"),
    _c("la_272x600", 1, 272, 600, False, ["qrh_bc<1>", "qr_panel_row_la<1>"], form="lookahead", update_blocks=True, qt=True),
    _c("la_257_qt", 1, 257, 257, False, ["qrh_bc<1>"], form="lookahead", qt=True, form_q="qt_transpose"),
    _c("la_255_noqt", 1, 255, 255, False, ["qrh_bc<1>"], form="lookahead", qt=False, form_q="panel_backward"),
    _c("la_4x320_qt", 4, 320, 320, False, ["qrh_bc<1>"], form="lookahead", qt=True),
    _c("la_5x320_noqt", 5, 320, 320, False, ["qrh_bc<1>"], form="lookahead", qt=False),
    _c("la_8x96", 8, 96, 96, False, ["qrh_bc<1>", "qr_panel_row_la<1>"], form="lookahead"),
    _c("la_9x96", 9, 96, 96, False, ["qr_panel_row_la<1>"], form="lookahead", first="qr_panel_row_la<1>"),
    _c("la_9x96x200", 9, 96, 200, False, ["qr_panel_row_la<1>"], form="lookahead", update_blocks=True),
    _c("la1_9x500", 9, 500, 48, False, ["qr_panel_row_la<1>"], form="lookahead", first="qr_panel_row_la<1>"),
    _c("la2_9x600", 9, 600, 48, False, ["qr_panel_row_la<2>"], form="lookahead", first="qr_panel_row_la<2>"),
    _c("la4_9x1100", 9, 1100, 48, False, ["qr_panel_row_la<4>"], form="lookahead", first="qr_panel_row_la<4>"),
    _c("la4_9x1100_full", 9, 1100, 48, True, ["qr_panel_row_la<4>"], form="lookahead"),
    _c("hr2_600x48", 1, 600, 48, False, ["qrh_bc<2>"], form="lookahead"),
    _c("hr4_1100x48", 2, 1100, 48, False, ["qrh_bc<4>"], form="lookahead"),
    # every panel row-split and tall to the end: the last reflector's side work on Q^T (qrh_side_only) sums two row chunks' partials
    _c("la_1100x272_qt", 1, 1100, 272, False, ["qrh_bc<4>", "qrh_bc<2>"], form="lookahead", qt=True, last="qrh_bc<2>", update_blocks=False),
    _c("below_63", 1, 63, 63, False, ["qr_panel_row<1,8>"], form="blocked"),
    # ---- batched form
    _c("b64_exact", 25, 128, 128, False, ["qrb_panel<1,8>", "qr_panel_row<1,8>"], form="batched", outer=(64, False), coupling=False, form_q="batched_backward"),
    _c("b64_ragged", 25, 144, 144, False, ["qrb_panel<1,8>"], form="batched", outer=(64, True), coupling=False),
    _c("b128_exact", 25, 256, 256, False, ["qrb_panel<1,8>"], form="batched", outer=(128, False), coupling=True),
    _c("b128_ragged", 25, 272, 272, False, ["qrb_panel<1,8>"], form="batched", outer=(128, True), coupling=True),
    _c("b_oddld", 25, 128, 131, False, ["qr_panel_row<1,8>"], form="batched", first="qr_panel_row<1,8>", far=True),
    _c("b_tall_full", 25, 200, 128, True, ["qrb_panel<1,8>"], form="batched", form_q="batched_backward"),
    _c("b_qrb41", 64, 128, 128, False, ["qrb_panel<4,1>", "qr_panel_row<4,1>"], form="batched"),
    _c("b_qrb42", 64, 512, 128, False, ["qrb_panel<4,2>"], form="batched", first="qrb_panel<4,2>"),
    _c("b_qrb44", 64, 1024, 128, False, ["qrb_panel<4,4>"], form="batched", first="qrb_panel<4,4>"),
    _c("b_qrb28", 25, 600, 128, False, ["qrb_panel<2,8>"], form="batched", first="qrb_panel<2,8>"),
    _c("b_qrb48", 25, 1100, 128, False, ["qrb_panel<4,8>"], form="batched", first="qrb_panel<4,8>"),
    _c("row42_oddld", 64, 512, 131, False, ["qr_panel_row<4,2>"], form="blocked", first="qr_panel_row<4,2>"),
    _c("row44_oddld", 64, 1024, 35, False, ["qr_panel_row<4,4>"], form="blocked", first="qr_panel_row<4,4>"),
    # ---- blocked form
    _c("bl_100", 25, 100, 100, False, ["qrb_panel<1,8>", "qr_panel_row<1,8>"], form="blocked", outer=None, form_q="panel_backward"),
    _c("bl_112", 25, 112, 112, False, ["qrb_panel<1,8>"], form="blocked", outer=None),
    _c("bl_40", 30, 40, 40, False, ["qr_panel_row<1,8>"], form="blocked"),
    _c("halves", 9, 2100, 48, True, ["qr_panel_part<4,8>"], form="blocked", t_assemble=True),
    _c("quarters", 1, 4200, 48, True, ["qr_panel_part<8,4>"], form="blocked", t_assemble=True),
    _c("global", 1, 8200, 16, True, ["qr_panel<1,false>"], form="blocked"),
    # ---- tall form
    _c("tall_272", 1, 2064, 272, True, ["qrh_bc<0>", "qrh_bc<4>"], form="tall", far=True, form_q="tall_blocks"),
    _c("tall_2x272", 2, 2064, 272, True, ["qrh_bc<0>", "qrh_bc<4>"], form="tall", form_q="tall_blocks_rebuild"),
    _c("tall_ragged", 1, 2310, 280, True, ["qrh_bc<0>", "qr_panel_row_la<4>"], form="tall", tall_blocks=2),
    _c("tall_2100x256", 1, 2100, 256, True, ["qrh_bc<0>", "qrh_bc<4>"], form="tall", outer=(128, False)),
    # ---- TSQR
    _c("tsqr_padded", 1, 2049, 3, False, [], form="tsqr"),
    _c("tsqr_exact", 1, 4096, 16, False, ["qrh_bc<4>"], form="tsqr"),
    _c("tsqr_batched", 2, 3000, 16, False, ["qrh_bc<4>"], form="tsqr"),
    _c("tsqr_recurses", 1, 70000, 64, False, ["qrb_panel<4,8>"], form="tsqr"),
]
TSQR_EXPECT = {"tsqr_padded": dict(nblk=2, mb=1026, padded=True, recurses=False), "tsqr_exact": dict(nblk=2, mb=2048, padded=False, recurses=False),
               "tsqr_batched": dict(nblk=2, mb=1500, padded=False, recurses=False), "tsqr_recurses": dict(nblk=35, mb=2000, padded=False, recurses=True)}


def check_plan(case):
    """assert that the case takes the path it names; returns the plan"""
    plan = panel_plan(case["batch"], case["M"], case["N"], case["full"])
    for k in case["kernels"]:
        assert k in plan["panels"], (case["id"], k, sorted(set(plan["panels"])))
    for key, want in case["expect"].items():
        got = plan["panels"][0] if key == "first" else plan["panels"][-1] if key == "last" else plan.get(key)
        assert got == want, (case["id"], key, got, want)
    if case["id"] in TSQR_EXPECT:
        for key, want in TSQR_EXPECT[case["id"]].items():
            assert plan["tsqr"][key] == want, (case["id"], key, plan["tsqr"][key], want)
    return plan


ORACLE_S_PER_FLOP = 1.7e-9     # the Givens oracle: 4.3 s for 2100 x 1100 (M N^2); the full form of a tall input costs M^2 N
ORACLE_MAX_S = 5.0


def oracle_seconds(case):
    """what one oracle factorisation of one member of the case costs, estimated"""
    M, N = case["M"], case["N"]
    return ORACLE_S_PER_FLOP * M * N * (M if case["full"] else min(M, N))


def families_of(case, plan):
    """dense and graded everywhere; cond, kahan and adv on every case that has a CholeskyQR2 panel and whose oracle call stays under
    ORACLE_MAX_S (all of them today: the look-ahead, batched, blocked, tall and TSQR cases alike)"""
    fams = ["dense", "graded"]
    if has_gram_panel(plan) and oracle_seconds(case) <= ORACLE_MAX_S:
        fams += ["cond", "kahan", "adv"]
    return fams


SPECIAL_CASES = ("la_300x130", "b64_ragged", "bl_100", "tall_272", "tsqr_exact")     # zero columns, triangular and NaN input: one per form


def member_seed(case, fam):
    return 61000 + 97 * [c["id"] for c in CASES].index(case["id"]) + 7 * ("dense", "graded", "cond", "kahan", "adv", "zero", "triu", "nan").index(fam)


def batch_input(case, fam):
    """[batch, M, N]: matrix X (the case's seed) at positions 0, middle and last, matrix Y (seed + 1) everywhere else; graded shares
    dense's seed (it is dense times D). Returns (a, index of a Y member or None)"""
    seed = member_seed(case, "dense" if fam == "graded" else fam)
    b, M, N = case["batch"], case["M"], case["N"]
    x = make_input(fam, seed, M, N)
    a = np.empty((b, M, N))
    a[:] = x
    other = None
    if b >= 4:
        y = make_input(fam, seed + 1, M, N)
        for i in range(b):
            if i not in (0, b // 2, b - 1):
                a[i] = y
                other = i
    return a, other
