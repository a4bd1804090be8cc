// Blocked Householder QR with explicit Q on row-major fp64 matrices, batched, with the reference's Givens sign convention restored
// afterwards (qr_signs.hip). Replaces src/la/qr.js:27-77 (qr_decomp_full) / :80-145 (qr_decomp); the algorithm differs (compact-WY
// Householder), the OUTPUT is the contract that is kept. DESIGN.md has the measurements and the history.
//
// This file: the drivers. qr_choose picks a form from the shape; each form takes its panels (width NB = 16) from these units:
//   QR_TSQR        row blocks as one batch, then their stacked R factors: two calls of nd4_geqrf_q_ex
//   QR_LOOKAHEAD   qr_rowsplit.hip (qrh_bc, up to QR_ROWSPLIT_MAX_BATCH matrices, while the panels are full and >= HR_MIN_ROWS tall),
//                  then qr_house.hip (qr_panel_row_la + qr_narrow_*: thread-per-row panels with look-ahead)
//   QR_TALL        qr_rowsplit.hip inside outer blocks of QR_OUTER columns, the rest of the matrix by qr_wy.hip; the tail as QR_LOOKAHEAD's
//   QR_BATCHED,    qr_block_panels picks per panel: qr_batched_panel.hip (qrb_panel: full panels of more than QR_ROWSPLIT_MAX_BATCH
//   QR_BLOCKED     matrices, m <= 2048, on the matrix cores), else qr_house.hip (qr_panel_row; qr_panel_part for 2048 < m <= 8192;
//                  qr_panel beyond). Each panel is followed by its block reflector on the outer block (qr_wy.hip: qr_vtc / qr_tw /
//                  rank-16 product), each outer block by its compact-WY update of the columns right of it
//   nd4_geqr2_panel  one panel on its own: qr_rowsplit.hip, qr_batched_panel.hip or qr_house.hip by (batch, M)
// Q is Q^T accumulated beside the panels (look-ahead), formed in one shot from the compact-WY factor, or the block reflectors applied
// backwards to the identity (qr_form_q). Declarations shared by the units: qr_internal.h.
#include "qr_rowsplit.h"
#include "dpp.h"
#include <cstdlib>
#include <cfloat>

namespace {
// ---- exact power-of-two normalisation: the reference's Givens kernel (_giv_rot.js:22-37) scales by max(|a|,|b|)
// and never overflows; Householder squares the entries. Per matrix: e = 0 if 2^-400 <= max|a| <= 2^400, else the
// exponent that brings max|a| to [1,2); the work copy is multiplied by 2^-e and R by 2^e (both exact).
__global__ __launch_bounds__(256) void qr_amax(const double* __restrict__ Am, long n_per, unsigned long long* __restrict__ amax_bits) {
  const double* A = Am + blockIdx.y * n_per;
  double mx = 0.0;
  for (long i = blockIdx.x * 256l + threadIdx.x; i < n_per; i += (long)gridDim.x * 256) { const double v = fabs(A[i]); mx = (v > mx) ? v : mx; }   // NaN ignored
  mx = nd4dpp::wave_max(mx);
  // the bit pattern of a non-negative double is monotone: an integer max is order independent (deterministic)
  if ((threadIdx.x & 63) == 0 && mx > 0.0) atomicMax(amax_bits + blockIdx.y, (unsigned long long)__double_as_longlong(mx));
}
__device__ __forceinline__ int qr_scale_exponent(unsigned long long bits) {
  const double m = __longlong_as_double((long long)bits);
  int e = 0;
  if (m > 0.0 && m < DBL_MAX * 2.0) { int ex; (void)frexp(m, &ex); if (ex > 400 || ex < -400) e = ex - 1; }
  return e;
}
__global__ __launch_bounds__(256) void qr_scale_apply(const double* __restrict__ src, double* __restrict__ dst, long n_per,
                                                       const unsigned long long* __restrict__ amax_bits, int sign) {
  const int e = sign * qr_scale_exponent(amax_bits[blockIdx.y]);
  const long i = blockIdx.x * 256l + threadIdx.x;
  if (i >= n_per) return;
  const double v = src[blockIdx.y * n_per + i];
  if (e != 0 || src != dst) dst[blockIdx.y * n_per + i] = (e == 0) ? v : ldexp(v, e);
}

int form_q_compact_wy(nd4hip_handle* h, const QrWs& ws, int batch, int M, int Lq, int npanels, double* Q, long sQ) {
  const int n = npanels * NB;                                       // == ws.ldv
  for (int m = 0; m < batch; m++)
    ND4_TRY(nd4_wy_form(h, M, n, ws.V + (long)m * ws.sV, ws.T + (long)m * ws.sT, NB, Q + (long)m * sQ, Lq));
  return 0;
}

}  // namespace

int nd4_geqrf_q(nd4hip_handle* h, int64_t batch, int64_t M, int64_t N, const double* A, double* Q, double* R) {
  return nd4_geqrf_q_ex(h, batch, M, N, A, Q, R, false);
}

// full = false: qr_decomp (qr.js:80-145): Q [M, L], R [L, N], tall input with the c >= 0 convention of :97-139.
// Q == nullptr (full = false, M <= N): R only. Q is never formed (no Q^T accumulation in the look-ahead form, no qr_form_q) and
//               the sign convention flips R's rows alone; R is bit-for-bit the R of the call with a Q, because everything that
//               touches R runs unchanged. Tall input (M > N, which includes every TSQR shape) keeps the Q-forming path on a workspace
//               Q: its c >= 0 convention is decided from Q's leading L x L block (nd4_givens_signs, lu_rule).
// full = true : qr_decomp_full (qr.js:27-77): Q [M, M], R [M, N] with the Givens-full convention for every shape
//               (R_jj >= 0 wherever something was eliminated; det Q = +1 fixes the last row when M <= N). For M > N the
//               trailing M-N columns of Q are an orthonormal completion (not unique; the reference's is the one its
//               rotation order happens to produce) and rows N.. of R are zero.
// Tall-skinny input (M > 2048 rows, M >= 4 N): TSQR. The rows are cut into blocks of <= 2048 (what the register-resident
// panel kernel holds), all blocks are factorised in ONE batched call, the stacked R factors (nblk N x N) are factorised
// again (recursively), and Q = blockwise Q1_b Q2_b is one strided-batched GEMM. A QR factorisation is unique up to the signs
// of R's rows, so the reference's convention is imposed on the final pair by nd4_givens_signs, whatever the levels did.
// Without it a 65536 x 32 panel would run on one workgroup through the global-memory fallback (31 ms instead of < 1 ms).
static int geqrf_tsqr(nd4hip_handle* h, int batch, int M, int N, const double* A, double* Q, double* R) {
  const int nblk = (M + 2047) / 2048;
  int mb = (M + nblk - 1) / nblk;
  mb = (mb + 1) & ~1;
  const long Mp = (long)nblk * mb;
  Nd4WsScope scope(h);
  void* p = nullptr;
  const size_t nAp = (size_t)batch * Mp * N, nR1 = (size_t)batch * nblk * N * N;
  ND4_TRY(nd4_ws_alloc(h, sizeof(double) * (2 * nAp + 2 * nR1 + (size_t)batch * Mp * N) + sizeof(int) * ((size_t)batch * N + 2) + 64, &p));
  double* Ap = static_cast<double*>(p);
  double* Q1 = Ap + nAp;
  double* R1 = Q1 + nAp;                                               // per matrix: the nblk R factors stacked = (nblk N) x N
  double* Q2 = R1 + nR1;
  double* Qp = Q2 + nR1;
  int* flips = reinterpret_cast<int*>(Qp + (size_t)batch * Mp * N);
  if (Mp != M) ND4_HIP(hipMemsetAsync(Ap, 0, sizeof(double) * nAp, h->stream));
  ND4_TRY(nd4_copy_matrix(h, M, N, A, N, Ap, N, batch, (long)M * N, Mp * N));
  ND4_TRY(nd4_geqrf_q_ex(h, (int64_t)batch * nblk, mb, N, Ap, Q1, R1, false));
  ND4_TRY(nd4_geqrf_q_ex(h, batch, (int64_t)nblk * N, N, R1, Q2, R, false));
  double* Qdst = (Mp == M) ? Q : Qp;
  ND4_TRY(nd4_gemm(h, false, false, mb, N, N, 1.0, Q1, N, (long)mb * N, Q2, N, (long)N * N, 0.0, Qdst, N, (long)mb * N, (int64_t)batch * nblk));
  if (Mp != M) ND4_TRY(nd4_copy_matrix(h, M, N, Qp, N, Q, N, batch, Mp * N, (long)M * N));
  return nd4_givens_signs(h, batch, M, N, N, true, Q, N, (long)M * N, R, N, (long)N * N, nullptr, 0, flips);
}

// ---- the strategies of nd4_geqrf_q_ex, chosen once from the shape ----
// tests/qr_common.py restates these constants, qr_choose and the drivers below (form(), panel_plan(), panel_entry()): every case of
// tests/test_gpu_qr_paths.py asserts through them which kernels it runs. Change a constant or a branch here and change it there.
constexpr int QR_LA_MAX_BATCH = 24;        // look-ahead form up to this many matrices; a batch that fills the chip takes the plain sequence
                                           // with the matrix-core panels (1024 x 512^2 48.6 -> 43.7 ms; 8 matrices 1.97 against 2.53 ms, 32: 2.91 against 2.87)
constexpr int QR_QT_MAX_BATCH = 4;         // Q^T accumulated (look-ahead) or Q formed in one shot (compact WY) up to this many matrices
constexpr int QR_TALL_MAX_ROWS = 16384;    // the tall row-split form for 2048 < M <= this
constexpr int QR_OUTER = 128;              // columns per outer block of the two-level forms ...
constexpr int QR_BATCH_OUTER_NARROW = 64;  // ... and of the batched form below 16 panels (1024 x 512^2: 43.8 one level, 30.5 (64), 23.6 ms (128))

enum QrForm {
  QR_TSQR,        // tall-skinny: row blocks factorised as one batch, then their stacked R factors (geqrf_tsqr)
  QR_LOOKAHEAD,   // 64 <= M <= 2048, few matrices: row-split panels while they are tall enough, then thread-per-row panels with look-ahead
  QR_TALL,        // 2048 < M <= QR_TALL_MAX_ROWS, few matrices: row-split panels inside outer blocks, block reflectors on the rest
  QR_BATCHED,     // M <= 2048, batches beyond the look-ahead form: two levels, every step batched
  QR_BLOCKED,     // the rest: one level, or two with a per-matrix far update when M > 2048
};

static int qr_batch_outer(int npanels) { return npanels >= 16 ? QR_OUTER : QR_BATCH_OUTER_NARROW; }

static QrForm qr_choose(int batch, int M, int N, bool full) {
  const int L = M < N ? M : N, npanels = (L + NB - 1) / NB;
  const long nblk = (M + 2047) / 2048;
  // TSQR: every block needs >= N rows, and the stacked R (nblk N rows) must either fit the fast panel kernel directly or be
  // at most half as tall as the input (so that the recursion terminates quickly)
  if (!full && M > 2048 && N <= 2048 && (long)batch * nblk <= 32768 && M / nblk >= N &&
      (nblk * N <= 2048 || 2 * nblk * N <= (long)M))
    return QR_TSQR;
  if (M <= 2048 && M >= 64 && batch <= QR_LA_MAX_BATCH) return QR_LOOKAHEAD;
  // (a ragged last panel must fit the thread-per-row kernel)
  if (batch <= QR_ROWSPLIT_MAX_BATCH && M > 2048 && M <= QR_TALL_MAX_ROWS && L >= 256 && (L % NB == 0 || M - (L / NB) * NB <= 2048))
    return QR_TALL;
  if (M <= 2048 && batch > 1 && L % NB == 0 && npanels >= 2 * (qr_batch_outer(npanels) / NB)) return QR_BATCHED;
  return QR_BLOCKED;
}

// one factorisation in flight: shapes, the working matrix W (R's buffer when M <= N, a workspace copy when tall), the workspace slices
struct QrJob {
  nd4hip_handle* h; QrForm form; int batch, M, N, L, npanels, Lq;
  double* W; long ld, sW;
  QrWs ws;
  double* QT; long sQT;                    // the look-ahead form's Q^T accumulator (nullptr: none)
  QrhHost hr; bool use_hr;                 // row-split panels
  // two-level forms: the outer blocks' compact-WY factors (bT, kept for Q) and the far update's scratch (bG, bTmp: wy_build_T; bX, bW)
  double *bT = nullptr, *bG = nullptr, *bTmp = nullptr, *bX = nullptr, *bW = nullptr;
  long bsT = 0, bsX = 0;                   // QR_BATCHED: per matrix
  int ppb = 0, first_low = 0;              // panels per outer block; QR_TALL: first panel of the one-level part
};

// matrix mt: the nblk reflector columns from J on — their factor Tb from the panels' factors first (wy_build_T) unless Tb holds it
// already — applied to the n columns of C (rows [J, M))
static int wy_block_update(QrJob& j, int mt, int J, int nblk, bool build, double* Tb, bool transT, double* C, long ldc, int n) {
  const QrWs& ws = j.ws;
  const int mJ = j.M - J;
  const double* Vb = ws.V + (long)mt * ws.sV + (long)J * ws.ldv + J;
  if (build) ND4_TRY(nd4_qr_wy_build_T(j.h, mJ, nblk, Vb, ws.ldv, ws.T + (long)mt * ws.sT + (long)(J / NB) * NB * NB, NB, Tb, j.bG, j.bTmp));
  return nd4_qr_block_update(j.h, transT, mJ, n, nblk, Vb, ws.ldv, 0, Tb, 0, C, ldc, 0, j.bX, j.bW, 0, 1);
}

// Thread-per-row panels from pnl on with look-ahead: panel p shares its launch with the update of the columns behind it (and of Q^T)
// by reflector p-1; only the 16 columns of panel p+1 are updated between two panels. See qr_colblock_update.
static int qr_rows_lookahead(QrJob& j, int pnl) {
  nd4hip_handle* h = j.h;
  const QrWs& ws = j.ws;
  const int M = j.M, N = j.N, L = j.L, npanels = j.npanels, batch = j.batch;
  double* W = j.W; double* QT = j.QT;
  const long ld = j.ld, sW = j.sW, sQT = j.sQT;
  const int nq = QT ? (M + NB - 1) / NB : 0;
  int pj0 = -1;                                              // first row/column of the previous panel
  for (; pnl < npanels; pnl++) {
    const int j0 = pnl * NB, nb = L - j0 < NB ? L - j0 : NB;
    // reflector p-1 has reached the 16 columns behind its own panel (the narrow launch: [pj0 + NB, pj0 + 2 NB), which contain this
    // panel); the columns from there on still lack it
    const int wide0 = pj0 + 2 * NB, nwide = (pj0 >= 0 && wide0 < N) ? (N - wide0 + NB - 1) / NB : 0;
    const int wc0 = j0 + nb;
    nd4_qr_panel_row_la(h, batch, 1 + nwide + (pj0 >= 0 ? nq : 0), W, M, N, ld, sW, ws.V, ws.ldv, ws.sV, ws.T, ws.sT, ws.taus, ws.sTau, j0, nb,
                        pj0 < 0 ? 0 : pj0, wide0, nwide, QT, sQT);
    if (wc0 < N) {                                           // the next panel's columns (or the first block right of the last panel)
      nd4_qr_narrow_x(h, batch, W, M, N, ld, sW, ws.V, ws.ldv, ws.sV, j0, wc0, ws.Wp, ws.sWb);
      nd4_qr_narrow_apply(h, batch, W, M, N, ld, sW, ws.V, ws.ldv, ws.sV, ws.T, ws.sT, j0, wc0, ws.Wp, ws.sWb, 0);
    }
    pj0 = j0;
  }
  if (pj0 >= 0) {   // the last panel was a thread-per-row one; wide input: its reflector on the columns right of the block the narrow launch has done
    const int j0 = (npanels - 1) * NB, nb = L - j0 < NB ? L - j0 : NB, wc0 = j0 + nb + NB;
    if (wc0 < N) nd4_qr_update_blocks(h, batch, (N - wc0 + NB - 1) / NB, W, M, N, ld, sW, ws.V, ws.ldv, ws.sV, ws.T, ws.sT, j0, wc0);
    if (QT) nd4_qr_update_blocks(h, batch, nq, QT, M, M, (long)M, sQT, ws.V, ws.ldv, ws.sV, ws.T, ws.sT, (npanels - 1) * NB, 0);
  }
  ND4_HIP(hipGetLastError());
  return 0;
}

// QR_LOOKAHEAD: row-split panels while they are full and tall enough (one launch each, the previous reflector's side work riding
// along on the trailing columns of W, then Q^T), then the thread-per-row look-ahead sequence
static int qr_factor_lookahead(QrJob& j) {
  if (j.QT) ND4_TRY(nd4_set_identity(j.h, j.M, j.M, j.QT, j.M, j.batch, j.sQT));
  int pnl = 0;
  if (j.use_hr) {
    for (; pnl < j.npanels; pnl++) {
      const int j0 = pnl * NB, nb = j.L - j0 < NB ? j.L - j0 : NB, m = j.M - j0;
      if (nb < NB || m < HR_MIN_ROWS) break;
      ND4_TRY(j.hr.panel(j0, j.N, j.QT != nullptr, false));
    }
    ND4_TRY(j.hr.finish(j.N, j.QT != nullptr, true));       // nothing pending afterwards: the remaining panels start afresh
    ND4_TRY(j.hr.dump_stamps());
  }
  return qr_rows_lookahead(j, pnl);
}

// QR_TALL (round 3). The split register panels (two 8-column halves / four 4-column quarters per 16-column slot, each followed by its
// own block-reflector launches and a Gram product) took ~165 us per slot, and every slot read-modify-wrote the whole trailing matrix.
// Now: outer blocks of 128 columns; inside a block the row-split panels of qrh_* (no height limit: the rows are cut into 512-row
// workgroups) with the previous reflector riding along on the block's own columns only; after the block its compact-WY factor T
// (128 x 128: the panels' 16 x 16 factors on the diagonal, T12 = -T1 (V1^T V2) T2 level by level from one Gram matrix) takes all 128
// reflectors to the columns right of it at once on the tiled MFMA kernel: X = V^T C, W = T^T X, C -= V W (K = 128). Once the panels
// fit the register kernel (m <= 2048) the rest is factorised with one level, as a 2048-row problem. Q is formed afterwards by applying
// the same block reflectors backwards (qr_form_q: 4/3 M^3 flop instead of the 6 M n^2 of the one-shot formation).
static int qr_factor_tall(QrJob& j) {
  const int M = j.M, N = j.N, L = j.L, npanels = j.npanels;
  const int ppb = QR_OUTER / NB;
  const size_t nbo = QR_OUTER, nblocks = (size_t)(npanels + ppb - 1) / ppb;
  void* q = nullptr;
  const int ncq = N > j.Lq ? N : j.Lq;
  ND4_TRY(nd4_ws_alloc(j.h, sizeof(double) * (nblocks * nbo * nbo + nbo * nbo * 2 + nbo * nbo / 2 + 16 + 2 * nbo * (size_t)ncq + 64), &q));
  j.bT = static_cast<double*>(q); j.bG = j.bT + nblocks * nbo * nbo; j.bTmp = j.bG + nbo * nbo;
  j.bX = j.bTmp + nbo * nbo / 2 + 16; j.bW = j.bX + nbo * (size_t)ncq; j.ppb = ppb;
  int pnl = 0;
  j.first_low = npanels;
  for (int P0 = 0; P0 < npanels && M - P0 * NB > 2048; P0 += ppb) {
    const int pend = P0 + ppb < npanels ? P0 + ppb : npanels;
    const int bend = pend < npanels ? pend * NB : N;
    // a ragged last panel (L no multiple of 16) takes the thread-per-row kernel: its block goes to the one-level part as a whole.
    // (Stopping at the ragged panel itself left the block's earlier panels factorised, with a reflector pending, and the one-level
    // part factorised them a second time: 2310 x 280, full.)
    if (pend == npanels && L % NB != 0) break;
    for (pnl = P0; pnl < pend; pnl++) ND4_TRY(j.hr.panel(pnl * NB, bend, false, pnl == pend - 1));
    ND4_TRY(j.hr.finish(bend, false, false));                 // the block's last reflector has no column of the block left to reach
    j.first_low = pend;
    if (bend < N) {
      const int J = P0 * NB, nblk = (pend - P0) * NB;
      for (int mt = 0; mt < j.batch; mt++)
        ND4_TRY(wy_block_update(j, mt, J, nblk, true, j.bT + (size_t)(P0 / ppb) * nbo * nbo, true, j.W + (long)mt * j.sW + (long)J * j.ld + bend, j.ld, N - bend));
    }
  }
  // the rest as one level: multi-workgroup panels with all remaining columns as side work, then the short tail panels
  for (pnl = j.first_low; pnl < npanels; pnl++) {
    const int j0 = pnl * NB, nb = L - j0 < NB ? L - j0 : NB, m = M - j0;
    if (nb < NB || m < HR_MIN_ROWS) break;
    ND4_TRY(j.hr.panel(j0, N, false, false));
  }
  ND4_TRY(j.hr.finish(N, false, true));
  ND4_TRY(qr_rows_lookahead(j, pnl));
  return j.hr.dump_stamps();
}

// the panels [P0, pend) of an outer block, each followed by its reflector on the block's columns up to bend
static int qr_block_panels(QrJob& j, int P0, int pend, int bend) {
  nd4hip_handle* h = j.h;
  const QrWs& ws = j.ws;
  const int M = j.M, L = j.L, batch = j.batch;
  double* W = j.W;
  const long ld = j.ld, sW = j.sW;
  for (int pnl = P0; pnl < pend; pnl++) {
    const int j0 = pnl * NB, nb = L - j0 < NB ? L - j0 : NB, m = M - j0;
    if (m > 2048 && m <= 8192) {
      // the 16-column slot in parts on 1024 threads: two 8-column halves (m <= 4096: 4 rows x 8 columns per lane) or four
      // 4-column quarters (m <= 8192: 8 rows x 4 columns per lane). After each part its reflectors are applied to the rest
      // of the slot (the live T holds only that part's block); at the end T is assembled from the side blocks and V^T V.
      const int w = m <= 4096 ? 8 : 4;
      for (int c = 0; c < nb; c += w) {
        const int nbp = nb - c < w ? nb - c : w;
        nd4_qr_panel_part(h, batch, w, W, M, ld, sW, ws.V, ws.ldv, ws.sV, ws.T, ws.Tside, ws.sT, ws.taus, ws.sTau, j0 + c, nbp);
        ND4_HIP(hipGetLastError());
        if (c + w < nb)
          ND4_TRY(nd4_qr_apply_block_reflector(h, ws, batch, M, j0, pnl, /*trans=*/1, W + (long)j0 * ld + j0 + c + w, ld, sW, nb - c - w));
      }
      if (nb > w) {
        const double* Vs = ws.V + (long)j0 * ws.ldv + j0;
        ND4_TRY(nd4_gemm(h, true, false, NB, NB, m, 1.0, Vs, ws.ldv, ws.sV, Vs, ws.ldv, ws.sV, 0.0, ws.W2, NB, ws.sW2, batch));
        nd4_qr_t_assemble(h, batch, ws.T, ws.Tside, ws.sT, pnl, ws.W2, ws.sW2, w);
        ND4_HIP(hipGetLastError());
      }
    } else
    if (m <= 2048) {
      // batches of full panels: one workgroup per panel on the matrix cores (qr_batched_panel.hip: V = Q - [S; 0], full T, like the
      // row-split panels of one matrix); short / narrow / odd-stride panels keep the thread-per-row Householder kernel
      if (batch > QR_ROWSPLIT_MAX_BATCH && nb == NB && m >= HR_MIN_ROWS && (ld & 1) == 0 && (ws.ldv & 1) == 0)
        nd4_qr_panel_mfma(h, batch, W, M, m, ld, sW, ws.V, ws.ldv, ws.sV, ws.T, ws.sT, ws.taus, ws.sTau, j0);
      else
        nd4_qr_panel_rows(h, batch, W, M, m, ld, sW, ws.V, ws.ldv, ws.sV, ws.T, ws.sT, ws.taus, ws.sTau, j0, nb);
    } else                nd4_qr_panel_global(h, batch, W, M, ld, sW, ws.V, ws.ldv, ws.sV, ws.T, ws.sT, ws.taus, ws.sTau, j0, nb);
    ND4_HIP(hipGetLastError());
    // trailing columns of the outer block: C <- H^T C = (I - V T^T V^T) C
    ND4_TRY(nd4_qr_apply_block_reflector(h, ws, batch, M, j0, pnl, /*trans=*/1, W + (long)j0 * ld + j0 + nb, ld, sW, bend - j0 - nb));
  }
  return 0;
}

// QR_BATCHED (round 4): two levels with outer blocks of 128 columns (64 below 256 columns), everything batched — G = Vb^T Vb and the
// three products of the far update as strided GEMMs over the batch, the block's T by one small workgroup per matrix (wy_t_small) — and
// Q formed backwards block by block from the stored T's: the rank-16 updates of every panel over the whole trailing matrix (56 % of
// 1024 x 512^2) become rank-128 updates, an eighth of the traffic.
static int qr_factor_batched(QrJob& j) {
  nd4hip_handle* h = j.h;
  const QrWs& ws = j.ws;
  const int M = j.M, N = j.N, npanels = j.npanels, batch = j.batch;
  const int ppb = qr_batch_outer(npanels) / NB;
  const size_t nbo = (size_t)ppb * NB, nblocks = (size_t)(npanels + ppb - 1) / ppb, wcols = (size_t)(N > j.Lq ? N : j.Lq);
  void* q = nullptr;
  ND4_TRY(nd4_ws_alloc(h, sizeof(double) * (size_t)batch * (nblocks * nbo * nbo + nbo * nbo + 2 * nbo * wcols) + 64, &q));
  j.bT = static_cast<double*>(q); j.bG = j.bT + (size_t)batch * nblocks * nbo * nbo; j.bX = j.bG + (size_t)batch * nbo * nbo; j.bW = j.bX + (size_t)batch * nbo * wcols;
  j.ppb = ppb; j.bsT = (long)(nblocks * nbo * nbo); j.bsX = (long)(nbo * wcols);
  ND4_HIP(hipMemsetAsync(j.bT, 0, sizeof(double) * (size_t)batch * nblocks * nbo * nbo, h->stream));   // (the blocks below the diagonal 64 x 64 blocks stay zero)
  const long nbo2 = (long)nbo * nbo;
  for (int P0 = 0; P0 < npanels; P0 += ppb) {
    const int pend = P0 + ppb < npanels ? P0 + ppb : npanels;
    const int bend = pend < npanels ? pend * NB : N;                              // the block's reflectors reach the columns up to here at once
    ND4_TRY(qr_block_panels(j, P0, pend, bend));
    // the block's T for every member; its reflectors on everything right of it
    const int J = P0 * NB, nblk = (pend - P0) * NB, mJ = M - J, far = N - bend;
    const double* Vb = ws.V + (long)J * ws.ldv + J;
    double* Tb = j.bT + (long)(P0 / ppb) * nbo2;
    ND4_TRY(nd4_gemm(h, true, false, nblk, nblk, mJ, 1.0, Vb, ws.ldv, ws.sV, Vb, ws.ldv, ws.sV, 0.0, j.bG, nblk, nbo2, batch));
    {
      // T of the block: 64-column halves in LDS (wy_t_small), the coupling of the two halves of a 128-column block by two products
      static_assert(QR_OUTER <= 2 * 64 && QR_BATCH_OUTER_NARROW <= 64, "a block is at most two halves of the 64 columns wy_t_small holds");
      const int n1 = nblk < 64 ? nblk : 64, n2 = nblk - n1;
      nd4_qr_wy_t_small(h, batch, ws.T + (long)P0 * NB * NB, ws.sT, j.bG, nblk, nbo2, Tb, nblk, j.bsT, n1);
      if (n2 > 0) {
        nd4_qr_wy_t_small(h, batch, ws.T + (long)(P0 + n1 / NB) * NB * NB, ws.sT, j.bG + (long)n1 * nblk + n1, nblk, nbo2, Tb + (long)n1 * nblk + n1, nblk, j.bsT, n2);
        ND4_TRY(nd4_gemm(h, false, false, n1, n2, n2, 1.0, j.bG + n1, nblk, nbo2, Tb + (long)n1 * nblk + n1, nblk, j.bsT, 0.0, j.bX, n2, j.bsX, batch));
        ND4_TRY(nd4_gemm(h, false, false, n1, n2, n1, -1.0, Tb, nblk, j.bsT, j.bX, n2, j.bsX, 0.0, Tb + n1, nblk, j.bsT, batch));
      }
      ND4_HIP(hipGetLastError());
    }
    if (far > 0)
      ND4_TRY(nd4_qr_block_update(h, true, mJ, far, nblk, Vb, ws.ldv, ws.sV, Tb, j.bsT, j.W + (long)J * j.ld + bend, j.ld, j.sW, j.bX, j.bW, j.bsX, batch));
  }
  return 0;
}

// QR_BLOCKED. M > 2048 (round 3): every panel used to read-modify-write the whole trailing matrix with a K = 16 update (qr_vtc / qr_tw /
// rank-16 product). Now the panels of an outer block of 128 columns apply their reflectors to the block's own columns only; then the
// block's compact-WY factor T (128 x 128: the panels' factors on the diagonal, T12 = -T1 (V1^T V2) T2 level by level from ONE Gram
// matrix, the routine Q is formed with) takes all 128 reflectors to the rest at once on the tiled MFMA kernel: X = V^T C, W = T^T X,
// C -= V W (K = 128). M <= 2048: one level.
static int qr_factor_blocked(QrJob& j) {
  const int M = j.M, N = j.N, npanels = j.npanels;
  const int ppb = M > 2048 ? QR_OUTER / NB : npanels;                             // panels per outer block
  if (ppb < npanels) {
    const size_t nbo = (size_t)ppb * NB;
    void* q = nullptr;
    ND4_TRY(nd4_ws_alloc(j.h, sizeof(double) * (nbo * nbo * 2 + nbo * nbo / 2 + 16 + 2 * nbo * (size_t)N + 64), &q));
    j.bT = static_cast<double*>(q); j.bG = j.bT + nbo * nbo; j.bTmp = j.bG + nbo * nbo; j.bX = j.bTmp + nbo * nbo / 2 + 16; j.bW = j.bX + nbo * (size_t)N;
  }
  for (int P0 = 0; P0 < npanels; P0 += ppb) {
    const int pend = P0 + ppb < npanels ? P0 + ppb : npanels;
    const int bend = pend < npanels ? pend * NB : N;                              // the block's reflectors reach the columns up to here at once
    ND4_TRY(qr_block_panels(j, P0, pend, bend));
    if (bend < N) {                                                               // the block's 128 reflectors on everything right of it
      const int J = P0 * NB, nblk = (pend - P0) * NB;
      for (int mt = 0; mt < j.batch; mt++)
        ND4_TRY(wy_block_update(j, mt, J, nblk, true, j.bT, true, j.W + (long)mt * j.sW + (long)J * j.ld + bend, j.ld, N - bend));
    }
  }
  return 0;
}

// Q = H_0 H_1 ... H_{p-1} [I; 0]
static int qr_form_q(QrJob& j, double* Q) {
  nd4hip_handle* h = j.h;
  const QrWs& ws = j.ws;
  const int M = j.M, Lq = j.Lq, npanels = j.npanels, batch = j.batch;
  const long sQ = (long)M * Lq;
  if (j.QT) return nd4_transpose(h, Lq, M, j.QT, M, Q, Lq, batch, j.sQT, sQ);          // Q = (first Lq rows of Q^T)^T
  if (j.form != QR_TALL && batch <= QR_QT_MAX_BATCH && j.L >= 256) return form_q_compact_wy(h, ws, batch, M, Lq, npanels, Q, sQ);
  ND4_TRY(nd4_set_identity(h, M, Lq, Q, Lq, batch, sQ));
  if (j.form == QR_TALL) {
    // the block reflectors of 128 columns applied backwards to E (the blocks of the one-level part get their T now; those of the tall
    // part of a single matrix still hold theirs)
    const int ncolsV = npanels * NB, nbo = QR_OUTER, nblocks = (npanels + j.ppb - 1) / j.ppb;
    for (int mt = 0; mt < batch; mt++) {
      for (int b = nblocks - 1; b >= 0; b--) {
        const int J = b * nbo, nblk = ncolsV - J < nbo ? ncolsV - J : nbo, nq2 = Lq - J;
        if (nq2 <= 0) continue;
        ND4_TRY(wy_block_update(j, mt, J, nblk, b * j.ppb >= j.first_low || batch > 1, j.bT + (size_t)b * nbo * nbo, false,
                                Q + (long)mt * sQ + (long)J * Lq + J, Lq, nq2));
      }
    }
  } else if (j.form == QR_BATCHED) {
    // Q <- (I - Vb Tb Vb^T) Q block by block, backwards, with the blocks' stored factors
    const long nbo2 = (long)j.ppb * NB * j.ppb * NB;
    for (int P0 = ((npanels - 1) / j.ppb) * j.ppb; P0 >= 0; P0 -= j.ppb) {
      const int pend = P0 + j.ppb < npanels ? P0 + j.ppb : npanels;
      const int J = P0 * NB, nblk = (pend - P0) * NB, mJ = M - J, nq2 = Lq - J;
      if (nq2 <= 0) continue;
      ND4_TRY(nd4_qr_block_update(h, false, mJ, nq2, nblk, ws.V + (long)J * ws.ldv + J, ws.ldv, ws.sV, j.bT + (long)(P0 / j.ppb) * nbo2, j.bsT,
                           Q + (long)J * Lq + J, Lq, sQ, j.bX, j.bW, j.bsX, batch));
    }
  } else {
    for (int pnl = npanels - 1; pnl >= 0; pnl--) {
      const int j0 = pnl * NB;
      ND4_TRY(nd4_qr_apply_block_reflector(h, ws, batch, M, j0, pnl, /*trans=*/0, Q + (long)j0 * Lq + j0, Lq, sQ, Lq - j0));
    }
  }
  return 0;
}

int nd4_geqrf_q_ex(nd4hip_handle* h, int64_t batch64, int64_t M64, int64_t N64, const double* A, double* Q, double* R, bool full) {
  ND4_CHECK_ARG(M64 < (1ll << 30) && N64 < (1ll << 30) && batch64 < 65536, "nd4_geqrf_q: extent out of range");
  const int M = (int)M64, N = (int)N64, batch = (int)batch64;
  ND4_CHECK_ARG(Q != nullptr || !full, "nd4_geqrf_q: the R-only mode is qr_decomp's (full = false)");
  if (!Q && M > N) {                                        // R only, tall: the sign rule reads Q (see above)
    Nd4WsScope scope(h);
    void* q = nullptr;
    ND4_TRY(nd4_ws_alloc(h, sizeof(double) * (size_t)batch * M * N, &q));
    return nd4_geqrf_q_ex(h, batch, M, N, A, static_cast<double*>(q), R, false);
  }
  const QrForm form = qr_choose(batch, M, N, full);
  if (form == QR_TSQR) return geqrf_tsqr(h, batch, M, N, A, Q, R);
  const int L = M < N ? M : N;
  const int npanels = (L + NB - 1) / NB;
  const bool tall = M > N;
  const int Lq = (full && tall) ? M : L;                    // columns of Q
  const int Lr = (full && tall) ? M : L;                    // rows of R

  // ---- workspace carve-up (all per-matrix blocks are multiples of 2 doubles -> 16-B aligned) ----
  QrJob j;
  j.h = h; j.form = form; j.batch = batch; j.M = M; j.N = N; j.L = L; j.npanels = npanels; j.Lq = Lq;
  QrWs& ws = j.ws;
  ws.ldv = ((L + NB - 1) / NB) * NB;                        // Vall: M x ldv, zero above each panel
  ws.sV = (long)M * ws.ldv;
  ws.sT = (long)npanels * NB * NB;
  ws.sTau = ws.ldv;
  const int ncols = (N > Lq ? N : Lq);
  ws.ldw = ((ncols + 1) / 2) * 2;
  ws.nchunks_max = (M + VTC_ROWS - 1) / VTC_ROWS;
  ws.sChunk = (long)NB * ws.ldw;
  ws.sWb = ws.sChunk * ws.nchunks_max;
  ws.sW2 = ws.sChunk;
  const long sWork = tall ? (long)M * N : 0;
  const bool use_qt = Q && form == QR_LOOKAHEAD && batch <= QR_QT_MAX_BATCH && L >= 256;   // Q^T accumulated in the shadow of the panels
  j.use_hr = (form == QR_LOOKAHEAD && batch <= QR_ROWSPLIT_MAX_BATCH) || form == QR_TALL;   // multi-workgroup panels (CholeskyQR2 + compact orthogonal completion)
  j.sQT = use_qt ? (long)M * M : 0;
  const int hr_parts = (M + NB + 511) / 512 + 1;
  const long sXch = j.use_hr ? (long)hr_parts * QX_ROW_SLOT : 0;                           // QX_ROW_SLOT tagged words per row workgroup (qrh_bc)
  const long hr_rcs = (M + 511) / 512;
  const long sXs = j.use_hr ? ((N + NB - 1) / NB + (use_qt ? (M + NB - 1) / NB : 0)) * hr_rcs * 256 : 0;   // side work: [column block][row chunk][256]
  const long sXsx = 2 * sXs;                                 // fused side work: 512 tagged words per (column block, row chunk)
  size_t doubles = (size_t)batch * (ws.sV + 2 * ws.sT + ws.sTau + ws.sWb + ws.sW2 + sWork + j.sQT + sXch + sXs + sXsx);
  size_t bytes = doubles * sizeof(double) + ((size_t)batch * L + 2) * sizeof(int) + (size_t)batch * 8 + (size_t)batch * sizeof(int) + 64;
  void* p = nullptr;
  Nd4WsScope scope(h);
  ND4_TRY(nd4_ws_alloc(h, bytes, &p));
  double* d = static_cast<double*>(p);
  ws.V = d; d += (size_t)batch * ws.sV;
  ws.T = d; d += (size_t)batch * ws.sT;
  ws.Tside = d; d += (size_t)batch * ws.sT;                 // diagonal blocks of slots factorised in parts (tall panels)
  ws.taus = d; d += (size_t)batch * ws.sTau;
  ws.Wp = d; d += (size_t)batch * ws.sWb;
  ws.W2 = d; d += (size_t)batch * ws.sW2;
  ws.work = tall ? d : nullptr; d += (size_t)batch * sWork;
  j.QT = use_qt ? d : nullptr; d += (size_t)batch * j.sQT;
  unsigned long long* hrXch = reinterpret_cast<unsigned long long*>(d); d += (size_t)batch * sXch;
  double* hrXs = d; d += (size_t)batch * sXs;
  unsigned long long* hrXsx = reinterpret_cast<unsigned long long*>(d); d += (size_t)batch * sXsx;
  ws.flips = reinterpret_cast<int*>(d);

  // working matrix: R's buffer when it has A's shape (M <= N), a workspace copy when tall
  j.W = tall ? ws.work : R;
  j.ld = N; j.sW = (long)M * N;
  double* W = j.W;
  const long sW = j.sW;
  unsigned long long* exps = reinterpret_cast<unsigned long long*>(ws.flips + (((size_t)batch * L + 1) & ~size_t(1)));   // max|a| bits per matrix
  int* hrFlag = reinterpret_cast<int*>(exps + batch);
  ND4_HIP(hipMemsetAsync(exps, 0, sizeof(unsigned long long) * batch, h->stream));
  {
    long nblk = (sW + 256 * 16 - 1) / (256 * 16); if (nblk > 2048) nblk = 2048;
    hipLaunchKernelGGL(qr_amax, dim3((unsigned)nblk, (unsigned)batch), dim3(256), 0, h->stream, A, sW, exps);
  }
  hipLaunchKernelGGL(qr_scale_apply, dim3((unsigned)((sW + 255) / 256), (unsigned)batch), dim3(256), 0, h->stream, A, W, sW, exps, -1);
  ND4_HIP(hipMemsetAsync(ws.V, 0, sizeof(double) * (size_t)batch * ws.sV, h->stream));
  if (M > 2048) ND4_HIP(hipMemsetAsync(ws.Tside, 0, sizeof(double) * (size_t)batch * ws.sT, h->stream));
  if (j.use_hr) {
    ND4_TRY(j.hr.init(h, batch, W, M, N, j.ld, sW, ws.V, ws.ldv, ws.sV, ws.T, ws.sT, ws.taus, ws.sTau, hrFlag, hrXch, sXch,
                      ws.Wp, ws.sWb, j.QT, j.sQT, hrXs, sXs, hrXsx, sXsx, (int)hr_rcs));
    static const bool want_stamps = [] { const char* e = getenv("ND4HIP_QR_STAMPS"); return e && *e && *e != '0'; }();
    QrhP& P = j.hr.P;
    if (want_stamps) { ND4_HIP(hipMalloc(&P.stamps, sizeof(long long) * 8 * 3 * (npanels + 1))); ND4_HIP(hipMemset(P.stamps, 0, sizeof(long long) * 8 * 3 * (npanels + 1))); }
  }

  // ---- factorisation: panels left to right ----
  switch (form) {
    case QR_LOOKAHEAD: ND4_TRY(qr_factor_lookahead(j)); break;
    case QR_TALL:      ND4_TRY(qr_factor_tall(j)); if (Q) ND4_TRY(qr_form_q(j, Q)); break;   // (Q right away, ahead of R)
    case QR_BATCHED:   ND4_TRY(qr_factor_batched(j)); break;
    default:           ND4_TRY(qr_factor_blocked(j)); break;
  }

  // ---- R out (tall: top N x N of the work matrix; else already in place, lower part zeroed by the panels) ----
  if (tall) {
    if (Lr > L) ND4_HIP(hipMemsetAsync(R, 0, sizeof(double) * (size_t)batch * Lr * N, h->stream));
    ND4_TRY(nd4_copy_matrix(h, L, N, W, j.ld, R, N, batch, sW, (long)Lr * N));
  }

  {   // undo the power-of-two normalisation on R (exact; a no-op when the exponent is 0)
    const long nR = (long)Lr * N;
    hipLaunchKernelGGL(qr_scale_apply, dim3((unsigned)((nR + 255) / 256), (unsigned)batch), dim3(256), 0, h->stream, R, R, nR, exps, +1);
  }
  if (form != QR_TALL && Q) ND4_TRY(qr_form_q(j, Q));

  // ---- reference sign convention ----
  const long sQ = (long)M * Lq;
  return nd4_givens_signs(h, batch, M, L, N, tall && !full, Q, Lq, sQ, R, N, (long)Lr * N, ws.taus, ws.sTau, ws.flips);
}

// One panel factorisation on its own (the building block north_star's "HBM fraction on the QR panel" is quoted on):
// A [batch, M, 16] -> R in the top 16 x 16 of A (in place), the reflector block V [batch, M, 16] and its factor T [batch, 16, 16] with
// Q_panel = I - V T V^T. Panels of < 64 rows: the thread-per-row Householder kernel (V unit lower trapezoidal, T upper triangular);
// otherwise CholeskyQR2 + the compact orthogonal completion (V = Q - [S; 0], T = K full): up to 8 panels as the row-split launch
// (qrh_bc), more as one workgroup per panel on the matrix cores (qr_batched_panel.hip).
int nd4_geqr2_panel(nd4hip_handle* h, int batch, int M, double* A, double* V, double* T) {
  Nd4WsScope scope(h);
  void* p = nullptr;
  const int parts = (M + NB + 511) / 512 + 1;
  ND4_TRY(nd4_ws_alloc(h, sizeof(double) * (size_t)batch * (NB + parts * QX_ROW_SLOT + 2) + 64, &p));
  double* taus = static_cast<double*>(p);
  const long sW = (long)M * NB;
  const int nb = M < NB ? M : NB;
  if (batch <= QR_ROWSPLIT_MAX_BATCH && M >= HR_MIN_ROWS) {
    // few panels: the row-split form (one launch, the rows over workgroups of 512): V = Q - [S; 0] and T = K of qrh_bc
    QrhHost hr;
    const long sXch = (long)parts * QX_ROW_SLOT;
    unsigned long long* Xch = reinterpret_cast<unsigned long long*>(taus + (size_t)batch * NB);
    ND4_TRY(hr.init(h, batch, A, M, NB, NB, sW, V, NB, sW, T, NB * NB, taus, NB, reinterpret_cast<int*>(Xch + (size_t)batch * sXch), Xch, sXch,
                    nullptr, 0, nullptr, 0, nullptr, 0, nullptr, 0, 1));
    ND4_TRY(hr.panel(0, NB, false, true));
    return 0;
  }
  // a batch of panels: one workgroup per panel on the matrix cores (qr_batched_panel.hip); V = Q - [S; 0], T = K as above
  if (nb == NB && M >= HR_MIN_ROWS) return nd4_qr_panel_mfma_alone(h, batch, M, A, V, T, taus);
  nd4_qr_panel_rows(h, batch, A, M, M, NB, sW, V, NB, sW, T, NB * NB, taus, NB, 0, nb);
  ND4_HIP(hipGetLastError());
  return 0;
}
