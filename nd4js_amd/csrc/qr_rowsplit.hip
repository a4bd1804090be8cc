// Row-split QR panels: the qrh_* kernels and the member functions of their host object QrhHost (qr_rowsplit.h).
#include "qr_rowsplit.h"
#include "qr_panel_row_body.h"
#include "qr_chain16.h"
#include "dpp.h"
#include "xchg.h"

namespace {

// =====================================================================================================================
// Multi-workgroup panel (round 3): CholeskyQR2 + a Householder-type representation of its orthonormal factor.
//
// qr_panel_row<R> is ONE workgroup walking a chain of 16 dependent column steps (reduce over all rows, barrier, reflector
// scalars, update): 27-48 us per panel on one CU, 79 % of a 2048^2 factorisation. Here the panel's ROWS are split over
// workgroups of 512 rows and every step that touches all rows is an fp64-MFMA pass whose only cross-workgroup coupling is the
// sum of 16 x 16 partial matrices, taken across a kernel boundary (the cheap grid barrier of this chip, ~1.5 us):
//   A  C <- (I - V T^T V^T) C for the panel's own 16 columns (the previous reflector, X = V^T C summed from the partials phase C
//      left behind), then partial Gram matrices G = C^T C of the updated rows;
//   B  every workgroup: R1 = chol(G) and R1^-1 (one wave, Gaussian elimination on [G | I], columns across lanes, pivot column
//      broadcast by v_readlane), Q1 = C R1^-1 in place, partial Gram matrices of Q1;
//   C  every workgroup: R2 = chol(Q1^T Q1) = I + F from two fixed-point steps of F = triu(E - F^T F) (E = Q1^T Q1 - I is
//      O(cond^2 eps): no chain; the elimination chain only when max|E| > 1e-5), Q = Q1 R2^-1 (CholeskyQR2: orthonormal to
//      O(eps)), R = S R2 R1, and the orthogonal completion of Q in compact form (Yamamoto's representation with the sign
//      choice of Ballard, Demmel, Grigori, Jacquelin, Nguyen, Solomonik, "Reconstructing Householder vectors from tall-skinny
//      QR", 2014):   H = I - W K W^T,  W = Q - [S; 0],  K = -S (Q_top - S)^-T,  S = diag(+-1) = -sign of the pivots of the
//      Gauss-Jordan elimination of Q_top - S (every pivot has magnitude >= 1).  H is orthogonal (K^-1 + K^-T = W^T W), its
//      first 16 columns are Q S, so H^T [panel] = [S R; 0]: (W, K, S R) is a (V, T, R) triple for everything downstream — V's
//      top block is full instead of unit lower triangular and T is a full 16 x 16 matrix, which is why every consumer of T
//      uses all 256 entries. The same launch leaves the partials of X = V^T C for the NEXT panel's columns.
// The three phases run in ONE launch per panel (qrh_bc), the partial matrices crossing between its row workgroups as tagged words.
// The previous reflector's work on the other column blocks (trailing columns of W, Q^T) rides along in the same launch, split over
// 512-row chunks like the panel itself (qrh_side_fused). Panels the Gram route must not take — (nearly) dependent columns (a Cholesky
// pivot below HR_PIVOT_THR of its diagonal entry), columns that are exactly zero below the top block (triangular / banded input,
// where the reference skips rotations: qr.js:60,63) or non-finite data — are flagged by phase B and factorised by
// qr_panel_row_body in workgroup 0: same result as before, at the old speed.
constexpr int QRH_LDS = 8 * 256 + 256 + NB * (NB + 1) + 16;      // doubles: what the row phases and the side work need ...
constexpr int QRH_SMEM = QRH_LDS + 11 * 256 + 32;                // ... and the whole per-workgroup buffer: phase C carves its 16 x 16 matrices behind QRH_LDS

// sum of n partials (256 doubles apart) of one entry, fixed order; the loads are issued together (a rolled loop of dependent
// global loads costs a full memory round trip per partial: 1-1.5 us each behind a kernel boundary)
__device__ __forceinline__ double qrh_sum_parts(const double* __restrict__ src, int n) {
  double x = 0.0;
  for (int p0 = 0; p0 < n; p0 += 8) {
    double v[8];
#pragma unroll
    for (int p = 0; p < 8; p++) v[p] = (p0 + p < n) ? src[(long)(p0 + p) * 256] : 0.0;
#pragma unroll
    for (int p = 0; p < 8; p++) x += v[p];
  }
  return x;
}
// fixed-order sum of the eight waves' 16 x 16 accumulators -> dst[256] (global)
__device__ __forceinline__ void qrh_reduce_store(double* __restrict__ s_part, const d4& a0, const d4& a1, double* __restrict__ dst) {
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, fx = lane & 15, fk = lane >> 4;
#pragma unroll
  for (int r = 0; r < 4; r++) s_part[wave * 256 + (fk + 4 * r) * 16 + fx] = a0[r] + a1[r];
  __syncthreads();
  if (t < 256) {
    double x = 0.0;
#pragma unroll
    for (int w = 0; w < 8; w++) x += s_part[w * 256 + t];
    dst[t] = x;
  }
}

// The wave's 64 rows [rb, rb + 64) of NBLK adjacent 16-column blocks: C <- C - V (T^T X), X (per block) = the sum of nx partials
// (256 doubles apart, fixed order, the same in every workgroup; block b's partials start at Xsrc + b * xstride). Vcol / Ccol point at
// (row 0, first column) of the reflector / the first block; nc = columns in all (<= 16 NBLK). On return c[b] holds the updated tile of
// block b in accumulator layout (c[b][q][r]: row rb + 16 q + fk + 4 r, column 16 b + fx; rows outside [0, M) are zero).
// s_w: 256 (NBLK + 1) doubles of LDS. Every thread of the workgroup must call it. The reflector rows are loaded ONCE for all blocks.
template <int NBLK>
__device__ __forceinline__ void qrh_apply_rows(double* __restrict__ s_w, const double* __restrict__ Xsrc, long xstride, int nx, const double* __restrict__ Tg,
                                               const double* __restrict__ Vcol, long ldv, double* __restrict__ Ccol, long ldc, int nc,
                                               int rb, int M, d4 (&c)[NBLK][4]) {
  const int t = threadIdx.x, lane = t & 63, fx = lane & 15, fk = lane >> 4;
  double av[4][4];
#pragma unroll
  for (int q = 0; q < 4; q++) {
#pragma unroll
    for (int b = 0; b < NBLK; b++) {
      const bool cok = b * NB + fx < nc;
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const int rc = rb + q * 16 + fk + 4 * r;
        c[b][q][r] = (rc >= 0 && rc < M && cok) ? Ccol[(long)rc * ldc + b * NB + fx] : 0.0;
      }
    }
    const int ra = rb + q * 16 + fx;
    if (ra >= 0 && ra < M) {                                           // 32 contiguous bytes per lane: k-step kk <-> column 4 fk + kk
      const double2 v0 = *reinterpret_cast<const double2*>(Vcol + (long)ra * ldv + 4 * fk);
      const double2 v1 = *reinterpret_cast<const double2*>(Vcol + (long)ra * ldv + 4 * fk + 2);
      av[q][0] = v0.x; av[q][1] = v0.y; av[q][2] = v1.x; av[q][3] = v1.y;
    } else { av[q][0] = av[q][1] = av[q][2] = av[q][3] = 0.0; }
  }
  double* s_X = s_w;                                                   // NBLK x 256
  double* s_Tm = s_w + NBLK * 256;
  if (t < NBLK * 256) {
    const int b = t >> 8, e = t & 255;
    s_X[t] = (b * NB < nc) ? qrh_sum_parts(Xsrc + b * xstride + e, nx) : 0.0;
    if (t < 256) s_Tm[t] = Tg[t];
  }
  __syncthreads();
  double wv = 0.0;
  if (t < NBLK * 256) {
    const int b = t >> 8, i = (t & 255) / 16, j = t % 16;
#pragma unroll
    for (int l = 0; l < NB; l++) wv += s_Tm[l * 16 + i] * s_X[b * 256 + l * 16 + j];        // T^T X, T a full 16 x 16 matrix
  }
  __syncthreads();
  if (t < NBLK * 256) s_X[t] = -wv;
  __syncthreads();
#pragma unroll
  for (int b = 0; b < NBLK; b++) {
    const bool cok = b * NB + fx < nc;
    double bw[4];
#pragma unroll
    for (int kk = 0; kk < 4; kk++) bw[kk] = s_X[b * 256 + (4 * fk + kk) * 16 + fx];
#pragma unroll
    for (int q = 0; q < 4; q++) {
#pragma unroll
      for (int kk = 0; kk < 4; kk++) c[b][q] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[q][kk], bw[kk], c[b][q], 0, 0, 0);
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const int rc = rb + q * 16 + fk + 4 * r;
        if (rc >= 0 && rc < M && cok) Ccol[(long)rc * ldc + b * NB + fx] = c[b][q][r];
      }
    }
  }
}

// ---- tagged words: the in-kernel exchange between co-resident workgroups (see qrh_bc) ----
// (qx_st / qx_sum: xchg.h)
// ---- side work: the previous reflector (panel pj0) on the other column blocks (trailing columns of W, then Q^T), split over
// 512-row chunks like the panel itself. Inside a panel launch both phases of a chunk run in one workgroup (SEG_F); after the last
// panel, two launches of their own: partial X = V^T C (SEG_NX), then C -= V (T^T X) (SEG_NA) ----
struct QrhSide { double* C; long ldc; int c0, nc, cb, rc; };   // cb: first block (index among W blocks, then Q^T blocks); nc: columns of the pair
__device__ __forceinline__ QrhSide qrh_near_of(const QrhP& P, int mat, int e) {
  QrhSide s;
  const int sh = P.na_shift;
  const int pr = e / P.nrc, nwp = (P.nnw - sh + 1) / 2;
  s.rc = e % P.nrc;
  if (pr < nwp) {
    s.cb = sh + 2 * pr; s.C = P.Wm + mat * P.strideW; s.ldc = P.ld; s.c0 = P.wide0 + s.cb * NB;
    const int end = P.wide0 + P.nnw * NB < P.N ? P.wide0 + P.nnw * NB : P.N;
    s.nc = end - s.c0 < 2 * NB ? end - s.c0 : 2 * NB;
  } else {
    const int qb = 2 * (pr - nwp);
    s.cb = P.nnw + qb; s.C = P.QT + mat * P.strideQT; s.ldc = P.M; s.c0 = qb * NB;
    s.nc = P.M - s.c0 < 2 * NB ? P.M - s.c0 : 2 * NB;
  }
  return s;
}
// partial X = V^T C over one 512-row chunk of a pair of column blocks (the reflector at vj0): the reflector slabs are loaded once
__device__ __forceinline__ void qrh_side_x(const QrhP& P, int mat, const QrhSide& s, int vj0, double* __restrict__ dst, double* __restrict__ s_buf) {
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, fx = lane & 15, fk = lane >> 4;
  const int rb = vj0 + s.rc * 512 + wave * 64;
  const double* V = P.Vall + mat * P.strideV + vj0;
  const bool ok0 = fx < s.nc, ok1 = NB + fx < s.nc;
  double c0[16], c1[16], v[16];
#pragma unroll
  for (int u = 0; u < 16; u++) {                                       // 16 slabs of 4 rows: all operands in the same (row fk, column fx) layout
    const int r = rb + 4 * u + fk;
    const bool rok = r < P.M;
    const double* cp = s.C + (long)r * s.ldc + s.c0 + fx;
    c0[u] = (rok && ok0) ? cp[0] : 0.0;
    c1[u] = (rok && ok1) ? cp[NB] : 0.0;
    v[u] = rok ? V[(long)r * P.ldv + fx] : 0.0;
  }
  d4 x0 = d4{0.0, 0.0, 0.0, 0.0}, x1 = x0, y0 = x0, y1 = x0;
#pragma unroll
  for (int u = 0; u < 16; u += 2) {
    x0 = __builtin_amdgcn_mfma_f64_16x16x4f64(v[u], c0[u], x0, 0, 0, 0);
    y0 = __builtin_amdgcn_mfma_f64_16x16x4f64(v[u], c1[u], y0, 0, 0, 0);
    x1 = __builtin_amdgcn_mfma_f64_16x16x4f64(v[u + 1], c0[u + 1], x1, 0, 0, 0);
    y1 = __builtin_amdgcn_mfma_f64_16x16x4f64(v[u + 1], c1[u + 1], y1, 0, 0, 0);
  }
  qrh_reduce_store(s_buf, x0, x1, dst);
  if (s.nc > NB) {                                                     // (uniform) the pair's second block: the next slot of Xs
    __syncthreads();
    qrh_reduce_store(s_buf, y0, y1, dst + (long)P.nrc * 256);
  }
}
// C -= V (T^T X) on one 512-row chunk of a pair of column blocks
__device__ __forceinline__ void qrh_near_apply(const QrhP& P, int mat, int e, double* __restrict__ s_buf) {
  const QrhSide s = qrh_near_of(P, mat, e);
  const int wave = threadIdx.x >> 6;
  d4 c[2][4];
  qrh_apply_rows<2>(s_buf, P.Xs + mat * P.strideXs + (long)s.cb * P.nrc * 256, (long)P.nrc * 256, P.nrc,
                    P.Tall + mat * P.strideT + (long)(P.pj0 / NB) * NB * NB,
                    P.Vall + mat * P.strideV + P.pj0, P.ldv, s.C + s.c0, s.ldc, s.nc, P.pj0 + s.rc * 512 + wave * 64, P.M, c);
}
// ---- the two side phases of one (pair of column blocks, 512-row chunk) in ONE workgroup (round 3, second half) ----
// Partial X = V^T C of the chunk, across to the nrc workgroups of the pair (consecutive workgroups of the launch: tagged words, see
// qrh_bc), C -= V (T^T X) on the tiles that are still in the registers: the side blocks are read once and written once per
// reflector instead of read twice and written once — the launches of the upper half of a 2048^2 factorisation are bound by exactly
// this traffic. (The accumulator image c[q][r] of a 16-row tile and the slab image of its rows 4 (4q + r) + fk are the same registers.)
__device__ __forceinline__ void qrh_side_fused(const QrhP& P, int mat, int e, double* __restrict__ s_buf) {
  const QrhSide s = qrh_near_of(P, mat, e);
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, fx = lane & 15, fk = lane >> 4;
  const int vj0 = P.pj0, rb = vj0 + s.rc * 512 + wave * 64;
  const double* V = P.Vall + mat * P.strideV + vj0;
  const bool ok0 = fx < s.nc, ok1 = NB + fx < s.nc;
  const unsigned tag = (unsigned)(vj0 / NB + 1);
  double c0[16], c1[16];
  d4 x0 = d4{0.0, 0.0, 0.0, 0.0}, x1 = x0, y0 = x0, y1 = x0;
  {
    double v[16];
#pragma unroll
    for (int u = 0; u < 16; u++) {
      const int r = rb + 4 * u + fk;
      const bool rok = r < P.M;
      const double* cp = s.C + (long)r * s.ldc + s.c0 + fx;
      c0[u] = (rok && ok0) ? cp[0] : 0.0;
      c1[u] = (rok && ok1) ? cp[NB] : 0.0;
      v[u] = rok ? V[(long)r * P.ldv + fx] : 0.0;
    }
#pragma unroll
    for (int u = 0; u < 16; u += 2) {
      x0 = __builtin_amdgcn_mfma_f64_16x16x4f64(v[u], c0[u], x0, 0, 0, 0);
      y0 = __builtin_amdgcn_mfma_f64_16x16x4f64(v[u], c1[u], y0, 0, 0, 0);
      x1 = __builtin_amdgcn_mfma_f64_16x16x4f64(v[u + 1], c0[u + 1], x1, 0, 0, 0);
      y1 = __builtin_amdgcn_mfma_f64_16x16x4f64(v[u + 1], c1[u + 1], y1, 0, 0, 0);
    }
  }
  // the reflector rows as A operands of C -= V W (32 contiguous bytes per lane), requested before the exchange
  double av[4][4];
#pragma unroll
  for (int q = 0; q < 4; q++) {
    const int ra = rb + q * 16 + fx;
    if (ra < P.M) {
      const double2 v0 = *reinterpret_cast<const double2*>(V + (long)ra * P.ldv + 4 * fk);
      const double2 v1 = *reinterpret_cast<const double2*>(V + (long)ra * P.ldv + 4 * fk + 2);
      av[q][0] = v0.x; av[q][1] = v0.y; av[q][2] = v1.x; av[q][3] = v1.y;
    } else { av[q][0] = av[q][1] = av[q][2] = av[q][3] = 0.0; }
  }
  // fixed-order sums over the eight waves, then across: slot (block, chunk), entry = position in the 16 x 16 matrix
  qx_u64* slots = P.Xsx + mat * P.strideXsx;
  double* s_Tm = s_buf + 8 * 256;
#pragma unroll
  for (int r = 0; r < 4; r++) s_buf[wave * 256 + (fk + 4 * r) * 16 + fx] = x0[r] + x1[r];
  if (t < 256) s_Tm[t] = P.Tall[mat * P.strideT + (long)(vj0 / NB) * NB * NB + t];
  __syncthreads();
  if (t < 256) {
    double xs = 0.0;
#pragma unroll
    for (int w = 0; w < 8; w++) xs += s_buf[w * 256 + t];
    qx_st(slots + ((long)s.cb * P.rcs_max + s.rc) * 512, t, xs, tag);
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < 4; r++) s_buf[wave * 256 + (fk + 4 * r) * 16 + fx] = y0[r] + y1[r];
  __syncthreads();
  if (t >= 256 && s.nc > NB) {
    double xs = 0.0;
#pragma unroll
    for (int w = 0; w < 8; w++) xs += s_buf[w * 256 + (t - 256)];
    qx_st(slots + ((long)(s.cb + 1) * P.rcs_max + s.rc) * 512, t - 256, xs, tag);
  }
  __syncthreads();
  double* s_X = s_buf;                                                 // 2 x 256
  {
    const int b = t >> 8, en = t & 255;
    double x = 0.0;
    if (b == 0 || s.nc > NB) {
      const qx_u64* base = slots + (long)(s.cb + b) * P.rcs_max * 512;
      int spins = 0;
      for (;;) {
        bool ok = true;
        x = qx_sum(base, en, P.nrc, tag, ok);
        if (ok) break;
        if (++spins > QX_SPIN_LIMIT) { x = __builtin_nan(""); qx_raise(P.status); break; }    // a stuck exchange must not pass silently
        __builtin_amdgcn_s_sleep(2);
      }
    }
    s_X[t] = x;
  }
  __syncthreads();
  double wv = 0.0;
  {
    const int b = t >> 8, i = (t & 255) / 16, j = t % 16;
#pragma unroll
    for (int l = 0; l < NB; l++) wv += s_Tm[l * 16 + i] * s_X[b * 256 + l * 16 + j];          // T^T X, T a full 16 x 16 matrix
  }
  __syncthreads();
  s_X[t] = -wv;
  __syncthreads();
#pragma unroll
  for (int b = 0; b < 2; b++) {
    const bool cok = b == 0 ? ok0 : ok1;
    double bw[4];
#pragma unroll
    for (int kk = 0; kk < 4; kk++) bw[kk] = s_X[b * 256 + (4 * fk + kk) * 16 + fx];
#pragma unroll
    for (int q = 0; q < 4; q++) {
      d4 c;
#pragma unroll
      for (int r = 0; r < 4; r++) c[r] = b == 0 ? c0[4 * q + r] : c1[4 * q + r];
#pragma unroll
      for (int kk = 0; kk < 4; kk++) c = __builtin_amdgcn_mfma_f64_16x16x4f64(av[q][kk], bw[kk], c, 0, 0, 0);
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const int rc = rb + q * 16 + fk + 4 * r;
        if (rc < P.M && cok) s.C[(long)rc * s.ldc + s.c0 + b * NB + fx] = c[r];
      }
    }
  }
}
// workgroup i of a launch's side work
__device__ __forceinline__ void qrh_side(const QrhP& P, int mat, int i, double* __restrict__ s_buf) {
  int kind = -1, e = 0;
  for (int sg = 0; sg < P.nseg; sg++) {
    if (i < P.seg[sg].count) { kind = P.seg[sg].kind; e = P.seg[sg].first + i; break; }
    i -= P.seg[sg].count;
  }
  if (kind == SEG_NX) {
    const QrhSide s = qrh_near_of(P, mat, e);
    qrh_side_x(P, mat, s, P.pj0, P.Xs + mat * P.strideXs + ((long)s.cb * P.nrc + s.rc) * 256, s_buf);
  } else if (kind == SEG_NA) {
    qrh_near_apply(P, mat, e, s_buf);
  } else if (kind == SEG_F) {
    qrh_side_fused(P, mat, e, s_buf);
  }
}
// side work on its own (the flush after the last such panel)
__global__ __launch_bounds__(512) void qrh_side_only(const QrhP P) {
  __shared__ double s_buf[QRH_SMEM];
  qrh_side(P, blockIdx.y, blockIdx.x, s_buf);
}

__device__ __forceinline__ void qrh_stamp(const QrhP& P, int k) {
  if (P.stamps != nullptr && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) P.stamps[P.stamp_slot * 8 + k] = wall_clock64();
}
// X = V^T C over all m rows by the eight waves of one workgroup -> dst[256] (the fall-back panel's share of phase C)
__device__ __forceinline__ void qrh_x_full(double* __restrict__ s_part, const double* __restrict__ V, long ldv, const double* __restrict__ C, long ldc,
                                           int m, int nc, double* __restrict__ dst) {
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, fx = lane & 15, fk = lane >> 4;
  const int rpw = ((m + 8 * 16 - 1) / (8 * 16)) * 16;
  const int r0 = wave * rpw, r1 = (r0 + rpw < m) ? r0 + rpw : m;
  const bool cok = fx < nc;
  d4 a0 = d4{0.0, 0.0, 0.0, 0.0}, a1 = a0;
  for (int rr = r0; rr < r1; rr += 8) {
    const int ra = rr + fk, rb2 = rr + 4 + fk;
    const double va = ra < r1 ? V[(long)ra * ldv + fx] : 0.0, ca = (ra < r1 && cok) ? C[(long)ra * ldc + fx] : 0.0;
    const double vb = rb2 < r1 ? V[(long)rb2 * ldv + fx] : 0.0, cb = (rb2 < r1 && cok) ? C[(long)rb2 * ldc + fx] : 0.0;
    a0 = __builtin_amdgcn_mfma_f64_16x16x4f64(va, ca, a0, 0, 0, 0);
    a1 = __builtin_amdgcn_mfma_f64_16x16x4f64(vb, cb, a1, 0, 0, 0);
  }
  qrh_reduce_store(s_part, a0, a1, dst);
}

// ---- phases B and C in ONE launch (round 3, second half) ----
// What phase C needs from the other row workgroups of phase B is one 16 x 16 matrix each (the partial Gram matrix of Q1). An exchange
// of that size inside a kernel costs ~1.4 us on this chip when it is made of agent-scope relaxed atomics only (sc1 stores are
// written through, sc1 loads miss the non-coherent caches: no write-back, no invalidate; tools/xwg_lat.hip, lu.hip: lu_panel_mw) —
// less than the kernel boundary it replaces, and the panel's rows need not be read a third time: Q1 stays in the registers (its
// accumulator image goes through LDS once to become the A operand of Q = Q1 R2^-1). Every 8-byte word that crosses carries 32 bits
// of payload and a 32-bit tag (panel number + 1): a double is valid as soon as both its words carry the tag, so there is no flag,
// no s_waitcnt and no ordering between words. The row partition is phase A's (rows from j0 - 16: tile 0 of workgroup 0 lies above
// the panel and only sees the previous reflector). The next panel's 16 columns get the previous reflector from the ROW workgroups
// here (X summed in the first exchange), each for its own rows, which it then holds for the partial X of the next
// panel: the side work of this launch starts one block later (na_shift) and covers W and Q^T in one go.
// Phase A rides in the same launch as well — the previous reflector on the panel's own columns, the partial Gram matrices and the
// partial X of the NEXT panel's block cross in a first exchange, so a panel is ONE launch (all side work rides in it).
// A flagged panel: workgroup 0 runs qr_panel_row_body (R > 0; tall panels: qr_panel_flagged in a launch of its own, as before) and
// nobody writes partials of X: qrh_x_flagged forms them over all rows ahead of the next launch (QrhHost::panel) and ahead of the last
// panel's narrow update (QrhHost::finish).
template <int R>
__global__ __launch_bounds__(512) void qrh_bc(const QrhP P) {
  __shared__ double s_buf[QRH_SMEM];
  __shared__ double s_G[256], s_R[256], s_Ri[256], s_db[16];
  __shared__ int s_flag, s_emax;
  const int mat = blockIdx.y;
  if ((int)blockIdx.x >= P.nrow) { qrh_side(P, mat, (int)blockIdx.x - P.nrow, s_buf); return; }
  const int g = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6, fx = lane & 15, fk = lane >> 4;
  double* A = P.Wm + mat * P.strideW;
  const int j0 = P.j0, M = P.M, N = P.N, ub = j0 - NB;
  const long ld = P.ld;
  const int c0 = j0 + NB, nc = P.skip_x ? 0 : (N - c0 < NB ? N - c0 : NB);   // the next panel's columns (nc <= 0: none)
  const int rb = ub + (g * 8 + wave) * 64;                                  // phase A's row partition
  const unsigned tag = (unsigned)(j0 / NB + 1);
  qx_u64* slots = P.Xch + mat * P.strideXch;
  qx_u64* myslot = slots + (long)g * QX_ROW_SLOT;
  double* Xdst = P.Xp + mat * P.strideXp + (long)g * 256;
  qrh_stamp(P, 0);
  d4 cs[4];
  double a[4][4];
  __shared__ double s_T2[256], s_Xs[256], s_Xn[256];
  d4 cnx[4]; double avp[4][4]; bool nextupd = false;       // the next block's tile, the previous reflector's rows
  // the next block through the previous reflector for this workgroup's rows: C -= V (T^T X), -T^T X in s_Xn
  auto apply_next = [&]() {
    double bwn[4];
#pragma unroll
    for (int kk = 0; kk < 4; kk++) bwn[kk] = s_Xn[(4 * fk + kk) * 16 + fx];
#pragma unroll
    for (int q = 0; q < 4; q++) {
#pragma unroll
      for (int kk = 0; kk < 4; kk++) cnx[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(avp[q][kk], bwn[kk], cnx[q], 0, 0, 0);
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const int rc = rb + q * 16 + fk + 4 * r;
        if (rc >= 0 && rc < M && fx < nc) A[(long)rc * ld + c0 + fx] = cnx[q][r];
      }
    }
  };
  {
    // ---- phase A: the previous reflector on the panel's own columns, partial Gram matrices, partial X of the next block ----
    // All loads first: the own tile and the next block's tile in the accumulator image (== slab image: slab u = 4 q + r), the
    // previous reflector's rows as A operands (avp) and as slabs (vs). The next block's tile and avp stay in registers until the
    // block is updated in the shadow of the second exchange.
    d4 c[4];
    const bool havep = P.pj0 >= 0;
    nextupd = nc > 0 && havep;
    const double* Vp = P.Vall + mat * P.strideV + ub;
    // first the loads that head the dependent chain of the own-column update (loads return in order): X partials and T
    double xsum0 = 0.0, tprev = 0.0, xp8[8];
#pragma unroll
    for (int p8 = 0; p8 < 8; p8++) xp8[p8] = 0.0;
    if (havep && t < 256) {
#pragma unroll
      for (int p8 = 0; p8 < 8; p8++) if (p8 < P.nxp) xp8[p8] = P.Xp[mat * P.strideXp + (long)p8 * 256 + t];   // (summed below, after the tile loads are under way)
      tprev = P.Tall[mat * P.strideT + (long)(ub / NB) * NB * NB + t];
    }
    double vs[16];
#pragma unroll
    for (int q = 0; q < 4; q++) {
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const int rc = rb + q * 16 + fk + 4 * r;
        const bool rok = rc >= 0 && rc < M;
        c[q][r] = rok ? A[(long)rc * ld + j0 + fx] : 0.0;
        cnx[q][r] = (rok && fx < nc && (nextupd || rc >= j0)) ? A[(long)rc * ld + c0 + fx] : 0.0;
        vs[4 * q + r] = (rok && nextupd) ? Vp[(long)rc * P.ldv + fx] : 0.0;
      }
      const int ra = rb + q * 16 + fx;
      if (havep && ra >= 0 && ra < M) {
        const double2 v0 = *reinterpret_cast<const double2*>(Vp + (long)ra * P.ldv + 4 * fk);
        const double2 v1 = *reinterpret_cast<const double2*>(Vp + (long)ra * P.ldv + 4 * fk + 2);
        avp[q][0] = v0.x; avp[q][1] = v0.y; avp[q][2] = v1.x; avp[q][3] = v1.y;
      } else { avp[q][0] = avp[q][1] = avp[q][2] = avp[q][3] = 0.0; }
    }
    const int i = (t & 255) / 16, j = t % 16;
    if (havep) {
      if (t < 256) {
#pragma unroll
        for (int p8 = 0; p8 < 8; p8++) xsum0 += xp8[p8];
        if (P.nxp > 8) xsum0 += qrh_sum_parts(P.Xp + mat * P.strideXp + 8 * 256 + t, P.nxp - 8);
        s_buf[t] = xsum0; s_T2[t] = tprev;
      }
      __syncthreads();
      double wv = 0.0;
      if (t < 256) {
#pragma unroll
        for (int l = 0; l < NB; l++) wv += s_T2[l * 16 + i] * s_buf[l * 16 + j];               // T^T X
      }
      __syncthreads();
      if (t < 256) s_buf[t] = -wv;
      __syncthreads();
      double bwp[4];
#pragma unroll
      for (int kk = 0; kk < 4; kk++) bwp[kk] = s_buf[(4 * fk + kk) * 16 + fx];
#pragma unroll
      for (int q = 0; q < 4; q++) {
#pragma unroll
        for (int kk = 0; kk < 4; kk++) c[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(avp[q][kk], bwp[kk], c[q], 0, 0, 0);
#pragma unroll
        for (int r = 0; r < 4; r++) {
          const int rc = rb + q * 16 + fk + 4 * r;
          if (rc >= 0 && rc < M) A[(long)rc * ld + j0 + fx] = c[q][r];
        }
      }
      __syncthreads();                                                  // s_buf is reused below
    }
    qrh_stamp(P, 1);
    d4 g0 = d4{0.0, 0.0, 0.0, 0.0}, g1 = g0, gt = g0;
#pragma unroll
    for (int q = 0; q < 4; q++) {
      const int ti = (g * 8 + wave) * 4 + q;                          // tile 0: the 16 rows above the panel, tile 1: its top block
      if (ti == 1) {
#pragma unroll
        for (int r = 0; r < 4; r++) gt = __builtin_amdgcn_mfma_f64_16x16x4f64(c[q][r], c[q][r], gt, 0, 0, 0);
      } else if (ti >= 2) {
        g0 = __builtin_amdgcn_mfma_f64_16x16x4f64(c[q][0], c[q][0], g0, 0, 0, 0);
        g1 = __builtin_amdgcn_mfma_f64_16x16x4f64(c[q][1], c[q][1], g1, 0, 0, 0);
        g0 = __builtin_amdgcn_mfma_f64_16x16x4f64(c[q][2], c[q][2], g0, 0, 0, 0);
        g1 = __builtin_amdgcn_mfma_f64_16x16x4f64(c[q][3], c[q][3], g1, 0, 0, 0);
      }
    }
    // partial X = V^T C of the next panel's block over this workgroup's rows (the previous reflector; slab images)
    d4 xn0 = d4{0.0, 0.0, 0.0, 0.0}, xn1 = xn0;
    if (nextupd) {
#pragma unroll
      for (int q = 0; q < 4; q++) {
        xn0 = __builtin_amdgcn_mfma_f64_16x16x4f64(vs[4 * q + 0], cnx[q][0], xn0, 0, 0, 0);
        xn1 = __builtin_amdgcn_mfma_f64_16x16x4f64(vs[4 * q + 1], cnx[q][1], xn1, 0, 0, 0);
        xn0 = __builtin_amdgcn_mfma_f64_16x16x4f64(vs[4 * q + 2], cnx[q][2], xn0, 0, 0, 0);
        xn1 = __builtin_amdgcn_mfma_f64_16x16x4f64(vs[4 * q + 3], cnx[q][3], xn1, 0, 0, 0);
      }
    }
    // the panel tile from its accumulator image to the A-operand image (tile 0 lies above the panel: zero), through the wave's own LDS
    {
      double* sw = s_buf + 8 * 256 + wave * 272;
#pragma unroll
      for (int q = 0; q < 4; q++) {
        const int ti = (g * 8 + wave) * 4 + q;
#pragma unroll
        for (int r = 0; r < 4; r++) sw[(fk + 4 * r) * 17 + fx] = ti >= 1 ? c[q][r] : 0.0;
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
        for (int kk = 0; kk < 4; kk++) a[q][kk] = sw[fx * 17 + 4 * fk + kk];
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      }
    }
    // first exchange: G partial, X partial, (workgroup 0, wave 0) the top tile's Gram matrix
#pragma unroll
    for (int r = 0; r < 4; r++) s_buf[wave * 256 + (fk + 4 * r) * 16 + fx] = g0[r] + g1[r];
    if (g == 0 && wave == 0) {
#pragma unroll
      for (int r = 0; r < 4; r++) qx_st(myslot, 512 + (fk + 4 * r) * 16 + fx, gt[r], tag);
    }
    __syncthreads();
    if (t < 256) {
      double xs = 0.0;
#pragma unroll
      for (int w = 0; w < 8; w++) xs += s_buf[w * 256 + t];
      if (!(P.drop_tag == (int)tag && g == P.nrow - 1)) qx_st(myslot, t, xs, tag);   // (tests: one dropped publication)
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 4; r++) s_buf[wave * 256 + (fk + 4 * r) * 16 + fx] = xn0[r] + xn1[r];
    __syncthreads();
    if (t >= 256) {
      double xs = 0.0;
#pragma unroll
      for (int w = 0; w < 8; w++) xs += s_buf[w * 256 + (t - 256)];
      qx_st(myslot, t, xs, tag);
    }
    qrh_stamp(P, 2);
    if (t < 256) {
      double x = 0.0, xn = 0.0, top = 0.0;
      int spins = 0;
      for (;;) {
        bool ok = true;
        x = qx_sum(slots, t, P.nrow, tag, ok, QX_ROW_SLOT);
        if (nextupd) xn = qx_sum(slots, 256 + t, P.nrow, tag, ok, QX_ROW_SLOT);
        const qx_u64 w0 = __hip_atomic_load(slots + 2 * (512 + t), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const qx_u64 w1 = __hip_atomic_load(slots + 2 * (512 + t) + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        ok = ok && (unsigned)(w0 >> 32) == tag && (unsigned)(w1 >> 32) == tag;
        top = __longlong_as_double((long long)((w1 << 32) | (w0 & 0xffffffffull)));
        if (ok) break;
        if (++spins > QX_SPIN_LIMIT) { x = __builtin_nan(""); qx_raise(P.status); break; }    // a stuck exchange must not pass silently
        __builtin_amdgcn_s_sleep(2);
      }
      s_G[t] = x + top;
      if (t % 17 == 0) s_db[t / 17] = x;                               // column sums of squares below the top block
      s_Xs[t] = xn;
    }
    if (t == 0) s_emax = 0;
    __syncthreads();
    qrh_stamp(P, 3);
    // while wave 0 walks the elimination chain below, waves 4..7 form -T^T X for the next block
    if (nextupd && t >= 256) {
      double wv = 0.0;
#pragma unroll
      for (int l = 0; l < NB; l++) wv += s_T2[l * 16 + i] * s_Xs[l * 16 + j];
      s_Xn[t - 256] = -wv;
    }
  }
  // ---- phase B: R1 = chol(G), the fall-back decision ----
  if (wave == 0) {
    __builtin_amdgcn_s_setprio(3);
    bool ok = qrc_chol16_inv(s_G, s_R, s_Ri, HR_PIVOT_THR);
    __builtin_amdgcn_s_setprio(0);
#pragma unroll
    for (int k = 0; k < 16; k++) ok = ok && (s_db[k] > 0.0);
    if (lane == 0) s_flag = ok ? 0 : 1;
  }
  __syncthreads();
  const int flag = s_flag;                                            // (the same in every row workgroup: same sums in the same order)
  if (g == 0 && t == 0) P.flag[mat] = flag;
  // the classic panel in place of the Gram route (rare path; the decision is the same in every row workgroup)
  auto fall_back = [&]() {
    if constexpr (R > 0) {
      // the panel's columns were written by all row workgroups of THIS launch: every workgroup pushes its stores out (release:
      // write back the L2) and says so; workgroup 0 waits for all, invalidates (acquire) and runs the classic panel. Rare path.
      __threadfence();
      __syncthreads();
      if (t == 0) qx_st(myslot, 768, 1.0, tag);
      if (g == 0) {
        if (t < P.nrow) {
          int spins = 0;
          for (;;) {
            bool ok = true;
            (void)qx_sum(slots + (long)t * QX_ROW_SLOT, 768, 1, tag, ok, QX_ROW_SLOT);
            if (ok) break;
            if (++spins > QX_SPIN_LIMIT) { qx_raise(P.status); break; }
            __builtin_amdgcn_s_sleep(4);
          }
        }
        __syncthreads();
        __threadfence();
      }
      if (g == 0) qr_panel_row_body<(R > 0 ? R : 1)>(mat, P.Wm, M, ld, P.strideW, P.Vall, P.ldv, P.strideV, P.Tall, P.strideT, P.taus, P.strideTau, j0, NB);
    }
  };
  if (flag) {
    if (nextupd) apply_next();                                        // (the next launch needs the block whatever happens to this panel)
    fall_back();
    return;
  }
  // ---- Q1 = C R1^-1 (registers), its partial Gram matrix across to the other row workgroups ----
  double bw[4];
#pragma unroll
  for (int kk = 0; kk < 4; kk++) bw[kk] = s_Ri[(4 * fk + kk) * 16 + fx];
  d4 acc[4];
#pragma unroll
  for (int q = 0; q < 4; q++) {
    acc[q] = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int kk = 0; kk < 4; kk++) acc[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[q][kk], bw[kk], acc[q], 0, 0, 0);
  }
  // One step of iterative refinement, Q1 += (C - Q1 R1) R1^-1. The product with the explicit inverse alone leaves a column-wise
  // residual of C - Q1 R1 that grows with the panel's condition (eps |C| |R1^-1| |R1|: 40 ... 800 eps on Kahan blocks of condition
  // 1.8e3 ... 1.4e6, 1e4 eps at 8.7e6, measured); the refined rows solve x R1 = c as backward stably as a substitution does (Skeel).
  // Tile by tile; both relayouts (accumulator image -> A-operand image) go through the wave's own piece of LDS, as in phase A.
  {
    double* sw = s_buf + 8 * 256 + wave * 272;
    double br[4];
#pragma unroll
    for (int kk = 0; kk < 4; kk++) br[kk] = s_R[(4 * fk + kk) * 16 + fx];
#pragma unroll
    for (int q = 0; q < 4; q++) {
      double qa[4];
#pragma unroll
      for (int r = 0; r < 4; r++) sw[(fk + 4 * r) * 17 + fx] = acc[q][r];
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
      for (int kk = 0; kk < 4; kk++) qa[kk] = sw[fx * 17 + 4 * fk + kk];
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      d4 pr = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int kk = 0; kk < 4; kk++) pr = __builtin_amdgcn_mfma_f64_16x16x4f64(qa[kk], br[kk], pr, 0, 0, 0);   // Q1 R1
#pragma unroll
      for (int r = 0; r < 4; r++) sw[(fk + 4 * r) * 17 + fx] = pr[r];
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
      for (int kk = 0; kk < 4; kk++) qa[kk] = a[q][kk] - sw[fx * 17 + 4 * fk + kk];                            // C - Q1 R1
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
      for (int kk = 0; kk < 4; kk++) acc[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(qa[kk], bw[kk], acc[q], 0, 0, 0);
    }
  }
  d4 g0 = d4{0.0, 0.0, 0.0, 0.0}, g1 = g0;
#pragma unroll
  for (int q = 0; q < 4; q++) {
    g0 = __builtin_amdgcn_mfma_f64_16x16x4f64(acc[q][0], acc[q][0], g0, 0, 0, 0);
    g1 = __builtin_amdgcn_mfma_f64_16x16x4f64(acc[q][1], acc[q][1], g1, 0, 0, 0);
    g0 = __builtin_amdgcn_mfma_f64_16x16x4f64(acc[q][2], acc[q][2], g0, 0, 0, 0);
    g1 = __builtin_amdgcn_mfma_f64_16x16x4f64(acc[q][3], acc[q][3], g1, 0, 0, 0);
  }
  double* s_E = s_buf + QRH_LDS; double* s_F = s_E + 256; double* s_P = s_F + 256; double* s_Qt = s_P + 512;
  double* s_R2 = s_Qt + 256; double* s_R2i = s_R2 + 256; double* s_Z = s_R2i + 256; double* s_Rm = s_Z + 256; double* s_K = s_Rm + 256; double* s_S = s_K + 256;
#pragma unroll
  for (int r = 0; r < 4; r++) s_buf[wave * 256 + (fk + 4 * r) * 16 + fx] = g0[r] + g1[r];
  __syncthreads();
  if (g == 0 && wave == 0) {                                           // top block of Q1 (tile 1); behind the barrier: s_Qt lies in the
#pragma unroll                                                         // LDS the other waves' refinement relayouts went through
    for (int r = 0; r < 4; r++) s_Qt[(fk + 4 * r) * 16 + fx] = acc[1][r];
  }
  const int i = (t & 255) / 16, j = t % 16;
  if (t < 256) {
    double xs = 0.0;
#pragma unroll
    for (int w = 0; w < 8; w++) xs += s_buf[w * 256 + t];
    qx_st(myslot, 1024 + t, xs, tag);
  }
  if (nextupd) apply_next();                                           // in the shadow of the exchange: the next block
#pragma unroll
  for (int q = 0; q < 4; q++) cs[q] = cnx[q];
  qrh_stamp(P, 3);
  double x = 0.0;
  if (t < 256) {
    int spins = 0;
    for (;;) {
      bool ok = true;
      x = qx_sum(slots, 1024 + t, P.nrow, tag, ok, QX_ROW_SLOT);
      if (ok) break;
      if (++spins > QX_SPIN_LIMIT) { x = __builtin_nan(""); qx_raise(P.status); break; }      // a stuck exchange must not pass silently
      __builtin_amdgcn_s_sleep(2);
    }
    x -= (i == j) ? 1.0 : 0.0;                                         // E = Q1^T Q1 - I
    s_E[t] = x;
    s_F[t] = (i < j) ? x : ((i == j) ? 0.5 * x : 0.0);
    const float ax = fabsf((float)x);
    atomicMax(&s_emax, (ax == ax) ? __float_as_int(ax) : 0x7f800000);
  }
  __syncthreads();
  const bool series = __int_as_float(s_emax) <= (float)HR_SERIES_MAX;
  // the pivot test does not bound the panel's condition number: beyond HR_PASS1_MAX the second pass no longer restores orthogonality.
  // Nothing of this panel has been stored yet (Q1 lives in registers, the panel's columns in memory are phase A's): the classic panel.
  if (!(__int_as_float(s_emax) <= (float)HR_PASS1_MAX)) {
    if (g == 0 && t == 0) P.flag[mat] = 1;
    fall_back();
    return;
  }
  qrh_stamp(P, 4);
  // Q1 from its accumulator image to the A-operand image, one tile at a time through the wave's own piece of LDS (rows padded to 17
  // doubles; the DS operations of one wave execute in order, the waits keep compiler and hardware from overlapping write and read;
  // the eight partial matrices that lay there were consumed before the barrier above)
  {
    double* sw = s_buf + wave * 272;                                   // 8 x 272 doubles: fits in front of QRH_LDS
#pragma unroll
    for (int q = 0; q < 4; q++) {
#pragma unroll
      for (int r = 0; r < 4; r++) sw[(fk + 4 * r) * 17 + fx] = acc[q][r];
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
      for (int kk = 0; kk < 4; kk++) a[q][kk] = sw[fx * 17 + 4 * fk + kk];
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    }
  }
  // R2 and R2^-1 on wave 0 (the products of the series on the matrix core, qr_chain16.h), then — workgroup 0 — the top block of Q,
  // R = R2 R1 and the elimination behind S and K, while the other waves form Q = Q1 R2^-1
  if (wave == 0) qrc_series16(s_E, series, s_R2, s_R2i, s_F);
  __syncthreads();
  if (g == 0 && wave == 0) {
    __builtin_amdgcn_s_setprio(3);
    qrc_zr16(s_Qt, s_R2i, s_R2, s_R, s_Z, s_Rm);
    qrh_stamp(P, 5);
    qrc_gj16(s_Z, s_K, s_S);
    __builtin_amdgcn_s_setprio(0);
  }
#pragma unroll
  for (int kk = 0; kk < 4; kk++) bw[kk] = s_R2i[(4 * fk + kk) * 16 + fx];
  d4 y[4];
#pragma unroll
  for (int q = 0; q < 4; q++) {
    y[q] = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int kk = 0; kk < 4; kk++) y[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[q][kk], bw[kk], y[q], 0, 0, 0);
  }
  if (g == 0) __syncthreads();                                         // s_K, s_S (uniform per workgroup)
  qrh_stamp(P, 6);
  double* V = P.Vall + mat * P.strideV + j0;
#pragma unroll
  for (int q = 0; q < 4; q++) {
    const bool top = (g == 0 && wave == 0 && q == 1);
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const int ii = fk + 4 * r, rc = rb + q * 16 + ii;
      double wv = 0.0;
      if (top) {                                                       // W = Q - [S; 0]; R = S R2 R1 in place
        if (ii == fx) y[q][r] -= s_S[ii];
        wv = (ii <= fx) ? s_S[ii] * s_Rm[ii * 16 + fx] : 0.0;
      }
      if (rc >= j0 && rc < M) { V[(long)rc * P.ldv + fx] = y[q][r]; A[(long)rc * ld + j0 + fx] = wv; }
    }
  }
  if (g == 0) {
    if (t < 256) P.Tall[mat * P.strideT + (long)(j0 / NB) * NB * NB + t] = s_K[t];
    if (t < 16) P.taus[mat * P.strideTau + j0 + t] = 1.0;             // "a reflector was needed" (qr_flips)
  }
  if (nc > 0) {
    d4 x0 = d4{0.0, 0.0, 0.0, 0.0}, x1 = x0;
#pragma unroll
    for (int q = 0; q < 4; q++) {
      x0 = __builtin_amdgcn_mfma_f64_16x16x4f64(y[q][0], cs[q][0], x0, 0, 0, 0);
      x1 = __builtin_amdgcn_mfma_f64_16x16x4f64(y[q][1], cs[q][1], x1, 0, 0, 0);
      x0 = __builtin_amdgcn_mfma_f64_16x16x4f64(y[q][2], cs[q][2], x0, 0, 0, 0);
      x1 = __builtin_amdgcn_mfma_f64_16x16x4f64(y[q][3], cs[q][3], x1, 0, 0, 0);
    }
    __syncthreads();                                                   // (the relayout pieces in s_buf are consumed)
    qrh_reduce_store(s_buf, x0, x1, Xdst);
  }
  qrh_stamp(P, 7);
}

// partials of X = V^T C for the next panel's columns after qr_panel_flagged (workgroup 0: all rows; the others: zero)
__global__ __launch_bounds__(512) void qrh_x_flagged(const QrhP P) {
  __shared__ double s_buf[QRH_LDS];
  const int mat = blockIdx.y, g = blockIdx.x, t = threadIdx.x;
  if (!P.flag[mat]) return;
  const int j0 = P.j0, c0 = j0 + NB, nc = P.N - c0 < NB ? P.N - c0 : NB;
  if (nc <= 0) return;
  double* Xdst = P.Xp + mat * P.strideXp + (long)g * 256;
  if (g == 0) qrh_x_full(s_buf, P.Vall + mat * P.strideV + (long)j0 * P.ldv + j0, P.ldv, P.Wm + mat * P.strideW + (long)j0 * P.ld + c0, P.ld, P.M - j0, nc, Xdst);
  else if (t < 256) Xdst[t] = 0.0;
}

}  // namespace

// ---- QrhHost (qr_rowsplit.h) ----
// every field of P; the slices a caller has no use for are nullptr (the panel entry point: no partials of X, side work or Q^T).
// Zeroes the exchange slots and the fall-back flags.
int QrhHost::init(nd4hip_handle* hh, int nmat, double* W, int M, int N, long ld, long sW, double* Vm, long ldv_, long sV_, double* Tm, long sT_,
                  double* taus, long sTau, int* flag, unsigned long long* Xch, long sXch, double* Xp, long sXp, double* QT, long sQT,
                  double* Xs, long sXs, unsigned long long* Xsx, long sXsx, int rcs_max) {
  h = hh; batch = nmat; nq = QT ? (M + NB - 1) / NB : 0; V = Vm; T = Tm; ldv = ldv_; sV = sV_; sT = sT_;
  P.Wm = W; P.M = M; P.N = N; P.ld = ld; P.strideW = sW; P.Vall = Vm; P.ldv = ldv_; P.strideV = sV_; P.Tall = Tm; P.strideT = sT_;
  P.taus = taus; P.strideTau = sTau; P.Xp = Xp; P.strideXp = sXp; P.flag = flag; P.QT = QT; P.strideQT = sQT; P.Xs = Xs; P.strideXs = sXs;
  P.Xch = Xch; P.strideXch = sXch; P.Xsx = Xsx; P.strideXsx = sXsx; P.rcs_max = rcs_max;
  P.nxp = 0; P.na_shift = 0; P.nseg = 0; P.wide0 = 0; P.nrc = 1; P.nnw = 0; P.nqb = 0; P.skip_x = 0; P.j0 = 0; P.pj0 = -1; P.nrow = 0;
  P.stamps = nullptr; P.stamp_slot = 0; P.status = h->xstat; { const int dp = nd4_test_drop_panel(); P.drop_tag = dp >= 0 ? dp + 1 : -1; }
  if (Xsx) ND4_HIP(hipMemsetAsync(Xsx, 0, sizeof(unsigned long long) * (size_t)batch * sXsx, h->stream));
  ND4_HIP(hipMemsetAsync(Xch, 0, sizeof(unsigned long long) * (size_t)batch * sXch, h->stream));
  ND4_HIP(hipMemsetAsync(flag, 0, sizeof(int) * (size_t)batch, h->stream));
  return 0;
}
void QrhHost::add_seg(int kind, int first, int count) { if (count > 0) { P.seg[P.nseg].kind = kind; P.seg[P.nseg].first = first; P.seg[P.nseg].count = count; P.nseg++; } }
int QrhHost::seg_total() const { int n = 0; for (int i = 0; i < P.nseg; i++) n += P.seg[i].count; return n; }
void QrhHost::side_launch() { if (P.nseg > 0) hipLaunchKernelGGL(qrh_side_only, dim3((unsigned)seg_total(), (unsigned)batch), dim3(512), 0, h->stream, P); P.nseg = 0; }
// the side work of the reflector at pj: column blocks of W from pj + 32 to near_end, then (with_qt) of Q^T; returns its
// workgroups when both phases run on their own
int QrhHost::side_of(int pj, int near_end, bool with_qt) {
  if (pj < 0) return 0;
  const int wide0 = pj + 2 * NB;
  P.wide0 = wide0; P.nrc = (P.M - pj + 511) / 512;
  P.nnw = wide0 < near_end ? (near_end - wide0 + NB - 1) / NB : 0;
  P.nqb = with_qt ? nq : 0;
  return ((P.nnw + 1) / 2 + (P.nqb + 1) / 2) * P.nrc;                            // a workgroup takes two adjacent column blocks
}
// ONE launch per panel (qrh_bc): phase A rides in front of B and C (first exchange: Gram partials + partial X of the next block);
// the row workgroups also take the next panel's columns through the previous reflector, so its side work (qrh_side_fused, W pairs
// then Q^T pairs) starts one block later
int QrhHost::panel(int j0, int near_end, bool with_qt, bool skip_x) {
  const int m = P.M - j0;
  if (pj0 >= 0) {
    // A flagged previous panel left no partials of X = V^T C for this panel's columns. They are formed here, over all rows, before
    // the panel's launch: inside it every row workgroup updates its rows of these columns in phase A, so a workgroup that formed X
    // over all rows there could read rows another workgroup had already updated (seen with batches: wrong columns from the panel
    // after a rank-deficient one). Not flagged: returns at once, the partials of the previous launch stay as they are.
    P.j0 = pj0; P.na_shift = 0;
    hipLaunchKernelGGL(qrh_x_flagged, dim3((unsigned)P.nxp, (unsigned)batch), dim3(512), 0, h->stream, P);
  }
  side_of(pj0, near_end, with_qt);
  P.j0 = j0; P.pj0 = pj0; P.skip_x = skip_x ? 1 : 0;
  const int nA = (m + NB + 511) / 512;
  const int sh = (pj0 >= 0 && !skip_x && j0 + NB < P.N) ? 1 : 0;
  const int nwp = pj0 >= 0 ? (P.nnw - sh + 1) / 2 : 0, nqp = pj0 >= 0 ? (P.nqb + 1) / 2 : 0;
  P.na_shift = sh;
  P.nrow = nA; P.nseg = 0; add_seg(SEG_F, 0, (nwp + nqp) * P.nrc);
  const dim3 gm((unsigned)(nA + seg_total()), (unsigned)batch);
  const auto kern = m <= 512 ? qrh_bc<1> : (m <= 1024 ? qrh_bc<2> : (m <= 2048 ? qrh_bc<4> : qrh_bc<0>));
  hipLaunchKernelGGL(kern, gm, dim3(512), 0, h->stream, P);
  // taller than the register-resident panel: a flagged panel is factorised by the global-memory panel kernel in a launch of its own
  if (m > 2048) nd4_qr_panel_flagged(h, batch, P.Wm, P.M, P.ld, P.strideW, P.Vall, P.ldv, P.strideV, P.Tall, P.strideT, P.taus, P.strideTau, j0, NB, P.flag);
  P.na_shift = 0;
  pj0 = j0; P.nxp = nA; P.nseg = 0; P.stamp_slot++;
  ND4_HIP(hipGetLastError());
  return 0;
}
// the last reflector: the 16 columns behind its panel (unless the caller's block update covers them), then its side work on its own
int QrhHost::finish(int near_end, bool with_qt, bool narrow) {
  if (pj0 < 0) return 0;
  if (narrow && pj0 + NB < P.N) {
    P.j0 = pj0; P.na_shift = 0;                         // a flagged panel left no partials of X behind
    hipLaunchKernelGGL(qrh_x_flagged, dim3((unsigned)P.nxp, (unsigned)batch), dim3(512), 0, h->stream, P);
    nd4_qr_narrow_apply(h, batch, P.Wm, P.M, P.N, P.ld, P.strideW, V, ldv, sV, T, sT, pj0, pj0 + NB, P.Xp, P.strideXp, P.nxp);
  }
  const int side_all = side_of(pj0, near_end, with_qt);
  P.pj0 = pj0;
  P.nseg = 0; add_seg(SEG_NX, 0, side_all); side_launch();
  add_seg(SEG_NA, 0, side_all); side_launch();
  pj0 = -1;
  ND4_HIP(hipGetLastError());
  return 0;
}
int QrhHost::dump_stamps() {                                      // debug: per launch, the stamps of workgroup 0 relative to the first one, in us
  if (!P.stamps) return 0;
  std::vector<long long> st((size_t)8 * P.stamp_slot);
  ND4_HIP(hipStreamSynchronize(h->stream));
  ND4_HIP(hipMemcpy(st.data(), P.stamps, sizeof(long long) * st.size(), hipMemcpyDeviceToHost));
  (void)hipFree(P.stamps); P.stamps = nullptr;
  for (int i = 0; i < P.stamp_slot; i++) {
    fprintf(stderr, "qrh stamp launch %d:", i);
    for (int k = 0; k < 8; k++) fprintf(stderr, " %.2f", st[i * 8 + k] ? (st[i * 8 + k] - st[0]) * 0.01 : 0.0);
    fprintf(stderr, "\n");
  }
  return 0;
}
