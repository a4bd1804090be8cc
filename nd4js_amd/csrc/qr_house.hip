// Householder panel kernels of the QR drivers (qr.hip) and what rides in their launches:
//   qr_panel, qr_panel_flagged       the global-memory panel on 1024 threads (any height; the fall-back of row-split panels > 2048 rows)
//   qr_panel_row                     thread-per-row, the panel in registers (m <= 2048; body: qr_panel_row_body.h)
//   qr_panel_row_la                  the same with the previous reflector's column blocks in the same launch (qr_colblock_update)
//   qr_narrow_x, qr_narrow_apply     the previous reflector on the next panel's 16 columns; qr_update_blocks: on the blocks left at the end
//   qr_panel_part, qr_t_assemble     2048 < m <= 8192: a 16-column slot in halves / quarters on 1024 threads, and its T put together
// The host launchers at the end are declared in qr_internal.h.
#include "qr_internal.h"
#include "qr_panel_row_body.h"
#include "dpp.h"
#include <type_traits>

namespace {

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}
// ------------------------------------------------------------------------------------ panel
// Slot i of lane group g is row j0 + g + 64*i; lane c of the group is column j0 + c.
struct Slots {
  double* base;        // &W[j0+g][j0+c]
  long step;           // 64 * ld
  int nslots;          // rows in range for this group
  bool col_ok;
  int g, M, j0;
  __device__ __forceinline__ int count() const { return nslots; }
  __device__ __forceinline__ bool valid(int i) const { return col_ok && (j0 + g + 64 * i) < M; }
  __device__ __forceinline__ double get(int i) const {
    return valid(i) ? base[i * step] : 0.0;
  }
  __device__ __forceinline__ void set(int i, double v) {
    if (valid(i)) base[i * step] = v;
  }
};

__device__ __forceinline__ void qr_panel_body(double* __restrict__ Wm, int M, long ld, long strideW,
                                              double* __restrict__ Vall, long ldv, long strideV,
                                              double* __restrict__ Tall, long strideT,
                                              double* __restrict__ taus, long strideTau, int j0, int nb) {
  __shared__ double s_red[16];
  __shared__ double s_w[16][NB];
  __shared__ double s_T[NB][NB + 1];
  __shared__ double s_Z[NB][NB];
  __shared__ double s_tau[NB];
  __shared__ double s_alpha;
  double* A = Wm + blockIdx.x * strideW;
  double* V = Vall + blockIdx.x * strideV;
  const int t = threadIdx.x;
  const int c = t & (NB - 1), g = t >> 4, wave = t >> 6;
  const int klane_base = t & 48;

  Slots S;
  S.base = A + (long)(j0 + g) * ld + j0 + c; S.step = 64 * ld; S.col_ok = c < nb; S.g = g; S.M = M; S.j0 = j0;
  S.nslots = (M - j0 - g + 63) / 64; if (S.nslots < 0) S.nslots = 0;
  if (t < NB * (NB + 1)) (&s_T[0][0])[t] = 0.0;
  __syncthreads();

  for (int k = 0; k < nb; k++) {
    // ---- 1. alpha = W[jc][jc], sigma = sum_{r > jc} W[r][jc]^2 (rows beyond M hold zeros) ----
    double part = 0.0;
    if (c == k) {
      const double x0 = S.get(0);
      if (g > k) part = x0 * x0;
      if (g == k) s_alpha = x0;
#pragma unroll
      for (int i = 1; i < S.count(); i++) { const double x = S.get(i); part += x * x; }
    }
    part = wave_sum(part);
    if ((t & 63) == 0) s_red[wave] = part;
    __syncthreads();
    double sigma = 0.0;
#pragma unroll
    for (int w = 0; w < 16; w++) sigma += s_red[w];
    const double alpha = s_alpha;
    double beta = alpha, tau = 0.0, scale = 0.0;
    if (!(sigma < QR_SIGMA_MIN)) {                                   // (0, tiny: no reflector; NaN: as before)
      beta = -copysign(sqrt(alpha * alpha + sigma), alpha);
      tau = (beta - alpha) / beta;
      scale = 1.0 / (alpha - beta);
    }
    // ---- 2. d_c = sum_r v_r * W[r][c]  (c > k: columns still to update; c < k: V_c^T v_k for T) ----
    double d = 0.0;
    {
      const double x = S.get(0);
      const double xk = __shfl(x, klane_base | k, 64);
      const double vr = (g > k) ? xk * scale : ((g == k) ? 1.0 : 0.0);
      d = vr * x;
    }
#pragma unroll
    for (int i = 1; i < S.count(); i++) {
      const double x = S.get(i);
      const double vr = __shfl(x, klane_base | k, 64) * scale;
      d += vr * x;
    }
    d += __shfl_xor(d, 16);
    d += __shfl_xor(d, 32);
    if ((t & 63) < NB) s_w[wave][c] = d;
    __syncthreads();
    double wc = 0.0;
#pragma unroll
    for (int w = 0; w < 16; w++) wc += s_w[w][c];
    // ---- 3. apply H_k to the columns right of k, store v_k in column k ----
    {
      const double x = S.get(0);
      const double xk = __shfl(x, klane_base | k, 64);
      const double vr = (g > k) ? xk * scale : ((g == k) ? 1.0 : 0.0);
      double y = x;
      if (c > k) y = x - tau * vr * wc;
      else if (c == k) y = (g > k) ? vr : ((g == k) ? beta : x);
      S.set(0, y);
    }
#pragma unroll
    for (int i = 1; i < S.count(); i++) {
      const double x = S.get(i);
      const double vr = __shfl(x, klane_base | k, 64) * scale;
      double y = x;
      if (c > k) y = x - tau * vr * wc;
      else if (c == k) y = vr;
      S.set(i, y);
    }
    // ---- 4. keep z_k = V[:,0:k]^T v_k and tau_k for T (built after the loop) ----
    if (t < k) s_Z[k][t] = wc;          // lane t < 16 has c == t
    if (t == 0) { s_tau[k] = tau; taus[blockIdx.x * strideTau + j0 + k] = tau; }
    // no barrier needed here: the next iteration's LDS writes all sit behind its own barriers
  }
  __syncthreads();
  // ---- T (larft, forward columnwise): T[i][i] = tau_i, T[i][k] = -tau_k * sum_{j=i}^{k-1} T[i][j] * z_k[j].
  // Row i of T depends only on row i -> thread i builds its row alone.
  if (t < nb) {
    double row[NB];
#pragma unroll
    for (int k = 0; k < NB; k++) row[k] = 0.0;
#pragma unroll
    for (int k = 0; k < NB; k++) {
      if (k == t) row[k] = s_tau[k];
      else if (k > t && k < nb) {
        double sum = 0.0;
#pragma unroll
        for (int j = 0; j < NB; j++) if (j >= t && j < k) sum += row[j] * s_Z[k][j];
        row[k] = -s_tau[k] * sum;
      }
    }
#pragma unroll
    for (int k = 0; k < NB; k++) s_T[t][k] = row[k];
  }
  __syncthreads();

  // ---- write back: R part (upper triangle incl. diagonal) stays in W, V goes to Vall explicitly ----
#pragma unroll
  for (int i = 0; i < S.count(); i++) {
    const int lr = g + 64 * i, r = j0 + lr;
    if (r < M && c < nb) {
      const double x = S.get(i);
      double* w = A + (long)r * ld + j0 + c;
      double* v = V + (long)r * ldv + j0 + c;
      if (lr <= c) { *w = x; *v = (lr == c) ? 1.0 : 0.0; }
      else { *w = 0.0; *v = x; }
    }
  }
  if (t < NB * NB) {
    const int i = t / NB, j = t % NB;
    Tall[blockIdx.x * strideT + (long)(j0 / NB) * NB * NB + t] = (i <= j && j < nb) ? s_T[i][j] : 0.0;
  }
}

// (<1, false> is the one instance: the template arguments are what is left of a register-resident form, kept because the
// kernel's name is what profiles, tools and the path tests know it by)
template <int R, bool REG>
__global__ __launch_bounds__(1024) void qr_panel(double* __restrict__ Wm, int M, long ld, long strideW,
                                                   double* __restrict__ Vall, long ldv, long strideV,
                                                   double* __restrict__ Tall, long strideT,
                                                   double* __restrict__ taus, long strideTau, int j0, int nb) {
  qr_panel_body(Wm, M, ld, strideW, Vall, ldv, strideV, Tall, strideT, taus, strideTau, j0, nb);
}
// the same panel, only for the matrices whose flag is set: the fall-back of a multi-workgroup panel taller than the register-resident
// kernel holds (m > 2048), as a launch of its own behind phase C (two short launches that do nothing in the common case)
__global__ __launch_bounds__(1024) void qr_panel_flagged(double* __restrict__ Wm, int M, long ld, long strideW,
                                                          double* __restrict__ Vall, long ldv, long strideV,
                                                          double* __restrict__ Tall, long strideT,
                                                          double* __restrict__ taus, long strideTau, int j0, int nb, const int* __restrict__ flag) {
  if (!flag[blockIdx.x]) return;
  qr_panel_body(Wm, M, ld, strideW, Vall, ldv, strideV, Tall, strideT, taus, strideTau, j0, nb);
}

template <int R, int NWV = 8>
__global__ __launch_bounds__(64 * NWV) void qr_panel_row(double* __restrict__ Wm, int M, long ld, long strideW,
                                                     double* __restrict__ Vall, long ldv, long strideV,
                                                     double* __restrict__ Tall, long strideT,
                                                     double* __restrict__ taus, long strideTau, int j0, int nb) {
  qr_panel_row_body<R, NWV>(blockIdx.x, Wm, M, ld, strideW, Vall, ldv, strideV, Tall, strideT, taus, strideTau, j0, nb);
}

// ---- look-ahead: the block reflector applied to ONE block of <= 16 columns by ONE workgroup ----
// C (m rows x nc columns) <- (I - V op(T) V^T) C is local to a column: X = V^T C (16 x nc; the waves split the rows, fixed-order
// LDS reduction), W = op(T) X, C -= V W, all on fp64 MFMA 16x16x4 fed straight from global memory. Because no other workgroup is
// involved, the update of the columns BEHIND the next panel can run in the same launch as the next panel's factorisation
// (qr_panel_row_la: the panel kernel keeps one workgroup busy for 30-50 us and the rest of the chip used to idle), and only the 16
// columns of the next panel itself are updated on the critical path (qr_update_narrow, one workgroup of 1024 threads).
// V: rows relative to the panel's first row, explicit zeros above the unit diagonal. s_X: NW * 256 + 256 doubles, s_Tm: 16 x 17.
template <int NT>
__device__ __forceinline__ void qr_colblock_update(double* __restrict__ s_X, double (*s_Tm)[NB + 1], const double* __restrict__ Tg, int trans,
                                                   const double* __restrict__ V, long ldv, double* __restrict__ C, long ldc, int m, int nc) {
  constexpr int NW = NT / 64;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, fx = lane & 15, fk = lane >> 4;
  if (t < NB * NB) s_Tm[t / NB][t % NB] = Tg[t];
  const int rpw = ((m + NW * 16 - 1) / (NW * 16)) * 16;            // rows per wave, a multiple of 16
  const int r0 = wave * rpw, r1 = (r0 + rpw < m) ? r0 + rpw : m;
  const bool cok = fx < nc;
  d4 acc0 = d4{0.0, 0.0, 0.0, 0.0}, acc1 = d4{0.0, 0.0, 0.0, 0.0};
  for (int rb = r0; rb < r1; rb += 64) {                           // 16 k-steps per batch: 32 loads in flight per lane
    double a[16], b[16];
#pragma unroll
    for (int kk = 0; kk < 16; kk++) {
      const int r = rb + kk * 4 + fk;
      const bool ok = r < r1;
      a[kk] = ok ? V[(long)r * ldv + fx] : 0.0;
      b[kk] = (ok && cok) ? C[(long)r * ldc + fx] : 0.0;
    }
#pragma unroll
    for (int kk = 0; kk < 16; kk += 2) {
      acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(a[kk], b[kk], acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(a[kk + 1], b[kk + 1], acc1, 0, 0, 0);
    }
  }
#pragma unroll
  for (int r = 0; r < 4; r++) s_X[wave * 256 + (fk + 4 * r) * 16 + fx] = acc0[r] + acc1[r];     // X[i = fk + 4r][j = fx]
  __syncthreads();
  double* s_Xs = s_X + NW * 256;                                  // the summed X, then W in its place
  if (t < 256) {
    double x = 0.0;
#pragma unroll
    for (int w = 0; w < NW; w++) x += s_X[w * 256 + t];           // fixed order
    s_Xs[t] = x;
  }
  __syncthreads();
  double wv = 0.0;
  if (t < 256) {
    const int i = t / 16, j = t % 16;
    if (trans) {
#pragma unroll
      for (int l = 0; l < NB; l++) wv += s_Tm[l][i] * s_Xs[l * 16 + j];
    } else {
#pragma unroll
      for (int l = 0; l < NB; l++) wv += s_Tm[i][l] * s_Xs[l * 16 + j];
    }
  }
  __syncthreads();
  if (t < 256) s_Xs[t] = -wv;                                     // -W[i][j]
  __syncthreads();
  double bw[4];
#pragma unroll
  for (int kk = 0; kk < 4; kk++) bw[kk] = s_Xs[(kk * 4 + fk) * 16 + fx];
  for (int rt = r0; rt < r1; rt += 64) {                          // four 16-row tiles per batch
    double av[4][4]; d4 c[4];
#pragma unroll
    for (int q = 0; q < 4; q++) {
      const int ra = rt + q * 16 + fx;
#pragma unroll
      for (int kk = 0; kk < 4; kk++) av[q][kk] = (ra < r1) ? V[(long)ra * ldv + kk * 4 + fk] : 0.0;
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const int rc = rt + q * 16 + fk + 4 * r;
        c[q][r] = (rc < r1 && cok) ? C[(long)rc * ldc + fx] : 0.0;
      }
    }
#pragma unroll
    for (int q = 0; q < 4; q++) {
#pragma unroll
      for (int kk = 0; kk < 4; kk++) c[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[q][kk], bw[kk], c[q], 0, 0, 0);
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const int rc = rt + q * 16 + fk + 4 * r;
        if (rc < r1 && cok) C[(long)rc * ldc + fx] = c[q][r];
      }
    }
  }
}

// The 16 columns of the NEXT panel are on the critical path, and one workgroup is bound there by the MFMA rate of a single CU
// (2 x 1 MFLOP at 2048 rows = 2 x 3.9 us; the one-workgroup form took 20 us per panel). Two small launches instead, the rows split over
// workgroups of 256: (x) partial X = V^T C per workgroup, (apply) every workgroup adds the partials in the same fixed order, forms
// W = op(T) X itself and updates its own rows. No device-scope fence: the launch boundary is the synchronisation.
__global__ __launch_bounds__(256) void qr_narrow_x(const double* __restrict__ Wm, int M, int N, long ld, long strideW,
                                                    const double* __restrict__ Vall, long ldv, long strideV, int pj0, int c0,
                                                    double* __restrict__ Xp, long strideXp) {
  __shared__ double s_X[4 * 256];
  const int mat = blockIdx.y, t = threadIdx.x, lane = t & 63, wave = t >> 6, fx = lane & 15, fk = lane >> 4;
  const int m = M - pj0, nc = N - c0 < NB ? N - c0 : NB;
  const double* V = Vall + mat * strideV + (long)pj0 * ldv + pj0;
  const double* C = Wm + mat * strideW + (long)pj0 * ld + c0;
  const int rb = blockIdx.x * 256 + wave * 64;
  const bool cok = fx < nc;
  double a[16], b[16];
#pragma unroll
  for (int kk = 0; kk < 16; kk++) {
    const int r = rb + kk * 4 + fk;
    const bool ok = r < m;
    a[kk] = ok ? V[(long)r * ldv + fx] : 0.0;
    b[kk] = (ok && cok) ? C[(long)r * ld + fx] : 0.0;
  }
  d4 acc0 = d4{0.0, 0.0, 0.0, 0.0}, acc1 = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int kk = 0; kk < 16; kk += 2) {
    acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(a[kk], b[kk], acc0, 0, 0, 0);
    acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(a[kk + 1], b[kk + 1], acc1, 0, 0, 0);
  }
#pragma unroll
  for (int r = 0; r < 4; r++) s_X[wave * 256 + (fk + 4 * r) * 16 + fx] = acc0[r] + acc1[r];
  __syncthreads();
  Xp[mat * strideXp + (long)blockIdx.x * 256 + t] = ((s_X[t] + s_X[256 + t]) + s_X[512 + t]) + s_X[768 + t];
}
__global__ __launch_bounds__(256) void qr_narrow_apply(double* __restrict__ Wm, int M, int N, long ld, long strideW,
                                                        const double* __restrict__ Vall, long ldv, long strideV,
                                                        const double* __restrict__ Tall, long strideT, int pj0, int c0,
                                                        const double* __restrict__ Xp, long strideXp, int nparts) {
  __shared__ double s_Xs[256];
  __shared__ double s_Tm[NB][NB + 1];
  const int mat = blockIdx.y, t = threadIdx.x, lane = t & 63, wave = t >> 6, fx = lane & 15, fk = lane >> 4;
  const int m = M - pj0, nc = N - c0 < NB ? N - c0 : NB;
  const double* V = Vall + mat * strideV + (long)pj0 * ldv + pj0;
  double* C = Wm + mat * strideW + (long)pj0 * ld + c0;
  const int rt = blockIdx.x * 256 + wave * 64;
  const bool cok = fx < nc;
  // this workgroup's rows first: their latency overlaps the small W computation
  double av[4][4]; d4 c[4];
#pragma unroll
  for (int q = 0; q < 4; q++) {
    const int ra = rt + q * 16 + fx;
#pragma unroll
    for (int kk = 0; kk < 4; kk++) av[q][kk] = (ra < m) ? V[(long)ra * ldv + kk * 4 + fk] : 0.0;
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const int rc = rt + q * 16 + fk + 4 * r;
      c[q][r] = (rc < m && cok) ? C[(long)rc * ld + fx] : 0.0;
    }
  }
  s_Tm[t / NB][t % NB] = Tall[mat * strideT + (long)(pj0 / NB) * NB * NB + t];
  double x = 0.0;
  if (nparts <= 0) nparts = (int)gridDim.x;                                                    // qr_narrow_x: one partial per workgroup
  for (int g = 0; g < nparts; g++) x += Xp[mat * strideXp + (long)g * 256 + t];               // fixed order, the same in every workgroup
  s_Xs[t] = x;
  __syncthreads();
  double wv = 0.0;
  {
    const int i = t / 16, j = t % 16;
#pragma unroll
    for (int l = 0; l < NB; l++) wv += s_Tm[l][i] * s_Xs[l * 16 + j];            // T^T X (T: full 16 x 16, see qrh_bc)
  }
  __syncthreads();
  s_Xs[t] = -wv;
  __syncthreads();
  double bw[4];
#pragma unroll
  for (int kk = 0; kk < 4; kk++) bw[kk] = s_Xs[(kk * 4 + fk) * 16 + fx];
#pragma unroll
  for (int q = 0; q < 4; q++) {
#pragma unroll
    for (int kk = 0; kk < 4; kk++) c[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[q][kk], bw[kk], c[q], 0, 0, 0);
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const int rc = rt + q * 16 + fk + 4 * r;
      if (rc < m && cok) C[(long)rc * ld + fx] = c[q][r];
    }
  }
}

// panel `pnl` (first row/column j0, workgroup 0 of a matrix) together with the previous panel's block reflector applied to the columns
// from `wc0` on, one workgroup per block of 16 columns (workgroups 1..). trans = 1 throughout (H^T C during the factorisation).
template <int R>
__global__ __launch_bounds__(512) void qr_panel_row_la(double* __restrict__ Wm, int M, int N, long ld, long strideW,
                                                        double* __restrict__ Vall, long ldv, long strideV,
                                                        double* __restrict__ Tall, long strideT,
                                                        double* __restrict__ taus, long strideTau, int j0, int nb, int pj0, int wc0, int nwide,
                                                        double* __restrict__ QT, long strideQT) {
  const int mat = blockIdx.y;
  if (blockIdx.x == 0) {
    qr_panel_row_body<R>(mat, Wm, M, ld, strideW, Vall, ldv, strideV, Tall, strideT, taus, strideTau, j0, nb);
    return;
  }
  __shared__ double s_X[8 * 256 + 256];
  __shared__ double s_Tm[NB][NB + 1];
  const int bx = (int)blockIdx.x - 1;
  const double* Tg = Tall + mat * strideT + (long)(pj0 / NB) * NB * NB;
  const double* Vp = Vall + mat * strideV + (long)pj0 * ldv + pj0;
  if (bx < nwide) {
    const int c0 = wc0 + bx * NB;
    qr_colblock_update<512>(s_X, s_Tm, Tg, 1, Vp, ldv, Wm + mat * strideW + (long)pj0 * ld + c0, ld, M - pj0, N - c0 < NB ? N - c0 : NB);
  } else {
    // Q^T = H_p^T ... H_0^T I is the same column-local update as the trailing columns ([A | I] -> [R | Q^T]): the reflectors reach an
    // M x M accumulator in the shadow of the panels instead of being multiplied together after the factorisation
    const int c0 = (bx - nwide) * NB;
    qr_colblock_update<512>(s_X, s_Tm, Tg, 1, Vp, ldv, QT + mat * strideQT + (long)pj0 * M + c0, M, M - pj0, M - c0 < NB ? M - c0 : NB);
  }
}
// the block reflector of the panel at pj0 applied to the column blocks from wc0 on (grid.x blocks): wide form (512 threads per block
// of 16 columns) and narrow form (ONE block on 1024 threads: the next panel's columns, on the critical path)
template <int NT>
__global__ __launch_bounds__(NT) void qr_update_blocks(double* __restrict__ Cm, int M, int ncols, long ld, long strideC,
                                                        const double* __restrict__ Vall, long ldv, long strideV,
                                                        const double* __restrict__ Tall, long strideT, int pj0, int wc0) {
  __shared__ double s_X[(NT / 64) * 256 + 256];
  __shared__ double s_Tm[NB][NB + 1];
  const int mat = blockIdx.y;
  const int c0 = wc0 + (int)blockIdx.x * NB;
  const int nc = ncols - c0 < NB ? ncols - c0 : NB;
  qr_colblock_update<NT>(s_X, s_Tm, Tall + mat * strideT + (long)(pj0 / NB) * NB * NB, 1,
                         Vall + mat * strideV + (long)pj0 * ldv + pj0, ldv, Cm + mat * strideC + (long)pj0 * ld + c0, ld, M - pj0, nc);
}

// ---- the same panel kernel for taller panels: 1024 threads leave 128 VGPRs per lane = R rows of W columns with R * W = 32:
// 2048 < m <= 4096 rows: R = 4, W = 8; 4096 < m <= 8192 rows: R = 8, W = 4.
// A 16-column panel slot is then factorised in parts (two 8-column halves / four 4-column quarters).
// Every part writes ONLY its own triangular factor into the live T slot (zeros elsewhere), so that the ordinary
// block-reflector machinery applies just this part's reflectors to the remaining columns of the slot, and also into a
// side slot that collects the diagonal blocks; qr_t_assemble then builds the full 16 x 16 factor from them and V^T V.
template <int W> __device__ __forceinline__ double qr_xor_lanes(double v) {       // value of lane ^ W inside a row of 16 lanes
  if constexpr (W == 1) return nd4dpp::xor1(v);
  else if constexpr (W == 2) return nd4dpp::xor2(v);
  else if constexpr (W == 4) return nd4dpp::xor4(v);
  else return nd4dpp::xor8(v);
}
template <int R, int W8>
__global__ __launch_bounds__(1024) void qr_panel_part(double* __restrict__ Wm, int M, long ld, long strideW,
                                                     double* __restrict__ Vall, long ldv, long strideV,
                                                     double* __restrict__ Tall, double* __restrict__ Tside, long strideT,
                                                     double* __restrict__ taus, long strideTau, int c0, int nb) {
  constexpr int NW = 16;                               // waves per workgroup (W8 = columns of this kernel)
  static_assert(W8 == 8 || W8 == 4, "two halves or four quarters of a 16-column slot");
  __shared__ double s_red[NW];
  __shared__ double s_w[NW][W8];
  __shared__ double s_T[W8][W8 + 1];
  __shared__ double s_Z[W8][W8];
  __shared__ double s_tau[W8];
  const int j0 = c0;                                   // rows and columns of this half start at its own diagonal
  __shared__ double s_alpha;
  double* A = Wm + blockIdx.x * strideW;
  double* V = Vall + blockIdx.x * strideV;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const bool b0 = lane & 1, b1 = lane & 2, b2 = lane & 4;
  const int mycol = W8 == 8 ? (b0 ? 4 : 0) + (b1 ? 2 : 0) + (b2 ? 1 : 0) : (b0 ? 2 : 0) + (b1 ? 1 : 0);   // column this lane ends up with

  double a[R][W8];
#pragma unroll
  for (int i = 0; i < R; i++) {
    const int r = j0 + t + 1024 * i;
#pragma unroll
    for (int c = 0; c < W8; c++) a[i][c] = 0.0;
    if (r < M) {
      const double* src = A + (long)r * ld + j0;
      if (nb == W8 && (ld & 1) == 0) {                   // 16-byte loads of the lane's own 128-B row segment
#pragma unroll
        for (int c = 0; c < W8; c += 2) { const double2 v = *reinterpret_cast<const double2*>(src + c); a[i][c] = v.x; a[i][c + 1] = v.y; }
      } else {
#pragma unroll
        for (int c = 0; c < W8; c++) if (c < nb) a[i][c] = src[c];
      }
    }
  }
  if (t < W8 * (W8 + 1)) (&s_T[0][0])[t] = 0.0;

  // one column step per compile-time k (generic lambda, see lu.hip: convergent DPP ops block `#pragma unroll`)
  auto column_step = [&](auto kc) __attribute__((always_inline)) {
    constexpr int k = decltype(kc)::value;
    if (k < nb) {
      const int jc = j0 + k;
      double part = 0.0;
#pragma unroll
      for (int i = 0; i < R; i++) {
        const int r = j0 + t + 1024 * i;
        if (i > 0 || r > jc) part += a[i][k] * a[i][k];              // row slots >= 1 are always below row jc
      }
      if (t == k) s_alpha = a[0][k];
      part = nd4dpp::wave_sum(part);
      if (lane == 0) s_red[wave] = part;
      __syncthreads();
      double sigma = 0.0;
#pragma unroll
      for (int w = 0; w < NW; w++) sigma += s_red[w];
      const double alpha = s_alpha;
      double beta = alpha, tau = 0.0, scale = 0.0;
      if (!(sigma < QR_SIGMA_MIN)) {                                   // (0, tiny: no reflector; NaN: as before)
        // sqrt and the two divisions sit on the column's critical path (~100 dependent instructions): one rsqrt and one
        // rcp with two Newton steps each instead. The work copy is normalised to max|a| in [1,2), so nothing over/underflows;
        // a few ulp in (beta, tau, scale) perturb H by a few ulp, like the rounding of the update itself.
        const double nn = alpha * alpha + sigma, ri = nd4dpp::fast_rsqrt(nn);
        beta = -copysign(nn * ri, alpha);
        tau = (beta - alpha) * -copysign(ri, alpha);
        scale = nd4dpp::fast_rcp(alpha - beta);
      }
      double vr[R], d[W8];
#pragma unroll
      for (int c = 0; c < W8; c++) d[c] = 0.0;
#pragma unroll
      for (int i = 0; i < R; i++) {
        const int r = j0 + t + 1024 * i;
        vr[i] = (i > 0 || r > jc) ? a[i][k] * scale : ((r == jc) ? 1.0 : 0.0);
#pragma unroll
        for (int c = 0; c < W8; c++) d[c] += vr[i] * a[i][c];
      }
      // halving butterfly over the W8 lanes of a group (W8/2 + ... + 1 exchanges), then across the groups of the wave
      double e4[4], e2[2], e1;
      if constexpr (W8 == 8) {
#pragma unroll
        for (int j = 0; j < 4; j++) { const double snd = b0 ? d[j] : d[j + 4], kp = b0 ? d[j + 4] : d[j]; e4[j] = kp + nd4dpp::xor1(snd); }
      } else {
#pragma unroll
        for (int j = 0; j < 4; j++) e4[j] = d[j];
      }
      {
        const bool bb = W8 == 8 ? b1 : b0;
#pragma unroll
        for (int j = 0; j < 2; j++) { const double snd = bb ? e4[j] : e4[j + 2], kp = bb ? e4[j + 2] : e4[j]; e2[j] = kp + qr_xor_lanes<W8 / 4>(snd); }
      }
      { const bool bb = W8 == 8 ? b2 : b1; const double snd = bb ? e2[0] : e2[1], kp = bb ? e2[1] : e2[0]; e1 = kp + qr_xor_lanes<W8 / 2>(snd); }
      if constexpr (W8 == 4) e1 += nd4dpp::xor4(e1);
      e1 += nd4dpp::xor8(e1);
      e1 += __shfl_xor(e1, 16);
      e1 += __shfl_xor(e1, 32);
      if (lane < W8) s_w[wave][mycol] = e1;
      __syncthreads();
      double tot = 0.0;                                   // lane -> column lane & (W8 - 1)
#pragma unroll
      for (int w = 0; w < NW; w++) tot += s_w[w][lane & (W8 - 1)];
      double wv[W8];                                      // wave-uniform totals
#define ND4_RL(C) wv[C] = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(tot), C), __builtin_amdgcn_readlane(__double2loint(tot), C));
      ND4_RL(0) ND4_RL(1) ND4_RL(2) ND4_RL(3)
      if constexpr (W8 == 8) { ND4_RL(4) ND4_RL(5) ND4_RL(6) ND4_RL(7) }
#undef ND4_RL
#pragma unroll
      for (int i = 0; i < R; i++) {
        const int r = j0 + t + 1024 * i;
        const double tv = tau * vr[i];
#pragma unroll
        for (int c = k + 1; c < W8; c++) a[i][c] -= tv * wv[c];
        a[i][k] = (i > 0 || r > jc) ? vr[i] : ((r == jc) ? beta : a[i][k]);
      }
      if (t == 0) {
#pragma unroll
        for (int c = 0; c < W8; c++) if (c < k) s_Z[k][c] = wv[c];
        s_tau[k] = tau;
        taus[blockIdx.x * strideTau + j0 + k] = tau;
      }
    }
    __builtin_amdgcn_sched_barrier(0);
  };
#define ND4_STEP(K) column_step(std::integral_constant<int, K>{});
  ND4_STEP(0) ND4_STEP(1) ND4_STEP(2) ND4_STEP(3)
  if constexpr (W8 == 8) { ND4_STEP(4) ND4_STEP(5) ND4_STEP(6) ND4_STEP(7) }
#undef ND4_STEP
  __syncthreads();
  if (t < nb) {                                          // larft: row t of T depends only on row t
    double row[W8];
#pragma unroll
    for (int k = 0; k < W8; k++) row[k] = 0.0;
#pragma unroll
    for (int k = 0; k < W8; k++) {
      if (k == t) row[k] = s_tau[k];
      else if (k > t && k < nb) {
        double sum = 0.0;
#pragma unroll
        for (int j = 0; j < W8; j++) if (j >= t && j < k) sum += row[j] * s_Z[k][j];
        row[k] = -s_tau[k] * sum;
      }
    }
#pragma unroll
    for (int k = 0; k < W8; k++) s_T[t][k] = row[k];
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < R; i++) {
    const int lr = t + 1024 * i, r = j0 + lr;
    if (r < M) {
      double* w = A + (long)r * ld + j0;
      double* v = V + (long)r * ldv + j0;
      double wv[W8], vv[W8];
#pragma unroll
      for (int c = 0; c < W8; c++) {
        wv[c] = (lr <= c) ? a[i][c] : 0.0;                       // R part (upper triangle incl. diagonal)
        vv[c] = (lr < c) ? 0.0 : ((lr == c) ? 1.0 : a[i][c]);    // explicit reflector: zeros above, unit diagonal
      }
      if (nb == W8 && (ld & 1) == 0) {
#pragma unroll
        for (int c = 0; c < W8; c += 2) {
          *reinterpret_cast<double2*>(w + c) = double2{wv[c], wv[c + 1]};
          *reinterpret_cast<double2*>(v + c) = double2{vv[c], vv[c + 1]};
        }
      } else {
#pragma unroll
        for (int c = 0; c < W8; c++) if (c < nb) { w[c] = wv[c]; v[c] = vv[c]; }
      }
    }
  }
  if (t < 16 * 16) {                                     // the 16 x 16 slot of the enclosing panel
    const int slot0 = (c0 / 16) * 16, part = (c0 - slot0) / W8;
    const int i = t / 16, j = t % 16;
    const long so = blockIdx.x * strideT + (long)(slot0 / 16) * 256;
    const bool mine = (i / W8 == part) && (j / W8 == part);
    const double val = (mine && (i % W8) <= (j % W8) && (j % W8) < nb) ? s_T[i % W8][j % W8] : 0.0;
    Tall[so + t] = val;                                  // live slot: ONLY this part's block (the partial block reflector)
    if (mine) Tside[so + t] = val;                       // side slot: collects the diagonal blocks of all parts
  }
}

// Full 16 x 16 triangular factor of a slot that was factorised in parts of bs columns: the diagonal blocks come from the
// side slot, the rest from T[1,2] = -T1 (V1^T V2) T2 applied level by level (groups of bs, 2 bs, ... columns); G = V^T V of
// the slot's 16 reflector columns (row-major 16 x 16). One small workgroup per matrix.
__global__ __launch_bounds__(256) void qr_t_assemble(double* __restrict__ Tall, const double* __restrict__ Tside, long strideT, int panel,
                                                      const double* __restrict__ Gm, long sG, int bs) {
  __shared__ double s_t[16][17], s_g[16][17], s_x[16][17];
  const long so = blockIdx.x * strideT + (long)panel * 256;
  const int t = threadIdx.x, i = t / 16, j = t % 16;
  s_t[i][j] = Tside[so + t];
  s_g[i][j] = Gm[blockIdx.x * sG + t];
  __syncthreads();
  for (int b = bs; b < 16; b *= 2) {
    // thread (i, j) with i in the first group of its pair and j in the second: x = (G12 T2)[i][j], then T12 = -T1 x
    const int pair0 = (i / (2 * b)) * 2 * b;
    const bool on = (i - pair0) < b && j >= pair0 + b && j < pair0 + 2 * b;
    double x = 0.0;
    if (on) for (int q = pair0 + b; q < pair0 + 2 * b; q++) x += s_g[i][q] * s_t[q][j];
    s_x[i][j] = x;
    __syncthreads();
    double y = 0.0;
    if (on) for (int q = pair0; q < pair0 + b; q++) y += s_t[i][q] * s_x[q][j];
    __syncthreads();
    if (on) s_t[i][j] = -y;
    __syncthreads();
  }
  Tall[so + t] = s_t[i][j];
}

using qr_panel_row_fn = decltype(&qr_panel_row<1, 8>);
qr_panel_row_fn qr_panel_row_for(QrPanelShape s) {
  if (s.NWV == 1) return qr_panel_row<4, 1>;
  if (s.NWV == 2) return qr_panel_row<4, 2>;
  if (s.NWV == 4) return qr_panel_row<4, 4>;
  return s.R == 1 ? qr_panel_row<1> : (s.R == 2 ? qr_panel_row<2> : qr_panel_row<4>);
}

}  // namespace

// The panel of m <= 2048 rows for `batch` matrices. One matrix is a latency problem: many waves with few rows each (R = 1, 2, 4 on
// 512 threads). A batch that fills the chip is a throughput problem: the same body on FEW waves with four rows per thread
// (128 threads for m <= 512, 256 for m <= 1024: 194 VGPRs, so four / two workgroups share a CU, their barriers cost next to nothing
// and a column step is ~530 instructions of ONE wave) — 2048 panels of 512 rows: 220 -> 151 us, 4096 of 256 rows: 315 -> 154 us
// (bench ops.qr_panel). All three shapes then run at the same 1.75 TB/s: the launch is bound by the instruction issue of the
// 4096 wave-panels (8500 instructions each, two waves per SIMD); forcing three waves per SIMD spills (196 us).
QrPanelShape nd4_qr_panel_shape(int batch, int m) {
  const bool many = batch >= QR_SMALL_WG_BATCH;
  if (many && m <= 256) return {4, 1};
  if (many && m <= 512) return {4, 2};
  if (many && m <= 1024) return {4, 4};
  if (m <= 512) return {1, 8};
  if (m <= 1024) return {2, 8};
  return {4, 8};
}

void nd4_qr_panel_global(nd4hip_handle* h, int batch, double* W, int M, long ld, long sW, double* V, long ldv, long sV,
                         double* T, long sT, double* taus, long sTau, int j0, int nb) {
  hipLaunchKernelGGL((qr_panel<1, false>), dim3(batch), dim3(1024), 0, h->stream, W, M, ld, sW, V, ldv, sV, T, sT, taus, sTau, j0, nb);
}
void nd4_qr_panel_flagged(nd4hip_handle* h, int batch, double* W, int M, long ld, long sW, double* V, long ldv, long sV,
                          double* T, long sT, double* taus, long sTau, int j0, int nb, const int* flag) {
  hipLaunchKernelGGL(qr_panel_flagged, dim3((unsigned)batch), dim3(1024), 0, h->stream, W, M, ld, sW, V, ldv, sV, T, sT, taus, sTau, j0, nb, flag);
}
void nd4_qr_panel_rows(nd4hip_handle* h, int batch, double* W, int M, int m, long ld, long sW, double* V, long ldv, long sV,
                       double* T, long sT, double* taus, long sTau, int j0, int nb) {
  const QrPanelShape s = nd4_qr_panel_shape(batch, m);
  hipLaunchKernelGGL(qr_panel_row_for(s), dim3(batch), dim3(64 * s.NWV), 0, h->stream, W, M, ld, sW, V, ldv, sV, T, sT, taus, sTau, j0, nb);
}
void nd4_qr_panel_row_la(nd4hip_handle* h, int batch, int nwg, double* W, int M, int N, long ld, long sW, double* V, long ldv, long sV,
                         double* T, long sT, double* taus, long sTau, int j0, int nb, int pj0, int wc0, int nwide, double* QT, long sQT) {
  const int m = M - j0;
  const auto kern = m <= 512 ? qr_panel_row_la<1> : (m <= 1024 ? qr_panel_row_la<2> : qr_panel_row_la<4>);
  hipLaunchKernelGGL(kern, dim3((unsigned)nwg, (unsigned)batch), dim3(512), 0, h->stream, W, M, N, ld, sW, V, ldv, sV, T, sT, taus, sTau, j0, nb, pj0, wc0, nwide, QT, sQT);
}
void nd4_qr_narrow_x(nd4hip_handle* h, int batch, const double* W, int M, int N, long ld, long sW, const double* V, long ldv, long sV,
                     int pj0, int c0, double* Xp, long sXp) {
  hipLaunchKernelGGL(qr_narrow_x, dim3((unsigned)((M - pj0 + 255) / 256), (unsigned)batch), dim3(256), 0, h->stream, W, M, N, ld, sW, V, ldv, sV, pj0, c0, Xp, sXp);
}
void nd4_qr_narrow_apply(nd4hip_handle* h, int batch, double* W, int M, int N, long ld, long sW, const double* V, long ldv, long sV,
                         const double* T, long sT, int pj0, int c0, const double* Xp, long sXp, int nparts) {
  hipLaunchKernelGGL(qr_narrow_apply, dim3((unsigned)((M - pj0 + 255) / 256), (unsigned)batch), dim3(256), 0, h->stream,
                     W, M, N, ld, sW, V, ldv, sV, T, sT, pj0, c0, Xp, sXp, nparts);
}
void nd4_qr_update_blocks(nd4hip_handle* h, int batch, int nblocks, double* C, int M, int ncols, long ld, long sC,
                          const double* V, long ldv, long sV, const double* T, long sT, int pj0, int wc0) {
  hipLaunchKernelGGL(qr_update_blocks<512>, dim3((unsigned)nblocks, (unsigned)batch), dim3(512), 0, h->stream, C, M, ncols, ld, sC, V, ldv, sV, T, sT, pj0, wc0);
}
void nd4_qr_panel_part(nd4hip_handle* h, int batch, int w, double* W, int M, long ld, long sW, double* V, long ldv, long sV,
                       double* T, double* Tside, long sT, double* taus, long sTau, int c0, int nb) {
  const auto kern = w == 8 ? qr_panel_part<4, 8> : qr_panel_part<8, 4>;
  hipLaunchKernelGGL(kern, dim3(batch), dim3(1024), 0, h->stream, W, M, ld, sW, V, ldv, sV, T, Tside, sT, taus, sTau, c0, nb);
}
void nd4_qr_t_assemble(nd4hip_handle* h, int batch, double* T, const double* Tside, long sT, int panel, const double* G, long sG, int bs) {
  hipLaunchKernelGGL(qr_t_assemble, dim3(batch), dim3(256), 0, h->stream, T, Tside, sT, panel, G, sG, bs);
}
