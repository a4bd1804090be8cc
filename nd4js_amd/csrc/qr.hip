// Blocked Householder QR with explicit Q on row-major fp64 matrices, batched, with the reference's
// Givens sign convention restored afterwards.
//
// Replaces src/la/qr.js:27-77 (qr_decomp_full, Givens, cache-blocked loop order) / :80-145
// (qr_decomp). The GPU algorithm is different (compact-WY Householder); the contract that is kept
// is the OUTPUT: for M <= N the reference's plane rotations give R_jj = +norm
// for every column that had something eliminated below it and det(Q) = +1, so
//   qr_signfix flips column j of Q / row j of R where tau_j != 0 and R_jj < 0, and then, if the
//   parity of (#reflectors + #flips) is odd, flips the last column of Q / last row of R.
//
// Per block column of width NB = 16 (work matrix W, reflectors kept explicitly in Vall):
//   qr_panel   geqr2 + larft for rows [j0,M) x cols [j0,j0+nb) by ONE workgroup: 16 lanes own a
//              row (one lane per panel column, coalesced 128-B rows), the panel stays in registers
//              (<= 48 rows per lane group). Column norm = wave shuffle reduction + LDS across waves;
//              the 16 dot products v^T [panel] of a step are reduced together (shuffle over the 4 row
//              groups of a wave, LDS across the 16 waves) and give both the update of the columns to
//              the right and the new column of T (V^T v).
//   qr_vtc     Wp = V^T C for the trailing columns: fp64 MFMA 16x16x4 fed straight from global
//              memory (both operands are "4 rows x 16 contiguous doubles" fragments), 256-row chunks
//              combined through LDS, chunk partials summed in
//   qr_tw      W2 = op(T) * sum_chunks(Wp)  (one thread per column)
//   nd4_gemm   C -= V * W2 (gemm.hip, K = 16)
// Q is formed by applying the block reflectors backwards to the identity with the same kernels.
#include "nd4hip_internal.h"
#include <cstdlib>
#include "dpp.h"
#include "xchg.h"
#include <type_traits>
#include <cfloat>

typedef double d4 __attribute__((ext_vector_type(4)));

namespace {

constexpr int NB = 16;
constexpr int RMAX = 48;   // (slots per lane group of the global-memory fallback panel)
[[maybe_unused]] constexpr int RMAX_USED = RMAX;
// A reflector is formed only when the column below the diagonal has sum of squares sigma >= QR_SIGMA_MIN (or is not finite). The work
// copy is normalised to max|a| in [1, 2), but a column can still shrink far below that: with bitwise identical columns (a matrix of
// ones) every reflector leaves the next column at eps times the previous one, and after ~10 columns the squares are subnormal. sigma
// and alpha^2 then carry only a few bits, beta and tau stop matching v, and H = I - tau v v^T is no longer orthogonal (Q of
// ones(96, 80) was off by 1e-3). Below 2^-960 the column (norm < 2^-480 against a max of 1) is left as it is (tau = 0, like an
// exactly zero column): a backward error far below eps. At or above it the subnormal terms change sigma by < 2^-90 relatively.
constexpr double QR_SIGMA_MIN = 0x1p-960;
constexpr int VTC_ROWS = 256;     // rows per workgroup of qr_vtc
constexpr int VTC_COLS = 64;      // columns per workgroup of qr_vtc

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

// ------------------------------------------------------------------------------------ panel
// Slot i of lane group g is row j0 + g + 64*i; lane c of the group is column j0 + c.
template <int R, bool REG>
struct Slots {
  double a[REG ? R : 1];
  double* base;        // &W[j0+g][j0+c]
  long step;           // 64 * ld
  int nslots;          // rows in range for this group (GLOBAL mode bound)
  bool col_ok;
  int g, M, j0;
  __device__ __forceinline__ int count() const { return REG ? R : nslots; }
  __device__ __forceinline__ bool valid(int i) const { return col_ok && (j0 + g + 64 * i) < M; }
  __device__ __forceinline__ double get(int i) const {
    if constexpr (REG) return a[i];
    else return valid(i) ? base[i * step] : 0.0;
  }
  __device__ __forceinline__ void set(int i, double v) {
    if constexpr (REG) a[i] = v;
    else if (valid(i)) base[i * step] = v;
  }
};

template <int R, bool REG>
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

  Slots<R, REG> S;
  S.base = A + (long)(j0 + g) * ld + j0 + c; S.step = 64 * ld; S.col_ok = c < nb; S.g = g; S.M = M; S.j0 = j0;
  S.nslots = (M - j0 - g + 63) / 64; if (S.nslots < 0) S.nslots = 0;
  if constexpr (REG) {
#pragma unroll
    for (int i = 0; i < R; i++) S.a[i] = S.valid(i) ? S.base[i * S.step] : 0.0;
  }
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

template <int R, bool REG>
__global__ __launch_bounds__(1024) void qr_panel(double* __restrict__ Wm, int M, long ld, long strideW,
                                                   double* __restrict__ Vall, long ldv, long strideV,
                                                   double* __restrict__ Tall, long strideT,
                                                   double* __restrict__ taus, long strideTau, int j0, int nb) {
  qr_panel_body<R, REG>(Wm, M, ld, strideW, Vall, ldv, strideV, Tall, strideT, taus, strideTau, j0, nb);
}
// the same panel, only for the matrices whose flag is set: the fall-back of a multi-workgroup panel taller than the register-resident
// kernel holds (m > 2048), as a launch of its own behind phase C (two short launches that do nothing in the common case)
__global__ __launch_bounds__(1024) void qr_panel_flagged(double* __restrict__ Wm, int M, long ld, long strideW,
                                                          double* __restrict__ Vall, long ldv, long strideV,
                                                          double* __restrict__ Tall, long strideT,
                                                          double* __restrict__ taus, long strideTau, int j0, int nb, const int* __restrict__ flag) {
  if (!flag[blockIdx.x]) return;
  qr_panel_body<1, false>(Wm, M, ld, strideW, Vall, ldv, strideV, Tall, strideT, taus, strideTau, j0, nb);
}

// ---- thread-per-row panel kernel (m <= 2048): each of 512 threads keeps R whole panel rows in registers ----
// Row r = j0 + t + 512*i. Per column k (fully unrolled -> static register indices, 2 barriers):
//   sigma = sum_{r>jc} a[r][k]^2        wave shuffle reduction + 8 LDS partials
//   d[c]  = sum_r v_r a[r][c], c=0..15  per-thread partials, then a HALVING butterfly: 8+4+2+1 shuffles leave
//                                       one column total per lane (+2 to finish the wave), 8 LDS partials per
//                                       column, and the 16 totals come back as wave-uniform readlane values
//   update a[r][c>k] -= tau v_r d[c];  a[r][k] = v_r;  z_k = d[c<k] feeds T.
template <int R, int NWV = 8>
__device__ __forceinline__ void qr_panel_row_body(const int mat, double* __restrict__ Wm, int M, long ld, long strideW,
                                                  double* __restrict__ Vall, long ldv, long strideV,
                                                  double* __restrict__ Tall, long strideT,
                                                  double* __restrict__ taus, long strideTau, int j0, int nb) {
  constexpr int TT = 64 * NWV;               // threads of the workgroup: row of (thread t, slot i) = j0 + t + TT * i
  __shared__ double s_w[2][NWV][NB];        // per-wave column sums, double-buffered by column parity (one barrier per column)
  __shared__ double s_top[2][NB];         // row jc of the tile as it stands before column k's reflector
  __shared__ double s_T[NB][NB + 1];
  __shared__ double s_Z[NB][NB];
  __shared__ double s_tau[NB];
  double* A = Wm + mat * strideW;
  double* V = Vall + mat * strideV;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const bool b0 = lane & 1, b1 = lane & 2, b2 = lane & 4, b3 = lane & 8;
  const int mycol = (b0 ? 8 : 0) + (b1 ? 4 : 0) + (b2 ? 2 : 0) + (b3 ? 1 : 0);   // column this lane ends up with

  double a[R][NB];
#pragma unroll
  for (int i = 0; i < R; i++) {
    const int r = j0 + t + TT * i;
#pragma unroll
    for (int c = 0; c < NB; c++) a[i][c] = 0.0;
    if (r < M) {
      const double* src = A + (long)r * ld + j0;
      if (nb == NB && (ld & 1) == 0) {                   // 16-byte loads of the lane's own 128-B row segment
#pragma unroll
        for (int c = 0; c < NB; c += 2) { const double2 v = *reinterpret_cast<const double2*>(src + c); a[i][c] = v.x; a[i][c + 1] = v.y; }
      } else {
#pragma unroll
        for (int c = 0; c < NB; c++) if (c < nb) a[i][c] = src[c];
      }
    }
  }
  for (int e = t; e < NB * (NB + 1); e += TT) (&s_T[0][0])[e] = 0.0;

  // one column step per compile-time k (generic lambda, see lu.hip: convergent DPP ops block `#pragma unroll`)
  auto column_step = [&](auto kc) __attribute__((always_inline)) {
    constexpr int k = decltype(kc)::value;
    if (k < nb) {
      const int jc = j0 + k;
      // ONE reduction per column: p[c] = sum_{r > jc} a[r][k] a[r][c] for all 16 columns. p[k] is the sigma of the reflector, and
      // with v = (1, scale * a[r > jc][k]) the products v^T a_c are scale * p[c] + a[jc][c] (columns c < k hold earlier
      // reflectors: the same expression gives the z_k that T needs). The norm used to be a reduction and a barrier of its own.
      double d[NB];
#pragma unroll
      for (int c = 0; c < NB; c++) d[c] = 0.0;
#pragma unroll
      for (int i = 0; i < R; i++) {
        const int r = j0 + t + TT * i;
        const double ak = (i > 0 || r > jc) ? a[i][k] : 0.0;           // row slots >= 1 are always below row jc
#pragma unroll
        for (int c = 0; c < NB; c++) d[c] += ak * a[i][c];
      }
      if (t == k) {
#pragma unroll
        for (int c = 0; c < NB; c++) s_top[k & 1][c] = a[0][c];
      }
      // halving butterfly over the 16 lanes of a group, then across the 4 groups of the wave
      double e8[8], e4[4], e2[2], e1;
#pragma unroll
      for (int j = 0; j < 8; j++) { const double snd = b0 ? d[j] : d[j + 8], kp = b0 ? d[j + 8] : d[j]; e8[j] = kp + nd4dpp::xor1(snd); }
#pragma unroll
      for (int j = 0; j < 4; j++) { const double snd = b1 ? e8[j] : e8[j + 4], kp = b1 ? e8[j + 4] : e8[j]; e4[j] = kp + nd4dpp::xor2(snd); }
#pragma unroll
      for (int j = 0; j < 2; j++) { const double snd = b2 ? e4[j] : e4[j + 2], kp = b2 ? e4[j + 2] : e4[j]; e2[j] = kp + nd4dpp::xor4(snd); }
      { const double snd = b3 ? e2[0] : e2[1], kp = b3 ? e2[1] : e2[0]; e1 = kp + nd4dpp::xor8(snd); }
      e1 += __shfl_xor(e1, 16);
      e1 += __shfl_xor(e1, 32);
      if (lane < NB) s_w[k & 1][wave][mycol] = e1;
      __syncthreads();
      double tot = 0.0;                                   // lane -> column lane & 15
#pragma unroll
      for (int w = 0; w < NWV; w++) tot += s_w[k & 1][w][lane & 15];
      double wv[NB];                                      // wave-uniform totals
#define ND4_RL(C) wv[C] = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(tot), C), __builtin_amdgcn_readlane(__double2loint(tot), C));
      ND4_RL(0) ND4_RL(1) ND4_RL(2) ND4_RL(3) ND4_RL(4) ND4_RL(5) ND4_RL(6) ND4_RL(7)
      ND4_RL(8) ND4_RL(9) ND4_RL(10) ND4_RL(11) ND4_RL(12) ND4_RL(13) ND4_RL(14) ND4_RL(15)
#undef ND4_RL
      const double sigma = wv[k], alpha = s_top[k & 1][k];
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
#pragma unroll
      for (int c = 0; c < NB; c++) wv[c] = fma(scale, wv[c], s_top[k & 1][c]);       // v^T a_c
      double vr[R];
#pragma unroll
      for (int i = 0; i < R; i++) {
        const int r = j0 + t + TT * i;
        vr[i] = (i > 0 || r > jc) ? a[i][k] * scale : ((r == jc) ? 1.0 : 0.0);
        const double tv = tau * vr[i];
#pragma unroll
        for (int c = k + 1; c < NB; c++) a[i][c] -= tv * wv[c];
        a[i][k] = (i > 0 || r > jc) ? vr[i] : ((r == jc) ? beta : a[i][k]);
      }
      if (t == 0) {
#pragma unroll
        for (int c = 0; c < NB; c++) if (c < k) s_Z[k][c] = wv[c];
        s_tau[k] = tau;
        taus[mat * strideTau + j0 + k] = tau;
      }
    }
    __builtin_amdgcn_sched_barrier(0);
  };
#define ND4_STEP(K) column_step(std::integral_constant<int, K>{});
  ND4_STEP(0) ND4_STEP(1) ND4_STEP(2) ND4_STEP(3) ND4_STEP(4) ND4_STEP(5) ND4_STEP(6) ND4_STEP(7)
  ND4_STEP(8) ND4_STEP(9) ND4_STEP(10) ND4_STEP(11) ND4_STEP(12) ND4_STEP(13) ND4_STEP(14) ND4_STEP(15)
#undef ND4_STEP
  __syncthreads();
  if (t < nb) {                                          // larft: row t of T depends only on row t
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
#pragma unroll
  for (int i = 0; i < R; i++) {
    const int lr = t + TT * i, r = j0 + lr;
    if (r < M) {
      double* w = A + (long)r * ld + j0;
      double* v = V + (long)r * ldv + j0;
      double wv[NB], vv[NB];
#pragma unroll
      for (int c = 0; c < NB; c++) {
        wv[c] = (lr <= c) ? a[i][c] : 0.0;                       // R part (upper triangle incl. diagonal)
        vv[c] = (lr < c) ? 0.0 : ((lr == c) ? 1.0 : a[i][c]);    // explicit reflector: zeros above, unit diagonal
      }
      if (nb == NB && (ld & 1) == 0) {
#pragma unroll
        for (int c = 0; c < NB; c += 2) {
          *reinterpret_cast<double2*>(w + c) = double2{wv[c], wv[c + 1]};
          *reinterpret_cast<double2*>(v + c) = double2{vv[c], vv[c + 1]};
        }
      } else {
#pragma unroll
        for (int c = 0; c < NB; c++) if (c < nb) { w[c] = wv[c]; v[c] = vv[c]; }
      }
    }
  }
  for (int e = t; e < NB * NB; e += TT) {
    const int i = e / NB, j = e % NB;
    Tall[mat * strideT + (long)(j0 / NB) * NB * NB + e] = (i <= j && j < nb) ? s_T[i][j] : 0.0;
  }
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
// (HR_* and QR_SMALL_WG_BATCH are restated in tests/qr_common.py, which models these decisions: keep the two in step)
constexpr double HR_PIVOT_THR = 1e-5;
constexpr double HR_SERIES_MAX = 1e-5;
// max |Q1^T Q1 - I| after the first pass beyond which the panel is flagged after all. With max |E| <= 1e-2, ||E||_2 <= 0.16 and
// cond(Q1)^2 <= 1.16 / 0.84 = 1.4: the second pass leaves Q orthonormal to 1.4 times what it leaves for a well-conditioned panel. Beyond
// (cond(panel) from about 1e7: max |E| ~ eps cond^2) CholeskyQR2 loses orthogonality: 1e4 ... 1e5 eps at cond = 3e11, measured.
constexpr double HR_PASS1_MAX = 1e-2;
constexpr int HR_MIN_ROWS = 64;

enum { SEG_NX = 0, SEG_NA, SEG_F };   // SEG_F: partial X, exchange, apply in one go
struct QrhSeg { int kind, first, count; };

struct QrhP {
  double* Wm; int M, N; long ld, strideW;
  double* Vall; long ldv, strideV;
  double* Tall; long strideT;
  double* taus; long strideTau;
  double* Xp; long strideXp;        // partials of X = V^T C on the next panel's columns: [part][256]
  int* flag;                        // per matrix: fall-back flag
  double* QT; long strideQT;
  double* Xs; long strideXs;        // side work: partials of X per (column block, row chunk): [cb][rc][256]
  int j0;                           // first row / column of the panel
  int pj0;                          // previous panel (-1: none): its reflector is what the side blocks and phase A apply
  int nxp;                          // partials of X to sum in phase A
  int nrow;                         // row workgroups of this launch
  int wide0, nnw, nqb, nrc;         // side work (reflector pj0): nnw column blocks of W from wide0 on, then nqb blocks of Q^T; nrc row chunks each;
                                    // a side workgroup takes TWO adjacent blocks (pairs of W blocks first, then pairs of Q^T blocks)
  int nseg; QrhSeg seg[2];          // the side work of this launch: workgroups nrow.. walk these segments
  int skip_x;                       // phase C: no partial X for the next panel (last panel of an outer block: the block update covers it)
  int na_shift;                     // the side pairs start at this block of W (1: the panel launch's row workgroups take the next panel's columns themselves)
  unsigned long long* Xch; long strideXch;   // the panel launch: the row workgroups' exchange slots (QX_ROW_SLOT tagged words each)
  unsigned long long* Xsx; long strideXsx;   // fused side work: [column block][row chunk] slots of 512 tagged words (rcs_max chunks per block)
  int rcs_max;
  long long* stamps; int stamp_slot; // debug (ND4HIP_QR_STAMPS): 100 MHz wall-clock stamps of workgroup 0, 8 per launch
  int* status;                      // the handle's exchange status word (host-coherent): raised when a spin limit is hit
  int drop_tag;                     // tests only (ND4HIP_TEST_DROP_PUBLISH): the last row workgroup of the panel with this tag skips its first publication
};

#include "qr_chain16.h"

#define ND4_CHOL16 qrc_chol16_inv      // the eliminations on the matrix core (qr_chain16.h)
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
constexpr long QX_ROW_SLOT = 2560;   // words per row workgroup: values [0,256) G, [256,512) X of the next block, [512,768) top-tile Gram, 768 "stores are out", [1024,1280) Gram of Q1
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
    bool ok = ND4_CHOL16(s_G, s_R, s_Ri, HR_PIVOT_THR);
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


// ------------------------------------------------------------------------------------ V^T C
// Wp[chunk][i][j] = sum_{r in chunk} V[r][i] * C[r][j]; V: m x 16 (ldv), C: m x n (ldc).
// grid (ceil(n/64), ceil(m/256), batch), 256 threads: wave w takes rows chunk*256 + w*64 .. +64 and
// all 4 column strips of 16; the 4 waves' tiles are summed through LDS.
__global__ __launch_bounds__(256) void qr_vtc(const double* __restrict__ V, long ldv, long strideV,
                                               const double* __restrict__ C, long ldc, long strideC,
                                               int m, int n, double* __restrict__ Wp, long ldw, long strideChunk, long strideWb) {
  __shared__ double s_acc[4][4][4][64];      // [wave][strip][reg][lane]
  V += blockIdx.z * strideV; C += blockIdx.z * strideC; Wp += blockIdx.z * strideWb + blockIdx.y * strideChunk;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int fx = lane & 15, fk = lane >> 4;
  const int col0 = blockIdx.x * VTC_COLS;
  const int row0 = blockIdx.y * VTC_ROWS + wave * 64;
  d4 acc[4];
#pragma unroll
  for (int s = 0; s < 4; s++) acc[s] = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll 4
  for (int kk = 0; kk < 16; kk++) {
    const int r = row0 + kk * 4 + fk;
    const bool rok = r < m;
    const double a = rok ? V[(long)r * ldv + fx] : 0.0;
    double b[4];
#pragma unroll
    for (int s = 0; s < 4; s++) {
      const int col = col0 + s * 16 + fx;
      b[s] = (rok && col < n) ? C[(long)r * ldc + col] : 0.0;
    }
#pragma unroll
    for (int s = 0; s < 4; s++) acc[s] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b[s], acc[s], 0, 0, 0);
  }
#pragma unroll
  for (int s = 0; s < 4; s++)
#pragma unroll
    for (int r = 0; r < 4; r++) s_acc[wave][s][r][lane] = acc[s][r];
  __syncthreads();
  // thread t -> (strip s = wave, lane): sums the four waves' copies, fixed order
#pragma unroll
  for (int r = 0; r < 4; r++) {
    const double v = ((s_acc[0][wave][r][lane] + s_acc[1][wave][r][lane]) + s_acc[2][wave][r][lane]) + s_acc[3][wave][r][lane];
    const int i = fk + 4 * r, col = col0 + wave * 16 + fx;
    if (col < n) Wp[(long)i * ldw + col] = v;
  }
}

// W2[:, j] = op(T) * sum_chunks Wp[chunk][:, j]; T upper triangular 16x16; trans -> T^T
__global__ __launch_bounds__(256) void qr_tw(const double* __restrict__ Tall, long strideT, int panel, int trans,
                                              const double* __restrict__ Wp, long ldw, long strideChunk, long strideWb, int nchunks,
                                              int n, double* __restrict__ W2, long strideW2) {
  __shared__ double s_T[NB][NB + 1];
  const double* T = Tall + blockIdx.y * strideT + (long)panel * NB * NB;
  Wp += blockIdx.y * strideWb; W2 += blockIdx.y * strideW2;
  const int t = threadIdx.x;
  s_T[t / NB][t % NB] = T[t];
  __syncthreads();
  const int col = blockIdx.x * 256 + t;
  if (col >= n) return;
  double w[NB];
#pragma unroll
  for (int i = 0; i < NB; i++) w[i] = 0.0;
  for (int ch = 0; ch < nchunks; ch++)
#pragma unroll
    for (int i = 0; i < NB; i++) w[i] += Wp[ch * strideChunk + (long)i * ldw + col];
#pragma unroll
  for (int i = 0; i < NB; i++) {
    double s = 0.0;
    if (trans) {
#pragma unroll
      for (int j = 0; j < NB; j++) s += s_T[j][i] * w[j];
    } else {
#pragma unroll
      for (int j = 0; j < NB; j++) s += s_T[i][j] * w[j];
    }
    W2[(long)i * ldw + col] = s;
  }
}

// ------------------------------------------------------------------------------------ sign fix
// One thread per matrix: decides the flips (reference convention, see file header).
// Tall input (M > N) follows the reference's other branch (qr.js:97-139): every rotation is normalised to
// c >= 0, which PRESERVES the sign of the pivot R_jj, so sign(R_jj) is whatever it was when row j finished its
// own eliminations = sign(det A[0:j+1,0:j+1] / det A[0:j,0:j]). With A[0:k,0:k] = Q[0:k,0:k] R[0:k,0:k] the
// flip of column j is the sign of the j-th pivot of Gaussian elimination WITHOUT pivoting on Q[0:N,0:N].
__global__ void qr_flips_tall(const double* __restrict__ LUq, int N, int* __restrict__ flips, int batch) {
  const long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
  if (i >= (long)batch * N) return;
  const long b = i / N, j = i % N;
  flips[i] = LUq[b * N * N + j * N + j] < 0.0 ? 1 : 0;
}
__global__ __launch_bounds__(256) void qr_flips(const double* __restrict__ Rm, long ldr, long strideR, const double* __restrict__ taus, long strideTau,
                                                 int M, int N, int L, int* __restrict__ flips, int batch) {
  // one workgroup per matrix: flags in parallel, parity by a block-wide XOR
  const int b = blockIdx.x;
  const double* R = Rm + b * strideR; const double* tau = taus + b * strideTau; int* f = flips + (long)b * L;
  __shared__ int s_par[4];
  int parity = 0;
  for (int j = threadIdx.x; j < L; j += 256) {
    int fl = 0;
    if (tau[j] != 0.0) { parity ^= 1; if (R[(long)j * ldr + j] < 0.0) { fl = 1; parity ^= 1; } }
    f[j] = fl;
  }
  parity = __popcll(__ballot(parity)) & 1;
  if ((threadIdx.x & 63) == 0) s_par[threadIdx.x >> 6] = parity;
  __syncthreads();
  // plane rotations never change the determinant: det(Q) = +1 whenever Q is square (M <= N)
  if (threadIdx.x == 0 && M <= N && ((s_par[0] ^ s_par[1] ^ s_par[2] ^ s_par[3]) & 1)) f[L - 1] ^= 1;
}
// scale rows of R (rows x cols, ld) by -1 where flips[row]
__global__ void qr_flip_rows(double* __restrict__ X, long ld, long strideX, int rows, int cols, const int* __restrict__ flips, int L) {
  X += blockIdx.z * strideX; flips += (long)blockIdx.z * L;
  const int col = blockIdx.x * blockDim.x + threadIdx.x;
  if (col >= cols) return;
  for (int r = blockIdx.y; r < rows; r += gridDim.y)
    if (flips[r]) X[(long)r * ld + col] = -X[(long)r * ld + col];
}
// scale columns of Q (rows x cols, ld) by -1 where flips[col]
__global__ void qr_flip_cols(double* __restrict__ X, long ld, long strideX, int rows, int cols, const int* __restrict__ flips, int L) {
  X += blockIdx.z * strideX; flips += (long)blockIdx.z * L;
  const int col = blockIdx.x * blockDim.x + threadIdx.x;
  if (col >= cols || !flips[col]) return;
  for (int r = blockIdx.y; r < rows; r += gridDim.y) X[(long)r * ld + col] = -X[(long)r * ld + col];
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

#include "qr_batched_panel.h"

template <int R, int NWV = 8>
void launch_panel_row(nd4hip_handle* h, int batch, double* W, int M, long ld, long sW, double* V, long ldv, long sV,
                      double* T, long sT, double* taus, long sTau, int j0, int nb) {
  hipLaunchKernelGGL((qr_panel_row<R, NWV>), dim3(batch), dim3(64 * NWV), 0, h->stream, W, M, ld, sW, V, ldv, sV, T, sT, taus, sTau, j0, nb);
}
// The panel of m <= 2048 rows for `batch` matrices. One matrix is a latency problem: many waves with few rows each (R = 1, 2, 4 on
// 512 threads). A batch that fills the chip is a throughput problem: the same body on FEW waves with four rows per thread
// (128 threads for m <= 512, 256 for m <= 1024: 194 VGPRs, so four / two workgroups share a CU, their barriers cost next to nothing
// and a column step is ~530 instructions of ONE wave) — 2048 panels of 512 rows: 220 -> 151 us, 4096 of 256 rows: 315 -> 154 us
// (bench ops.qr_panel). All three shapes then run at the same 1.75 TB/s: the launch is bound by the instruction issue of the
// 4096 wave-panels (8500 instructions each, two waves per SIMD); forcing three waves per SIMD spills (196 us).
// Batches of full panels on the matrix cores (qr_batched_panel.h). ZERO: the rows below the top block are zeroed in W.
constexpr int QR_SMALL_WG_BATCH = 64;
template <int R, int NWV, bool ZERO>
static void launch_qrb(nd4hip_handle* h, int batch, double* W, int M, long ld, long sW, double* V, long ldv, long sV,
                       double* T, long sT, double* taus, long sTau, int j0, long long* stamps) {
  hipLaunchKernelGGL((qrb_panel<R, NWV, ZERO>), dim3(batch), dim3(64 * NWV), 0, h->stream, W, M, ld, sW, V, ldv, sV, T, sT, taus, sTau, j0, stamps);
}
template <bool ZERO>
static void launch_panel_mfma(nd4hip_handle* h, int batch, double* W, int M, int m, long ld, long sW, double* V, long ldv, long sV,
                              double* T, long sT, double* taus, long sTau, int j0, long long* stamps = nullptr) {
  const bool many = batch >= QR_SMALL_WG_BATCH;
  if (many && m <= 256)       launch_qrb<4, 1, ZERO>(h, batch, W, M, ld, sW, V, ldv, sV, T, sT, taus, sTau, j0, stamps);
  else if (many && m <= 512)  launch_qrb<4, 2, ZERO>(h, batch, W, M, ld, sW, V, ldv, sV, T, sT, taus, sTau, j0, stamps);
  else if (many && m <= 1024) launch_qrb<4, 4, ZERO>(h, batch, W, M, ld, sW, V, ldv, sV, T, sT, taus, sTau, j0, stamps);
  else if (m <= 512)          launch_qrb<1, 8, ZERO>(h, batch, W, M, ld, sW, V, ldv, sV, T, sT, taus, sTau, j0, stamps);
  else if (m <= 1024)         launch_qrb<2, 8, ZERO>(h, batch, W, M, ld, sW, V, ldv, sV, T, sT, taus, sTau, j0, stamps);
  else                        launch_qrb<4, 8, ZERO>(h, batch, W, M, ld, sW, V, ldv, sV, T, sT, taus, sTau, j0, stamps);
}
static void launch_panel_rows(nd4hip_handle* h, int batch, double* W, int M, int m, long ld, long sW, double* V, long ldv, long sV,
                              double* T, long sT, double* taus, long sTau, int j0, int nb) {
  const bool many = batch >= QR_SMALL_WG_BATCH;
  if (many && m <= 256)       launch_panel_row<4, 1>(h, batch, W, M, ld, sW, V, ldv, sV, T, sT, taus, sTau, j0, nb);
  else if (many && m <= 512)  launch_panel_row<4, 2>(h, batch, W, M, ld, sW, V, ldv, sV, T, sT, taus, sTau, j0, nb);
  else if (many && m <= 1024) launch_panel_row<4, 4>(h, batch, W, M, ld, sW, V, ldv, sV, T, sT, taus, sTau, j0, nb);
  else if (m <= 512)          launch_panel_row<1>(h, batch, W, M, ld, sW, V, ldv, sV, T, sT, taus, sTau, j0, nb);
  else if (m <= 1024)         launch_panel_row<2>(h, batch, W, M, ld, sW, V, ldv, sV, T, sT, taus, sTau, j0, nb);
  else                        launch_panel_row<4>(h, batch, W, M, ld, sW, V, ldv, sV, T, sT, taus, sTau, j0, nb);
}
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

template <int R, bool REG>
void launch_panel(nd4hip_handle* h, int batch, double* W, int M, long ld, long sW, double* V, long ldv, long sV,
                  double* T, long sT, double* taus, long sTau, int j0, int nb) {
  hipLaunchKernelGGL((qr_panel<R, REG>), dim3(batch), dim3(1024), 0, h->stream, W, M, ld, sW, V, ldv, sV, T, sT, taus, sTau, j0, nb);
}

struct QrWs {
  double *V, *T, *Tside, *taus, *Wp, *W2, *work; int* flips;
  long ldv, sV, sT, sTau, ldw, sChunk, sWb, sW2;
  int nchunks_max;
};

// C (rows [j0,M) x n columns starting at C0) <- (I - V op(T) V^T) C, V = Vall[j0:, j0:j0+nb]
int apply_block_reflector(nd4hip_handle* h, const QrWs& ws, int batch, int M, int j0, int panel, int trans,
                          double* C0, long ldc, long strideC, int n) {
  if (n <= 0) return 0;
  const int m = M - j0;
  const int nchunks = (m + VTC_ROWS - 1) / VTC_ROWS;
  const double* Vp = ws.V + (long)j0 * ws.ldv + j0;
  hipLaunchKernelGGL(qr_vtc, dim3((unsigned)((n + VTC_COLS - 1) / VTC_COLS), (unsigned)nchunks, (unsigned)batch), dim3(256), 0, h->stream,
                     Vp, ws.ldv, ws.sV, C0, ldc, strideC, m, n, ws.Wp, ws.ldw, ws.sChunk, ws.sWb);
  hipLaunchKernelGGL(qr_tw, dim3((unsigned)((n + 255) / 256), (unsigned)batch), dim3(256), 0, h->stream,
                     ws.T, ws.sT, panel, trans, ws.Wp, ws.ldw, ws.sChunk, ws.sWb, nchunks, n, ws.W2, ws.sW2);
  ND4_HIP(hipGetLastError());
  return nd4_gemm(h, false, false, m, n, NB, -1.0, Vp, ws.ldv, ws.sV, ws.W2, ws.ldw, ws.sW2, 1.0, C0, ldc, strideC, batch);
}

// diagonal bs x bs blocks of the n x n compact-WY factor <- the given blocks (everything else zero); bs = 1: the taus
__global__ void wy_t_diag(const double* __restrict__ Tp, double* __restrict__ Tall, int n, int bs) {
  const int blk = blockIdx.x, t = threadIdx.x;                      // bs * bs threads
  Tall[(long)(blk * bs + t / bs) * n + blk * bs + t % bs] = Tp[(long)blk * bs * bs + t];
}

int form_q_compact_wy(nd4hip_handle* h, const QrWs& ws, int batch, int M, int Lq, int npanels, double* Q, long sQ) {
  const int n = npanels * NB;                                       // == ws.ldv
  for (int m = 0; m < batch; m++)
    ND4_TRY(nd4_wy_form(h, M, n, ws.V + (long)m * ws.sV, ws.T + (long)m * ws.sT, NB, Q + (long)m * sQ, Lq));
  return 0;
}


// host side of the multi-workgroup panels: one launch per panel (+ a conditional one for panels taller than the register kernel),
// the previous reflector's side work riding along on the column blocks of W up to near_end (then, optionally, Q^T)
struct QrhHost {
  nd4hip_handle* h; QrhP P; int batch; int nq;          // nq: column blocks of Q^T (0: no Q^T accumulation)
  double *V, *T; long ldv, sV, sT;                        // for qr_narrow_apply
  int pj0 = -1;                                           // the reflector whose narrow / side work is pending (-1: none)
  // every field of P; the slices a caller has no use for are nullptr (the panel entry point: no partials of X, side work or Q^T).
  // Zeroes the exchange slots and the fall-back flags.
  int init(nd4hip_handle* hh, int nmat, double* W, int M, int N, long ld, long sW, double* Vm, long ldv_, long sV_, double* Tm, long sT_,
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
  void add_seg(int kind, int first, int count) { if (count > 0) { P.seg[P.nseg].kind = kind; P.seg[P.nseg].first = first; P.seg[P.nseg].count = count; P.nseg++; } }
  int seg_total() const { int n = 0; for (int i = 0; i < P.nseg; i++) n += P.seg[i].count; return n; }
  void side_launch() { if (P.nseg > 0) hipLaunchKernelGGL(qrh_side_only, dim3((unsigned)seg_total(), (unsigned)batch), dim3(512), 0, h->stream, P); P.nseg = 0; }
  // the side work of the reflector at pj: column blocks of W from pj + 32 to near_end, then (with_qt) of Q^T; returns its
  // workgroups when both phases run on their own
  int side_of(int pj, int near_end, bool with_qt) {
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
  int panel(int j0, int near_end, bool with_qt, bool skip_x) {
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
    if (m <= 512)       hipLaunchKernelGGL(qrh_bc<1>, gm, dim3(512), 0, h->stream, P);
    else if (m <= 1024) hipLaunchKernelGGL(qrh_bc<2>, gm, dim3(512), 0, h->stream, P);
    else if (m <= 2048) hipLaunchKernelGGL(qrh_bc<4>, gm, dim3(512), 0, h->stream, P);
    else {
      // taller than the register-resident panel: a flagged panel is factorised by the global-memory panel kernel in a launch of its own
      hipLaunchKernelGGL(qrh_bc<0>, gm, dim3(512), 0, h->stream, P);
      hipLaunchKernelGGL(qr_panel_flagged, dim3((unsigned)batch), dim3(1024), 0, h->stream, P.Wm, P.M, P.ld, P.strideW, P.Vall, P.ldv, P.strideV,
                         P.Tall, P.strideT, P.taus, P.strideTau, j0, NB, P.flag);
    }
    P.na_shift = 0;
    pj0 = j0; P.nxp = nA; P.nseg = 0; P.stamp_slot++;
    ND4_HIP(hipGetLastError());
    return 0;
  }
  // the last reflector: the 16 columns behind its panel (unless the caller's block update covers them), then its side work on its own
  int finish(int near_end, bool with_qt, bool narrow) {
    if (pj0 < 0) return 0;
    if (narrow && pj0 + NB < P.N) {
      const int m = P.M - pj0;
      P.j0 = pj0; P.na_shift = 0;                         // a flagged panel left no partials of X behind
      hipLaunchKernelGGL(qrh_x_flagged, dim3((unsigned)P.nxp, (unsigned)batch), dim3(512), 0, h->stream, P);
      hipLaunchKernelGGL(qr_narrow_apply, dim3((unsigned)((m + 255) / 256), (unsigned)batch), dim3(256), 0, h->stream,
                         P.Wm, P.M, P.N, P.ld, P.strideW, V, ldv, sV, T, sT, pj0, pj0 + NB, P.Xp, P.strideXp, P.nxp);
    }
    const int side_all = side_of(pj0, near_end, with_qt);
    P.pj0 = pj0;
    P.nseg = 0; add_seg(SEG_NX, 0, side_all); side_launch();
    add_seg(SEG_NA, 0, side_all); side_launch();
    pj0 = -1;
    ND4_HIP(hipGetLastError());
    return 0;
  }
  int dump_stamps() {                                      // debug: per launch, the stamps of workgroup 0 relative to the first one, in us
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
};

}  // namespace

// Compact-WY factor of up to 64 reflector columns = up to four panels of a batch member: T (n x n) from the panels' 16 x 16 factors
// on its diagonal and G = V^T V, T12 = -T1 (V1^T V2) T2 level by level (16, then 32 columns; valid for the FULL factors of the
// matrix-core panels as well as for triangular ones). One workgroup per matrix, everything in LDS: each G12 block is used once, so
// G12 T2 overwrites it. Batches beyond the look-ahead form (qr_batch: the rank-16 updates were 56 % of the run).
__global__ __launch_bounds__(256) void wy_t_small(const double* __restrict__ Tdiag, long sTd, const double* __restrict__ G, int ldg, long sG,
                                                   double* __restrict__ Tout, int ldt, long sTo, int n) {
  __shared__ double s_t[64 * 64], s_g[64 * 64];
  const long m = blockIdx.x;
  const int t = threadIdx.x;
  for (int e = t; e < 4096; e += 256) {
    const int i = e >> 6, j = e & 63;
    const bool in = i < n && j < n;
    s_g[e] = in ? G[m * sG + (long)i * ldg + j] : 0.0;
    s_t[e] = (in && (i >> 4) == (j >> 4)) ? Tdiag[m * sTd + (long)(i >> 4) * 256 + (i & 15) * 16 + (j & 15)] : 0.0;
  }
  __syncthreads();
  for (int b = 16; b < n; b <<= 1) {
    double v[16];
#pragma unroll
    for (int k = 0; k < 16; k++) {                                    // X = G12 T2 on the 12-blocks of this level
      const int e = t + 256 * k, i = e >> 6, j = e & 63, p0 = i & ~(2 * b - 1);
      const int qe = (p0 + 2 * b < n) ? p0 + 2 * b : n;
      double x = 0.0;
      if (i - p0 < b && j >= p0 + b && j < qe) for (int q = p0 + b; q < qe; q++) x += s_g[i * 64 + q] * s_t[q * 64 + j];
      v[k] = x;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 16; k++) {
      const int e = t + 256 * k, i = e >> 6, j = e & 63, p0 = i & ~(2 * b - 1);
      const int qe = (p0 + 2 * b < n) ? p0 + 2 * b : n;
      if (i - p0 < b && j >= p0 + b && j < qe) s_g[e] = v[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 16; k++) {                                    // T12 = -T1 X
      const int e = t + 256 * k, i = e >> 6, j = e & 63, p0 = i & ~(2 * b - 1);
      const int qe = (p0 + 2 * b < n) ? p0 + 2 * b : n;
      double y = 0.0;
      if (i - p0 < b && j >= p0 + b && j < qe) for (int q = p0; q < p0 + b; q++) y += s_t[i * 64 + q] * s_g[q * 64 + j];
      v[k] = y;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 16; k++) {
      const int e = t + 256 * k, i = e >> 6, j = e & 63, p0 = i & ~(2 * b - 1);
      const int qe = (p0 + 2 * b < n) ? p0 + 2 * b : n;
      if (i - p0 < b && j >= p0 + b && j < qe) s_t[e] = -v[k];
    }
    __syncthreads();
  }
  for (int e = t; e < 4096; e += 256) {
    const int i = e >> 6, j = e & 63;
    if (i < n && j < n) Tout[m * sTo + (long)i * ldt + j] = s_t[e];
  }
}

static int wy_build_T(nd4hip_handle* h, int M, int n, const double* V, long ldv, const double* Tdiag, int bs, double* Tall, double* G, double* tmp);

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
constexpr int QR_ROWSPLIT_MAX_BATCH = 8;   // row-split panels (qrh_bc) up to this many matrices; more: one workgroup per panel
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

// C <- (I - V op(T) V^T) C for nblk reflector columns V [m, nblk] and their nblk x nblk factor T: X = V^T C, W = op(T) X, C -= V W
// (X, W: nblk x n, leading dimension n); strides per matrix of the batch (0 for one matrix)
static int block_update(nd4hip_handle* h, bool transT, int m, int n, int nblk, const double* V, long ldv, long sV, const double* T, long sT,
                        double* C, long ldc, long sC, double* X, double* W, long sX, int batch) {
  ND4_TRY(nd4_gemm(h, true, false, nblk, n, m, 1.0, V, ldv, sV, C, ldc, sC, 0.0, X, n, sX, batch));
  ND4_TRY(nd4_gemm(h, transT, false, nblk, n, nblk, 1.0, T, nblk, sT, X, n, sX, 0.0, W, n, sX, batch));
  return nd4_gemm(h, false, false, m, n, nblk, -1.0, V, ldv, sV, W, n, sX, 1.0, C, ldc, sC, batch);
}

// matrix mt: the nblk reflector columns from J on — their factor Tb from the panels' factors first (wy_build_T) unless Tb holds it
// already — applied to the n columns of C (rows [J, M))
static int wy_block_update(QrJob& j, int mt, int J, int nblk, bool build, double* Tb, bool transT, double* C, long ldc, int n) {
  const QrWs& ws = j.ws;
  const int mJ = j.M - J;
  const double* Vb = ws.V + (long)mt * ws.sV + (long)J * ws.ldv + J;
  if (build) ND4_TRY(wy_build_T(j.h, mJ, nblk, Vb, ws.ldv, ws.T + (long)mt * ws.sT + (long)(J / NB) * NB * NB, NB, Tb, j.bG, j.bTmp));
  return block_update(j.h, transT, mJ, n, nblk, Vb, ws.ldv, 0, Tb, 0, C, ldc, 0, j.bX, j.bW, 0, 1);
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
    const int j0 = pnl * NB, nb = L - j0 < NB ? L - j0 : NB, m = M - j0;
    // reflector p-1 has reached the 16 columns behind its own panel (the narrow launch: [pj0 + NB, pj0 + 2 NB), which contain this
    // panel); the columns from there on still lack it
    const int wide0 = pj0 + 2 * NB, nwide = (pj0 >= 0 && wide0 < N) ? (N - wide0 + NB - 1) / NB : 0;
    const int wc0 = j0 + nb;
    const dim3 grid((unsigned)(1 + nwide + (pj0 >= 0 ? nq : 0)), (unsigned)batch);
    if (m <= 512)       hipLaunchKernelGGL(qr_panel_row_la<1>, grid, dim3(512), 0, h->stream, W, M, N, ld, sW, ws.V, ws.ldv, ws.sV, ws.T, ws.sT, ws.taus, ws.sTau, j0, nb, pj0 < 0 ? 0 : pj0, wide0, nwide, QT, sQT);
    else if (m <= 1024) hipLaunchKernelGGL(qr_panel_row_la<2>, grid, dim3(512), 0, h->stream, W, M, N, ld, sW, ws.V, ws.ldv, ws.sV, ws.T, ws.sT, ws.taus, ws.sTau, j0, nb, pj0 < 0 ? 0 : pj0, wide0, nwide, QT, sQT);
    else                hipLaunchKernelGGL(qr_panel_row_la<4>, grid, dim3(512), 0, h->stream, W, M, N, ld, sW, ws.V, ws.ldv, ws.sV, ws.T, ws.sT, ws.taus, ws.sTau, j0, nb, pj0 < 0 ? 0 : pj0, wide0, nwide, QT, sQT);
    if (wc0 < N) {                                           // the next panel's columns (or the first block right of the last panel)
      const dim3 gn((unsigned)((m + 255) / 256), (unsigned)batch);
      hipLaunchKernelGGL(qr_narrow_x, gn, dim3(256), 0, h->stream, W, M, N, ld, sW, ws.V, ws.ldv, ws.sV, j0, wc0, ws.Wp, ws.sWb);
      hipLaunchKernelGGL(qr_narrow_apply, gn, dim3(256), 0, h->stream, W, M, N, ld, sW, ws.V, ws.ldv, ws.sV, ws.T, ws.sT, j0, wc0, ws.Wp, ws.sWb, 0);
    }
    pj0 = j0;
  }
  if (pj0 >= 0) {   // the last panel was a thread-per-row one; wide input: its reflector on the columns right of the block the narrow launch has done
    const int j0 = (npanels - 1) * NB, nb = L - j0 < NB ? L - j0 : NB, wc0 = j0 + nb + NB;
    if (wc0 < N)
      hipLaunchKernelGGL(qr_update_blocks<512>, dim3((unsigned)((N - wc0 + NB - 1) / NB), (unsigned)batch), dim3(512), 0, h->stream,
                         W, M, N, ld, sW, ws.V, ws.ldv, ws.sV, ws.T, ws.sT, j0, wc0);
    if (QT) hipLaunchKernelGGL(qr_update_blocks<512>, dim3((unsigned)nq, (unsigned)batch), dim3(512), 0, h->stream,
                               QT, M, M, (long)M, sQT, ws.V, ws.ldv, ws.sV, ws.T, ws.sT, (npanels - 1) * NB, 0);
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
        if (w == 8) hipLaunchKernelGGL((qr_panel_part<4, 8>), dim3(batch), dim3(1024), 0, h->stream, W, M, ld, sW, ws.V, ws.ldv, ws.sV, ws.T, ws.Tside, ws.sT,
                                       ws.taus, ws.sTau, j0 + c, nbp);
        else        hipLaunchKernelGGL((qr_panel_part<8, 4>), dim3(batch), dim3(1024), 0, h->stream, W, M, ld, sW, ws.V, ws.ldv, ws.sV, ws.T, ws.Tside, ws.sT,
                                       ws.taus, ws.sTau, j0 + c, nbp);
        ND4_HIP(hipGetLastError());
        if (c + w < nb)
          ND4_TRY(apply_block_reflector(h, ws, batch, M, j0, pnl, /*trans=*/1, W + (long)j0 * ld + j0 + c + w, ld, sW, nb - c - w));
      }
      if (nb > w) {
        const double* Vs = ws.V + (long)j0 * ws.ldv + j0;
        ND4_TRY(nd4_gemm(h, true, false, NB, NB, m, 1.0, Vs, ws.ldv, ws.sV, Vs, ws.ldv, ws.sV, 0.0, ws.W2, NB, ws.sW2, batch));
        hipLaunchKernelGGL(qr_t_assemble, dim3(batch), dim3(256), 0, h->stream, ws.T, ws.Tside, ws.sT, pnl, ws.W2, ws.sW2, w);
        ND4_HIP(hipGetLastError());
      }
    } else
    if (m <= 2048) {
      // batches of full panels: one workgroup per panel on the matrix cores (qr_batched_panel.h: V = Q - [S; 0], full T, like the
      // row-split panels of one matrix); short / narrow / odd-stride panels keep the thread-per-row Householder kernel
      if (batch > QR_ROWSPLIT_MAX_BATCH && nb == NB && m >= HR_MIN_ROWS && (ld & 1) == 0 && (ws.ldv & 1) == 0)
        launch_panel_mfma<true>(h, batch, W, M, m, ld, sW, ws.V, ws.ldv, ws.sV, ws.T, ws.sT, ws.taus, ws.sTau, j0);
      else
        launch_panel_rows(h, batch, W, M, m, ld, sW, ws.V, ws.ldv, ws.sV, ws.T, ws.sT, ws.taus, ws.sTau, j0, nb);
    } else                launch_panel<1, false>(h, batch, W, M, ld, sW, ws.V, ws.ldv, ws.sV, ws.T, ws.sT, ws.taus, ws.sTau, j0, nb);
    ND4_HIP(hipGetLastError());
    // trailing columns of the outer block: C <- H^T C = (I - V T^T V^T) C
    ND4_TRY(apply_block_reflector(h, ws, batch, M, j0, pnl, /*trans=*/1, W + (long)j0 * ld + j0 + nb, ld, sW, bend - j0 - nb));
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
      const int n1 = nblk < 64 ? nblk : 64, n2 = nblk - n1;
      hipLaunchKernelGGL(wy_t_small, dim3((unsigned)batch), dim3(256), 0, h->stream, ws.T + (long)P0 * NB * NB, ws.sT, j.bG, nblk, nbo2, Tb, nblk, j.bsT, n1);
      if (n2 > 0) {
        hipLaunchKernelGGL(wy_t_small, dim3((unsigned)batch), dim3(256), 0, h->stream, ws.T + (long)(P0 + 4) * NB * NB, ws.sT, j.bG + (long)n1 * nblk + n1, nblk, nbo2,
                           Tb + (long)n1 * nblk + n1, nblk, j.bsT, n2);
        ND4_TRY(nd4_gemm(h, false, false, n1, n2, n2, 1.0, j.bG + n1, nblk, nbo2, Tb + (long)n1 * nblk + n1, nblk, j.bsT, 0.0, j.bX, n2, j.bsX, batch));
        ND4_TRY(nd4_gemm(h, false, false, n1, n2, n1, -1.0, Tb, nblk, j.bsT, j.bX, n2, j.bsX, 0.0, Tb + n1, nblk, j.bsT, batch));
      }
      ND4_HIP(hipGetLastError());
    }
    if (far > 0)
      ND4_TRY(block_update(h, true, mJ, far, nblk, Vb, ws.ldv, ws.sV, Tb, j.bsT, j.W + (long)J * j.ld + bend, j.ld, j.sW, j.bX, j.bW, j.bsX, batch));
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
      ND4_TRY(block_update(h, false, mJ, nq2, nblk, ws.V + (long)J * ws.ldv + J, ws.ldv, ws.sV, j.bT + (long)(P0 / j.ppb) * nbo2, j.bsT,
                           Q + (long)J * Lq + J, Lq, sQ, j.bX, j.bW, j.bsX, batch));
    }
  } else {
    for (int pnl = npanels - 1; pnl >= 0; pnl--) {
      const int j0 = pnl * NB;
      ND4_TRY(apply_block_reflector(h, ws, batch, M, j0, pnl, /*trans=*/0, Q + (long)j0 * Lq + j0, Lq, sQ, Lq - j0));
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
// (qrh_bc), more as one workgroup per panel on the matrix cores (qr_batched_panel.h).
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
  if (nb == NB && M >= HR_MIN_ROWS) {
    // a batch of panels: one workgroup per panel on the matrix cores (qr_batched_panel.h); V = Q - [S; 0], T = K as above
    static const bool stamps_on = [] { const char* e = getenv("ND4HIP_QRB_STAMPS"); return e && *e && *e != '0'; }();
    long long* stamps = nullptr;
    if (stamps_on) { static long long* dbuf = nullptr; if (!dbuf) ND4_HIP(hipMalloc(&dbuf, 512)); stamps = dbuf; }
    static const bool copy_only = [] { const char* e = getenv("ND4HIP_QRB_COPY_ONLY"); return e && *e && *e != '0'; }();
    static const int copy_mode = [] { const char* e = getenv("ND4HIP_QRB_COPY_ONLY"); return e ? atoi(e) : 0; }();
    if (copy_only) {                                                   // debug: the kernel's data movement alone (see qrb_copy_only)
      if (M <= 256)       hipLaunchKernelGGL((qrb_copy_only<4, 1>), dim3(batch), dim3(64), 0, h->stream, A, M, (long)NB, sW, V, (long)NB, sW, 0, copy_mode);
      else if (M <= 512)  hipLaunchKernelGGL((qrb_copy_only<4, 2>), dim3(batch), dim3(128), 0, h->stream, A, M, (long)NB, sW, V, (long)NB, sW, 0, copy_mode);
      else if (M <= 1024) hipLaunchKernelGGL((qrb_copy_only<4, 4>), dim3(batch), dim3(256), 0, h->stream, A, M, (long)NB, sW, V, (long)NB, sW, 0, copy_mode);
      else                hipLaunchKernelGGL((qrb_copy_only<4, 8>), dim3(batch), dim3(512), 0, h->stream, A, M, (long)NB, sW, V, (long)NB, sW, 0, copy_mode);
      ND4_HIP(hipGetLastError());
      return 0;
    }
    launch_panel_mfma<false>(h, batch, A, M, M, NB, sW, V, NB, sW, T, NB * NB, taus, NB, 0, stamps);
    ND4_HIP(hipGetLastError());
    if (stamps) {
      long long hs[64];
      static const char* names[13] = {"load+gram", "wait all", "chol", "barrier", "q1", "gram2", "wait all", "series", "barrier", "q", "gj", "stores", "T"};
      ND4_HIP(hipStreamSynchronize(h->stream));
      ND4_HIP(hipMemcpy(hs, stamps, 512, hipMemcpyDeviceToHost));
      fprintf(stderr, "qrb stamps %d x %d rows (us | shader cycles; workgroup 0):", batch, M);
      for (int k = 0; k < 13; k++) fprintf(stderr, " %s %.2f|%lld", names[k], (hs[2 * k + 2] - hs[2 * k]) * 0.01, hs[2 * k + 3] - hs[2 * k + 1]);
      fprintf(stderr, " total %.2f|%lld; columns 4/8/12 of q1 at %lld %lld %lld of q at %lld %lld %lld\n", (hs[26] - hs[0]) * 0.01, hs[27] - hs[1],
              hs[29] - hs[9], hs[31] - hs[9], hs[33] - hs[9], hs[35] - hs[19], hs[37] - hs[19], hs[39] - hs[19]);
    }
    return 0;
  }
  launch_panel_rows(h, batch, A, M, M, NB, sW, V, NB, sW, T, NB * NB, taus, NB, 0, nb);
  ND4_HIP(hipGetLastError());
  return 0;
}

// Sign convention of the reference's Givens-built factors, applied to a Householder-built pair (Q [M, >= L] with leading
// dimension ldq, R [L, ncols] with leading dimension ldr; column j of Q and row j of R are flipped together):
//   lu_rule = false (qr_decomp_full, the square / wide branches): R_jj >= 0 wherever a reflector was needed (tau_j != 0),
//             and det Q = +1 (plane rotations) decides the last one when Q is square (M == L);
//   lu_rule = true  (the c >= 0 branches for tall input, qr.js:97-139 / bidiag.js:49-61): every leading principal minor of
//             Q's top L x L block is positive = positive pivots in its LU factorisation WITHOUT pivoting.
// flips: L ints per matrix of scratch. Q == nullptr (lu_rule = false only): R's rows are flipped and there is no Q to follow them.
int nd4_givens_signs(nd4hip_handle* h, int batch, int M, int L, int ncols, bool lu_rule, double* Q, long ldq, long sQ,
                     double* R, long ldr, long sR, const double* taus, long sTau, int* flips) {
  ND4_CHECK_ARG(Q != nullptr || !lu_rule, "nd4_givens_signs: the c >= 0 rule needs Q");
  if (lu_rule) {
    Nd4WsScope scope2(h);
    void* q = nullptr;
    ND4_TRY(nd4_ws_alloc(h, sizeof(double) * (size_t)batch * L * L + sizeof(int32_t) * (size_t)batch * L, &q));
    double* LUq = static_cast<double*>(q);
    int32_t* Pq = reinterpret_cast<int32_t*>(LUq + (size_t)batch * L * L);
    ND4_TRY(nd4_copy_matrix(h, L, L, Q, ldq, LUq, L, batch, sQ, (long)L * L));
    ND4_TRY(nd4_getrf_nopivot(h, batch, L, LUq, LUq, Pq));
    hipLaunchKernelGGL(qr_flips_tall, dim3((unsigned)(((long)batch * L + 255) / 256)), dim3(256), 0, h->stream, LUq, L, flips, batch);
  } else {
    // qr_flips decides the parity flip by "M <= N": pass N = M when Q is square, N = M - 1 otherwise
    hipLaunchKernelGGL(qr_flips, dim3((unsigned)batch), dim3(256), 0, h->stream,
                       R, ldr, sR, taus, sTau, M, (M == L ? M : M - 1), L, flips, batch);
  }
  {
    const unsigned gy = (unsigned)(L < 512 ? L : 512);
    hipLaunchKernelGGL(qr_flip_rows, dim3((unsigned)((ncols + 255) / 256), gy, (unsigned)batch), dim3(256), 0, h->stream,
                       R, ldr, sR, L, ncols, flips, L);
    const unsigned gq = (unsigned)(M < 512 ? M : 512);
    if (Q) hipLaunchKernelGGL(qr_flip_cols, dim3((unsigned)((L + 255) / 256), gq, (unsigned)batch), dim3(256), 0, h->stream,
                       Q, ldq, sQ, M, L, flips, L);
  }
  ND4_HIP(hipGetLastError());
  return 0;
}

// Q [M, Lq] (row-major, ld Lq) = (H_0 H_1 ... H_{n-1}) [I; 0] for reflectors H_j = I - tau_j v_j v_j^T given as the columns of
// V [M, n] (ld n), formed at once from their compact-WY representation H_0 ... H_{n-1} = I - V T V^T: T is upper triangular
// with the given bs x bs factors on its diagonal (bs = 1: the taus themselves) and T[1,2] = -T1 (V1^T V2) T2 for two adjacent
// groups, applied level by level (groups of bs, 2 bs, 4 bs, ... columns). One Gram matrix V^T V (TN GEMM), two
// strided-batched small GEMMs per level, W = T V[0:Lq,:]^T and Q = E - V W: ~20-30 launches and 6 M n^2 flop on the MFMA
// kernels instead of a backward loop of rank-bs updates. n must be a multiple of bs; zero columns of V are harmless.
// The n x n compact-WY factor T of n reflector columns V [M, n] (leading dimension ldv) from its bs x bs diagonal blocks Tdiag
// ([n / bs][bs][bs]; bs = 1: the taus) and the Gram matrix V^T V: T[1,2] = -T1 (V1^T V2) T2 for two adjacent groups, level by level
// (groups of bs, 2 bs, 4 bs, ... columns). G, tmp: workspaces of n * n and n * n / 2 + 16 doubles. n must be a multiple of bs.
static int wy_build_T(nd4hip_handle* h, int M, int n, const double* V, long ldv, const double* Tdiag, int bs, double* Tall, double* G, double* tmp) {
  ND4_TRY(nd4_gemm(h, true, false, n, n, M, 1.0, V, ldv, 0, V, ldv, 0, 0.0, G, n, 0, 1));
  ND4_HIP(hipMemsetAsync(Tall, 0, sizeof(double) * (size_t)n * n, h->stream));
  hipLaunchKernelGGL(wy_t_diag, dim3((unsigned)(n / bs)), dim3((unsigned)(bs * bs)), 0, h->stream, Tdiag, Tall, n, bs);
  ND4_HIP(hipGetLastError());
  for (int b = bs; b < n; b *= 2) {
    const long step = 2l * b * (n + 1);                             // from one pair of groups to the next, along the diagonal
    const int full = n / (2 * b);
    for (int f0 = 0; f0 < full; f0 += 32768) {                      // gridDim.y limit of the batched launch
      const int nf = full - f0 < 32768 ? full - f0 : 32768;
      const long o = f0 * step;
      ND4_TRY(nd4_gemm(h, false, false, b, b, b, 1.0, G + b + o, n, step, Tall + (long)b * (n + 1) + o, n, step, 0.0, tmp, b, (long)b * b, nf));
      ND4_TRY(nd4_gemm(h, false, false, b, b, b, -1.0, Tall + o, n, step, tmp, b, (long)b * b, 0.0, Tall + b + o, n, step, nf));
    }
    const int i0 = full * 2 * b, n2 = n - i0 - b;                    // ragged last pair: second group narrower
    if (n2 > 0) {
      ND4_TRY(nd4_gemm(h, false, false, b, n2, n2, 1.0, G + (long)i0 * n + i0 + b, n, 0, Tall + (long)(i0 + b) * (n + 1), n, 0, 0.0, tmp, n2, 0, 1));
      ND4_TRY(nd4_gemm(h, false, false, b, n2, b, -1.0, Tall + (long)i0 * (n + 1), n, 0, tmp, n2, 0, 0.0, Tall + (long)i0 * n + i0 + b, n, 0, 1));
    }
  }
  return 0;
}

int nd4_wy_form(nd4hip_handle* h, int M, int n, const double* V, const double* Tdiag, int bs, double* Q, int Lq) {
  Nd4WsScope scope(h);
  void* p = nullptr;
  ND4_TRY(nd4_ws_alloc(h, sizeof(double) * ((size_t)n * n * 2 + (size_t)n * n / 2 + (size_t)n * Lq + 64), &p));
  double* G = static_cast<double*>(p);
  double* Tall = G + (size_t)n * n;
  double* tmp = Tall + (size_t)n * n;
  double* W = tmp + (size_t)n * n / 2 + 16;
  ND4_TRY(wy_build_T(h, M, n, V, n, Tdiag, bs, Tall, G, tmp));
  ND4_TRY(nd4_gemm(h, false, true, n, Lq, n, 1.0, Tall, n, 0, V, n, 0, 0.0, W, Lq, 0, 1));                   // W = T V[0:Lq,:]^T
  ND4_TRY(nd4_set_identity(h, M, Lq, Q, Lq, 1, (long)M * Lq));
  return nd4_gemm(h, false, false, M, Lq, n, -1.0, V, n, 0, W, Lq, 0, 1.0, Q, Lq, 0, 1);                     // Q = E - V W
}
