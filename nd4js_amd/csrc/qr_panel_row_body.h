// The thread-per-row Householder panel (m <= 2048 rows) as a device function: the body of qr_panel_row and qr_panel_row_la
// (qr_house.hip) and the fall-back inside qrh_bc (qr_rowsplit.hip) and qrb_panel (qr_batched_panel.hip).
#pragma once
#include "qr_internal.h"
#include "dpp.h"
#include <type_traits>

// (internal linkage: an inline function with external linkage has its __shared__ arrays placed differently in each kernel's LDS)
namespace {
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

}  // namespace
