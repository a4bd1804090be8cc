// Complex128 QR by Householder reflectors on the device: zqr_factor / zqr_apply_q / zqr_decomp / zqr_lstsq, LAPACK's
// zgeqrf / zunmqr / zungqr / zgels on row-major members [M, N], 1 <= N <= M <= 2048, interleaved (re, im) doubles.
//   A = H_0 H_1 ... H_{N-1} [R; 0], H_k = I - tau_k v_k v_k^H, v_k zero above row k, 1 in row k, its tail in F[k+1:, k]; R on and above
//   the diagonal of F. The reflector of x = A[k:, k] = [alpha; tail] is hetrd.hip's (zlarfg.h): diag(R) is exactly real, a column
//   with an empty or zero tail and Im alpha != 0 gets a pure phase reflector. The trailing columns receive H_k^H = I - conj(tau_k) v v^H.
// Every member is scaled on load by 2^-e1, e1 the exponent that puts max(|Re a_ij|, |Im a_ij|) in [0.5, 1); R gets 2^e1 back on its
// store, exactly: A -> 2^m A leaves tails and tau bit-identical. Columns below 2^-450 of the maximum are lifted as in hetrd.hip.
// Every sum has an order fixed by (M, N, k): no atomics on doubles; the only synchronisation is __syncthreads(), wave shuffles and the
// kernel boundary; every loop bound comes from M, N or K (the lift: at most two rounds). The file is built without FMA contraction.
//
// LDS tier: a member goes here when its factorisation fits one workgroup's 163840 bytes and M <= 152, so that a 64-column tile of
// zqr_apply_q fits too:
//     16 (M (N | 1) + M + 5 N + 256) + 96 <= 163840  (the tile at an odd pitch in 16-byte elements, v, w, the partial dot products,
//                                                     the reduction scratch)                         square members: up to 96 x 96
//     16 (64 M + 2 M + N) <= 163840                  (the tile of Z, v twice, tau)                   holds for every N <= M <= 152
//   zgeqr2_small   one workgroup of 256 threads per member, one launch per call. Per column: the norm of the tail by het_block_sum, the
//                  reflector, w = v^H A[k:, k+1:] by 256 / CW groups of rows (group q takes the rows k + q, k + q + 256 / CW, ... in
//                  order; CW = 8, 16, 32 or 64 lanes of columns, the least that covers min(N, 64); the groups are added in order), the
//                  rank-1 update.
//   zunmqr_small   one workgroup of 64 threads per 64 columns of Z, reflector by reflector, as unmtr_small.
//   Both return the bits of the numpy model in tests/zqr_common.py.
// Blocked tier, everything else: column blocks of 16 (ZQR_NB), per block
//   zqr_panel<R, IB> one workgroup of 512 threads per member factorises the block in inner panels of IB columns held in registers
//                  (thread t holds the rows j0 + t + 512 s, s < R; R = 1, 2, 4 by the rows left). IB = 4 in every instantiation:
//                  with 8 or 16 columns the compiler's resource report showed scratch, so a block is four inner
//                  panels. Norms and the dot products v^H a of the remaining panel columns meet in LDS, wave tree first, then the
//                  eight waves in order. The reflectors of the earlier inner panels reach the next one when it is loaded, one by
//                  one, their vectors read back from V by the thread that wrote them. Writes the dense V [rows, 16] (unit diagonal,
//                  zeros above and right of the block) and tau.
//   zqr_vhc        W = V^H C on v_mfma_f64_16x16x4_f64 with V read as stored: a lane loads V[k0 + (lane >> 4)][lane & 15], which is
//                  element (i, k) = (lane & 15, lane >> 4) of the A operand up to conjugation, and C[k0 + (lane >> 4)][n0 + (lane & 15)]
//                  for B, both contiguous over 16 lanes and straight into registers: no LDS, no transposed copy. The conjugate lives
//                  in the four chains Vr Cr, Vi Ci, Vr Ci, (-Vi) Cr, which are added in pairs at the end. grid (tiles of 64
//                  columns, chunks of 256 rows, members): each chunk writes its partial [16, n], the next kernel adds them in order.
//                  G = V^H V is the same kernel with C = V.
//   zqr_t          T (16 x 16, zlarft forward columnwise, unmtr_wy_t's recurrence) from G and tau.
//   zqr_tw         W2 = T^H (sum of the partials) for Q^H, T (...) for Q; one workgroup per 64 columns.
//   zlu_update     C -= V W2 (zgetrf.hip, K = 16).
//   zqr_apply_q above the LDS tier: zqr_wy_v (V from F), then the four kernels above per block on Z, blocks ascending with T^H for
//   Q^H, descending with T for Q. zqr_decomp's Q is that on [I; 0]. zqr_lstsq: Q^H Y on a copy, its top N rows, nd4_zgetrs_upper.
// Flags of zqr_lstsq: [0] the OR over the members of a pass, [1 + member] = 1 + the first column whose r_kk is zero or not finite.
#include "nd4hip_internal.h"
#include "zgemm_stage.h"
#include "zlarfg.h"
#include <cfloat>

namespace {

constexpr int ZQR_MAXN = 2048;
constexpr int ZQR_NB = 16;                      // columns per block, a multiple of 16 up to 64 (32 was timed once: DESIGN.md 4.27)
static_assert(ZQR_NB % 16 == 0 && ZQR_NB <= 64, "zqr_vhc takes V in tiles of 16 columns, zqr_t has 64 threads");
constexpr int ZQR_T = 256;
constexpr int ZQR_PT = 512;                     // threads of the panel kernel
constexpr int ZQR_CH = 256;                     // rows per chunk of zqr_vhc
constexpr int ZQR_ZT = 64;                      // columns of Z per workgroup
constexpr size_t ZQR_LDS = 163840;
constexpr int ZQR_SMALL_M = 152;                 // the LDS tier ends here: 16 (66 M + N) bytes of zunmqr_small fit for every N <= M
constexpr int64_t ZQR_CHUNK = 32768;            // members per pass
constexpr int64_t ZQR_WS_ELEMS = 1ll << 26;     // a pass's workspace takes at most 1 GiB

__host__ __device__ inline int zqr_cw(int N) { return N > 32 ? 64 : N > 16 ? 32 : N > 8 ? 16 : 8; }

// ---- LDS tier -------------------------------------------------------------------------------------------------------------------
// grid (members), 256 threads. A, F [members, M, N], tau [members, N]
__global__ __launch_bounds__(ZQR_T) void zgeqr2_small(const cd* __restrict__ A, cd* __restrict__ F, cd* __restrict__ tau, int M, int N) {
  extern __shared__ __attribute__((aligned(16))) char zqr_smem[];
  const int P = N | 1, t = threadIdx.x;
  const long b = blockIdx.x;
  cd* S = reinterpret_cast<cd*>(zqr_smem);                    // [M][P]
  cd* v = S + (size_t)M * P;                                  // [M]
  cd* wv = v + M;                                             // [N] conj(tau) v^H a_c
  cd* part = wv + N;                                          // [256 / CW][N]: at most 4 N + 256
  double* red = reinterpret_cast<double*>(part + 4 * N + 256);   // [8]
  u64* redu = reinterpret_cast<u64*>(red + 8);                // [4]
  const cd* a = A + b * M * N;
  u64 m = 0;
  for (int e = t; e < M * N; e += ZQR_T) {
    const int i = e / N, j = e - i * N;
    const cd x = a[e];
    const u64 br = het_bits(x.x), bi = het_bits(x.y);
    m = br > m ? br : m; m = bi > m ? bi : m;
    S[i * P + j] = x;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) { const u64 o = __shfl_xor(m, off); m = o > m ? o : m; }
  if ((t & 63) == 0) redu[t >> 6] = m;
  __syncthreads();
  for (int q = 0; q < 4; ++q) m = redu[q] > m ? redu[q] : m;
  const int e1 = syev_exp(m);
  for (int e = t; e < M * N; e += ZQR_T) {
    const int i = e / N, j = e - i * N;
    const cd x = S[i * P + j];
    S[i * P + j] = cmk(ldexp(x.x, -e1), ldexp(x.y, -e1));
  }
  __syncthreads();
  const int CW = zqr_cw(N), RG = ZQR_T / CW, cl = t % CW, q = t / CW;
  for (int k = 0; k < N; ++k) {
    double acc = 0.0, cnt = 0.0;
    for (int i = k + 1 + t; i < M; i += ZQR_T) {
      const cd x = S[i * P + k];
      acc += x.x * x.x + x.y * x.y; cnt += x.x != 0.0 || x.y != 0.0 ? 1.0 : 0.0;
    }
    const cd alpha = S[k * P + k];
    const cd sn = het_block_sum(cmk(acc, cnt), red);
    double sigma = sn.x, c = 1.0;
    for (int lvl = 0; lvl < 2 && het_tiny(alpha, c, sigma, sn.y); ++lvl) {
      c *= HET_LIFT;
      double a2 = 0.0;
      for (int i = k + 1 + t; i < M; i += ZQR_T) { const double xr = c * S[i * P + k].x, xi = c * S[i * P + k].y; a2 += xr * xr + xi * xi; }
      sigma = het_block_sum(cmk(a2, 0.0), red).x;
    }
    const HetRefl r = het_reflector(alpha, sigma, c);
    if (r.on) {                                               // (uniform) else: the step changes nothing but r_kk
      for (int i = k + t; i < M; i += ZQR_T) v[i] = i == k ? cmk(1.0, 0.0) : cdiv_re(S[i * P + k], r.div);
      __syncthreads();
      for (int col = k + 1 + cl; col < N; col += CW) {
        cd s = cmk(0.0, 0.0);
        for (int i = k + q; i < M; i += RG) s = cadd(s, cmulc(S[i * P + col], v[i]));   // conj(v_i) a_ic
        part[q * N + col] = s;
      }
      __syncthreads();
      const cd ctau = cconj(r.tau);
      for (int col = k + 1 + t; col < N; col += ZQR_T) {
        cd s = part[col];
        for (int g = 1; g < RG; ++g) s = cadd(s, part[g * N + col]);
        wv[col] = cmul(ctau, s);
      }
      __syncthreads();
      const int mm = M - k, nn = N - k - 1;
      for (int idx = t; idx < mm * nn; idx += ZQR_T) {
        const int i = k + idx / nn, col = k + 1 + idx % nn;
        S[i * P + col] = csub(S[i * P + col], cmul(v[i], wv[col]));
      }
      for (int i = k + t; i < M; i += ZQR_T) S[i * P + k] = i == k ? cmk(r.beta, 0.0) : v[i];
    } else if (t == 0) S[k * P + k] = cmk(r.beta, 0.0);
    if (t == 0) tau[b * N + k] = r.tau;
    __syncthreads();
  }
  cd* f = F + b * M * N;
  for (int e = t; e < M * N; e += ZQR_T) {
    const int i = e / N, j = e - i * N;
    const cd x = S[i * P + j];
    f[e] = j >= i ? cmk(ldexp(x.x, e1), ldexp(x.y, e1)) : x;
  }
}

// grid (ceil(K / 64), members), 64 threads, one column of Z [members, M, K] per thread, in LDS (M x 64 + 2 M + N complex). Reflector k:
// z -= v (tau (v^H z)); Q Z applies k = N-1 .. 0 with tau, Q^H Z applies k = 0 .. N-1 with conj(tau). sF, sTau = 0: one (F, tau) for all
__global__ __launch_bounds__(64) void zunmqr_small(const cd* __restrict__ F, long sF, const cd* __restrict__ tau, long sTau, cd* __restrict__ Z, int M,
                                                   int N, int K, int adjoint) {
  extern __shared__ __attribute__((aligned(16))) char zqr_smem[];
  cd* z = reinterpret_cast<cd*>(zqr_smem);                    // [M][64]
  cd* vb = z + (size_t)M * ZQR_ZT;                            // [2][M]
  cd* tl = vb + 2 * (size_t)M;                                // [N]
  const int t = threadIdx.x, c = blockIdx.x * ZQR_ZT + t;
  const long b = blockIdx.y;
  const bool active = c < K;
  const cd* f = F + b * sF;
  const cd* tb = tau + b * sTau;
  cd* zb = Z + b * M * K;
  for (int i = 0; i < M; ++i) z[i * ZQR_ZT + t] = active ? zb[(size_t)i * K + c] : cmk(0.0, 0.0);
  for (int i = t; i < N; i += 64) tl[i] = adjoint ? cconj(tb[i]) : tb[i];   // (made visible by the first step's barrier)
  for (int s = 0; s < N; ++s) {
    const int k = adjoint ? s : N - 1 - s;
    cd* v = vb + (s & 1) * M;
    for (int i = k + t; i < M; i += 64) v[i] = i == k ? cmk(1.0, 0.0) : f[(size_t)i * N + k];
    __syncthreads();                                          // one per step: v alternates between two buffers
    cd dot = cmk(0.0, 0.0);
    for (int i = k; i < M; ++i) dot = cadd(dot, cmulc(z[i * ZQR_ZT + t], v[i]));   // conj(v_i) z_i
    dot = cmul(tl[k], dot);
    for (int i = k; i < M; ++i) z[i * ZQR_ZT + t] = csub(z[i * ZQR_ZT + t], cmul(v[i], dot));
  }
  if (active)
    for (int i = 0; i < M; ++i) zb[(size_t)i * K + c] = z[i * ZQR_ZT + t];
}

// ---- blocked tier ---------------------------------------------------------------------------------------------------------------
// mx[b] = the bits of max(|Re|, |Im|) over A[b] (mx zero on entry; the maximum of integers: any order gives the same word);
// grid (256, members)
__global__ __launch_bounds__(ZQR_T) void zqr_absmax(const cd* __restrict__ A, long count, u64* __restrict__ mx) {
  const cd* s = A + (long)blockIdx.y * count;
  u64 m = 0;
  for (long e = (long)blockIdx.x * ZQR_T + threadIdx.x; e < count; e += (long)gridDim.x * ZQR_T) {
    const u64 br = het_bits(s[e].x), bi = het_bits(s[e].y);
    m = br > m ? br : m; m = bi > m ? bi : m;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) { const u64 o = __shfl_xor(m, off); m = o > m ? o : m; }
  if ((threadIdx.x & 63) == 0 && m) atomicMax(mx + blockIdx.y, m);
}
// F[b] = 2^-e1 A[b] (unscale = 0), or the upper triangle of F[b] times 2^e1 in place (unscale = 1); grid (tiles of 256 elements, members)
__global__ __launch_bounds__(ZQR_T) void zqr_scale(const cd* __restrict__ A, cd* __restrict__ F, long count, int N, const u64* __restrict__ mx,
                                                   int unscale) {
  const long e = (long)blockIdx.x * ZQR_T + threadIdx.x;
  if (e >= count) return;
  const int e1 = syev_exp(mx[blockIdx.y]);
  cd* f = F + (long)blockIdx.y * count + e;
  if (unscale) {
    if (e % N >= e / N) *f = cmk(ldexp(f->x, e1), ldexp(f->y, e1));
  } else {
    const cd x = A[(long)blockIdx.y * count + e];
    *f = cmk(ldexp(x.x, -e1), ldexp(x.y, -e1));
  }
}

// the sums of x[0 .. NV) over the 512 threads: the xor tree of each wave, then the eight waves in order; red [8][NV]. from: the
// first entry that is wanted
template <int NV>
__device__ __forceinline__ void zqr_panel_sum(cd (&x)[NV], cd* red, int from) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int c = 0; c < NV; ++c)
    if (c >= from) {
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) { x[c].x += __shfl_xor(x[c].x, off); x[c].y += __shfl_xor(x[c].y, off); }
    }
  __syncthreads();
  if (lane == 0) {
#pragma unroll
    for (int c = 0; c < NV; ++c)
      if (c >= from) red[wave * NV + c] = x[c];
  }
  __syncthreads();
#pragma unroll
  for (int c = 0; c < NV; ++c)
    if (c >= from) {
      cd s = red[c];
#pragma unroll
      for (int w = 1; w < ZQR_PT / 64; ++w) s = cadd(s, red[w * NV + c]);
      x[c] = s;
    }
}

// The columns j0 .. j0 + nb - 1 (nb <= 16) and rows j0 .. M - 1 of every member of F [members, M, N], in place; tau [members, N];
// V [members][M x 16 reserved]: the block's reflectors as a dense [M - j0, 16]. grid (members); (M - j0) <= 512 R
template <int R, int IB>
__global__ __launch_bounds__(ZQR_PT) void zqr_panel(cd* __restrict__ F, cd* __restrict__ tau, cd* __restrict__ V, int M, int N, int j0, int nb) {
  __shared__ cd red[(ZQR_PT / 64) * IB], stau[ZQR_NB], salpha[2];
  const int t = threadIdx.x, rows = M - j0;
  cd* Fm = F + (long)blockIdx.x * M * N + (long)j0 * N + j0;   // row r, column c of the block: Fm[r N + c]
  cd* Vm = V + (long)blockIdx.x * M * ZQR_NB;
  const cd zero = cmk(0.0, 0.0);
  for (int c0 = 0; c0 < nb; c0 += IB) {
    const int w = nb - c0 < IB ? nb - c0 : IB;
    cd a[R][IB];
#pragma unroll
    for (int s = 0; s < R; ++s) {
      const int r = t + ZQR_PT * s;
#pragma unroll
      for (int c = 0; c < IB; ++c) a[s][c] = (r < rows && c < w) ? Fm[(long)r * N + c0 + c] : zero;
    }
    // the reflectors of the inner panels before this one, one by one; a thread reads back the rows of V that it wrote
    for (int k = 0; IB < ZQR_NB && k < c0; ++k) {
      cd vk[R], d[IB];
#pragma unroll
      for (int s = 0; s < R; ++s) { const int r = t + ZQR_PT * s; vk[s] = (r >= k && r < rows) ? Vm[(long)r * ZQR_NB + k] : zero; }
#pragma unroll
      for (int c = 0; c < IB; ++c) {
        d[c] = zero;
#pragma unroll
        for (int s = 0; s < R; ++s) d[c] = cadd(d[c], cmulc(a[s][c], vk[s]));
      }
      zqr_panel_sum<IB>(d, red, 0);
      const cd ctau = cconj(stau[k]);
#pragma unroll
      for (int c = 0; c < IB; ++c) {
        const cd tw = cmul(ctau, d[c]);
#pragma unroll
        for (int s = 0; s < R; ++s) { const int r = t + ZQR_PT * s; if (r >= k && r < rows) a[s][c] = csub(a[s][c], cmul(vk[s], tw)); }
      }
    }
#pragma unroll
    for (int jj = 0; jj < IB; ++jj) {
      if (jj < w) {                                            // (the whole workgroup)
        const int gk = c0 + jj;
        __builtin_amdgcn_sched_barrier(0);                     // (a column step at a time: the steps interleaved cost scratch)
        cd sn[1] = {zero};
#pragma unroll
        for (int s = 0; s < R; ++s) {
          const int r = t + ZQR_PT * s;
          const cd x = a[s][jj];
          if (r > gk && r < rows) { sn[0].x += x.x * x.x + x.y * x.y; sn[0].y += x.x != 0.0 || x.y != 0.0 ? 1.0 : 0.0; }
          if (r == gk) salpha[jj & 1] = x;
        }
        zqr_panel_sum<1>(sn, red, 0);                          // (its barriers publish alpha)
        const cd alpha = salpha[jj & 1];
        double sigma = sn[0].x, lift = 1.0;
        for (int lvl = 0; lvl < 2 && het_tiny(alpha, lift, sigma, sn[0].y); ++lvl) {
          lift *= HET_LIFT;
          cd s2[1] = {zero};
#pragma unroll
          for (int s = 0; s < R; ++s) {
            const int r = t + ZQR_PT * s;
            if (r > gk && r < rows) { const double xr = lift * a[s][jj].x, xi = lift * a[s][jj].y; s2[0].x += xr * xr + xi * xi; }
          }
          zqr_panel_sum<1>(s2, red, 0);
          sigma = s2[0].x;
        }
        const HetRefl h = het_reflector(alpha, sigma, lift);
        cd vj[R];
#pragma unroll
        for (int s = 0; s < R; ++s) {
          const int r = t + ZQR_PT * s;
          vj[s] = (r > gk && r < rows) ? (h.on ? cdiv_re(a[s][jj], h.div) : a[s][jj]) : (r == gk ? cmk(1.0, 0.0) : zero);
        }
        if (h.on) {                                            // (uniform)
          cd d[IB];
#pragma unroll
          for (int c = 0; c < IB; ++c) {
            d[c] = zero;
            if (c > jj) {
#pragma unroll
              for (int s = 0; s < R; ++s) d[c] = cadd(d[c], cmulc(a[s][c], vj[s]));   // (v is zero above row gk)
            }
          }
          zqr_panel_sum<IB>(d, red, jj + 1);
          const cd ctau = cconj(h.tau);
#pragma unroll
          for (int c = 0; c < IB; ++c)
            if (c > jj) {
              const cd tw = cmul(ctau, d[c]);
#pragma unroll
              for (int s = 0; s < R; ++s) { const int r = t + ZQR_PT * s; if (r >= gk && r < rows) a[s][c] = csub(a[s][c], cmul(vj[s], tw)); }
            }
        }
#pragma unroll
        for (int s = 0; s < R; ++s) {
          const int r = t + ZQR_PT * s;
          if (r > gk) a[s][jj] = vj[s];
          if (r == gk) a[s][jj] = cmk(h.beta, 0.0);
        }
        if (t == 0) stau[gk] = h.tau;
      }
    }
#pragma unroll
    for (int s = 0; s < R; ++s) {
      const int r = t + ZQR_PT * s;
      if (r < rows) {
#pragma unroll
        for (int c = 0; c < IB; ++c)
          if (c < w) {
            Fm[(long)r * N + c0 + c] = a[s][c];
            Vm[(long)r * ZQR_NB + c0 + c] = r < c0 + c ? zero : (r == c0 + c ? cmk(1.0, 0.0) : a[s][c]);
          }
      }
    }
  }
#pragma unroll
  for (int s = 0; s < R; ++s) {
    const int r = t + ZQR_PT * s;
    if (r < rows)
      for (int c = nb; c < ZQR_NB; ++c) Vm[(long)r * ZQR_NB + c] = zero;
  }
  __syncthreads();
  if (t < nb) tau[(long)blockIdx.x * N + j0 + t] = stau[t];
}

// V [members][M x 16 reserved] as [rows = M - j0, 16] from the reflectors j0 .. j0 + nb - 1 in F (members sF apart): unit diagonal, zero
// above, columns >= nb zero; grid (tiles of 256 over rows x 16, members)
__global__ __launch_bounds__(ZQR_T) void zqr_wy_v(const cd* __restrict__ F, long sF, int M, int N, int j0, int nb, cd* __restrict__ V) {
  const int e = blockIdx.x * ZQR_T + threadIdx.x, r = e / ZQR_NB, c = e % ZQR_NB;
  if (r >= M - j0) return;
  cd x = cmk(0.0, 0.0);
  if (c < nb) x = r < c ? cmk(0.0, 0.0) : (r == c ? cmk(1.0, 0.0) : F[(long)blockIdx.y * sF + (long)(j0 + r) * N + j0 + c]);
  V[(long)blockIdx.y * M * ZQR_NB + e] = x;
}

// W [members][chunks][16][n] (members sW apart) = per chunk of 256 rows V^H C: V [rows, 16] (members sV apart), C [rows, n] with row
// pitch ldc (members sC apart); pointers to interleaved doubles, everything else in complex elements.
// grid (ceil(n / 64) x tiles of 16 columns of V, chunks, members), 256 threads: wave w takes the columns 64 (blockIdx.x / tiles) + 16 w ..
struct ZqrVhc { const double* V; long sV; const double* C; long ldc, sC; double* W; long sW; int rows, n; };
__global__ __launch_bounds__(ZQR_T) void zqr_vhc(ZqrVhc g) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, fx = lane & 15, fk = lane >> 4;
  const int it = blockIdx.x % (ZQR_NB / 16) * 16;               // the tile of 16 columns of V: rows it .. it + 15 of W
  const int col = blockIdx.x / (ZQR_NB / 16) * 64 + wave * 16 + fx;
  if (col - fx >= g.n) return;                                 // (the whole wave; the kernel has no barrier)
  const bool cin = col < g.n;
  const int r0 = blockIdx.y * ZQR_CH, r1 = g.rows < r0 + ZQR_CH ? g.rows : r0 + ZQR_CH;
  const double* __restrict__ V = g.V + 2 * (long)blockIdx.z * g.sV;
  const double* __restrict__ C = g.C + 2 * (long)blockIdx.z * g.sC;
  d4 rr = {0.0, 0.0, 0.0, 0.0}, ri = rr, ir = rr, ii = rr;    // the chains Vr Cr, Vi Ci, Vr Ci, (-Vi) Cr
#pragma unroll 2
  for (int k0 = r0; k0 < r1; k0 += 16) {                       // four steps of four rows: the eight loads first
    d2 v[4], c[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int row = k0 + 4 * u + fk;
      v[u] = d2{0.0, 0.0}; c[u] = d2{0.0, 0.0};
      if (row < r1) {
        v[u] = *reinterpret_cast<const d2*>(V + 2 * ((long)row * ZQR_NB + it + fx));
        if (cin) c[u] = *reinterpret_cast<const d2*>(C + 2 * ((long)row * g.ldc + col));
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const double nvi = -v[u].y;
      rr = __builtin_amdgcn_mfma_f64_16x16x4f64(v[u].x, c[u].x, rr, 0, 0, 0);
      ri = __builtin_amdgcn_mfma_f64_16x16x4f64(v[u].y, c[u].y, ri, 0, 0, 0);
      ir = __builtin_amdgcn_mfma_f64_16x16x4f64(v[u].x, c[u].y, ir, 0, 0, 0);
      ii = __builtin_amdgcn_mfma_f64_16x16x4f64(nvi, c[u].x, ii, 0, 0, 0);
    }
  }
  if (!cin) return;
  double* W = g.W + 2 * ((long)blockIdx.z * g.sW + (long)blockIdx.y * ZQR_NB * g.n);
#pragma unroll
  for (int r = 0; r < 4; ++r)                                 // the lane holds the rows fk + 4 r of its column
    *reinterpret_cast<d2*>(W + 2 * ((long)(it + fk + 4 * r) * g.n + col)) = d2{rr[r] + ri[r], ir[r] + ii[r]};
}

// T [members, 16, 16] upper triangular with I - V T V^H = H_j0 ... H_{j0+nb-1} from the chunks of G = V^H V in Gp [members][chunks][16][16]
// (added in order) and tau (members sTau apart): T_jj = tau_j, T[0:j, j] = -tau_j T[0:j, 0:j] G[0:j, j]; rows and columns >= nb zero.
// grid (members), 64 threads; thread i < 16 owns row i
__global__ __launch_bounds__(64) void zqr_t(const cd* __restrict__ Gp, long sG, int chunks, const cd* __restrict__ tau, long sTau, int j0, int nb,
                                            cd* __restrict__ T) {
  __shared__ cd g[ZQR_NB][ZQR_NB + 1], tl[ZQR_NB][ZQR_NB + 1];
  const int i = threadIdx.x;
  const long b = blockIdx.x;
  for (int e = i; e < ZQR_NB * ZQR_NB; e += 64) {
    cd s = Gp[b * sG + e];
    for (int ch = 1; ch < chunks; ++ch) s = cadd(s, Gp[b * sG + (long)ch * ZQR_NB * ZQR_NB + e]);
    g[e / ZQR_NB][e % ZQR_NB] = s;
    tl[e / ZQR_NB][e % ZQR_NB] = cmk(0.0, 0.0);
  }
  __syncthreads();
  for (int j = 0; j < nb; ++j) {
    const cd tj = tau[b * sTau + j0 + j];
    if (i < j) {
      cd s = cmk(0.0, 0.0);
      for (int l = i; l < j; ++l) s = cadd(s, cmul(tl[i][l], g[l][j]));
      const cd x = cmul(tj, s);
      tl[i][j] = cmk(-x.x, -x.y);
    } else if (i == j) tl[i][j] = tj;
    __syncthreads();
  }
  for (int e = i; e < ZQR_NB * ZQR_NB; e += 64) T[b * ZQR_NB * ZQR_NB + e] = tl[e / ZQR_NB][e % ZQR_NB];
}

// W2 [members, 16, n] = op(T) (the chunks of Wp [members][chunks][16][n] added in order), op(T) = T^H (adjoint) or T;
// grid (ceil(n / 64), members), 256 threads: thread t takes the column t & 63 and the rows (t >> 6) + 4 r
__global__ __launch_bounds__(ZQR_T) void zqr_tw(const cd* __restrict__ Wp, long sW, int chunks, const cd* __restrict__ T, int adjoint,
                                                cd* __restrict__ W2, int n) {
  __shared__ cd S[ZQR_NB][65], Ts[ZQR_NB][ZQR_NB + 1];
  const int t = threadIdx.x, lane = t & 63, c = blockIdx.x * 64 + lane;
  const long b = blockIdx.y;
  const cd* wp = Wp + b * sW;
  for (int e = t; e < ZQR_NB * ZQR_NB; e += ZQR_T) {
    const cd x = T[b * ZQR_NB * ZQR_NB + e];
    if (adjoint) Ts[e % ZQR_NB][e / ZQR_NB] = cconj(x); else Ts[e / ZQR_NB][e % ZQR_NB] = x;
  }
#pragma unroll
  for (int r = 0; r < ZQR_NB / 4; ++r) {
    const int i = (t >> 6) + 4 * r;
    cd s = cmk(0.0, 0.0);
    if (c < n) {
      s = wp[(long)i * n + c];
      for (int ch = 1; ch < chunks; ++ch) s = cadd(s, wp[((long)ch * ZQR_NB + i) * n + c]);
    }
    S[i][lane] = s;
  }
  __syncthreads();
  if (c >= n) return;
#pragma unroll
  for (int r = 0; r < ZQR_NB / 4; ++r) {
    const int i = (t >> 6) + 4 * r;
    cd acc = cmk(0.0, 0.0);
#pragma unroll
    for (int l = 0; l < ZQR_NB; ++l) acc = cadd(acc, cmul(Ts[i][l], S[l][lane]));
    W2[(b * ZQR_NB + i) * n + c] = acc;
  }
}

// ---- the small kernels of the routes --------------------------------------------------------------------------------------------
// mode 0: D [members, rows, cols] = the first `cols` columns of the identity; 1: D [members, N = rows = cols] = the upper triangle of the
// top N rows of S (members sS apart, row pitch cols); 2: D [members, rows, cols] = the top `rows` rows of S (row pitch cols).
// grid (tiles of 256, members)
__global__ __launch_bounds__(ZQR_T) void zqr_fill(int mode, const cd* __restrict__ S, long sS, cd* __restrict__ D, int rows, int cols) {
  const long e = (long)blockIdx.x * ZQR_T + threadIdx.x;
  if (e >= (long)rows * cols) return;
  const int i = (int)(e / cols), j = (int)(e - (long)i * cols);
  cd x = cmk(0.0, 0.0);
  if (mode == 0) x = cmk(i == j ? 1.0 : 0.0, 0.0);
  else if (mode == 2 || j >= i) x = S[(long)blockIdx.y * sS + e];
  D[(long)blockIdx.y * rows * cols + e] = x;
}
// flags[1 + member] = 1 + the first k with r_kk zero or not finite (0: none), flags[0] |= 1 if any; one thread per member
__global__ __launch_bounds__(ZQR_T) void zqr_rank_flags(const cd* __restrict__ F, long sF, int N, long members, int* __restrict__ flags) {
  const long b = (long)blockIdx.x * ZQR_T + threadIdx.x;
  if (b >= members) return;
  int flag = 0;
  for (int k = N - 1; k >= 0; --k) {
    const double d = fabs(F[b * sF + (long)k * N + k].x);
    if (!(d > 0.0 && d <= DBL_MAX)) flag = k + 1;
  }
  flags[1 + b] = flag;
  if (flag) atomicOr(&flags[0], 1);
}

// ---- host side ------------------------------------------------------------------------------------------------------------------
inline const cd* ccd(const double* p) { return reinterpret_cast<const cd*>(p); }
inline cd* mcd(double* p) { return reinterpret_cast<cd*>(p); }
inline const double* cdb(const cd* p) { return reinterpret_cast<const double*>(p); }
inline double* mdb(cd* p) { return reinterpret_cast<double*>(p); }
inline bool zqr_al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
inline unsigned zqr_tiles(int64_t n, int per) { return (unsigned)((n + per - 1) / per); }

int zqr_attr(const void* fn, size_t lds) {
  if (lds > 64 * 1024) ND4_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  return 0;
}
template <class T> int zqr_alloc(nd4hip_handle* h, size_t n, T** out) {
  void* p = nullptr;
  ND4_TRY(nd4_ws_alloc(h, sizeof(T) * (n ? n : 1), &p));
  *out = static_cast<T*>(p);
  return 0;
}

inline size_t zqr_factor_lds(int64_t M, int64_t N) { return 16 * (size_t)(M * (N | 1) + M + 5 * N + 256) + 96; }
inline size_t zqr_apply_lds(int64_t M, int64_t N) { return 16 * (size_t)(ZQR_ZT * M + 2 * M + N); }
inline int zqr_chunks(int64_t rows) { return (int)((rows + ZQR_CH - 1) / ZQR_CH); }

// the workspace of the blocked kernels for a pass of nbm members and products up to n columns wide
struct ZqrWs { cd *V, *Wp, *W2, *T; u64* mx; int64_t n; };
inline int64_t zqr_ws_elems(int64_t M, int64_t n) {           // complex elements per member: V, Wp, W2, T
  if (n < ZQR_NB) n = ZQR_NB;
  return M * ZQR_NB + (int64_t)zqr_chunks(M) * ZQR_NB * n + ZQR_NB * n + ZQR_NB * ZQR_NB;
}
int zqr_ws(nd4hip_handle* h, int64_t nbm, int64_t M, int64_t n, ZqrWs* ws) {
  if (n < ZQR_NB) n = ZQR_NB;
  ws->n = n;
  ND4_TRY(zqr_alloc(h, (size_t)(nbm * M * ZQR_NB), &ws->V));
  ND4_TRY(zqr_alloc(h, (size_t)(nbm * zqr_chunks(M) * ZQR_NB * n), &ws->Wp));
  ND4_TRY(zqr_alloc(h, (size_t)(nbm * ZQR_NB * n), &ws->W2));
  ND4_TRY(zqr_alloc(h, (size_t)(nbm * ZQR_NB * ZQR_NB), &ws->T));
  ND4_TRY(zqr_alloc(h, (size_t)nbm, &ws->mx));
  return 0;
}

// C [rows, n] (row pitch ldc, members sC apart) -= V op(T) V^H C for the block whose V [rows, 16] is in ws.V; tau + j0 .. are its scalars
int zqr_block_apply(nd4hip_handle* h, int64_t nbm, int M, int rows, int n, int j0, int nb, const cd* tau, int64_t sTau, bool adjoint, cd* C,
                    int64_t ldc, int64_t sC, const ZqrWs& ws) {
  const int chunks = zqr_chunks(rows);
  const long sV = (long)M * ZQR_NB, sW = (long)zqr_chunks(M) * ZQR_NB * ws.n;
  const ZqrVhc gg{cdb(ws.V), sV, cdb(ws.V), ZQR_NB, sV, mdb(ws.Wp), sW, rows, ZQR_NB};
  hipLaunchKernelGGL(zqr_vhc, dim3(zqr_tiles(ZQR_NB, 64) * (ZQR_NB / 16), (unsigned)chunks, (unsigned)nbm), dim3(ZQR_T), 0, h->stream, gg);
  ND4_HIP(hipGetLastError());
  hipLaunchKernelGGL(zqr_t, dim3((unsigned)nbm), dim3(64), 0, h->stream, ws.Wp, sW, chunks, tau, (long)sTau, j0, nb, ws.T);
  ND4_HIP(hipGetLastError());
  const ZqrVhc gc{cdb(ws.V), sV, cdb(C), (long)ldc, (long)sC, mdb(ws.Wp), sW, rows, n};
  hipLaunchKernelGGL(zqr_vhc, dim3(zqr_tiles(n, 64) * (ZQR_NB / 16), (unsigned)chunks, (unsigned)nbm), dim3(ZQR_T), 0, h->stream, gc);
  ND4_HIP(hipGetLastError());
  hipLaunchKernelGGL(zqr_tw, dim3(zqr_tiles(n, 64), (unsigned)nbm), dim3(ZQR_T), 0, h->stream, ws.Wp, sW, chunks, ws.T, adjoint ? 1 : 0, ws.W2, n);
  ND4_HIP(hipGetLastError());
  const ZluUpd u{cdb(ws.V), ZQR_NB, sV, cdb(ws.W2), n, (long)ZQR_NB * n, mdb(C), (long)ldc, (long)sC, rows, n, ZQR_NB};
  return zlu_update_launch(h, nbm, u);
}

// F, tau of nbm members from A; ws: of the blocked tier (unused in the LDS tier)
int zqr_factor(nd4hip_handle* h, int64_t nbm, int M, int N, const cd* A, cd* F, cd* tau, const ZqrWs& ws) {
  if (nd4_zgeqrf_tier(M, N) == 0) {
    const size_t lds = zqr_factor_lds(M, N);
    ND4_TRY(zqr_attr(reinterpret_cast<const void*>(&zgeqr2_small), lds));
    hipLaunchKernelGGL(zgeqr2_small, dim3((unsigned)nbm), dim3(ZQR_T), lds, h->stream, A, F, tau, M, N);
    ND4_HIP(hipGetLastError());
    return 0;
  }
  const long mn = (long)M * N;
  const dim3 egrid(zqr_tiles(mn, ZQR_T), (unsigned)nbm);
  ND4_HIP(hipMemsetAsync(ws.mx, 0, sizeof(u64) * (size_t)nbm, h->stream));
  hipLaunchKernelGGL(zqr_absmax, dim3(256u, (unsigned)nbm), dim3(ZQR_T), 0, h->stream, A, mn, ws.mx);
  hipLaunchKernelGGL(zqr_scale, egrid, dim3(ZQR_T), 0, h->stream, A, F, mn, N, ws.mx, 0);
  ND4_HIP(hipGetLastError());
  for (int j0 = 0; j0 < N; j0 += ZQR_NB) {
    const int kb = N - j0 < ZQR_NB ? N - j0 : ZQR_NB, j1 = j0 + kb, rest = N - j1, rows = M - j0;
    const dim3 grid((unsigned)nbm), block(ZQR_PT);
    if (rows <= ZQR_PT)          hipLaunchKernelGGL((zqr_panel<1, 4>), grid, block, 0, h->stream, F, tau, ws.V, M, N, j0, kb);
    else if (rows <= 2 * ZQR_PT) hipLaunchKernelGGL((zqr_panel<2, 4>), grid, block, 0, h->stream, F, tau, ws.V, M, N, j0, kb);
    else                         hipLaunchKernelGGL((zqr_panel<4, 4>), grid, block, 0, h->stream, F, tau, ws.V, M, N, j0, kb);
    ND4_HIP(hipGetLastError());
    if (rest == 0) break;
    ND4_TRY(zqr_block_apply(h, nbm, M, rows, rest, j0, kb, tau, N, true, F + (long)j0 * N + j1, N, mn, ws));
  }
  hipLaunchKernelGGL(zqr_scale, egrid, dim3(ZQR_T), 0, h->stream, A, F, mn, N, ws.mx, 1);
  ND4_HIP(hipGetLastError());
  return 0;
}

// Z [nbm, M, K] <- Q Z or Q^H Z in place; F, tau members sF, sTau apart (0: one for all)
int zqr_apply(nd4hip_handle* h, int64_t nbm, int M, int N, int K, bool adjoint, const cd* F, int64_t sF, const cd* tau, int64_t sTau, cd* Z,
              const ZqrWs& ws) {
  if (nd4_zgeqrf_tier(M, N) == 0) {
    const size_t lds = zqr_apply_lds(M, N);
    ND4_TRY(zqr_attr(reinterpret_cast<const void*>(&zunmqr_small), lds));
    hipLaunchKernelGGL(zunmqr_small, dim3(zqr_tiles(K, ZQR_ZT), (unsigned)nbm), dim3(64), lds, h->stream, F, (long)sF, tau, (long)sTau, Z, M, N, K,
                       adjoint ? 1 : 0);
    ND4_HIP(hipGetLastError());
    return 0;
  }
  const int nblocks = (N + ZQR_NB - 1) / ZQR_NB;
  for (int s = 0; s < nblocks; ++s) {
    const int j0 = (adjoint ? s : nblocks - 1 - s) * ZQR_NB, kb = N - j0 < ZQR_NB ? N - j0 : ZQR_NB, rows = M - j0;
    hipLaunchKernelGGL(zqr_wy_v, dim3(zqr_tiles((int64_t)rows * ZQR_NB, ZQR_T), (unsigned)nbm), dim3(ZQR_T), 0, h->stream, F, (long)sF, M, N, j0, kb, ws.V);
    ND4_HIP(hipGetLastError());
    ND4_TRY(zqr_block_apply(h, nbm, M, rows, K, j0, kb, tau, sTau, adjoint, Z + (long)j0 * K, K, (int64_t)M * K, ws));
  }
  return 0;
}

int zqr_fill_launch(nd4hip_handle* h, int64_t nbm, int mode, const cd* S, int64_t sS, cd* D, int rows, int cols) {
  hipLaunchKernelGGL(zqr_fill, dim3(zqr_tiles((int64_t)rows * cols, ZQR_T), (unsigned)nbm), dim3(ZQR_T), 0, h->stream, mode, S, (long)sS, D, rows, cols);
  ND4_HIP(hipGetLastError());
  return 0;
}

#define ZQR_CHECK_SHAPE(op, M, N)                                                                                  \
  ND4_CHECK_ARG((N) >= 1 && (N) <= (M) && (M) <= ZQR_MAXN, "nd4hip_" op "_batched: 1 <= N <= M <= 2048")

}  // namespace

// ---- the host-side arithmetic of the tiers (tools/zqr_host_check.hip) ----
// 0: a member in LDS, 1: blocked
int nd4_zgeqrf_tier(int64_t M, int64_t N) { return zqr_factor_lds(M, N) <= ZQR_LDS && M <= ZQR_SMALL_M ? 0 : 1; }
// the largest dynamic LDS request of any kernel that runs at this shape
size_t nd4_zgeqrf_lds(int64_t M, int64_t N) {
  if (nd4_zgeqrf_tier(M, N) == 1) return 0;
  return zqr_factor_lds(M, N) > zqr_apply_lds(M, N) ? zqr_factor_lds(M, N) : zqr_apply_lds(M, N);
}
// members per pass: at most 32768, and `extra` + the blocked workspace (products n columns wide) complex elements per member within 1 GiB
int64_t nd4_zgeqrf_chunk(int64_t batch, int64_t M, int64_t N, int64_t n, int64_t extra) {
  const int64_t per = extra + (nd4_zgeqrf_tier(M, N) == 1 ? zqr_ws_elems(M, n) : 0);
  int64_t c = ZQR_CHUNK;
  if (per > 0 && ZQR_WS_ELEMS / per < c) c = ZQR_WS_ELEMS / per;
  if (c < 1) c = 1;
  return batch < c ? batch : c;
}

// zqr_factor: F [batch, M, N], tau [batch, N] from A. Arguments already checked, batch >= 1. Enqueues only
int nd4_zgeqrf(nd4hip_handle* h, int64_t batch, int64_t M64, int64_t N64, const double* A, double* F, double* tau) {
  ZQR_CHECK_SHAPE("zgeqrf", M64, N64);
  ND4_CHECK_ARG(zqr_al16(A) && zqr_al16(F) && zqr_al16(tau), "nd4hip_zgeqrf_batched: complex operands must be 16-byte aligned");
  const int M = (int)M64, N = (int)N64;
  const int64_t mn = M64 * N64, chunk = nd4_zgeqrf_chunk(batch, M, N, N, 0);
  Nd4WsScope scope(h);
  ZqrWs ws{};
  if (nd4_zgeqrf_tier(M, N) == 1) ND4_TRY(zqr_ws(h, chunk, M, N, &ws));
  for (int64_t b0 = 0; b0 < batch; b0 += chunk) {
    const int64_t nbm = batch - b0 < chunk ? batch - b0 : chunk;
    ND4_TRY(zqr_factor(h, nbm, M, N, ccd(A) + b0 * mn, mcd(F) + b0 * mn, mcd(tau) + b0 * N64, ws));
  }
  return 0;
}

// zqr_apply_q: Z [batch, M, K] <- Q Z (adjoint: Q^H Z) in place; F, tau members sF, sTau apart (0: one for all). Enqueues only
int nd4_zunmqr(nd4hip_handle* h, int64_t batch, int64_t M64, int64_t N64, int64_t K64, bool adjoint, const double* F, int64_t sF, const double* tau,
               int64_t sTau, double* Z) {
  ZQR_CHECK_SHAPE("zunmqr", M64, N64);
  ND4_CHECK_ARG(zqr_al16(F) && zqr_al16(tau) && zqr_al16(Z), "nd4hip_zunmqr_batched: complex operands must be 16-byte aligned");
  const int M = (int)M64, N = (int)N64, K = (int)K64;
  const int64_t chunk = nd4_zgeqrf_chunk(batch, M, N, K, 0);
  Nd4WsScope scope(h);
  ZqrWs ws{};
  if (nd4_zgeqrf_tier(M, N) == 1) ND4_TRY(zqr_ws(h, chunk, M, K, &ws));
  for (int64_t b0 = 0; b0 < batch; b0 += chunk) {
    const int64_t nbm = batch - b0 < chunk ? batch - b0 : chunk;
    ND4_TRY(zqr_apply(h, nbm, M, N, K, adjoint, ccd(F) + b0 * sF, sF, ccd(tau) + b0 * sTau, sTau, mcd(Z) + b0 * M64 * K64, ws));
  }
  return 0;
}

// zqr_decomp: the thin Q [batch, M, N] = H_0 ... H_{N-1} [I; 0] and R [batch, N, N] of A, F and tau in workspace. Enqueues only
int nd4_zungqr(nd4hip_handle* h, int64_t batch, int64_t M64, int64_t N64, const double* A, double* Q, double* R) {
  ZQR_CHECK_SHAPE("zungqr", M64, N64);
  ND4_CHECK_ARG(zqr_al16(A) && zqr_al16(Q) && zqr_al16(R), "nd4hip_zungqr_batched: complex operands must be 16-byte aligned");
  const int M = (int)M64, N = (int)N64;
  const int64_t mn = M64 * N64, chunk = nd4_zgeqrf_chunk(batch, M, N, N, mn + N64);
  Nd4WsScope scope(h);
  ZqrWs ws{};
  cd *F = nullptr, *tau = nullptr;
  ND4_TRY(zqr_alloc(h, (size_t)(chunk * mn), &F));
  ND4_TRY(zqr_alloc(h, (size_t)(chunk * N64), &tau));
  if (nd4_zgeqrf_tier(M, N) == 1) ND4_TRY(zqr_ws(h, chunk, M, N, &ws));
  for (int64_t b0 = 0; b0 < batch; b0 += chunk) {
    const int64_t nbm = batch - b0 < chunk ? batch - b0 : chunk;
    cd* q = mcd(Q) + b0 * mn;
    ND4_TRY(zqr_factor(h, nbm, M, N, ccd(A) + b0 * mn, F, tau, ws));
    ND4_TRY(zqr_fill_launch(h, nbm, 1, F, mn, mcd(R) + b0 * N64 * N64, N, N));
    ND4_TRY(zqr_fill_launch(h, nbm, 0, nullptr, 0, q, M, N));
    ND4_TRY(zqr_apply(h, nbm, M, N, N, false, F, mn, tau, N, q, ws));
  }
  return 0;
}

// zqr_lstsq: X [batch, N, K] = R^-1 (Q^H Y)[:N]. tau = NULL: A is the matrix [batch, M, N] (sA = M N) and is factorised into workspace;
// else A is F of zqr_factor with its tau, members sA and (sA ? N : 0) apart. A member whose R has a diagonal entry that is zero or not
// finite: info (device, int32 [batch]) receives 1 + the first such column (0: none) and nothing is raised; with info = NULL one flag
// word per pass is read back, the members' flags only if it is raised: ND4HIP_ERR_SINGULAR with the lowest flagged member (member0: the
// index of the first member in the caller's batch), also in *first_bad (may be NULL). Synchronises only with info = NULL
int nd4_zgels(nd4hip_handle* h, int64_t batch, int64_t M64, int64_t N64, int64_t K64, const double* A, int64_t sA, const double* tau_in,
              const double* Y, double* X, int32_t* info, int64_t member0, int64_t* first_bad) {
  ZQR_CHECK_SHAPE("zgels", M64, N64);
  ND4_CHECK_ARG(zqr_al16(A) && zqr_al16(tau_in) && zqr_al16(Y) && zqr_al16(X), "nd4hip_zgels_batched: complex operands must be 16-byte aligned");
  const int M = (int)M64, N = (int)N64, K = (int)K64;
  const bool factored = tau_in != nullptr;
  const int64_t mn = M64 * N64, mk = M64 * K64, nk = N64 * K64;
  const int64_t wide = factored || K64 > N64 ? K64 : N64;       // the widest product: the trailing columns, then Y
  const int64_t chunk = nd4_zgeqrf_chunk(batch, M, N, wide, mk + (factored ? 0 : mn + N64) + 1);
  Nd4WsScope scope(h);
  ZqrWs ws{};
  cd *F = nullptr, *tau = nullptr, *Zw = nullptr;
  int* flags = nullptr;
  ND4_TRY(zqr_alloc(h, (size_t)(chunk + 1), &flags));
  ND4_TRY(zqr_alloc(h, (size_t)(chunk * mk), &Zw));
  if (!factored) { ND4_TRY(zqr_alloc(h, (size_t)(chunk * mn), &F)); ND4_TRY(zqr_alloc(h, (size_t)(chunk * N64), &tau)); }
  if (nd4_zgeqrf_tier(M, N) == 1) ND4_TRY(zqr_ws(h, chunk, M, wide, &ws));
  int* host = nullptr;
  if (!info) { void* hp = nullptr; ND4_TRY(nd4_pinned(h, sizeof(int) * (size_t)(chunk + 1), &hp)); host = static_cast<int*>(hp); }
  for (int64_t b0 = 0; b0 < batch; b0 += chunk) {
    const int64_t nbm = batch - b0 < chunk ? batch - b0 : chunk;
    const cd *f = F, *tb = tau;
    int64_t sF = mn, sTau = N64;
    if (factored) { f = ccd(A) + b0 * sA; sF = sA; sTau = sA ? N64 : 0; tb = ccd(tau_in) + b0 * sTau; }
    else ND4_TRY(zqr_factor(h, nbm, M, N, ccd(A) + b0 * mn, F, tau, ws));
    ND4_HIP(hipMemsetAsync(flags, 0, sizeof(int), h->stream));
    hipLaunchKernelGGL(zqr_rank_flags, dim3(zqr_tiles(nbm, ZQR_T)), dim3(ZQR_T), 0, h->stream, f, (long)sF, N, (long)nbm, flags);
    ND4_HIP(hipGetLastError());
    ND4_HIP(hipMemcpyAsync(Zw, ccd(Y) + b0 * mk, sizeof(cd) * (size_t)(nbm * mk), hipMemcpyDeviceToDevice, h->stream));
    ND4_TRY(zqr_apply(h, nbm, M, N, K, true, f, sF, tb, sTau, Zw, ws));
    cd* x = mcd(X) + b0 * nk;
    ND4_TRY(zqr_fill_launch(h, nbm, 2, Zw, mk, x, N, K));
    ND4_TRY(nd4_zgetrs_upper(h, nbm, N, K, cdb(f), sF, mdb(x)));
    if (info) {
      ND4_HIP(hipMemcpyAsync(info + b0, flags + 1, sizeof(int) * (size_t)nbm, hipMemcpyDeviceToDevice, h->stream));
      continue;
    }
    ND4_HIP(hipMemcpyAsync(host, flags, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    ND4_HIP(hipStreamSynchronize(h->stream));
    if (host[0] == 0) continue;
    ND4_HIP(hipMemcpyAsync(host, flags, sizeof(int) * (size_t)(nbm + 1), hipMemcpyDeviceToHost, h->stream));
    ND4_HIP(hipStreamSynchronize(h->stream));
    int64_t b = 0;
    while (b < nbm - 1 && host[1 + b] == 0) ++b;
    if (first_bad) *first_bad = member0 + b0 + b;
    nd4_set_error("zqr_lstsq(A,Y): A is rank-deficient. (matrix %lld)", (long long)(member0 + b0 + b));
    return ND4HIP_ERR_SINGULAR;
  }
  return 0;
}
