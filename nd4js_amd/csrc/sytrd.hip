// tridiag_factor / tridiag_apply_q / tridiag_decomp: the symmetric tridiagonal reduction S = Q tridiag(d, e) Q^T and the
// application of its Q (LAPACK's dsytrd / dormtr, lower, on row-major members), DESIGN.md 4.21. The reference has neither.
//   Q = H_0 H_1 ... H_{N-3}, H_k = I - tau_k v_k v_k^T, v_k zero in rows 0..k, 1 in row k+1, its tail in F[k+2:, k].
//   Step k takes the column x = A[k+1:, k] = [alpha; tail] of the matrix as the steps before left it:
//     sigma = |tail|^2;  sigma = 0: tau_k = 0, e_k = alpha, v's tail = 0 (the step changes nothing);
//     else beta = -sign(alpha) sqrt(alpha^2 + sigma) (sign(0) = +1), tau_k = (beta - alpha) / beta, tail / (alpha - beta), e_k = beta;
//     p = tau A v,  w = p - (tau / 2)(p^T v) v,  A -= v w^T + w v^T  on the trailing block (rows and columns > k).
// Every member is scaled on load by 2^-e1, e1 the exponent that puts max|s_ij| over its lower triangle in [0.5, 1); d and e get
// 2^e1 back on their store, exactly. So S -> 2^m S leaves tails, tau and Q bit-identical (while no entry leaves the normal range)
// and the sums of squares above cannot overflow. NaN or Inf in the lower triangle shows in the bit pattern of that maximum (the
// bits of |x| order like |x|, NaN above Inf): one flag word per call, read back by the caller of these launchers.
// Every sum has a fixed order that depends on N and k alone: no atomics on doubles, no dependence on the batch or on the run.
// The only synchronisation is __syncthreads() and the kernel boundary; the host decides nothing from data.
//   Tier A (N <= 128): sytrd_small, one workgroup per member and one launch per call; the member stays in LDS, mirrored to a full
//     square at an odd pitch, for all N - 2 steps.
//   Tier B (N <= 2048): sytrd_step, one launch per column k = 0 .. N-1 over a grid (blocks of 64 rows, batch) on the scaled lower
//     triangle in F. Launch k first finishes step k-1: p from the row sums and the per-block column partials that launch k-1 left
//     (added in block order), then w. It then updates column k, which gives d_k, e_k, tau_k and v_k; every workgroup does these two
//     parts for itself, the last one stores them. Then, in one pass over its rows of the trailing triangle, it applies the rank-2
//     update of step k-1 and accumulates its share of A v_k: row sums complete, column sums as partials[block][j]. That is one read
//     and one write of the shrinking triangle per step. Column k is only read in launch k; its tails are stored in launch k+1.
//   dormtr: N <= 128: ormtr_small, one workgroup per 128 columns of a member's Z, in LDS, reflector by reflector. Above: blocks of
//     64 reflectors in compact WY form, I - V T V^T, on the batched fp64 GEMM (four products per block).
#include "syev_internal.h"
#include <algorithm>

namespace {

constexpr int TRD_MAXN = 2048;
constexpr int TRD_SMALL = 128;             // tier A: N (N | 1) + 3 N + 264 doubles of LDS, 137 KB at N = 128
constexpr int TRD_ROWS = 64;               // tier B: rows of the triangle per workgroup
constexpr int TRD_WY = 64;                 // dormtr above tier A: reflectors per compact WY block

// the sum of x over the 256 threads in a fixed order: the xor tree of each wave, then the four waves in order. red: 4 doubles
__device__ __forceinline__ double trd_block_sum(double x, double* red) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = x;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}

// tau, beta = e_k and the divisor of the tail for x = [alpha; tail], sigma = |tail|^2 (a NaN sigma takes the tau = 0 branch)
struct TrdRefl { double tau, beta, div; };
__device__ __forceinline__ TrdRefl trd_reflector(double alpha, double sigma) {
  TrdRefl r;
  if (!(sigma > 0.0)) { r.tau = 0.0; r.beta = alpha; r.div = 0.0; return r; }
  const double nrm = sqrt(alpha * alpha + sigma);
  r.beta = alpha >= 0.0 ? -nrm : nrm;
  r.tau = (r.beta - alpha) / r.beta;
  r.div = alpha - r.beta;
  return r;
}

// ---- tier A ---------------------------------------------------------------------------------------------------------------------
// grid (batch), 256 threads, dynamic LDS. F [batch, N, N], tau [batch, N-1], d [batch, N] and e [batch, N-1] (both may be NULL),
// mx [batch] (may be NULL) receives the bits of max|s_ij|. unscale = 0 leaves d and e on F's diagonals scaled by 2^-e1.
__global__ __launch_bounds__(256) void sytrd_small(const double* __restrict__ S, int N, double* __restrict__ F, double* __restrict__ tau,
                                                   double* __restrict__ d, double* __restrict__ e, u64* __restrict__ mx, int unscale,
                                                   int* __restrict__ flag) {
  extern __shared__ __attribute__((aligned(16))) char trd_smem[];
  const int P = N | 1, t = threadIdx.x, b = blockIdx.x;
  double* A = reinterpret_cast<double*>(trd_smem);            // [N][P], the full symmetric square
  double* v = A + (size_t)N * P;                              // [N]
  double* w = v + N;                                          // [N]: p, then w
  double* part = w + N;                                       // [2][128]
  double* red = part + 256;                                   // [4]
  u64* redu = reinterpret_cast<u64*>(red + 4);                // [4]
  const double* s = S + (size_t)b * N * N;
  double* f = F + (size_t)b * N * N;
  u64 m = 0;
  for (int idx = t; idx < N * N; idx += 256) {
    const int i = idx / N, j = idx - i * N;
    if (j <= i) {
      const double x = s[idx];
      const u64 bits = (u64)__double_as_longlong(fabs(x));
      m = bits > m ? bits : m;
      A[i * P + j] = x; A[j * P + i] = x;
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) { const u64 o = __shfl_xor(m, off); m = o > m ? o : m; }
  if ((t & 63) == 0) redu[t >> 6] = m;
  __syncthreads();
  for (int q = 0; q < 4; ++q) m = redu[q] > m ? redu[q] : m;
  const int e1 = syev_exp(m);
  if (t == 0) { if (mx) mx[b] = m; if (m > SYEV_MAX_BITS) atomicMax(flag, 1); }
  for (int idx = t; idx < N * N; idx += 256) {
    const int i = idx / N, j = idx - i * N;
    A[i * P + j] = ldexp(A[i * P + j], -e1);
  }
  __syncthreads();
  double* tb = tau + (size_t)b * (N > 1 ? N - 1 : 0);
  for (int k = 0; k + 2 < N; ++k) {
    // x = A[k, k+1:] (row k of the mirrored square is column k of the lower triangle)
    const int it = k + 2 + t;
    const double xt = it < N ? A[k * P + it] : 0.0;
    const double sigma = trd_block_sum(xt * xt, red);
    const TrdRefl r = trd_reflector(A[k * P + k + 1], sigma);
    if (t < N) v[t] = t <= k ? 0.0 : (t == k + 1 ? 1.0 : (r.tau != 0.0 ? A[k * P + t] / r.div : 0.0));
    __syncthreads();
    // p = tau A v over the trailing block: two threads per row, the even and the odd columns
    const int row = k + 1 + (t & 127), half = t >> 7;
    if (row < N) {
      double acc = 0.0;
      for (int j = k + 1 + half; j < N; j += 2) acc += A[row * P + j] * v[j];
      part[half * 128 + (t & 127)] = acc;
    }
    __syncthreads();
    double pi = 0.0, pv = 0.0;
    if (t < 128 && row < N) { pi = r.tau * (part[t] + part[128 + t]); pv = pi * v[row]; }
    const double dot = trd_block_sum(pv, red);
    if (t < 128 && row < N) w[row] = pi - (0.5 * r.tau * dot) * v[row];
    __syncthreads();
    {                                                         // A -= v w^T + w v^T, each product rounded on its own: A stays symmetric
#pragma clang fp contract(off)
      const int mm = N - k - 1;
      for (int idx = t; idx < mm * mm; idx += 256) {
        const int i = k + 1 + idx / mm, j = k + 1 + idx % mm;
        const double a1 = v[i] * w[j], a2 = w[i] * v[j];
        A[i * P + j] -= a1 + a2;
      }
    }
    // column k of the lower triangle is finished: e_k and the tail of v_k (row k of the square is not read again)
    if (t < N && t > k) A[t * P + k] = t == k + 1 ? r.beta : v[t];
    if (t == 0) tb[k] = r.tau;
    __syncthreads();
  }
  if (t == 0 && N > 1) tb[N - 2] = 0.0;
  for (int idx = t; idx < N * N; idx += 256) {
    const int i = idx / N, j = idx - i * N;
    double x = j <= i ? A[i * P + j] : 0.0;
    if (j + 1 >= i && j <= i) {                               // d_i and e_j
      if (unscale) x = ldexp(x, e1);
      if (d && j == i) d[(size_t)b * N + i] = x;
      if (e && j + 1 == i) e[(size_t)b * (N - 1) + j] = x;
    }
    f[idx] = x;
  }
}

// ---- tier B ---------------------------------------------------------------------------------------------------------------------
// mx[b] = bits of max|S[b, i, j]| over j <= i; grid (rows, batch). The maximum of integers: any order gives the same word.
__global__ __launch_bounds__(256) void sytrd_absmax(const double* __restrict__ S, int N, u64* __restrict__ mx) {
  const double* s = S + (size_t)blockIdx.y * N * N;
  u64 m = 0;
  for (int r = blockIdx.x; r < N; r += gridDim.x)
    for (int c = threadIdx.x; c <= r; c += 256) {
      const u64 bits = (u64)__double_as_longlong(fabs(s[(size_t)r * N + c]));
      m = bits > m ? bits : m;
    }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) { const u64 o = __shfl_xor(m, off); m = o > m ? o : m; }
  if ((threadIdx.x & 63) == 0 && m) atomicMax(mx + blockIdx.y, m);
}

// F[b] = 2^-e1 lower(S[b]), zero above the diagonal; grid (N, batch)
__global__ __launch_bounds__(256) void sytrd_load(const double* __restrict__ S, double* __restrict__ F, int N, const u64* __restrict__ mx) {
  const int i = blockIdx.x, e1 = syev_exp(mx[blockIdx.y]);
  const double* s = S + ((size_t)blockIdx.y * N + i) * N;
  double* f = F + ((size_t)blockIdx.y * N + i) * N;
  for (int j = threadIdx.x; j < N; j += 256) f[j] = j <= i ? ldexp(s[j], -e1) : 0.0;
}

// the work of one member between launches: everything [batch, ...]
struct TrdWs {
  double* tau;      // [N-1] (the caller's)
  double* dsc;      // [N] scaled d
  double* esc;      // [N] scaled e
  double* vd;       // [2][N] v_k, dense, by the parity of k
  double* rowsum;   // [2][N] row sums of A v_k, by the parity of k
  double* colpart;  // [2][nblk][N] column partials of A v_k per row block, by the parity of k
};

// launch k of tier B; grid (nblk, batch), 256 threads, dynamic LDS of 7 N + 4 doubles
__global__ __launch_bounds__(256) void sytrd_step(double* __restrict__ F, int N, int k, TrdWs ws) {
  extern __shared__ __attribute__((aligned(16))) char trd_smem[];
  double* vp = reinterpret_cast<double*>(trd_smem);           // [N] v_{k-1}
  double* wp = vp + N;                                        // [N] w_{k-1}
  double* vk = wp + N;                                        // [N] v_k
  double* cw = vk + N;                                        // [4][N] column sums per wave
  double* red = cw + 4 * (size_t)N;                           // [4]
  const int t = threadIdx.x, b = blockIdx.y, blk = blockIdx.x, nblk = gridDim.x;
  const int r0 = blk * TRD_ROWS, r1 = min(N, r0 + TRD_ROWS);
  const bool last = blk == nblk - 1;
  if (r1 <= k + 1 && !last) return;                           // rows <= k are finished (the last block stores the scalars)
  double* A = F + (size_t)b * N * N;
  double* tb = ws.tau + (size_t)b * (N - 1);
  const int par = k & 1, ppar = par ^ 1;
  // (i) w_{k-1} over the trailing indices of step k-1, j >= k
  if (k == 0) {
    for (int j = t; j < N; j += 256) { vp[j] = 0.0; wp[j] = 0.0; }
  } else {
    const double taup = tb[k - 1];
    const double* vprev = ws.vd + ((size_t)b * 2 + ppar) * N;
    const double* rs = ws.rowsum + ((size_t)b * 2 + ppar) * N;
    const double* cp = ws.colpart + ((size_t)b * 2 + ppar) * nblk * N;
    double acc = 0.0;
    for (int j = k + t; j < N; j += 256) {
      double s = rs[j];
      for (int q = j / TRD_ROWS; q < nblk; ++q) s += cp[(size_t)q * N + j];
      const double pj = taup * s, vj = vprev[j];
      vp[j] = vj; wp[j] = pj; acc += pj * vj;
    }
    const double dot = trd_block_sum(acc, red);
    for (int j = k + t; j < N; j += 256) wp[j] -= (0.5 * taup * dot) * vp[j];
  }
  __syncthreads();
  // (ii) column k after step k-1: d_k, then the reflector of [alpha; tail]
  {
    const double wk = wp[k], vpk = vp[k];
    double acc = 0.0;
    for (int i = k + t; i < N; i += 256) {
      const double c = A[(size_t)i * N + k] - (vp[i] * wk + wp[i] * vpk);
      vk[i] = c;
      if (i >= k + 2) acc += c * c;
    }
    const double sigma = trd_block_sum(acc, red);
    const double dk = vk[k];
    TrdRefl r; r.tau = 0.0; r.beta = 0.0; r.div = 0.0;
    if (k + 1 < N) r = trd_reflector(vk[k + 1], sigma);
    __syncthreads();
    double* vout = ws.vd + ((size_t)b * 2 + par) * N;
    for (int i = k + t; i < N; i += 256) {
      const double x = i == k ? 0.0 : (i == k + 1 ? 1.0 : (r.tau != 0.0 ? vk[i] / r.div : 0.0));
      vk[i] = x;
      if (last) vout[i] = x;
    }
    if (last && t == 0) {
      ws.dsc[(size_t)b * N + k] = dk;
      if (k + 1 < N) { ws.esc[(size_t)b * N + k] = r.beta; tb[k] = r.tau; }
    }
  }
  __syncthreads();
  // (iii) rows max(r0, k+1) .. r1-1, columns k+1 .. row: the update of step k-1, and the sums of A v_k
  const int wv = t >> 6, lane = t & 63;
  double rowacc[TRD_ROWS / 4];
#pragma unroll
  for (int r = 0; r < TRD_ROWS / 4; ++r) rowacc[r] = 0.0;
  for (int j0 = k + 1; j0 < r1; j0 += 64) {
    const int j = j0 + lane;
    const bool jin = j < N;
    const double vkj = jin ? vk[j] : 0.0, vpj = jin ? vp[j] : 0.0, wpj = jin ? wp[j] : 0.0;
    double colacc = 0.0;
#pragma unroll
    for (int r = 0; r < TRD_ROWS / 4; ++r) {
      const int i = r0 + wv + 4 * r;
      if (i > k && i < r1 && j <= i) {                        // j <= i < r1 <= N
        const double a = A[(size_t)i * N + j] - (vp[i] * wpj + wp[i] * vpj);
        A[(size_t)i * N + j] = a;
        rowacc[r] += a * vkj;
        if (j < i) colacc += a * vk[i];
      }
    }
    if (jin) cw[(size_t)wv * N + j] = colacc;
  }
  double* rs = ws.rowsum + ((size_t)b * 2 + par) * N;
#pragma unroll
  for (int r = 0; r < TRD_ROWS / 4; ++r) {
    double x = rowacc[r];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off);
    const int i = r0 + wv + 4 * r;
    if (lane == 0 && i > k && i < r1) rs[i] = x;
  }
  // the tail of v_{k-1} takes the place of column k-1, which launch k-1 was the last to read
  if (k > 0)
    for (int i = max(r0, k + 1) + t; i < r1; i += 256) A[(size_t)i * N + k - 1] = vp[i];
  __syncthreads();
  double* cp = ws.colpart + (((size_t)b * 2 + par) * nblk + blk) * N;
  for (int j = k + 1 + t; j < r1; j += 256) cp[j] = ((cw[j] + cw[(size_t)N + j]) + cw[2 * (size_t)N + j]) + cw[3 * (size_t)N + j];
}

// after the last launch: d and e onto F's diagonals and into their own arrays, the flag; grid (batch)
__global__ __launch_bounds__(256) void sytrd_finish(double* __restrict__ F, int N, TrdWs ws, const u64* __restrict__ mx, double* __restrict__ d,
                                                    double* __restrict__ e, int unscale, int* __restrict__ flag) {
  const int b = blockIdx.x, e1 = unscale ? syev_exp(mx[b]) : 0;
  double* f = F + (size_t)b * N * N;
  for (int i = threadIdx.x; i < N; i += 256) {
    const double di = ldexp(ws.dsc[(size_t)b * N + i], e1);
    f[(size_t)i * N + i] = di;
    if (d) d[(size_t)b * N + i] = di;
    if (i + 1 < N) {
      const double ei = ldexp(ws.esc[(size_t)b * N + i], e1);
      f[(size_t)(i + 1) * N + i] = ei;
      if (e) e[(size_t)b * (N - 1) + i] = ei;
    }
  }
  if (threadIdx.x == 0 && mx[b] > SYEV_MAX_BITS) atomicMax(flag, 1);
}

// ---- dormtr ---------------------------------------------------------------------------------------------------------------------
// N <= 128: grid (ceil(K / 128), batch), 128 threads, one column of Z [batch, N, K] per thread, in LDS (N x 128 + 3 N doubles).
// Reflector k: z -= v (tau (v^T z)); Q Z applies k = N-3 .. 0, Q^T Z applies k = 0 .. N-3. The tail of the next reflector is fetched
// while the current one is applied.
__global__ __launch_bounds__(128) void ormtr_small(const double* __restrict__ F, const double* __restrict__ tau, double* __restrict__ Z, int N,
                                                   int K, int transpose) {
  extern __shared__ __attribute__((aligned(16))) char trd_smem[];
  double* z = reinterpret_cast<double*>(trd_smem);            // [N][128]
  double* vb = z + (size_t)N * 128;                           // [2][N]
  double* tl = vb + 2 * (size_t)N;                            // [N] tau
  const int t = threadIdx.x, b = blockIdx.y, c = blockIdx.x * 128 + t;
  const bool active = c < K;
  const double* f = F + (size_t)b * N * N;
  const double* tb = tau + (size_t)b * (N - 1);
  double* zb = Z + (size_t)b * N * K;
  for (int i = 0; i < N; ++i) z[i * 128 + t] = active ? zb[(size_t)i * K + c] : 0.0;
  if (t < N - 1) tl[t] = tb[t];                               // (made visible by the first step's barrier)
  const int nref = N - 2;                                     // N >= 3 here
  int k = transpose ? 0 : nref - 1;
  double vnext = t > k + 1 && t < N ? f[(size_t)t * N + k] : 0.0;   // N <= 128: thread t holds row t of a reflector
  for (int s = 0; s < nref; ++s) {
    k = transpose ? s : nref - 1 - s;
    double* v = vb + (s & 1) * N;
    if (t < N) v[t] = t == k + 1 ? 1.0 : vnext;               // rows <= k: 0
    if (s + 1 < nref) {
      const int kn = transpose ? s + 1 : nref - 2 - s;
      vnext = t > kn + 1 && t < N ? f[(size_t)t * N + kn] : 0.0;
    }
    __syncthreads();                                          // one per step: v alternates between two buffers
    double dot = 0.0;
    for (int i = k + 1; i < N; ++i) dot += v[i] * z[i * 128 + t];
    dot *= tl[k];
    for (int i = k + 1; i < N; ++i) z[i * 128 + t] -= v[i] * dot;
  }
  if (active)
    for (int i = 0; i < N; ++i) zb[(size_t)i * K + c] = z[i * 128 + t];
}

// compact WY, the reflectors k0 .. k0 + nb - 1 of every member as the dense V [batch, rows, TRD_WY], rows = N - k0 - 1 (row r is
// row k0 + 1 + r of the member): unit diagonal, zero above, columns >= nb zero. grid (rows, batch), 64 threads
__global__ __launch_bounds__(64) void ormtr_wy_v(const double* __restrict__ F, int N, int k0, int nb, double* __restrict__ V) {
  const int r = blockIdx.x, c = threadIdx.x, rows = N - k0 - 1;
  const double* f = F + (size_t)blockIdx.y * N * N;
  double x = 0.0;
  if (c < nb) x = r < c ? 0.0 : (r == c ? 1.0 : f[(size_t)(k0 + 1 + r) * N + k0 + c]);
  V[((size_t)blockIdx.y * rows + r) * TRD_WY + c] = x;
}

// T [batch, 64, 64] upper triangular with I - V T V^T = H_k0 ... H_{k0+nb-1}, from G = V^T V [batch, 64, 64] (dlarft, forward,
// columnwise): T_jj = tau_j, T[0:j, j] = -tau_j T[0:j, 0:j] G[0:j, j]. transpose: T^T is stored. One workgroup of 64 per member;
// thread i owns row i of T, column after column (G[l, j] is one address for the whole wave).
__global__ __launch_bounds__(64) void ormtr_wy_t(const double* __restrict__ G, const double* __restrict__ tau, int N, int k0, int nb,
                                                 int transpose, double* __restrict__ T) {
  __shared__ double tl[TRD_WY][TRD_WY + 1];
  const int i = threadIdx.x, b = blockIdx.x;
  const double* g = G + (size_t)b * TRD_WY * TRD_WY;
  for (int r = 0; r < TRD_WY; ++r) tl[r][i] = 0.0;
  __syncthreads();
  const double* tb = tau + (size_t)b * (N - 1) + k0;
  for (int j = 0; j < nb; ++j) {
    const double tj = tb[j];
    if (i < j) {
      double s = 0.0;
      for (int l = i; l < j; ++l) s += tl[i][l] * g[l * TRD_WY + j];
      tl[i][j] = -tj * s;
    } else if (i == j) tl[i][j] = tj;
    __syncthreads();
  }
  double* tt = T + (size_t)b * TRD_WY * TRD_WY;
  for (int r = 0; r < TRD_WY; ++r) tt[r * TRD_WY + i] = transpose ? tl[i][r] : tl[r][i];
}

template <class T> int trd_alloc(nd4hip_handle* h, size_t count, T** out) {
  void* p = nullptr;
  ND4_TRY(nd4_ws_alloc(h, sizeof(T) * (count ? count : 1), &p));
  *out = static_cast<T*>(p);
  return 0;
}

// above 64 KB of dynamic LDS the launch needs the function attribute (set every time: it is per device)
int trd_lds_attr(const void* fn, size_t lds) {
  if (lds > 64 * 1024) ND4_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  return 0;
}

}  // namespace

// the host-side arithmetic of the two tiers (also what the stand-alone host check exercises)
int nd4_sytrd_tier(int64_t N) { return N <= TRD_SMALL ? 0 : 1; }
size_t nd4_sytrd_lds(int64_t N) {
  return sizeof(double) * (nd4_sytrd_tier(N) == 0 ? (size_t)N * (size_t)(N | 1) + 3 * (size_t)N + 264 : 7 * (size_t)N + 4);
}
int64_t nd4_sytrd_blocks(int64_t N) { return (N + TRD_ROWS - 1) / TRD_ROWS; }
// doubles of workspace per member of tier B: dsc, esc, vd, rowsum, colpart
size_t nd4_sytrd_ws_doubles(int64_t N) { return (size_t)N * (2 + 2 + 2 + 2 * (size_t)nd4_sytrd_blocks(N)); }

// S [batch, N, N] -> F, tau [batch, N-1]; d [batch, N] and e [batch, N-1] may be NULL. mx [batch] must be ZERO on entry and
// receives the bits of max|s_ij| per member; *flag (zero on entry) is raised for NaN or Inf. unscale = false leaves d and e on F's
// diagonals (and in d, e) scaled by 2^-e1, e1 = syev_exp(mx). batch <= 32768 (the grids' y axis), 1 <= N <= 2048. Enqueues only.
int nd4_sytrd(nd4hip_handle* h, int64_t batch, int64_t N64, const double* S, double* F, double* tau, double* d, double* e, u64* mx,
              bool unscale, int* flag) {
  ND4_CHECK_ARG(N64 >= 1 && N64 <= TRD_MAXN && batch >= 1 && batch <= 32768, "nd4hip_dsytrd_batched: extent out of range");
  const int N = (int)N64;
  const size_t lds = nd4_sytrd_lds(N);
  if (nd4_sytrd_tier(N) == 0) {
    ND4_TRY(trd_lds_attr(reinterpret_cast<const void*>(&sytrd_small), lds));
    hipLaunchKernelGGL(sytrd_small, dim3((unsigned)batch), dim3(256), lds, h->stream, S, N, F, tau, d, e, mx, unscale ? 1 : 0, flag);
    ND4_HIP(hipGetLastError());
    return 0;
  }
  const int nblk = (int)nd4_sytrd_blocks(N);
  TrdWs ws;
  ws.tau = tau;
  ND4_TRY(trd_alloc(h, (size_t)batch * N, &ws.dsc)); ND4_TRY(trd_alloc(h, (size_t)batch * N, &ws.esc));
  ND4_TRY(trd_alloc(h, (size_t)batch * 2 * N, &ws.vd)); ND4_TRY(trd_alloc(h, (size_t)batch * 2 * N, &ws.rowsum));
  ND4_TRY(trd_alloc(h, (size_t)batch * 2 * nblk * N, &ws.colpart));
  hipLaunchKernelGGL(sytrd_absmax, dim3(256u, (unsigned)batch), dim3(256), 0, h->stream, S, N, mx);
  hipLaunchKernelGGL(sytrd_load, dim3((unsigned)N, (unsigned)batch), dim3(256), 0, h->stream, S, F, N, mx);
  ND4_TRY(trd_lds_attr(reinterpret_cast<const void*>(&sytrd_step), lds));
  for (int k = 0; k < N; ++k) hipLaunchKernelGGL(sytrd_step, dim3((unsigned)nblk, (unsigned)batch), dim3(256), lds, h->stream, F, N, k, ws);
  hipLaunchKernelGGL(sytrd_finish, dim3((unsigned)batch), dim3(256), 0, h->stream, F, N, ws, mx, d, e, unscale ? 1 : 0, flag);
  ND4_HIP(hipGetLastError());
  return 0;
}

// Z [batch, N, K] <- Q Z (transpose: Q^T Z) in place, Q from F, tau of nd4_sytrd. batch <= 32768, 1 <= N <= 2048, K >= 1. Enqueues only.
int nd4_ormtr(nd4hip_handle* h, int64_t batch, int64_t N64, int64_t K64, bool transpose, const double* F, const double* tau, double* Z) {
  ND4_CHECK_ARG(N64 >= 1 && N64 <= TRD_MAXN && batch >= 1 && batch <= 32768 && K64 >= 1 && K64 < (1 << 30),
                "nd4hip_dormtr_batched: extent out of range");
  const int N = (int)N64, K = (int)K64, nref = N - 2;
  if (nref <= 0) return 0;                                    // Q = I
  if (N <= TRD_SMALL) {
    const size_t lds = sizeof(double) * ((size_t)N * 128 + 3 * (size_t)N);
    const int64_t tiles = (K64 + 127) / 128;
    ND4_CHECK_ARG(tiles <= 0x7fffffffll, "nd4hip_dormtr_batched: extent out of range");
    ND4_TRY(trd_lds_attr(reinterpret_cast<const void*>(&ormtr_small), lds));
    hipLaunchKernelGGL(ormtr_small, dim3((unsigned)tiles, (unsigned)batch), dim3(128), lds, h->stream, F, tau, Z, N, K, transpose ? 1 : 0);
    ND4_HIP(hipGetLastError());
    return 0;
  }
  Nd4WsScope scope(h);
  double *V, *G, *T, *Y, *W;
  ND4_TRY(trd_alloc(h, (size_t)batch * N * TRD_WY, &V)); ND4_TRY(trd_alloc(h, (size_t)batch * TRD_WY * TRD_WY, &G));
  ND4_TRY(trd_alloc(h, (size_t)batch * TRD_WY * TRD_WY, &T));
  ND4_TRY(trd_alloc(h, (size_t)batch * TRD_WY * K, &Y)); ND4_TRY(trd_alloc(h, (size_t)batch * TRD_WY * K, &W));
  const int nblocks = (nref + TRD_WY - 1) / TRD_WY;
  const int64_t w2 = (int64_t)TRD_WY * TRD_WY, wk = (int64_t)TRD_WY * K;
  for (int s = 0; s < nblocks; ++s) {
    const int k0 = (transpose ? s : nblocks - 1 - s) * TRD_WY, nb = std::min(TRD_WY, nref - k0), rows = N - k0 - 1;
    const int64_t sv = (int64_t)rows * TRD_WY;
    double* Zs = Z + (size_t)(k0 + 1) * K;                    // rows k0 + 1 .. N - 1 of every member
    hipLaunchKernelGGL(ormtr_wy_v, dim3((unsigned)rows, (unsigned)batch), dim3(64), 0, h->stream, F, N, k0, nb, V);
    ND4_HIP(hipGetLastError());
    ND4_TRY(nd4_gemm(h, true, false, TRD_WY, TRD_WY, rows, 1.0, V, TRD_WY, sv, V, TRD_WY, sv, 0.0, G, TRD_WY, w2, batch));
    hipLaunchKernelGGL(ormtr_wy_t, dim3((unsigned)batch), dim3(64), 0, h->stream, G, tau, N, k0, nb, transpose ? 1 : 0, T);
    ND4_HIP(hipGetLastError());
    ND4_TRY(nd4_gemm(h, true, false, TRD_WY, K, rows, 1.0, V, TRD_WY, sv, Zs, K, (int64_t)N * K, 0.0, Y, K, wk, batch));
    ND4_TRY(nd4_gemm(h, false, false, TRD_WY, K, TRD_WY, 1.0, T, TRD_WY, w2, Y, K, wk, 0.0, W, K, wk, batch));
    ND4_TRY(nd4_gemm(h, false, false, rows, K, TRD_WY, -1.0, V, TRD_WY, sv, W, K, wk, 1.0, Zs, K, (int64_t)N * K, batch));
  }
  return 0;
}

namespace {
int trd_read_flag(nd4hip_handle* h, const int* flag, int* value) {
  void* hp = nullptr;
  ND4_TRY(nd4_pinned(h, sizeof(int), &hp));
  ND4_HIP(hipMemcpyAsync(hp, flag, sizeof(int), hipMemcpyDeviceToHost, h->stream));
  ND4_HIP(hipStreamSynchronize(h->stream));
  *value = *static_cast<int*>(hp);
  return 0;
}
}  // namespace

// tridiag_factor on device pointers: arguments already checked, batch in 1 .. 32768, 1 <= N <= 2048. Synchronises (the flag word).
int nd4_sytrd_run(nd4hip_handle* h, int64_t batch, int64_t N, const double* S, double* F, double* tau, double* d, double* e) {
  Nd4WsScope scope(h);
  u64* mx = nullptr; int* flag = nullptr; int bad = 0;
  ND4_TRY(trd_alloc(h, (size_t)batch, &mx)); ND4_TRY(trd_alloc(h, 1, &flag));
  ND4_HIP(hipMemsetAsync(mx, 0, sizeof(u64) * (size_t)batch, h->stream));
  ND4_HIP(hipMemsetAsync(flag, 0, sizeof(int), h->stream));
  ND4_TRY(nd4_sytrd(h, batch, N, S, F, tau, d, e, mx, true, flag));
  ND4_TRY(trd_read_flag(h, flag, &bad));
  if (bad) {
    nd4_set_error("tridiag_decomp(S): S contains NaN or Infinity in its lower triangle.");
    return ND4HIP_ERR_NOCONV;
  }
  return 0;
}
