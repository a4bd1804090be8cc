// Complex128 reduction to Hessenberg form on the device: zhess_factor / zhess_apply_q / zhess_decomp, LAPACK's zgehrd /
// zunmhr on row-major members, interleaved (re, im) doubles.
//   A = Q H Q^H for 1 <= N <= 2048, H upper Hessenberg with an exactly real subdiagonal.
//   Q = H_0 ... H_{N-2}, H_k = I - tau_k v_k v_k^H, v_k zero in rows 0..k, 1 in row k+1, its tail in F[k+2:, k]: hetrd.hip's layout, so
//   nd4_zunmtr applies Q. As there, the last reflector has an empty tail and exists only to make h_{N-1,N-2} real: tau is [N-1].
//   Step k: x = A[k+1:, k] is reflected (zlarfg.h), then A <- H_k^H A H_k = A - y v^H - v z^H with
//     y = tau A[:, k+1:] v (all N rows),  z^H = conj(tau) (v^H A[k+1:, k+1:] - (v^H y) v^H).
// Every member is scaled on load by 2^-e1, e1 the exponent that puts max(|Re a_ij|, |Im a_ij|) in [0.5, 1); H gets 2^e1 back on its
// store, exactly: A -> 2^m A leaves tails and tau bit-identical. Tiny columns are lifted as in hetrd.hip. NaN or Inf shows in the bits of
// the maximum: one flag word per call, INT_MAX - (the lowest such member).
// Every sum has an order fixed by (N, k): no atomics on doubles; the only synchronisation is __syncthreads(), wave shuffles and the
// kernel boundary; every loop bound comes from the shape. The file is built without FMA contraction.
//   Tier A, zgehrd_small: the member in one workgroup's LDS at the odd pitch N | 1, one launch per call, when
//       16 (N (N | 1) + 7 N + 256) + 96 <= 163840   (the member, v, y, z, the partial column sums of at most 4 N + 256, the reduction
//                                                    scratch): N <= 95 (159232 bytes; N = 96 would take 163936)
//     y by rows (CW lanes per row, xor tree), one pass writes A - y v^H, the column sums v^H (A - y v^H) by 256 / CW groups of rows
//     added in group order, a last pass subtracts v z^H.
//   Tier B, zgehrd_step: ONE launch per column over a grid (blocks of 64 rows, members); the rank-2 update is applied lazily. Launch k:
//     every block forms z^H of step k-1 from the per-block column partials (added in block order) and the pending (v, y), brings
//     column k up to date on its own (O(N)) and reflects it; in one pass over its 64 rows and the columns right of k it applies
//     A -= y v^H + v z^H of step k-1 and accumulates its rows of A v_k (row sums, complete inside the block) and its column partials
//     of v_k^H A. v, y and the partials alternate between two buffers by the parity of k: a block never writes what another block of the
//     same launch reads. Column k of F (H above, the tail below) is written one launch later from a dense copy. 48 N bytes of dynamic
//     LDS beside 11 KB of static LDS: 98304 at N = 2048. zgehrd_finish applies the last pending update to column N-1 and unscales.
//   A blocked zlahr2 form is not built: one large matrix is launch-bound (DESIGN.md 4.29 has the numbers).
#include "nd4hip_internal.h"
#include "zlarfg.h"
#include <cfloat>
#include <climits>

namespace {

constexpr int ZHRD_MAXN = 2048;
constexpr int ZHRD_T = 256;
constexpr int ZHRD_ROWS = 64;                    // tier B: rows per workgroup
constexpr size_t ZHRD_LDS = 163840;
constexpr int64_t ZHRD_CHUNK = 32768;            // members per pass
constexpr int64_t ZHRD_WS_ELEMS = 1ll << 26;     // a pass's workspace takes about 1 GiB

__host__ __device__ inline int zhrd_cw(int N) { return N > 32 ? 64 : N > 16 ? 32 : N > 8 ? 16 : 8; }
__device__ __forceinline__ cd zhrd_sq(cd x) { return cmk(x.x * x.x + x.y * x.y, x.x != 0.0 || x.y != 0.0 ? 1.0 : 0.0); }
__device__ __forceinline__ int zhrd_flag_of(long member) { return INT_MAX - (int)(member < INT_MAX - 1 ? member : INT_MAX - 1); }

template <class Again>
__device__ __forceinline__ HetRefl zhrd_reflect(cd alpha, cd sn, double* red, Again again) {
  double sigma = sn.x, c = 1.0;
  for (int lvl = 0; lvl < 2 && het_tiny(alpha, c, sigma, sn.y); ++lvl) {
    c *= HET_LIFT;
    sigma = het_block_sum(cmk(again(c), 0.0), red).x;
  }
  return het_reflector(alpha, sigma, c);
}

// ---- tier A ---------------------------------------------------------------------------------------------------------------------
// grid (members), 256 threads. A, F [members, N, N], tau [members, N - 1]
__global__ __launch_bounds__(ZHRD_T) void zgehrd_small(const cd* __restrict__ A, cd* __restrict__ F, cd* __restrict__ tau, int N, long member0,
                                                       int* __restrict__ flag) {
  extern __shared__ __attribute__((aligned(16))) char zhrd_smem[];
  const int P = N | 1, t = threadIdx.x;
  const long b = blockIdx.x;
  cd* S = reinterpret_cast<cd*>(zhrd_smem);                   // [N][P]
  cd* v = S + (size_t)N * P;                                  // [N]
  cd* y = v + N;                                              // [N]
  cd* z = y + N;                                              // [N] z^H
  cd* part = z + N;                                           // [256 / CW][N]: at most 4 N + 256
  double* red = reinterpret_cast<double*>(part + 4 * N + 256);   // [8]
  u64* redu = reinterpret_cast<u64*>(red + 8);                // [4]
  const cd* a = A + b * N * N;
  const cd zero = cmk(0.0, 0.0), one = cmk(1.0, 0.0);
  u64 m = 0;
  for (int idx = t; idx < N * N; idx += ZHRD_T) {
    const int i = idx / N, j = idx - i * N;
    const cd x = a[idx];
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
  if (t == 0 && m > SYEV_MAX_BITS) atomicMax(flag, zhrd_flag_of(member0 + b));
  for (int idx = t; idx < N * N; idx += ZHRD_T) {
    const int i = idx / N, j = idx - i * N;
    const cd x = S[i * P + j];
    S[i * P + j] = cmk(ldexp(x.x, -e1), ldexp(x.y, -e1));
  }
  __syncthreads();
  const int CW = zhrd_cw(N), RG = ZHRD_T / CW, cl = t % CW, q = t / CW;
  cd* tb = tau + b * (N - 1);
  for (int k = 0; k + 1 < N; ++k) {
    cd sn = zero;
    for (int i = k + 2 + t; i < N; i += ZHRD_T) sn = cadd(sn, zhrd_sq(S[i * P + k]));
    const cd alpha = S[(k + 1) * P + k];
    sn = het_block_sum(sn, red);
    const HetRefl r = zhrd_reflect(alpha, sn, red, [&](double c) {
      double a2 = 0.0;
      for (int i = k + 2 + t; i < N; i += ZHRD_T) { const double xr = c * S[i * P + k].x, xi = c * S[i * P + k].y; a2 += xr * xr + xi * xi; }
      return a2;
    });
    if (t == 0) tb[k] = r.tau;
    if (!r.on) continue;                                      // (uniform) tau = 0: the step changes nothing, h_{k+1,k} = Re alpha already
    for (int i = t; i < N; i += ZHRD_T) v[i] = i <= k ? zero : (i == k + 1 ? one : cdiv_re(S[i * P + k], r.div));
    __syncthreads();
    // y = tau A[:, k+1:] v by rows
    for (int i0 = 0; i0 < N; i0 += RG) {                      // (uniform bounds: the shuffles below are reached by whole groups)
      const int i = i0 + q;
      cd acc = zero;
      if (i < N)
        for (int col = k + 1 + cl; col < N; col += CW) acc = cadd(acc, cmul(S[i * P + col], v[col]));
      for (int off = CW >> 1; off > 0; off >>= 1) { acc.x += __shfl_xor(acc.x, off); acc.y += __shfl_xor(acc.y, off); }
      if (cl == 0 && i < N) y[i] = cmul(r.tau, acc);
    }
    __syncthreads();
    // A - y v^H on the columns right of k, all rows
    const int nn = N - k - 1;
    for (int idx = t; idx < N * nn; idx += ZHRD_T) {
      const int i = idx / nn, col = k + 1 + idx % nn;
      S[i * P + col] = csub(S[i * P + col], cmulc(y[i], v[col]));
    }
    __syncthreads();
    // z^H = conj(tau) v^H (A - y v^H) over the rows below k
    for (int col = k + 1 + cl; col < N; col += CW) {
      cd s = zero;
      for (int i = k + 1 + q; i < N; i += RG) s = cadd(s, cmulc(S[i * P + col], v[i]));   // conj(v_i) a_ic
      part[q * N + col] = s;
    }
    __syncthreads();
    const cd ctau = cconj(r.tau);
    for (int col = k + 1 + t; col < N; col += ZHRD_T) {
      cd s = part[col];
      for (int g = 1; g < RG; ++g) s = cadd(s, part[g * N + col]);
      z[col] = cmul(ctau, s);
    }
    __syncthreads();
    for (int idx = t; idx < nn * nn; idx += ZHRD_T) {
      const int i = k + 1 + idx / nn, col = k + 1 + idx % nn;
      S[i * P + col] = csub(S[i * P + col], cmul(v[i], z[col]));
    }
    for (int i = k + 1 + t; i < N; i += ZHRD_T) S[i * P + k] = i == k + 1 ? cmk(r.beta, 0.0) : v[i];
    __syncthreads();
  }
  cd* f = F + b * N * N;
  for (int idx = t; idx < N * N; idx += ZHRD_T) {
    const int i = idx / N, j = idx - i * N;
    const cd x = S[i * P + j];
    f[idx] = j + 1 >= i ? cmk(ldexp(x.x, e1), ldexp(x.y, e1)) : x;
  }
}

// ---- tier B ---------------------------------------------------------------------------------------------------------------------
// mx[b] = the bits of max(|Re|, |Im|) over A[b] (mx zero on entry; the maximum of integers: any order gives the same word), the flag
// for NaN or Inf; grid (256, members)
__global__ __launch_bounds__(ZHRD_T) void zeig_absmax_k(const cd* __restrict__ A, long count, u64* __restrict__ mx, long member0, int* __restrict__ flag) {
  const cd* s = A + (long)blockIdx.y * count;
  u64 m = 0;
  for (long i = (long)blockIdx.x * ZHRD_T + threadIdx.x; i < count; i += (long)gridDim.x * ZHRD_T) {
    const u64 br = het_bits(s[i].x), bi = het_bits(s[i].y);
    m = br > m ? br : m; m = bi > m ? bi : m;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) { const u64 o = __shfl_xor(m, off); m = o > m ? o : m; }
  if ((threadIdx.x & 63) == 0 && m) { atomicMax(mx + blockIdx.y, m); if (m > SYEV_MAX_BITS) atomicMax(flag, zhrd_flag_of(member0 + blockIdx.y)); }
}
// F[b] = 2^-e1 A[b]; grid (tiles of 256 elements, members)
__global__ __launch_bounds__(ZHRD_T) void zhrd_load(const cd* __restrict__ A, cd* __restrict__ F, long count, const u64* __restrict__ mx) {
  const long i = (long)blockIdx.x * ZHRD_T + threadIdx.x;
  if (i >= count) return;
  const int e1 = syev_exp(mx[blockIdx.y]);
  const cd x = A[(long)blockIdx.y * count + i];
  F[(long)blockIdx.y * count + i] = cmk(ldexp(x.x, -e1), ldexp(x.y, -e1));
}
// x[0 .. n) = 0
__global__ __launch_bounds__(ZHRD_T) void zeig_clear_k(double* __restrict__ x, long n) {
  const long i = (long)blockIdx.x * ZHRD_T + threadIdx.x;
  if (i < n) x[i] = 0.0;
}

// the work of one member between launches: everything [members, ...]
struct ZhrdWs {
  cd* tau;          // [N - 1] (the caller's)
  cd* vd;           // [2][N] v_k, dense, by the parity of k
  cd* yd;           // [2][N] y of step k
  cd* colout;       // [2][N] column k of F as step k leaves it
  cd* colpart;      // [2][nblk][N] column partials of v_k^H A per row block
};

// z^H of step k-1 for the columns j0 <= j < N into zs (LDS), from the pending buffers of parity pp; every thread calls it
__device__ __forceinline__ void zhrd_pending_z(const ZhrdWs& ws, long b, int N, int nblk, int k, int j0, cd* zs, double* red) {
  const int t = threadIdx.x, pp = (k & 1) ^ 1;
  const cd zero = cmk(0.0, 0.0);
  if (k == 0) {
    for (int j = j0 + t; j < N; j += ZHRD_T) zs[j] = zero;
    __syncthreads();
    return;
  }
  const cd* vp = ws.vd + (b * 2 + pp) * N;
  const cd* yp = ws.yd + (b * 2 + pp) * N;
  const cd* cp = ws.colpart + (b * 2 + pp) * (long)nblk * N;
  cd dot = zero;
  for (int i = k + t; i < N; i += ZHRD_T) dot = cadd(dot, cmulc(yp[i], vp[i]));   // conj(v_i) y_i
  dot = het_block_sum(dot, red);
  const cd ctau = cconj(ws.tau[b * (N - 1) + k - 1]);
  const int q0 = k / ZHRD_ROWS;
  for (int j = j0 + t; j < N; j += ZHRD_T) {
    cd s = cp[(long)q0 * N + j];
    for (int q = q0 + 1; q < nblk; ++q) s = cadd(s, cp[(long)q * N + j]);
    zs[j] = cmul(ctau, csub(s, cmulc(dot, vp[j])));
  }
  __syncthreads();
}

// launch k = 0 .. N-2; grid (nblk, members), 256 threads, 48 N bytes of dynamic LDS
__global__ __launch_bounds__(ZHRD_T) void zgehrd_step(cd* __restrict__ F, int N, int k, ZhrdWs ws) {
  extern __shared__ __attribute__((aligned(16))) char zhrd_smem[];
  __shared__ cd cw[2][4][64], vps[ZHRD_ROWS], yps[ZHRD_ROWS];
  __shared__ double red[8];
  cd* zs = reinterpret_cast<cd*>(zhrd_smem);                  // [N] z^H of step k-1
  cd* ck = zs + N;                                            // [N] column k
  cd* vk = ck + N;                                            // [N] v_k
  const int t = threadIdx.x, blk = blockIdx.x, nblk = gridDim.x;
  const long b = blockIdx.y;
  const int r0 = blk * ZHRD_ROWS, r1 = min(N, r0 + ZHRD_ROWS);
  const bool last = blk == nblk - 1;
  cd* A = F + b * N * N;
  const int par = k & 1, pp = par ^ 1;
  const cd* vp = ws.vd + (b * 2 + pp) * N;
  const cd* yp = ws.yd + (b * 2 + pp) * N;
  const cd zero = cmk(0.0, 0.0), one = cmk(1.0, 0.0);
  zhrd_pending_z(ws, b, N, nblk, k, k, zs, red);
  // column k after step k-1, its reflector
  const cd zk = zs[k], cvk = cconj(vp[k]);
  cd sn = zero;
  for (int i = t; i < N; i += ZHRD_T) {
    const cd c = csub(csub(A[(long)i * N + k], cmul(vp[i], zk)), cmul(yp[i], cvk));
    ck[i] = c;
    if (i > k + 1) sn = cadd(sn, zhrd_sq(c));
  }
  if (t < ZHRD_ROWS && r0 + t < N) { vps[t] = vp[r0 + t]; yps[t] = yp[r0 + t]; }
  sn = het_block_sum(sn, red);                                // (its barriers publish ck)
  const HetRefl r = zhrd_reflect(ck[k + 1], sn, red, [&](double c) {
    double a2 = 0.0;
    for (int i = k + 2 + t; i < N; i += ZHRD_T) { const double xr = c * ck[i].x, xi = c * ck[i].y; a2 += xr * xr + xi * xi; }
    return a2;
  });
  cd* vout = ws.vd + (b * 2 + par) * N;
  cd* cout = ws.colout + (b * 2 + par) * N;
  for (int i = t; i < N; i += ZHRD_T) {
    const cd x = i <= k ? zero : (i == k + 1 ? one : (r.on ? cdiv_re(ck[i], r.div) : zero));
    vk[i] = x;
    if (last) { vout[i] = x; cout[i] = i <= k ? ck[i] : (i == k + 1 ? cmk(r.beta, 0.0) : (r.on ? x : ck[i])); }
  }
  if (last && t == 0) ws.tau[b * (N - 1) + k] = r.tau;
  __syncthreads();
  // rows r0 .. r1 - 1, columns k + 1 .. N - 1: the update of step k-1, the row sums of a_ij v_j and the column sums of conj(v_i) a_ij
  const int wv = t >> 6, lane = t & 63;
  cd* cp = ws.colpart + ((b * 2 + par) * (long)nblk + blk) * N;
  cd rowacc[ZHRD_ROWS / 4];
#pragma unroll
  for (int rr = 0; rr < ZHRD_ROWS / 4; ++rr) rowacc[rr] = zero;
  int chunk = 0;
  for (int j0 = k + 1; j0 < N; j0 += 64, ++chunk) {           // (uniform bounds: the barrier below is reached by all)
    const int j = j0 + lane;
    const bool jin = j < N;
    const cd zj = jin ? zs[j] : zero, cvj = jin ? cconj(vp[j]) : zero, vkj = jin ? vk[j] : zero;
    cd colacc = zero;
#pragma unroll
    for (int rr = 0; rr < ZHRD_ROWS / 4; ++rr) {
      const int i = r0 + wv + 4 * rr;
      if (i < r1 && jin) {
        const cd x = csub(csub(A[(long)i * N + j], cmul(vps[i - r0], zj)), cmul(yps[i - r0], cvj));
        A[(long)i * N + j] = x;
        rowacc[rr] = cadd(rowacc[rr], cmul(x, vkj));
        colacc = cadd(colacc, cmulc(x, vk[i]));
      }
    }
    cd* buf = &cw[chunk & 1][0][0];
    buf[wv * 64 + lane] = colacc;
    __syncthreads();                                          // one per chunk: the buffers alternate
    if (t < 64 && jin) cp[j] = cadd(cadd(cadd(buf[lane], buf[64 + lane]), buf[128 + lane]), buf[192 + lane]);
  }
  cd* yo = ws.yd + (b * 2 + par) * N;
#pragma unroll
  for (int rr = 0; rr < ZHRD_ROWS / 4; ++rr) {
    cd x = rowacc[rr];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { x.x += __shfl_xor(x.x, off); x.y += __shfl_xor(x.y, off); }
    const int i = r0 + wv + 4 * rr;
    if (lane == 0 && i < r1) yo[i] = cmul(r.tau, x);
  }
  // column k-1 takes its place in F: launch k-1 was the last to read it
  if (k > 0) {
    const cd* cprev = ws.colout + (b * 2 + pp) * N;
    for (int i = r0 + t; i < r1; i += ZHRD_T) A[(long)i * N + k - 1] = cprev[i];
  }
}

// after launch N-2: the pending update on column N-1, column N-2 into its place, H unscaled; grid (nblk, members), 16 N bytes of LDS
__global__ __launch_bounds__(ZHRD_T) void zgehrd_finish(cd* __restrict__ F, int N, ZhrdWs ws, const u64* __restrict__ mx) {
  extern __shared__ __attribute__((aligned(16))) char zhrd_smem[];
  __shared__ double red[8];
  cd* zs = reinterpret_cast<cd*>(zhrd_smem);
  const int t = threadIdx.x, blk = blockIdx.x, nblk = gridDim.x, k = N - 1, pp = (k & 1) ^ 1;
  const long b = blockIdx.y;
  const int r0 = blk * ZHRD_ROWS, r1 = min(N, r0 + ZHRD_ROWS);
  cd* A = F + b * N * N;
  zhrd_pending_z(ws, b, N, nblk, k, k, zs, red);
  const cd* vp = ws.vd + (b * 2 + pp) * N;
  const cd* yp = ws.yd + (b * 2 + pp) * N;
  const cd* cprev = ws.colout + (b * 2 + pp) * N;
  const cd zk = zs[k], cvk = cconj(vp[k]);
  const int e1 = syev_exp(mx[b]);
  for (int i = r0 + t; i < r1; i += ZHRD_T) {
    A[(long)i * N + k] = csub(csub(A[(long)i * N + k], cmul(vp[i], zk)), cmul(yp[i], cvk));
    A[(long)i * N + k - 1] = cprev[i];
  }
  __syncthreads();
  for (int idx = t; idx < (r1 - r0) * N; idx += ZHRD_T) {
    const int i = r0 + idx / N, j = idx % N;
    if (j + 1 >= i) { const cd x = A[(long)i * N + j]; A[(long)i * N + j] = cmk(ldexp(x.x, e1), ldexp(x.y, e1)); }
  }
}

// H [members, N, N] = F with zeros below the subdiagonal; grid (tiles of 256, members)
__global__ __launch_bounds__(ZHRD_T) void zhrd_clean(const cd* F, cd* H, int N) {   // (H may be F)
  const long idx = (long)blockIdx.x * ZHRD_T + threadIdx.x, b = blockIdx.y;
  if (idx >= (long)N * N) return;
  const int i = (int)(idx / N), j = (int)(idx - (long)i * N);
  H[b * N * N + idx] = j + 1 >= i ? F[b * N * N + idx] : cmk(0.0, 0.0);
}
// Q [members, N, N] = I
__global__ __launch_bounds__(ZHRD_T) void zhrd_identity(cd* __restrict__ Q, int N) {
  const long idx = (long)blockIdx.x * ZHRD_T + threadIdx.x, b = blockIdx.y;
  if (idx >= (long)N * N) return;
  const int i = (int)(idx / N), j = (int)(idx - (long)i * N);
  Q[b * N * N + idx] = cmk(i == j ? 1.0 : 0.0, 0.0);
}

inline unsigned zhrd_tiles(int64_t n, int per) { return (unsigned)((n + per - 1) / per); }
inline bool zhrd_al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
template <class T> int zhrd_alloc(nd4hip_handle* h, size_t n, T** out) {
  void* p = nullptr;
  ND4_TRY(nd4_ws_alloc(h, sizeof(T) * (n ? n : 1), &p));
  *out = static_cast<T*>(p);
  return 0;
}
int zhrd_attr(const void* fn, size_t lds) {
  if (lds > 64 * 1024) ND4_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  return 0;
}
inline size_t zhrd_small_lds(int64_t N) { return 16 * (size_t)(N * (N | 1) + 7 * N + 256) + 96; }
inline int64_t zhrd_blocks(int64_t N) { return (N + ZHRD_ROWS - 1) / ZHRD_ROWS; }

}  // namespace

// ---- the host-side arithmetic of the tiers (tools/zeig_host_check.hip) ----
// 0: a member in LDS, 1: one launch per column
int nd4_zgehrd_tier(int64_t N) { return zhrd_small_lds(N) <= ZHRD_LDS ? 0 : 1; }
size_t nd4_zgehrd_lds(int64_t N) { return nd4_zgehrd_tier(N) == 0 ? zhrd_small_lds(N) : 48 * (size_t)N; }
// complex elements of tier B's workspace per member: vd, yd, colout and colpart in their two parities
int64_t nd4_zgehrd_ws_elems(int64_t N) { return nd4_zgehrd_tier(N) == 0 ? 0 : 6 * N + 2 * zhrd_blocks(N) * N; }
// members per pass: at most 32768, and `extra` + the reduction's workspace complex elements per member within about 1 GiB
int64_t nd4_zgehrd_chunk(int64_t batch, int64_t N, int64_t extra) { return nd4_zeig_chunk(batch, extra + nd4_zgehrd_ws_elems(N)); }
// the same for a pass without a reduction: `per` complex elements of workspace per member
int64_t nd4_zeig_chunk(int64_t batch, int64_t per) {
  int64_t c = ZHRD_CHUNK;
  if (per > 0 && ZHRD_WS_ELEMS / per < c) c = ZHRD_WS_ELEMS / per;
  if (c < 1) c = 1;
  return batch < c ? batch : c;
}

// the pieces the Schur routes share (zhseqr.hip): all enqueue only. mx [nbm] ZERO on entry; flag: one word, zero on entry
int nd4_zeig_absmax(nd4hip_handle* h, int64_t nbm, int64_t count, const double* A, unsigned long long* mx, int64_t member0, int* flag) {
  hipLaunchKernelGGL(zeig_absmax_k, dim3(256u, (unsigned)nbm), dim3(ZHRD_T), 0, h->stream, reinterpret_cast<const cd*>(A), (long)count, mx, (long)member0,
                     flag);
  ND4_HIP(hipGetLastError());
  return 0;
}
int nd4_zeig_clear(nd4hip_handle* h, void* p, size_t bytes) {
  const int64_t n = (int64_t)(bytes / 8);
  hipLaunchKernelGGL(zeig_clear_k, dim3(zhrd_tiles(n, ZHRD_T)), dim3(ZHRD_T), 0, h->stream, static_cast<double*>(p), (long)n);
  ND4_HIP(hipGetLastError());
  return 0;
}
int nd4_zeig_read_flags(nd4hip_handle* h, const int* flags, int n, int* out) {
  void* hp = nullptr;
  ND4_TRY(nd4_pinned(h, sizeof(int) * (size_t)n, &hp));
  ND4_HIP(hipMemcpyAsync(hp, flags, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost, h->stream));
  ND4_HIP(hipStreamSynchronize(h->stream));
  for (int i = 0; i < n; ++i) out[i] = static_cast<int*>(hp)[i];
  return 0;
}
int nd4_zhess_clean(nd4hip_handle* h, int64_t nbm, int N, const double* F, double* H) {
  hipLaunchKernelGGL(zhrd_clean, dim3(zhrd_tiles((int64_t)N * N, ZHRD_T), (unsigned)nbm), dim3(ZHRD_T), 0, h->stream, reinterpret_cast<const cd*>(F),
                     reinterpret_cast<cd*>(H), N);
  ND4_HIP(hipGetLastError());
  return 0;
}
int nd4_zeig_identity(nd4hip_handle* h, int64_t nbm, int N, double* Q) {
  hipLaunchKernelGGL(zhrd_identity, dim3(zhrd_tiles((int64_t)N * N, ZHRD_T), (unsigned)nbm), dim3(ZHRD_T), 0, h->stream, reinterpret_cast<cd*>(Q), N);
  ND4_HIP(hipGetLastError());
  return 0;
}

// F, tau of nbm <= 32768 members from A; *flag zero on entry. Allocates from the caller's scope; enqueues only
int nd4_zgehrd(nd4hip_handle* h, int64_t nbm, int64_t N64, const double* Am, double* Fm, double* taum, int64_t member0, int* flag) {
  ND4_CHECK_ARG(N64 >= 1 && N64 <= ZHRD_MAXN && nbm >= 1 && nbm <= ZHRD_CHUNK, "nd4hip_zgehrd_batched: extent out of range");
  ND4_CHECK_ARG(zhrd_al16(Am) && zhrd_al16(Fm) && zhrd_al16(taum), "nd4hip_zgehrd_batched: complex operands must be 16-byte aligned");
  const int N = (int)N64;
  const cd* A = reinterpret_cast<const cd*>(Am);
  cd* F = reinterpret_cast<cd*>(Fm);
  cd* tau = reinterpret_cast<cd*>(taum);
  if (nd4_zgehrd_tier(N) == 0) {
    const size_t lds = zhrd_small_lds(N);
    ND4_TRY(zhrd_attr(reinterpret_cast<const void*>(&zgehrd_small), lds));
    hipLaunchKernelGGL(zgehrd_small, dim3((unsigned)nbm), dim3(ZHRD_T), lds, h->stream, A, F, tau, N, (long)member0, flag);
    ND4_HIP(hipGetLastError());
    return 0;
  }
  const int nblk = (int)zhrd_blocks(N);
  const long nn = (long)N * N;
  ZhrdWs ws;
  ws.tau = tau;
  cd* pend = nullptr;
  u64* mx = nullptr;
  const size_t pn = (size_t)nbm * (size_t)nd4_zgehrd_ws_elems(N);
  ND4_TRY(zhrd_alloc(h, pn, &pend)); ND4_TRY(zhrd_alloc(h, (size_t)nbm, &mx));
  ws.vd = pend; ws.yd = ws.vd + (size_t)nbm * 2 * N; ws.colout = ws.yd + (size_t)nbm * 2 * N; ws.colpart = ws.colout + (size_t)nbm * 2 * N;
  ND4_TRY(nd4_zeig_clear(h, mx, sizeof(u64) * (size_t)nbm));
  ND4_TRY(nd4_zeig_clear(h, pend, 16 * pn));
  hipLaunchKernelGGL(zeig_absmax_k, dim3(256u, (unsigned)nbm), dim3(ZHRD_T), 0, h->stream, A, nn, mx, (long)member0, flag);
  hipLaunchKernelGGL(zhrd_load, dim3(zhrd_tiles(nn, ZHRD_T), (unsigned)nbm), dim3(ZHRD_T), 0, h->stream, A, F, nn, mx);
  ND4_HIP(hipGetLastError());
  const size_t lds = 48 * (size_t)N;
  ND4_TRY(zhrd_attr(reinterpret_cast<const void*>(&zgehrd_step), lds));
  const dim3 grid((unsigned)nblk, (unsigned)nbm);
  for (int k = 0; k + 1 < N; ++k) hipLaunchKernelGGL(zgehrd_step, grid, dim3(ZHRD_T), lds, h->stream, F, N, k, ws);
  hipLaunchKernelGGL(zgehrd_finish, grid, dim3(ZHRD_T), 16 * (size_t)N, h->stream, F, N, ws, mx);
  ND4_HIP(hipGetLastError());
  return 0;
}

// zhess_factor: arguments already checked, batch >= 1. Synchronises once per pass (the flag word): NaN or Inf in A is ND4HIP_ERR_NOCONV
// with '<what> contains NaN or Infinity. (matrix <b>)' (what = "<fn>(..): <operand>"), b the lowest such member counted from member0 (also in *first_bad, may be NULL)
int nd4_zgehrd_run(nd4hip_handle* h, int64_t batch, int64_t N, const double* A, double* F, double* tau, const char* what, int64_t member0,
                   int64_t* first_bad) {
  ND4_CHECK_ARG(N >= 1 && N <= ZHRD_MAXN, "nd4hip_zgehrd_batched: 1 <= N <= 2048");
  const int64_t chunk = nd4_zgehrd_chunk(batch, N, 0);
  for (int64_t b0 = 0; b0 < batch; b0 += chunk) {
    const int64_t nbm = batch - b0 < chunk ? batch - b0 : chunk;
    Nd4WsScope scope(h);
    int* flag = nullptr; int bad = 0;
    ND4_TRY(zhrd_alloc(h, 2, &flag));
    ND4_TRY(nd4_zeig_clear(h, flag, 8));
    ND4_TRY(nd4_zgehrd(h, nbm, N, A + 2 * b0 * N * N, F + 2 * b0 * N * N, tau + 2 * b0 * (N - 1), member0 + b0, flag));
    ND4_TRY(nd4_zeig_read_flags(h, flag, 1, &bad));
    if (bad) {
      const long long mb = (long long)INT_MAX - bad;
      if (first_bad) *first_bad = mb;
      nd4_set_error("%s contains NaN or Infinity. (matrix %lld)", what, mb);
      return ND4HIP_ERR_NOCONV;
    }
  }
  return 0;
}

// zhess_apply_q: Z [batch, N, K] <- Q Z (adjoint: Q^H Z) in place through nd4_zunmtr, in passes of at most 32768 members whose compact
// WY workspace stays within about 1 GiB. Enqueues only
int nd4_zunmhr(nd4hip_handle* h, int64_t batch, int64_t N, int64_t K, bool adjoint, const double* F, const double* tau, double* Z) {
  ND4_CHECK_ARG(N >= 1 && N <= ZHRD_MAXN, "nd4hip_zunmhr_batched: 1 <= N <= 2048");
  ND4_CHECK_ARG(zhrd_al16(F) && zhrd_al16(tau) && zhrd_al16(Z), "nd4hip_zunmhr_batched: complex operands must be 16-byte aligned");
  if (N < 2) return 0;                                        // Q = I
  const int64_t chunk = nd4_zeig_chunk(batch, nd4_zunmtr_ws_elems(N, K));
  for (int64_t b0 = 0; b0 < batch; b0 += chunk) {
    const int64_t nbm = batch - b0 < chunk ? batch - b0 : chunk;
    ND4_TRY(nd4_zunmtr(h, nbm, N, K, adjoint, F + 2 * b0 * N * N, tau + 2 * b0 * (N - 1), Z + 2 * b0 * N * K));
  }
  return 0;
}
