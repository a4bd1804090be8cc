// Pivoted symmetric indefinite LDL^T (Bunch-Kaufman partial pivoting, 1x1 and 2x2 pivots) and its solve:
// src/la/pldlp.js:35-188 (_pldlp_decomp, after LAPACK's DSYTF2) and :441-516 (_pldlp_solve).
//
// The factorisation gives the reference's BITS for LD and P on every tier. The reference is right-looking and unblocked: each
// element of the trailing lower triangle receives one subtraction per pivot step, in step order, so any distribution of the
// elements (i, j) of one step over threads gives the same bits as long as every operation is rounded on its own. This unit is
// therefore compiled without FMA contraction (the pragma below and -ffp-contract=off in build.py); division is IEEE.
//
// One step, shared by all tiers (bk_pivot):
//   * argmax of |column k| below the diagonal with the reference's `!(best >= x)`: the first maximum wins, and once a NaN has
//     been met every later element replaces, so with a NaN anywhere the LAST element of the scan is taken;
//   * max(A_rk, A_kk) not > 0 (zero column or NaN, Math.max propagates NaN) raises the matrix's flag and stops it; the last step
//     (k = N-1) is not checked;
//   * A_kk < alpha A_rk, then A_kk < (alpha A_rk) (A_rk / A_sr), then A_rr < alpha A_sr, in this order; a 2x2 step complements
//     P[r] BEFORE rows/columns k+1 and r are interchanged (_pldlp_swap on the lower triangle);
//   * the multipliers of the step go to four vectors and the pivot columns are overwritten at once:
//       1x1: u0[i] = a_ik / d, v0[j] = a_jk (unscaled)          a_ij -= u0[i] * v0[j]
//       2x2: u0[i] = a_ik, u1[i] = a_i,k+1 (old), v0 = s0, v1 = s1      a_ij -= (u0[i] * v0[j] + u1[i] * v1[j])
//     so the trailing update reads the vectors only and writes the trailing triangle only: it can be split over any threads.
//
// Tiers (ND4HIP_PLDLP_TIER_*):
//   LDS     one workgroup per matrix, the lower triangle in LDS with an odd row pitch; N <= 64 in 33 KiB (256 threads, several
//           workgroups per CU) or N <= PLDLP_LDS_MAX_N = 128 in 129 KiB of the CU's 160 KiB (512 threads);
//   GLOBAL  one workgroup of 1024 threads per matrix, working in place on LD in global memory (its own CU's L1 is coherent
//           across the workgroup barriers), the four vectors in LDS; N <= PLDLP_GLOBAL_MAX_N = 2048;
//   GRID    one matrix over the whole chip by plain launches: bk_grid_pivot (one workgroup: searches, decision, swap, the step
//           record and the vectors) and bk_grid_update (a grid of PLDLP_GRID_TILE^2 tiles over the trailing triangle). A 2x2
//           step takes two columns, so the number of steps depends on the data: N rounds are enqueued without any host
//           synchronisation and the record's column counter k turns the rounds after the end into no-ops. No exchange between
//           workgroups inside a kernel, no spinning, no cooperative launch. A batch loops over its members.
#include "nd4hip_internal.h"
#include <cmath>
#pragma clang fp contract(off)

namespace {

constexpr int PLDLP_LDS_SMALL_N = 64;       // LDS tier, small instance: 64 * 65 doubles
constexpr int PLDLP_LDS_MAX_N = 128;        // LDS tier, big instance: 128 * 129 doubles = 129 KiB (+ 4 KiB of vectors) of 160 KiB
constexpr int PLDLP_GLOBAL_MAX_N = 2048;    // GLOBAL tier: 4 vectors of N doubles in 64 KiB of LDS
constexpr int PLDLP_GRID_TILE = 64;         // GRID tier: the update kernel's tile edge (256 threads: 64 columns x 4 rows at a time)

// the record of one GRID step, in device memory (k: the next column, N after the end or after a failure; kind 0: nothing to apply)
struct BkStep { int k, kind, k0, pad; double d, D00, D11, D10, tmp; };

struct BkRed { double v[16]; int i[16]; int nan[16]; double rv; int ri; };

// argmax over f(0) .. f(cnt-1) (cnt >= 1, values >= 0 or NaN) as the reference's sequential scan `if (!(best >= x))` finds it
template <class F>
__device__ __forceinline__ void bk_argmax(F f, int cnt, int tid, int nt, BkRed& red, double& val, int& idx) {
  double bv = -INFINITY; int bi = 0x7fffffff, nan = 0;
  for (int q = tid; q < cnt; q += nt) { const double x = f(q); if (x != x) nan = 1; else if (x > bv) { bv = x; bi = q; } }
  for (int o = 32; o > 0; o >>= 1) {
    const double ov = __shfl_xor(bv, o); const int oi = __shfl_xor(bi, o); nan |= __shfl_xor(nan, o);
    if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
  }
  if ((tid & 63) == 0) { red.v[tid >> 6] = bv; red.i[tid >> 6] = bi; red.nan[tid >> 6] = nan; }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < (nt >> 6); w++) {
      const double ov = red.v[w]; const int oi = red.i[w]; nan |= red.nan[w];
      if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
    }
    if (nan) { bi = cnt - 1; bv = f(cnt - 1); }      // after a NaN every element replaces: the last one stays
    red.rv = bv; red.ri = bi;
  }
  __syncthreads();
  val = red.rv; idx = red.ri;
  __syncthreads();
}

// _pldlp_swap(k, l), k < l, on the lower triangle (pldlp.js:88-118); every pair of elements is touched by one thread
__device__ __forceinline__ void bk_swap(double* a, long ld, int M, int k, int l, int tid, int nt) {
  for (int i = tid; i < M; i += nt) {
    double *x, *y;
    if (i < k)       { x = a + k * ld + i; y = a + l * ld + i; }
    else if (i == k) { x = a + k * ld + k; y = a + l * ld + l; }
    else if (i < l)  { x = a + i * ld + k; y = a + l * ld + i; }
    else if (i == l) continue;
    else             { x = a + i * ld + k; y = a + i * ld + l; }
    const double t = *x; *x = *y; *y = t;
  }
}

// One pivot step at column k of the M x M matrix a (row pitch ld): search, decision, interchange, multipliers. Returns 0 for a
// zero column or NaN, else the pivot size 1 or 2; *k0 is the first row/column of the trailing matrix. Every thread of the
// workgroup calls it and gets the same answer. rec (may be NULL) receives the scalars of the step.
__device__ __forceinline__ int bk_pivot(double* a, long ld, int M, int k, int* P, double alpha, double* u0, double* u1, double* v0,
                                        double* v1, BkRed& red, BkStep* rec, int* k0, int tid, int nt) {
  int kind = 1, kp = k;       // kp: the 1x1 pivot column, or the second column of the 2x2 block
  if (k < M - 1) {
    double A_rk; int q;
    bk_argmax([&](int x) { return fabs(a[(long)(k + 1 + x) * ld + k]); }, M - 1 - k, tid, nt, red, A_rk, q);
    const int r = k + 1 + q;
    const double A_kk = fabs(a[(long)k * ld + k]);
    if (A_rk != A_rk || A_kk != A_kk || !(A_rk > 0.0 || A_kk > 0.0)) return 0;
    const double aA = alpha * A_rk;
    if (A_kk < aA) {
      double A_sr;
      bk_argmax([&](int x) { return x < r - k ? fabs(a[(long)r * ld + k + x]) : fabs(a[(long)(r + 1 + x - (r - k)) * ld + r]); },
                (r - k) + (M - 1 - r), tid, nt, red, A_sr, q);
      if (A_kk < aA * (A_rk / A_sr)) {
        const double A_rr = fabs(a[(long)r * ld + r]);
        if (A_rr < alpha * A_sr) { kind = 2; kp = k + 1; }
        __syncthreads();            // every thread has read a[r, r] before the interchange moves it
        if (tid == 0) {
          if (kind == 2) P[r] ^= -1;
          if (kp != r) { const int t = P[kp]; P[kp] = P[r]; P[r] = t; }
        }
        if (kp != r) bk_swap(a, ld, M, kp, r, tid, nt);
        __syncthreads();
      }
    }
  }
  if (kind == 1) {
    const double d = a[(long)kp * ld + kp];
    for (int i = kp + 1 + tid; i < M; i += nt) {
      const double c = a[(long)i * ld + kp], t = c / d;
      v0[i] = c; u0[i] = t; a[(long)i * ld + kp] = t;
    }
    if (rec && tid == 0) rec->d = d;
  } else {
    const int kf = kp - 1;
    const double tmp = a[(long)kp * ld + kf], D00 = a[(long)kp * ld + kp] / tmp, D11 = a[(long)kf * ld + kf] / tmp,
                 D10 = (1.0 / (D00 * D11 - 1.0)) / tmp;
    for (int j = kp + 1 + tid; j < M; j += nt) {
      const double c0 = a[(long)j * ld + kf], c1 = a[(long)j * ld + kp];
      const double s0 = D10 * (D00 * c0 - c1), s1 = D10 * (D11 * c1 - c0);
      u0[j] = c0; u1[j] = c1; v0[j] = s0; v1[j] = s1;
      a[(long)j * ld + kf] = s0; a[(long)j * ld + kp] = s1;
    }
    if (rec && tid == 0) { rec->D00 = D00; rec->D11 = D11; rec->D10 = D10; rec->tmp = tmp; }
  }
  *k0 = kp + 1;
  __syncthreads();
  return kind;
}

// the trailing update of one step by one workgroup: a wave per row, lanes along the row
__device__ __forceinline__ void bk_update_wg(double* a, long ld, int M, int k0, int kind, const double* u0, const double* u1,
                                             const double* v0, const double* v1, int tid, int nt) {
  const int lane = tid & 63, nw = nt >> 6;
  for (int i = k0 + (tid >> 6); i < M; i += nw) {
    double* row = a + (long)i * ld;
    if (kind == 1) {
      const double t = u0[i];
      for (int j = k0 + lane; j <= i; j += 64) row[j] = row[j] - t * v0[j];
    } else {
      const double c0 = u0[i], c1 = u1[i];
      for (int j = k0 + lane; j <= i; j += 64) row[j] = row[j] - (c0 * v0[j] + c1 * v1[j]);
    }
  }
  __syncthreads();
}

// LDS (LDSD > 0: doubles of the matrix image) and GLOBAL (LDSD = 0) tiers: one workgroup per matrix. S may be LD.
template <int LDSD, int VN, int NT>
__global__ __launch_bounds__(NT) void bk_factor_wg(int N, const double* S, double* LD, int* P, int* flags, double alpha) {
  __shared__ double sh[LDSD > 0 ? LDSD : 1];
  __shared__ double vec[4][VN];
  __shared__ BkRed red;
  const int tid = threadIdx.x;
  const double* s = S + (long)blockIdx.x * N * N;
  double* out = LD + (long)blockIdx.x * N * N;
  int* p = P + (long)blockIdx.x * N;
  double* a; long ld;
  if constexpr (LDSD > 0) {
    a = sh; ld = N | 1;
    for (int e = tid; e < N * N; e += NT) { const int i = e / N, j = e - i * N; if (j <= i) sh[i * ld + j] = s[e]; }
  } else {
    a = out; ld = N;
    for (int e = tid; e < N * N; e += NT) { const int i = e / N, j = e - i * N; out[e] = j <= i ? s[e] : 0.0; }
  }
  for (int i = tid; i < N; i += NT) p[i] = i;
  __syncthreads();
  for (int k = 0; k < N;) {
    int k0;
    const int kind = bk_pivot(a, ld, N, k, p, alpha, vec[0], vec[1], vec[2], vec[3], red, nullptr, &k0, tid, NT);
    if (kind == 0) { if (tid == 0) flags[blockIdx.x] = 1; break; }
    bk_update_wg(a, ld, N, k0, kind, vec[0], vec[1], vec[2], vec[3], tid, NT);
    k = k0;
  }
  if constexpr (LDSD > 0) {
    __syncthreads();
    for (int e = tid; e < N * N; e += NT) { const int i = e / N, j = e - i * N; out[e] = j <= i ? sh[i * ld + j] : 0.0; }
  }
}

// ---- GRID tier
__global__ __launch_bounds__(256) void bk_grid_prepare(int N, const double* S, double* LD, int* P, BkStep* rec) {
  const long g = (long)blockIdx.x * 256 + threadIdx.x, step = (long)gridDim.x * 256;
  for (long e = g; e < (long)N * N; e += step) { const long i = e / N, j = e - i * N; LD[e] = j <= i ? S[e] : 0.0; }
  for (long i = g; i < N; i += step) P[i] = (int)i;
  if (g == 0) { rec->k = 0; rec->kind = 0; rec->k0 = 0; }
}

__global__ __launch_bounds__(1024) void bk_grid_pivot(int N, double* LD, int* P, int* flag, BkStep* rec, double* vecs, double alpha) {
  __shared__ BkRed red;
  const int tid = threadIdx.x;
  const int k = rec->k;
  __syncthreads();
  if (k >= N) { if (tid == 0) rec->kind = 0; return; }
  int k0;
  const int kind = bk_pivot(LD, N, N, k, P, alpha, vecs, vecs + N, vecs + 2 * (long)N, vecs + 3 * (long)N, red, rec, &k0, tid, 1024);
  if (tid == 0) {
    if (kind == 0) { *flag = 1; rec->k = N; rec->kind = 0; }
    else { rec->k = k0; rec->kind = kind; rec->k0 = k0; }
  }
}

// tiles (t0 + blockIdx.y, t0 + blockIdx.x) of the PLDLP_GRID_TILE grid anchored at (0, 0); the host sizes the launch for the
// largest trailing matrix the round can have, the record says where it really starts
__global__ __launch_bounds__(256) void bk_grid_update(int N, double* LD, const BkStep* rec, const double* vecs, int t0) {
  const int kind = rec->kind;
  if (kind == 0) return;
  const int k0 = rec->k0;
  const int tj = t0 + blockIdx.x, ti = t0 + blockIdx.y;
  if (tj > ti || (ti + 1) * PLDLP_GRID_TILE <= k0) return;
  const int j = tj * PLDLP_GRID_TILE + (threadIdx.x & 63);
  if (j < k0 || j >= N) return;
  const double *u0 = vecs, *u1 = vecs + N, *v0 = vecs + 2 * (long)N, *v1 = vecs + 3 * (long)N;
  const double v0j = v0[j], v1j = kind == 2 ? v1[j] : 0.0;
  for (int r = threadIdx.x >> 6; r < PLDLP_GRID_TILE; r += 4) {
    const int i = ti * PLDLP_GRID_TILE + r;
    if (i >= N) break;
    if (i < j) continue;
    double* p = LD + (long)i * N + j;
    if (kind == 1) *p = *p - u0[i] * v0j;
    else           *p = *p - (u0[i] * v0j + u1[i] * v1j);
  }
}

// ---- solve: X = P L^-T D^-1 L^-1 P^T Y (pldlp.js:441-516)
// the row of Y that P[i] names, with the complement undone; -1 if P[i] cannot be used (out of range, or a second row at i = 0)
__device__ __forceinline__ int bk_row(const int* P, int i, int N) {
  const int p = P[i], I = p < 0 ? ~p : p;
  return (I >= 0 && I < N && !(p < 0 && i == 0)) ? I : -1;
}

// scatter = false: W[b, i, :] = Y[b, I(i), :]; scatter = true: X[b, I(i), :] = W[b, i, :]
template <bool SCATTER>
__global__ __launch_bounds__(256) void bk_permute_rows(int N, int J, const int* __restrict__ Pm, long sP, const double* src, long sSrc,
                                                       double* dst, int* flag) {
  const int col = blockIdx.x * 256 + threadIdx.x;
  if (col >= J) return;
  const int* P = Pm + blockIdx.z * sP;
  const double* s = src + blockIdx.z * sSrc;
  double* d = dst + (long)blockIdx.z * N * J;
  for (int i = blockIdx.y; i < N; i += gridDim.y) {
    const int I = bk_row(P, i, N);
    if (I < 0) { *flag = 1; if (!SCATTER) d[(long)i * J + col] = 0.0; continue; }
    if (SCATTER) d[(long)I * J + col] = s[(long)i * J + col];
    else         d[(long)i * J + col] = s[(long)I * J + col];
  }
}

// the unit lower triangle of LD with the entry INSIDE each 2x2 block, LD[i, i-1] where P[i] < 0, taken as zero
__global__ __launch_bounds__(256) void bk_extract_l(int N, const double* __restrict__ LDm, long sLD, const int* __restrict__ Pm, long sP,
                                                    double* __restrict__ Lm) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= N) return;
  const double* LD = LDm + blockIdx.z * sLD; const int* P = Pm + blockIdx.z * sP;
  double* L = Lm + (long)blockIdx.z * N * N;
  for (int i = blockIdx.y; i < N; i += gridDim.y) {
    const bool inner = i > 0 && j == i - 1 && P[i] < 0;
    L[(long)i * N + j] = j < i ? (inner ? 0.0 : LD[(long)i * N + j]) : (j == i ? 1.0 : 0.0);
  }
}

// W <- D^-1 W with the reference's 2x2 inverse (pldlp.js:479-502)
__global__ __launch_bounds__(256) void bk_scale_blocks(int N, int J, const double* __restrict__ LDm, long sLD, const int* __restrict__ Pm,
                                                       long sP, double* Wm) {
  const int col = blockIdx.x * 256 + threadIdx.x;
  if (col >= J) return;
  const double* LD = LDm + blockIdx.z * sLD; const int* P = Pm + blockIdx.z * sP;
  double* W = Wm + (long)blockIdx.z * N * J;
  for (int i = blockIdx.y; i < N; i += gridDim.y) {
    if (i > 0 && P[i] < 0) continue;                       // second row of a block: done by the first
    if (i < N - 1 && P[i + 1] < 0) {
      const double s = LD[(long)(i + 1) * N + i], D00 = LD[(long)(i + 1) * N + i + 1] / s, D11 = LD[(long)i * N + i] / s,
                   D10 = (1.0 / (D00 * D11 - 1.0)) / s;
      const double y0 = W[(long)i * J + col], y1 = W[(long)(i + 1) * J + col];
      W[(long)i * J + col] = D10 * (D00 * y0 - y1);
      W[(long)(i + 1) * J + col] = D10 * (D11 * y1 - y0);
    } else {
      W[(long)i * J + col] /= LD[(long)i * N + i];
    }
  }
}

}  // namespace

void nd4_sytrf_bk_limits(int* lds_max_n, int* global_max_n, int* grid_tile) {
  if (lds_max_n) *lds_max_n = PLDLP_LDS_MAX_N;
  if (global_max_n) *global_max_n = PLDLP_GLOBAL_MAX_N;
  if (grid_tile) *grid_tile = PLDLP_GRID_TILE;
}

// the tier (ND4HIP_PLDLP_TIER_LDS / _GLOBAL / _GRID) a batch of N x N matrices takes under `tier`; 0 if that tier cannot hold N
int nd4_sytrf_bk_tier(const nd4hip_handle* h, int64_t batch, int64_t N, int tier) {
  if (tier == ND4HIP_PLDLP_TIER_AUTO)
    return N <= PLDLP_LDS_MAX_N ? ND4HIP_PLDLP_TIER_LDS
         : (batch >= h->num_cu && N <= PLDLP_GLOBAL_MAX_N) ? ND4HIP_PLDLP_TIER_GLOBAL : ND4HIP_PLDLP_TIER_GRID;
  if (tier == ND4HIP_PLDLP_TIER_LDS) return N <= PLDLP_LDS_MAX_N ? tier : 0;
  if (tier == ND4HIP_PLDLP_TIER_GLOBAL) return N <= PLDLP_GLOBAL_MAX_N ? tier : 0;
  return tier == ND4HIP_PLDLP_TIER_GRID ? tier : 0;
}

// S [batch, N, N] (lower triangle read) -> LD [batch, N, N], P [batch, N]; flags [batch] zero on entry, 1 where a zero column or
// NaN stopped the matrix. tier: a value nd4_sytrf_bk_tier returned. S may be LD.
int nd4_sytrf_bk(nd4hip_handle* h, int64_t batch, int64_t N64, const double* S, double* LD, int32_t* P, int* flags, int tier) {
  if (batch == 0 || N64 == 0) return 0;
  ND4_CHECK_ARG(batch < (1ll << 31) && N64 <= 46340, "nd4hip_dsytrf_bk_batched: extent out of range");
  const int N = (int)N64;
  const double alpha = (std::sqrt(17.0) + 1.0) / 8.0;
  const dim3 grid((unsigned)batch);
  if (tier == ND4HIP_PLDLP_TIER_LDS) {
    ND4_CHECK_ARG(N <= PLDLP_LDS_MAX_N, "nd4hip_dsytrf_bk_batched: the LDS tier holds N <= %d", PLDLP_LDS_MAX_N);
    if (N <= PLDLP_LDS_SMALL_N)
      hipLaunchKernelGGL((bk_factor_wg<PLDLP_LDS_SMALL_N * (PLDLP_LDS_SMALL_N + 1), PLDLP_LDS_SMALL_N, 256>), grid, dim3(256), 0, h->stream,
                         N, S, LD, P, flags, alpha);
    else
      hipLaunchKernelGGL((bk_factor_wg<PLDLP_LDS_MAX_N * (PLDLP_LDS_MAX_N + 1), PLDLP_LDS_MAX_N, 512>), grid, dim3(512), 0, h->stream,
                         N, S, LD, P, flags, alpha);
  } else if (tier == ND4HIP_PLDLP_TIER_GLOBAL) {
    ND4_CHECK_ARG(N <= PLDLP_GLOBAL_MAX_N, "nd4hip_dsytrf_bk_batched: the GLOBAL tier holds N <= %d", PLDLP_GLOBAL_MAX_N);
    hipLaunchKernelGGL((bk_factor_wg<0, PLDLP_GLOBAL_MAX_N, 1024>), grid, dim3(1024), 0, h->stream, N, S, LD, P, flags, alpha);
  } else {
    ND4_CHECK_ARG(tier == ND4HIP_PLDLP_TIER_GRID, "nd4hip_dsytrf_bk_batched: unknown tier %d", tier);
    Nd4WsScope scope(h);
    void* p = nullptr;
    ND4_TRY(nd4_ws_alloc(h, 256 + sizeof(double) * 4 * (size_t)N, &p));
    BkStep* rec = static_cast<BkStep*>(p);
    double* vecs = reinterpret_cast<double*>(static_cast<char*>(p) + 256);
    const int T = (N + PLDLP_GRID_TILE - 1) / PLDLP_GRID_TILE;
    const long cells = ((long)N * N + 255) / 256;
    for (int64_t b = 0; b < batch; b++) {
      double* ld = LD + b * N * N; int32_t* pb = P + b * N;
      hipLaunchKernelGGL(bk_grid_prepare, dim3((unsigned)(cells < 4096 ? cells : 4096)), dim3(256), 0, h->stream, N, S + b * N * N, ld, pb, rec);
      for (int n = 0; n < N; n++) {
        hipLaunchKernelGGL(bk_grid_pivot, dim3(1), dim3(1024), 0, h->stream, N, ld, pb, flags + b, rec, vecs, alpha);
        if (n + 1 < N) {      // after round n the trailing matrix starts at row n + 1 or later
          const int t0 = (n + 1) / PLDLP_GRID_TILE;
          hipLaunchKernelGGL(bk_grid_update, dim3((unsigned)(T - t0), (unsigned)(T - t0)), dim3(256), 0, h->stream, N, ld, rec, vecs, t0);
        }
      }
      ND4_HIP(hipGetLastError());
    }
  }
  ND4_HIP(hipGetLastError());
  return 0;
}

// X [batch, N, J] = P L^-T D^-1 L^-1 P^T Y; strides in elements, 0 = broadcast; batch < 65536. *flag (device, zero on entry) is
// raised if an entry of P cannot be used; such rows are skipped, nothing is read or written out of bounds. X may be Y.
int nd4_sytrs_bk(nd4hip_handle* h, int64_t batch, int64_t N64, int64_t J64, const double* LD, int64_t sLD, const int32_t* P, int64_t sP,
                 const double* Y, int64_t sY, double* X, int* flag) {
  if (batch == 0 || N64 == 0 || J64 == 0) return 0;
  ND4_CHECK_ARG(batch < 65536 && N64 < (1ll << 30) && J64 < (1ll << 30), "nd4hip_dsytrs_bk_batched: extent out of range");
  const int N = (int)N64, J = (int)J64;
  const int64_t nL = (sLD == 0 && sP == 0) ? 1 : batch;
  Nd4WsScope scope(h);
  void *pl = nullptr, *pw = nullptr;
  ND4_TRY(nd4_ws_alloc(h, sizeof(double) * (size_t)nL * (size_t)N * (size_t)N, &pl));
  ND4_TRY(nd4_ws_alloc(h, sizeof(double) * (size_t)batch * (size_t)N * (size_t)J, &pw));
  double *L = static_cast<double*>(pl), *W = static_cast<double*>(pw);
  const int64_t sL = nL == 1 ? 0 : (int64_t)N * N;
  const unsigned gy = (unsigned)(N < 1024 ? N : 1024);
  const dim3 gJ((unsigned)((J + 255) / 256), gy, (unsigned)batch), gN((unsigned)((N + 255) / 256), gy, (unsigned)nL);
  hipLaunchKernelGGL(bk_permute_rows<false>, gJ, dim3(256), 0, h->stream, N, J, P, (long)sP, Y, (long)sY, W, flag);
  hipLaunchKernelGGL(bk_extract_l, gN, dim3(256), 0, h->stream, N, LD, (long)sLD, P, (long)sP, L);
  ND4_HIP(hipGetLastError());
  ND4_TRY(nd4_trsm_ld(h, false, true, batch, N, J, L, N, sL, W, (int64_t)N * J));
  hipLaunchKernelGGL(bk_scale_blocks, gJ, dim3(256), 0, h->stream, N, J, LD, (long)sLD, P, (long)sP, W);
  ND4_HIP(hipGetLastError());
  ND4_TRY(nd4_trsm_t_ex(h, true, batch, N, J, L, N, sL, W, (int64_t)N * J));
  hipLaunchKernelGGL(bk_permute_rows<true>, gJ, dim3(256), 0, h->stream, N, J, P, (long)sP, W, (long)N * J, X, flag);
  ND4_HIP(hipGetLastError());
  return 0;
}
