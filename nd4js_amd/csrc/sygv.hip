// Generalised symmetric-definite eigenproblem A x = lambda B x on the device: eigen_sym_gen / eigenvals_sym_gen.
// A symmetric, B symmetric positive definite, both read from their lower triangles only. The route is LAPACK's dsygvd:
//   1. L = chol(B)                     2. C = L^-1 A L^-T (lower triangle)
//   3. (lambda, Y) of C by the existing solvers, unchanged: nd4_syevd (syev.hip) or nd4_syevj (syevj.hip)
//   4. X = L^-T Y                      so that A X = B X diag(lambda) and X^T B X = I.
//
// Small tier, N <= 64: two kernels, one workgroup of one wave per member, the member index in blockIdx.x, no workgroup waits on
// another and every loop has a bound fixed by N.
//   sygv_reduce_small  the lower triangles of A (mirrored) and B go to LDS (leading dimension N | 1 doubles: a column walk and a row
//                      walk are both conflict-free for ds_read_b64, whose bank is (a / 4) mod 64). B is factorised in place, lane i
//                      owning row i, left-looking, four columns at a time (one barrier per four columns). Then lane c owns column c of
//                      W = L^-1 A (forward substitution in place), and after one barrier ROW c of W, which is column c of W^T: it
//                      is replaced in place by column c of C = L^-1 W^T, so the tile ends up holding C^T and no third tile is needed.
//                      L and the lower triangle of C (exact zeros above it) go to the workspace; a radicand that is not a finite
//                      number > 0 raises bit 1 of the member's flag, a non-finite entry of C's lower triangle bit 2.
//   sygv_back_small    X = L^-T Y in place on X, L and Y in LDS, lane c owning column c (backward substitution); Y may have fewer
//                      than N columns (k of them, in rows ldx apart): the selected eigenvectors of nd4_sygvx.
// A broadcast B (strideB = 0) is factorised once per call by a pass of its own (sygv_chol_small, the same device function); the
// members then read L from the workspace.
// The order of every operation is that of the numpy model in tests/sygv_common.py, and the file is built without FMA contraction:
// every sum starts from the matrix entry and subtracts its products in ascending index order, each operation rounded on its own,
//   L_ij = (b_ij - sum_{k<j} L_ik L_jk) / L_jj,  L_jj = sqrt(b_jj - sum_{k<j} L_jk L_jk)
//   W_ic = (a_ic - sum_{k<i} L_ik W_kc) / L_ii,  C_ic = (W_ci - sum_{k<i} L_ik C_kc) / L_ii   (C's lower triangle is kept)
//   X_ic = (Y_ic - sum_{k>i} L_ki X_kc) / L_ii
// so the device returns the model's bits. 2 * 64 * 65 doubles are 66 560 bytes: dynamic LDS, sized by N (1 152 bytes at N = 8).
//
// Large tier, 64 < N <= 2048: nd4_potrf, a mirror of A's lower triangle, nd4_trsm, nd4_transpose, nd4_trsm, and nd4_trsm_t for
// step 4 (on k columns where nd4_sygvx selected k eigenvectors); new are only sygv_diag_check (diag(L) finite and > 0 per member: it sees the exact zero in the LAST pivot, which makes no
// NaN and which nd4_potrf's flag does not see) and sygv_finish_c (zeros above C's diagonal, bit 2 for a non-finite entry below).
// Two 2048^2 triangular solves with 2048 right-hand sides cost about 1 ms against 27 ms for the solver: no symmetry-aware reduction.
#include "nd4hip_internal.h"
#include <cfloat>
#include <cmath>

namespace {

constexpr int SYGV_SMALL_N = 64;
constexpr int64_t SYGV_CHUNK = 32768;          // members per pass (the launchers called take batch < 65536)
constexpr int64_t SYGV_WS_DOUBLES = 1ll << 27;  // large tier: a pass's L, W and C take at most 1 GiB each
constexpr int SYGV_BAD_B = 1, SYGV_BAD_C = 2;  // flag bits

__host__ __device__ inline int sygv_ld(int N) { return N | 1; }
// members per pass: the small tier's workspace is tiny; the large tier's is N^2 doubles per member, three times, and the
// solver's own on top, so its passes are sized by memory (32 members at 2048^2, 512 at 512^2)
inline int64_t sygv_chunk(int64_t batch, int64_t N) {
  int64_t c = SYGV_CHUNK;
  if (N > SYGV_SMALL_N && SYGV_WS_DOUBLES / (N * N) < c) c = SYGV_WS_DOUBLES / (N * N);
  if (c < 1) c = 1;
  return batch < c ? batch : c;
}
inline size_t sygv_lds_bytes(int N) { return sizeof(double) * 2 * (size_t)N * sygv_ld(N); }

// the lower triangle of src [N, N] into the LDS tile; `mirror`: also into the upper triangle, else zeros there
__device__ __forceinline__ void sygv_load_lower(const double* __restrict__ src, double* tile, int N, int ld, bool mirror) {
  for (int e = threadIdx.x; e < N * N; e += 64) {
    const int i = e / N, j = e - i * N;
    if (j <= i) {
      const double v = src[e];
      tile[i * ld + j] = v;
      if (mirror) tile[j * ld + i] = v;
    } else if (!mirror) tile[i * ld + j] = 0.0;
  }
}

// Ls: the lower triangle of B -> L in place. Lane i owns row i. Returns (the same in every lane) whether a radicand was bad.
// The sums are latency chains (each subtraction waits for the one before), so SYGV_R of them run side by side: SYGV_R columns here,
// SYGV_R rows in sygv_forward. The terms k < j0 of a block are common work; the terms inside the block follow in ascending k, from
// registers (the other lane's through __shfl): every entry still sees its own terms in ascending order. One barrier per block.
// Indices beyond N - 1 are clamped: those chains compute something that is never stored.
constexpr int SYGV_R = 4;

__device__ bool sygv_chol_lds(double* Ls, int N, int ld) {
  const int t = threadIdx.x;
  const bool active = t < N;
  const int row = active ? t : N - 1;
  bool bad = false;
  for (int j0 = 0; j0 < N; j0 += SYGV_R) {
    double v[SYGV_R], x[SYGV_R];
    int col[SYGV_R];
#pragma unroll
    for (int r = 0; r < SYGV_R; ++r) { col[r] = j0 + r < N ? j0 + r : N - 1; v[r] = Ls[row * ld + col[r]]; x[r] = 0.0; }
    for (int k = 0; k < j0; ++k) {
      const double a = Ls[row * ld + k];
#pragma unroll
      for (int r = 0; r < SYGV_R; ++r) v[r] = v[r] - a * Ls[col[r] * ld + k];
    }
#pragma unroll
    for (int r = 0; r < SYGV_R; ++r) {
      if (j0 + r < N) {                         // (uniform)
#pragma unroll
        for (int q = 0; q < r; ++q) v[r] = v[r] - x[q] * __shfl(x[q], j0 + r);   // L[t][j0+q] L[j0+r][j0+q]
        const double s = __shfl(v[r], j0 + r);  // the radicand: lane j0+r's sum
        if (!(s > 0.0 && s <= DBL_MAX)) bad = true;
        const double d = sqrt(s);
        x[r] = t == j0 + r ? d : v[r] / d;
        if (active && t >= j0 + r) Ls[t * ld + j0 + r] = x[r];
      }
    }
    __syncthreads();
  }
  return bad;
}

// forward substitution with L for one right-hand side in LDS, in place: unknown i lives at x[i * sx];
// x_i = (x_i - sum_{k<i} L_ik x_k) / L_ii
__device__ __forceinline__ void sygv_forward(const double* Ls, double* x, int sx, int N, int ld) {
  for (int i0 = 0; i0 < N; i0 += SYGV_R) {
    double v[SYGV_R];
    int row[SYGV_R];
#pragma unroll
    for (int r = 0; r < SYGV_R; ++r) { row[r] = i0 + r < N ? i0 + r : N - 1; v[r] = x[row[r] * sx]; }
    for (int k = 0; k < i0; ++k) {
      const double w = x[k * sx];
#pragma unroll
      for (int r = 0; r < SYGV_R; ++r) v[r] = v[r] - Ls[row[r] * ld + k] * w;
    }
#pragma unroll
    for (int r = 0; r < SYGV_R; ++r) {
      if (i0 + r < N) {
#pragma unroll
        for (int q = 0; q < r; ++q) v[r] = v[r] - Ls[row[r] * ld + i0 + q] * v[q];
        v[r] = v[r] / Ls[row[r] * ld + row[r]];
        x[row[r] * sx] = v[r];
      }
    }
  }
}

__global__ __launch_bounds__(64) void sygv_chol_small(const double* __restrict__ B, double* __restrict__ L, int* __restrict__ flags, int N) {
  extern __shared__ __align__(16) double sygv_smem[];
  const int ld = sygv_ld(N);
  double* Ls = sygv_smem;
  sygv_load_lower(B, Ls, N, ld, false);
  __syncthreads();
  const bool bad = sygv_chol_lds(Ls, N, ld);
  for (int e = threadIdx.x; e < N * N; e += 64) { const int i = e / N, j = e - i * N; L[e] = Ls[i * ld + j]; }
  if (threadIdx.x == 0 && bad) { flags[0] = SYGV_BAD_B; flags[1] = SYGV_BAD_B; }
}

// flags: [0] the OR over the members, [1 + member] per member (zero on entry); NULL: no verdict wanted (dsygst).
// have_L: T holds L (stride sT, 0 = one for all), else B. Lout may be NULL.
__global__ __launch_bounds__(64) void sygv_reduce_small(const double* __restrict__ A, const double* __restrict__ T, long sT, int have_L,
                                                        double* __restrict__ Lout, double* __restrict__ C, int* __restrict__ flags, int N) {
  extern __shared__ __align__(16) double sygv_smem[];
  const int ld = sygv_ld(N), t = threadIdx.x;
  const long mat = blockIdx.x;
  double* As = sygv_smem;
  double* Ls = sygv_smem + N * ld;
  sygv_load_lower(A + mat * N * N, As, N, ld, true);
  sygv_load_lower(T + mat * sT, Ls, N, ld, false);
  __syncthreads();
  bool bad = false;
  if (!have_L) bad = sygv_chol_lds(Ls, N, ld);
  if (Lout)
    for (int e = t; e < N * N; e += 64) { const int i = e / N, j = e - i * N; Lout[mat * N * N + e] = Ls[i * ld + j]; }
  if (t < N) sygv_forward(Ls, As + t, ld, N, ld);         // column t of W = L^-1 A
  __syncthreads();
  if (t < N) sygv_forward(Ls, As + t * ld, 1, N, ld);     // row t of W becomes column t of C = L^-1 W^T: the tile holds C^T
  __syncthreads();
  int nonfinite = 0;
  for (int e = t; e < N * N; e += 64) {
    const int i = e / N, j = e - i * N;
    const double v = j <= i ? As[j * ld + i] : 0.0;
    if (!(fabs(v) <= DBL_MAX)) nonfinite = 1;
    C[mat * N * N + e] = v;
  }
  if (flags) {
    const int f = (bad ? SYGV_BAD_B : 0) | (__any(nonfinite) ? SYGV_BAD_C : 0);
    if (t == 0 && f) { flags[1 + mat] = f; atomicOr(&flags[0], f); }
  }
}

// X <- L^-T X per member, on the first k <= N columns of X [N, ldx]; L stride sL (0 = one for all). Lane c < k owns column c: the
// order of a column's operations does not depend on k
__global__ __launch_bounds__(64) void sygv_back_small(const double* __restrict__ L, long sL, double* __restrict__ X, int N, int k, long ldx) {
  extern __shared__ __align__(16) double sygv_smem[];
  const int ld = sygv_ld(N), t = threadIdx.x;
  const long mat = blockIdx.x;
  double* Ls = sygv_smem;
  double* Xs = sygv_smem + N * ld;
  X += mat * N * ldx;
  sygv_load_lower(L + mat * sL, Ls, N, ld, false);
  for (int e = t; e < N * k; e += 64) { const int i = e / k, j = e - i * k; Xs[i * ld + j] = X[i * ldx + j]; }
  __syncthreads();
  if (t < k) {
    for (int i = N - 1; i >= 0; --i) {
      double v = Xs[i * ld + t];
      for (int r = i + 1; r < N; ++r) v = v - Ls[r * ld + i] * Xs[r * ld + t];
      Xs[i * ld + t] = v / Ls[i * ld + i];
    }
  }
  __syncthreads();
  for (int e = t; e < N * k; e += 64) { const int i = e / k, j = e - i * k; X[i * ldx + j] = Xs[i * ld + j]; }
}

// ---- large tier: the three elementwise kernels beside the existing launchers. grid (tiles of 256 entries, members) ----
__global__ __launch_bounds__(256) void sygv_mirror_lower(const double* __restrict__ A, double* __restrict__ W, int N) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= (long)N * N) return;
  const long off = (long)blockIdx.y * N * N;
  const int i = (int)(e / N), j = (int)(e - (long)i * N);
  W[off + e] = j <= i ? A[off + e] : A[off + (long)j * N + i];
}

// flags as in sygv_reduce_small; grid (members), L stride sL
__global__ __launch_bounds__(256) void sygv_diag_check(const double* __restrict__ L, long sL, int* __restrict__ flags, int N) {
  const long mat = blockIdx.x;
  int bad = 0;
  for (int i = threadIdx.x; i < N; i += 256) {
    const double d = L[mat * sL + (long)i * N + i];
    if (!(d > 0.0 && d <= DBL_MAX)) bad = 1;
  }
  if (bad) { atomicOr(&flags[1 + mat], SYGV_BAD_B); atomicOr(&flags[0], SYGV_BAD_B); }
}

// the flags nd4_potrf raised (NaN pivot) join the verdict
__global__ __launch_bounds__(256) void sygv_merge_flags(const int* __restrict__ potrf_flags, int* __restrict__ flags, long batch) {
  const long b = (long)blockIdx.x * 256 + threadIdx.x;
  if (b < batch && potrf_flags[b]) { atomicOr(&flags[1 + b], SYGV_BAD_B); atomicOr(&flags[0], SYGV_BAD_B); }
}

__global__ __launch_bounds__(256) void sygv_finish_c(double* __restrict__ C, int* __restrict__ flags, int N) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= (long)N * N) return;
  const long off = (long)blockIdx.y * N * N;
  const int i = (int)(e / N), j = (int)(e - (long)i * N);
  if (j > i) { C[off + e] = 0.0; return; }
  if (flags && !(fabs(C[off + e]) <= DBL_MAX)) { atomicOr(&flags[1 + blockIdx.y], SYGV_BAD_C); atomicOr(&flags[0], SYGV_BAD_C); }
}

int sygv_small_attr(const void* fn, size_t lds) {
  // above 64 KB the launch needs the function attribute (set every time: it is per device)
  if (lds > 64 * 1024) ND4_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  return 0;
}

// L [nL, N, N] of B [nL, N, N]; flags [1 + nL] zero on entry
int sygv_factor(nd4hip_handle* h, int64_t nL, int N, const double* B, double* L, int* flags) {
  Nd4WsScope scope(h);
  void* p = nullptr;
  ND4_TRY(nd4_ws_alloc(h, sizeof(int) * (size_t)nL, &p));
  int* pf = static_cast<int*>(p);
  ND4_TRY(nd4_potrf(h, nL, N, B, L, pf));
  hipLaunchKernelGGL(sygv_merge_flags, dim3((unsigned)((nL + 255) / 256)), dim3(256), 0, h->stream, pf, flags, (long)nL);
  hipLaunchKernelGGL(sygv_diag_check, dim3((unsigned)nL), dim3(256), 0, h->stream, L, (long)N * N, flags, N);
  ND4_HIP(hipGetLastError());
  return 0;
}

// C [nb, N, N] = L^-1 A L^-T, lower triangle and zeros above; W [nb, N, N] scratch; N > 64
int sygv_reduce_large(nd4hip_handle* h, int64_t nb, int N, const double* A, const double* L, int64_t sL, double* W, double* C, int* flags) {
  const int64_t nn = (int64_t)N * N;
  const dim3 grid((unsigned)((nn + 255) / 256), (unsigned)nb);
  hipLaunchKernelGGL(sygv_mirror_lower, grid, dim3(256), 0, h->stream, A, W, N);
  ND4_HIP(hipGetLastError());
  ND4_TRY(nd4_trsm(h, false, false, nb, N, N, L, sL, W));                       // W = L^-1 A
  ND4_TRY(nd4_transpose(h, N, N, W, N, C, N, nb, nn, nn));                      // C = W^T = A L^-T
  ND4_TRY(nd4_trsm(h, false, false, nb, N, N, L, sL, C));                       // C = L^-1 A L^-T
  hipLaunchKernelGGL(sygv_finish_c, grid, dim3(256), 0, h->stream, C, flags, N);
  ND4_HIP(hipGetLastError());
  return 0;
}

int sygv_reduce_small_launch(nd4hip_handle* h, int64_t nb, int N, const double* A, const double* T, int64_t sT, bool have_L, double* Lout,
                             double* C, int* flags) {
  const size_t lds = sygv_lds_bytes(N);
  ND4_TRY(sygv_small_attr(reinterpret_cast<const void*>(&sygv_reduce_small), lds));
  hipLaunchKernelGGL(sygv_reduce_small, dim3((unsigned)nb), dim3(64), lds, h->stream, A, T, (long)sT, have_L ? 1 : 0, Lout, C, flags, N);
  ND4_HIP(hipGetLastError());
  return 0;
}

// one read-back of the OR word; the member flags follow only when it is raised
int sygv_verdict(nd4hip_handle* h, const int* flags, int64_t nb, int64_t member0) {
  void* hp = nullptr;
  ND4_TRY(nd4_pinned(h, sizeof(int) * (size_t)(nb + 1), &hp));
  int* host = static_cast<int*>(hp);
  ND4_HIP(hipMemcpyAsync(host, flags, sizeof(int), hipMemcpyDeviceToHost, h->stream));
  ND4_HIP(hipStreamSynchronize(h->stream));
  if (host[0] == 0) return 0;
  if (host[0] & SYGV_BAD_B) {
    ND4_HIP(hipMemcpyAsync(host, flags, sizeof(int) * (size_t)(nb + 1), hipMemcpyDeviceToHost, h->stream));
    ND4_HIP(hipStreamSynchronize(h->stream));
    int64_t b = 0;
    while (b < nb - 1 && !(host[1 + b] & SYGV_BAD_B)) ++b;
    nd4_set_error("eigen_sym_gen(A,B): B is not positive definite. (matrix %lld)", (long long)(member0 + b));
    return ND4HIP_ERR_SINGULAR;
  }
  nd4_set_error("eigen_sym_gen(A,B): L^-1 A L^-T is not finite (NaN or Infinity in the lower triangle of A, or overflow).");
  return ND4HIP_ERR_NOCONV;
}

}  // namespace

// A [batch, N, N], B [batch (stride sB = N*N, or 0: one B), N, N] -> lambda [batch, N] descending, X [batch, N, N] or NULL; sweeps
// [batch] or NULL (algo 1 only). 1 <= N <= 2048 (128 for algo 1), batch >= 1: checked by the entry points. member0: the index of the
// first member in the caller's batch, for the error text. Synchronises.
int nd4_sygvd(nd4hip_handle* h, int algo, int64_t batch, int64_t N64, const double* A, const double* B, int64_t sB, double* lambda,
              double* X, int32_t* sweeps, int64_t member0) {
  const Nd4SygvSel all{0, 0, 0, 0, 0, nullptr, nullptr, nullptr};
  return nd4_sygvx(h, algo, all, batch, N64, A, B, sB, lambda, X, sweeps, member0);
}

// The same with step 3 chosen by sel (nd4hip_internal.h): the reduction of C, and all of its eigenpairs, the subset (i0, i1) or the
// interval bounds [batch, 2]. lambda [batch, K] and X [batch, N, K] with K = N, i1 - i0 or kcap; the interval's results are ragged as
// nd4_syevxv's, with range and *kmax. Steps 1-2, their verdicts and the passes over the batch do not depend on sel; step 4 runs on
// the columns that step 3 computed: K of them, or the kmax of the pass. sel.select = 0 and sel.reduction = 0 is nd4_sygvd.
int nd4_sygvx(nd4hip_handle* h, int algo, const Nd4SygvSel& sel, int64_t batch, int64_t N64, const double* A, const double* B, int64_t sB,
              double* lambda, double* X, int32_t* sweeps, int64_t member0) {
  const int N = (int)N64;
  const int64_t K = sel.select == 0 ? N64 : sel.select == 1 ? sel.i1 - sel.i0 : sel.kcap;
  int64_t kmax = 0; bool uneven = false;
  const int64_t nn = N64 * N64;
  const bool small = N <= SYGV_SMALL_N, shared = sB == 0;
  const int64_t chunk = sygv_chunk(batch, N64);
  Nd4WsScope scope(h);
  void* p = nullptr;
  ND4_TRY(nd4_ws_alloc(h, sizeof(int) * (size_t)(chunk + 1), &p));
  int* flags = static_cast<int*>(p);
  ND4_TRY(nd4_ws_alloc(h, sizeof(double) * (size_t)((shared ? 1 : chunk) * nn), &p));
  double* Lw = static_cast<double*>(p);
  ND4_TRY(nd4_ws_alloc(h, sizeof(double) * (size_t)(chunk * nn), &p));
  double* Cw = static_cast<double*>(p);
  double* Ww = nullptr;
  if (!small) { ND4_TRY(nd4_ws_alloc(h, sizeof(double) * (size_t)(chunk * nn), &p)); Ww = static_cast<double*>(p); }
  const size_t lds = sygv_lds_bytes(N);

  if (shared) {                                 // one B: factorised once, before the passes over the members
    ND4_HIP(hipMemsetAsync(flags, 0, sizeof(int) * 2, h->stream));
    if (small) {
      hipLaunchKernelGGL(sygv_chol_small, dim3(1), dim3(64), lds / 2, h->stream, B, Lw, flags, N);
      ND4_HIP(hipGetLastError());
    } else ND4_TRY(sygv_factor(h, 1, N, B, Lw, flags));
    ND4_TRY(sygv_verdict(h, flags, 1, member0));
  }
  for (int64_t b0 = 0; b0 < batch; b0 += chunk) {
    const int64_t nb = batch - b0 < chunk ? batch - b0 : chunk;
    const double* Ab = A + b0 * nn;
    double* lam = lambda + b0 * K;
    double* Xb = X ? X + b0 * N64 * K : nullptr;
    ND4_HIP(hipMemsetAsync(flags, 0, sizeof(int) * (size_t)(nb + 1), h->stream));
    if (small) {
      ND4_TRY(sygv_reduce_small_launch(h, nb, N, Ab, shared ? Lw : B + b0 * sB, sB, shared, (shared || !X) ? nullptr : Lw, Cw, flags));
    } else {
      if (!shared) ND4_TRY(sygv_factor(h, nb, N, B + b0 * sB, Lw, flags));
      ND4_TRY(sygv_reduce_large(h, nb, N, Ab, Lw, shared ? 0 : nn, Ww, Cw, flags));
    }
    ND4_TRY(sygv_verdict(h, flags, nb, member0 + b0));
    int64_t k = K;                              // the columns of X that step 3 computes
    if (sel.select == 2) {
      ND4_TRY(nd4_syevxv(h, sel.reduction != 0, nb, N, sel.kcap, sel.bounds + 2 * b0, Cw, lam, Xb, sel.range + 2 * b0, &k));
      uneven = uneven || (b0 > 0 && k != kmax);
      kmax = k > kmax ? k : kmax;
    } else if (sel.select == 1) {
      ND4_TRY((sel.reduction ? nd4_syevx_tr : nd4_syevx)(h, nb, N, sel.i0, sel.i1, Cw, lam, Xb));
    } else if (sel.reduction) ND4_TRY(nd4_syevd_tr(h, nb, N, Cw, lam, Xb));
    else if (algo == 1)       ND4_TRY(nd4_syevj(h, nb, N, Cw, lam, Xb, sweeps ? sweeps + b0 : nullptr));
    else                      ND4_TRY(nd4_syevd(h, nb, N, Cw, lam, Xb));
    if (!Xb || k == 0) continue;
    if (small) {
      ND4_TRY(sygv_small_attr(reinterpret_cast<const void*>(&sygv_back_small), lds));
      hipLaunchKernelGGL(sygv_back_small, dim3((unsigned)nb), dim3(64), lds, h->stream, Lw, (long)(shared ? 0 : nn), Xb, N, (int)k, (long)K);
      ND4_HIP(hipGetLastError());
    } else if (k == K) {
      ND4_TRY(nd4_trsm_t(h, nb, N, K, Lw, N, shared ? 0 : nn, Xb, N64 * K));
    } else {                                    // the kmax columns of an interval, out of kcap: solved in a dense copy
      Nd4WsScope pass(h);
      ND4_TRY(nd4_ws_alloc(h, sizeof(double) * (size_t)(nb * N64 * k), &p));
      double* Xc = static_cast<double*>(p);
      ND4_TRY(nd4_copy_matrix(h, N, k, Xb, K, Xc, k, nb, N64 * K, N64 * k));
      ND4_TRY(nd4_trsm_t(h, nb, N, k, Lw, N, shared ? 0 : nn, Xc, N64 * k));
      ND4_TRY(nd4_copy_matrix(h, N, k, Xc, k, Xb, K, nb, N64 * k, N64 * K));
    }
  }
  if (sel.select == 2) {
    *sel.kmax = kmax;
    if (uneven) {                               // the passes found different kmax: the padding of every member reaches the largest
      ND4_TRY(nd4_stxv_pad(h, batch, N64, sel.kcap, kmax, sel.range, lambda, X, false));
      ND4_HIP(hipStreamSynchronize(h->stream));
    }
  }
  return 0;
}

// step 2 on its own: C [batch, N, N] = L^-1 A L^-T (lower triangle, exact zeros above) from a given L (stride sL, 0 = one L)
int nd4_sygst(nd4hip_handle* h, int64_t batch, int64_t N64, const double* A, const double* L, int64_t sL, double* C) {
  const int N = (int)N64;
  const int64_t nn = N64 * N64;
  const bool small = N <= SYGV_SMALL_N;
  const int64_t chunk = sygv_chunk(batch, N64);
  Nd4WsScope scope(h);
  double* Ww = nullptr;
  if (!small) { void* p = nullptr; ND4_TRY(nd4_ws_alloc(h, sizeof(double) * (size_t)(chunk * nn), &p)); Ww = static_cast<double*>(p); }
  for (int64_t b0 = 0; b0 < batch; b0 += chunk) {
    const int64_t nb = batch - b0 < chunk ? batch - b0 : chunk;
    if (small) ND4_TRY(sygv_reduce_small_launch(h, nb, N, A + b0 * nn, L + b0 * sL, sL, true, nullptr, C + b0 * nn, nullptr));
    else       ND4_TRY(sygv_reduce_large(h, nb, N, A + b0 * nn, L + b0 * sL, sL, Ww, C + b0 * nn, nullptr));
  }
  return 0;
}
