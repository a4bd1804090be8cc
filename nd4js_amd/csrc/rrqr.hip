// Column-pivoted QR (rrqr_decomp / rrqr_decomp_full, src/la/rrqr.js:88-395), its rank estimate (_rrqr_rank, :57-85) and
// least squares (rrqr_lstsq, :447-580).
//
// The pivot pass decides P only. It is an unblocked right-looking Householder QR on a column-major copy of A (column j of the
// matrix is row j of the workspace, so every column access is contiguous), two launches per column step:
//   qp3_pivot   one workgroup per matrix: the first maximum of the column norms (the reference's strict `<`, :126-132: an earlier
//               index wins ties, a NaN never wins), the swap, the Householder vector of the pivot column;
//   qp3_update  one wave per remaining column, the whole chip over columns x batch: apply the reflector and RECOMPUTE the column's
//               norm below the diagonal from the updated entries, as the reference does before every step (:124, :151) — no
//               downdating, so every norm that feeds a comparison is accurate to a few ulp.
// Every reduction is a fixed butterfly inside one wave or a fixed sequence in one thread: no atomics, no exchange between
// workgroups inside a kernel, and two identical columns keep bit-identical norms. Q and R are then those of the unpivoted QR of
// A[:, P] (the existing dgeqrf_q / dgeqrf_full path), which is what the reference's R and Q are up to rounding.
#include "nd4hip_internal.h"
#include <climits>
#include <cmath>

namespace {

constexpr int WAVE = 64;

__device__ inline double wave_sum(double x) {
  for (int o = WAVE / 2; o > 0; o >>= 1) x += __shfl_xor(x, o, WAVE);    // butterfly: every lane ends with the same bits
  return x;
}
// max that propagates NaN (a NaN norm must stay NaN, like the reference's _norm, :48-54)
__device__ inline double nan_max(double a, double b) { return (a != a) ? a : ((b != b) ? b : (a > b ? a : b)); }
__device__ inline double wave_max(double x) {
  for (int o = WAVE / 2; o > 0; o >>= 1) x = nan_max(x, __shfl_xor(x, o, WAVE));
  return x;
}
// ||x|| from the wave's max |x| and the sum of (x 2^-e)^2, e = exponent of the max: power-of-two scaling is exact, so this is as
// accurate as the plain sum of squares and cannot overflow or underflow (the reference's scaled form, :29-45)
__device__ inline int norm_exp(double mx) { return (mx > 0.0 && mx <= 1.79769313486231570e308) ? ilogb(mx) : 0; }
__device__ inline double norm_finish(double mx, double s, int e) {
  if (!(mx <= 1.79769313486231570e308)) return mx;             // Inf or NaN
  if (mx == 0.0) return 0.0;
  return ldexp(sqrt(s), e);
}

// ---- the pivot step ---------------------------------------------------------------------------------------------------------
// W [batch][N][M]: column j of the matrix at W + j M. nrm[j] = ||W[j][i:M]|| for j >= i. On return column i of the workspace
// holds beta at row i and the reflector v (v_i = 1 implied) below; tau[b] its factor. stop[b] = 1 ends the pass of matrix b
// (largest remaining norm exactly zero, :138, or no comparable norm at all).
__global__ __launch_bounds__(256) void qp3_pivot(int M, int N, int i, double* __restrict__ W, double* __restrict__ nrm,
                                                 int32_t* __restrict__ perm, double* __restrict__ tau, int* __restrict__ stop) {
  const long b = blockIdx.x;
  if (stop[b]) return;
  W += b * (long)M * N; nrm += b * (long)N; perm += b * (long)N;
  const int t = threadIdx.x, lane = t & (WAVE - 1), wv = t >> 6;
  double best = -INFINITY; int idx = INT_MAX;
  for (int j = i + t; j < N; j += 256) { const double v = nrm[j]; if (best < v) { best = v; idx = j; } }
  for (int o = WAVE / 2; o > 0; o >>= 1) {
    const double ob = __shfl_xor(best, o, WAVE); const int oi = __shfl_xor(idx, o, WAVE);
    if (ob > best || (ob == best && oi < idx)) { best = ob; idx = oi; }
  }
  __shared__ double s_best[4]; __shared__ int s_idx[4];
  if (lane == 0) { s_best[wv] = best; s_idx[wv] = idx; }
  __syncthreads();
  best = s_best[0]; idx = s_idx[0];
  for (int w = 1; w < 4; w++)
    if (s_best[w] > best || (s_best[w] == best && s_idx[w] < idx)) { best = s_best[w]; idx = s_idx[w]; }
  if (idx == INT_MAX || best == 0.0) {                             // nothing left to eliminate: the remaining columns keep their order
    if (t == 0) stop[b] = 1;
    return;
  }
  const int p = idx;
  double* ci = W + (long)i * M;
  double* cp = W + (long)p * M;
  const double alpha = cp[i];
  __syncthreads();                                                 // every thread has alpha before row i of column i changes
  // Householder of x = column p rows i.., ||x|| = best:  beta = -sign(alpha) ||x||, v = x / (alpha - beta), tau = (beta - alpha) / beta
  // (a division, not a multiplication by 1/(alpha - beta): that reciprocal overflows for a pivot norm below ~5.6e-309)
  const double beta = -copysign(best, alpha);
  const double den = alpha - beta;
  for (int k = i + t; k < M; k += 256) {
    const double xk = cp[k];
    if (p != i) cp[k] = ci[k];
    ci[k] = (k == i) ? beta : xk / den;
  }
  if (t == 0) {
    tau[b] = (beta - alpha) / beta;
    if (p != i) { const int32_t q = perm[i]; perm[i] = perm[p]; perm[p] = q; nrm[p] = nrm[i]; }
  }
}

// ---- the update of the remaining columns: one wave per column -----------------------------------------------------------------
// i >= 0: column j = i+1+(wave index) gets H_i applied to rows i.., then nrm[j] = ||rows i+1..||.  i < 0: the initial norms of
// every column (rows 0..), nothing else. E > 0 keeps the column (and v) in registers: E elements per lane cover 64 E rows.
template <int E>
__global__ __launch_bounds__(256) void qp3_update(int M, int N, int i, double* __restrict__ W, double* __restrict__ nrm,
                                                  const double* __restrict__ tau, const int* __restrict__ stop) {
  const long b = blockIdx.y;
  if (stop[b]) return;
  const int lane = threadIdx.x & (WAVE - 1);
  const int j = (i < 0 ? 0 : i + 1) + (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6);
  if (j >= N) return;
  W += b * (long)M * N;
  const int k0 = i < 0 ? 0 : i, len = M - k0;
  double* col = W + (long)j * M + k0;
  const double* v = W + (long)(i < 0 ? 0 : i) * M + k0;          // v[0] = 1 is implied (row i holds beta)
  const double tb = i < 0 ? 0.0 : tau[b];
  const int nfrom = i < 0 ? 0 : 1;                                 // first row (relative to k0) of the norm
  double mx = 0.0, s = 0.0;
  if constexpr (E > 0) {
    double x[E], vv[E];
#pragma unroll
    for (int e = 0; e < E; e++) {
      const int k = lane + WAVE * e;
      x[e] = k < len ? col[k] : 0.0;
      vv[e] = (k < len && i >= 0) ? (k == 0 ? 1.0 : v[k]) : 0.0;
    }
    if (i >= 0) {
      double d = 0.0;
#pragma unroll
      for (int e = 0; e < E; e++) d += vv[e] * x[e];
      const double w = tb * wave_sum(d);
#pragma unroll
      for (int e = 0; e < E; e++) {
        const int k = lane + WAVE * e;
        if (k < len) { x[e] -= w * vv[e]; col[k] = x[e]; }
      }
    }
#pragma unroll
    for (int e = 0; e < E; e++) { const int k = lane + WAVE * e; if (k >= nfrom && k < len) mx = nan_max(mx, fabs(x[e])); }
    mx = wave_max(mx);
    const int ex = norm_exp(mx);
#pragma unroll
    for (int e = 0; e < E; e++) { const int k = lane + WAVE * e; if (k >= nfrom && k < len) { const double y = ldexp(x[e], -ex); s += y * y; } }
  } else {
    if (i >= 0) {
      double d = 0.0;
      for (int k = lane; k < len; k += WAVE) d += (k == 0 ? 1.0 : v[k]) * col[k];
      const double w = tb * wave_sum(d);
      for (int k = lane; k < len; k += WAVE) col[k] -= w * (k == 0 ? 1.0 : v[k]);
    }
    for (int k = lane; k < len; k += WAVE) if (k >= nfrom) mx = nan_max(mx, fabs(col[k]));
    mx = wave_max(mx);
    const int ex = norm_exp(mx);
    for (int k = lane; k < len; k += WAVE) if (k >= nfrom) { const double y = ldexp(col[k], -ex); s += y * y; }
  }
  s = wave_sum(s);
  if (lane == 0) nrm[b * (long)N + j] = norm_finish(mx, s, norm_exp(mx));
}

__global__ void qp3_init(int N, int32_t* __restrict__ perm, int* __restrict__ stop) {
  const long b = blockIdx.y;
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j < N) perm[b * (long)N + j] = j;
  if (j == 0) stop[b] = 0;
}

// Ap[b][r][c] = A[b][r][P[b][c]]
__global__ void qp3_gather(int M, int N, const double* __restrict__ A, const int32_t* __restrict__ P, double* __restrict__ Ap) {
  const long b = blockIdx.z;
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= N) return;
  const int pc = P[b * (long)N + c];
  const double* a = A + b * (long)M * N;
  double* o = Ap + b * (long)M * N;
  for (int r = blockIdx.y; r < M; r += gridDim.y) o[(long)r * N + c] = a[(long)r * N + pc];
}

int launch_update(nd4hip_handle* h, int M, int N, int i, double* W, double* nrm, const double* tau, const int* stop, int nb) {
  const int ncols = i < 0 ? N : N - i - 1;
  if (ncols <= 0) return 0;
  const int len = i < 0 ? M : M - i;
  const dim3 grid((unsigned)((ncols + 3) / 4), (unsigned)nb);
  if (len <= 64)        hipLaunchKernelGGL(qp3_update<1>, grid, dim3(256), 0, h->stream, M, N, i, W, nrm, tau, stop);
  else if (len <= 256)  hipLaunchKernelGGL(qp3_update<4>, grid, dim3(256), 0, h->stream, M, N, i, W, nrm, tau, stop);
  else if (len <= 1024) hipLaunchKernelGGL(qp3_update<16>, grid, dim3(256), 0, h->stream, M, N, i, W, nrm, tau, stop);
  else if (len <= 2048) hipLaunchKernelGGL(qp3_update<32>, grid, dim3(256), 0, h->stream, M, N, i, W, nrm, tau, stop);
  else                  hipLaunchKernelGGL(qp3_update<0>, grid, dim3(256), 0, h->stream, M, N, i, W, nrm, tau, stop);
  ND4_HIP(hipGetLastError());
  return 0;
}

// ---- rank (_rrqr_rank, rrqr.js:57-85) ---------------------------------------------------------------------------------------
// per row i < L of R [M, N] (batch stride sR): exponent and scaled sum of squares of R[i, i:N]; a non-finite row stores s = NaN/Inf
__global__ __launch_bounds__(256) void qp3_rownorm(int M, int N, int L, const double* __restrict__ R, long sR,
                                                   int* __restrict__ re, double* __restrict__ rs) {
  const long b = blockIdx.y;
  const int lane = threadIdx.x & (WAVE - 1);
  const int i = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6);
  if (i >= L) return;
  const double* row = R + b * sR + (long)i * N;
  double mx = 0.0, s = 0.0;
  for (int k = i + lane; k < N; k += WAVE) mx = nan_max(mx, fabs(row[k]));
  mx = wave_max(mx);
  const int ex = norm_exp(mx);
  for (int k = i + lane; k < N; k += WAVE) { const double y = ldexp(row[k], -ex); s += y * y; }
  s = wave_sum(s);
  if (lane == 0) {
    const bool fin = mx <= 1.79769313486231570e308;
    re[b * (long)L + i] = ex;
    rs[b * (long)L + i] = fin ? s : mx;
  }
}

// one wave per matrix: tmp[i] = ||R[i:L, upper]|| accumulated from the bottom row up in one thread (fixed order), then the
// threshold T = 2 eps max(M,N) tmp[0] and rank = 1 + the last i with tmp[i] > T (the reference's `while( tmp[r-1] <= T ) --r`).
// rank[b] = -1 when a tmp[i] is not finite ('Infinity or NaN encountered during rank estimation.', :78-79).
__global__ __launch_bounds__(64) void qp3_rank(int M, int N, int L, const int* __restrict__ re, const double* __restrict__ rs,
                                               double* __restrict__ tmp, int* __restrict__ rank) {
  const long b = blockIdx.x;
  re += b * (long)L; rs += b * (long)L; tmp += b * (long)L;
  const int lane = threadIdx.x;
  constexpr int CH = 1024;
  __shared__ int s_e[CH];
  __shared__ double s_s[CH];
  __shared__ int s_bad;
  double S = 0.0; int EX = 0; bool bad = false;
  for (int hi = L; hi > 0; hi -= CH) {
    const int lo = hi - CH > 0 ? hi - CH : 0;
    for (int k = lo + lane; k < hi; k += WAVE) { s_e[k - lo] = re[k]; s_s[k - lo] = rs[k]; }
    __syncthreads();
    if (lane == 0) {
      for (int k = hi - 1; k >= lo; k--) {
        const double si = s_s[k - lo]; const int ei = s_e[k - lo];
        if (!(si <= 1.79769313486231570e308)) bad = true;
        else if (si > 0.0) {
          if (S == 0.0) { S = si; EX = ei; }
          else if (ei > EX) { S = ldexp(S, 2 * (EX - ei)) + si; EX = ei; }
          else S += ldexp(si, 2 * (ei - EX));
        }
        tmp[k] = bad ? NAN : ldexp(sqrt(S), EX);
      }
    }
    __syncthreads();
  }
  if (lane == 0) s_bad = bad ? 1 : 0;
  __syncthreads();
  if (s_bad) { if (lane == 0) rank[b] = -1; return; }
  const double T = 2.220446049250313e-16 * 2 * (double)(M > N ? M : N) * tmp[0];   // read back by every lane (written by lane 0)
  int last = -1;
  for (int k = lane; k < L; k += WAVE) if (tmp[k] > T) last = k;
  for (int o = WAVE / 2; o > 0; o >>= 1) { const int ol = __shfl_xor(last, o, WAVE); last = ol > last ? ol : last; }
  if (lane == 0) rank[b] = last + 1;
}

// Tm [L,L] = R[0:L, 0:L] inside the rank, identity outside; Z rows >= rank zeroed (so the triangular solve leaves them 0)
__global__ void qp3_mask(int L, int I, int J, const double* __restrict__ R, long sR, const int* __restrict__ rank,
                         double* __restrict__ Tm, double* __restrict__ Z) {
  const long b = blockIdx.z;
  const int r = rank[b] < 0 ? 0 : rank[b];
  const int c = blockIdx.x * 256 + threadIdx.x;
  const double* Rb = R + b * sR;
  double* T = Tm + b * (long)L * L;
  double* z = Z + b * (long)L * J;
  for (int row = blockIdx.y; row < L; row += gridDim.y) {
    if (c < L) T[(long)row * L + c] = (row < r && c < r) ? Rb[(long)row * I + c] : (row == c ? 1.0 : 0.0);
    if (c < J && row >= r) z[(long)row * J + c] = 0.0;
  }
}

// X[b][P[b][i]][:] = Z[b][i][:] (0 for i >= L); indices outside [0, I) are skipped (the host forms refuse such a P beforehand)
__global__ void qp3_unperm(int L, int I, int J, const double* __restrict__ Z, const int32_t* __restrict__ P, long sP,
                           double* __restrict__ X) {
  const long b = blockIdx.z;
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= J) return;
  const int32_t* p = P + b * sP;
  for (int i = blockIdx.y; i < I; i += gridDim.y) {
    const int d = p[i];
    if (d < 0 || d >= I) continue;
    X[b * (long)I * J + (long)d * J + c] = i < L ? Z[b * (long)L * J + (long)i * J + c] : 0.0;
  }
}

}  // namespace

// ---- internal launchers -------------------------------------------------------------------------------------------------------
// P [batch, N] and Q / R as dgeqrf_q (full = false: Q [M, L], R [L, N]) or dgeqrf_full (Q [M, M], R [M, N]); batch <= 32768.
int nd4_geqp3(nd4hip_handle* h, int64_t batch, int64_t M64, int64_t N64, const double* A, double* Q, double* R, int32_t* P, bool full) {
  ND4_CHECK_ARG(M64 < (1ll << 30) && N64 < (1ll << 30) && M64 * N64 < (1ll << 40) && batch <= 32768, "nd4_geqp3: extent out of range");
  const int M = (int)M64, N = (int)N64, K = M < N ? M : N;
  if (batch == 0 || M == 0 || N == 0) return 0;
  // the workspace copy is M N per matrix: at most ~1 GiB of it at a time
  const int64_t per_ws = (int64_t)M * N;
  int64_t step = ((int64_t)1 << 27) / per_ws;
  if (step < 1) step = 1;
  if (step > batch) step = batch;
  const int64_t L = K;
  for (int64_t b0 = 0; b0 < batch; b0 += step) {
    const int nb = (int)(batch - b0 < step ? batch - b0 : step);
    const double* Ab = A + b0 * per_ws;
    int32_t* Pb = P + b0 * N;
    Nd4WsScope scope(h);
    void* p = nullptr;
    ND4_TRY(nd4_ws_alloc(h, sizeof(double) * (size_t)(nb * per_ws + (int64_t)nb * N + nb) + sizeof(int) * (size_t)nb, &p));
    double* W = static_cast<double*>(p);
    double* nrm = W + (size_t)nb * per_ws;
    double* tau = nrm + (size_t)nb * N;
    int* stop = reinterpret_cast<int*>(tau + nb);
    hipLaunchKernelGGL(qp3_init, dim3((unsigned)((N + 255) / 256), (unsigned)nb), dim3(256), 0, h->stream, N, Pb, stop);
    ND4_HIP(hipGetLastError());
    ND4_TRY(nd4_transpose(h, M, N, Ab, N, W, M, nb, per_ws, per_ws));           // column j of A -> row j of W
    ND4_TRY(launch_update(h, M, N, -1, W, nrm, tau, stop, nb));
    for (int i = 0; i < K; i++) {
      hipLaunchKernelGGL(qp3_pivot, dim3((unsigned)nb), dim3(256), 0, h->stream, M, N, i, W, nrm, Pb, tau, stop);
      ND4_HIP(hipGetLastError());
      if (i + 1 < K) ND4_TRY(launch_update(h, M, N, i, W, nrm, tau, stop, nb));   // the last step's update feeds no comparison
    }
    // Q and R: the unpivoted QR of A[:, P] (W is free now)
    const dim3 g((unsigned)((N + 255) / 256), (unsigned)(M < 1024 ? M : 1024), (unsigned)nb);
    hipLaunchKernelGGL(qp3_gather, g, dim3(256), 0, h->stream, M, N, Ab, Pb, W);
    ND4_HIP(hipGetLastError());
    if (full) ND4_TRY(nd4_geqrf_q_ex(h, nb, M, N, W, Q + b0 * M64 * M64, R + b0 * M64 * N64, true));
    else      ND4_TRY(nd4_geqrf_q(h, nb, M, N, W, Q + b0 * M64 * L, R + b0 * L * N64));
  }
  return 0;
}

// rank [batch] (int32, -1 = a non-finite partial norm) of R [M, N] with batch stride sR; tmp: workspace of batch * min(M,N) doubles
int nd4_qp3rank(nd4hip_handle* h, int64_t batch, int64_t M, int64_t N, const double* R, int64_t sR, int* rank) {
  ND4_CHECK_ARG(M < (1ll << 30) && N < (1ll << 30) && batch <= 65535, "nd4_qp3rank: extent out of range");
  const int64_t L = M < N ? M : N;
  if (batch == 0) return 0;
  if (L == 0) { ND4_HIP(hipMemsetAsync(rank, 0, sizeof(int) * (size_t)batch, h->stream)); return 0; }
  Nd4WsScope scope(h);
  void* p = nullptr;
  ND4_TRY(nd4_ws_alloc(h, (sizeof(double) * 2 + sizeof(int)) * (size_t)(batch * L), &p));
  double* rs = static_cast<double*>(p);
  double* tmp = rs + batch * L;
  int* re = reinterpret_cast<int*>(tmp + batch * L);
  hipLaunchKernelGGL(qp3_rownorm, dim3((unsigned)((L + 3) / 4), (unsigned)batch), dim3(256), 0, h->stream, (int)M, (int)N, (int)L, R, (long)sR, re, rs);
  ND4_HIP(hipGetLastError());
  hipLaunchKernelGGL(qp3_rank, dim3((unsigned)batch), dim3(64), 0, h->stream, (int)M, (int)N, (int)L, re, rs, tmp, rank);
  ND4_HIP(hipGetLastError());
  return 0;
}

// rrqr_lstsq (rrqr.js:447-580) for Q [N, M], R [M, I], P [I], Y [N, J] -> X [I, J]; rank_out [batch] (device, may be NULL)
int nd4_qp3ls(nd4hip_handle* h, int64_t batch, int64_t N, int64_t M, int64_t I, int64_t J, const double* Q, int64_t sQ,
              const double* R, int64_t sR, const int32_t* P, int64_t sP, const double* Y, int64_t sY, double* X, int* rank_out) {
  ND4_CHECK_ARG(I < (1ll << 30) && J < (1ll << 30) && M < (1ll << 30) && batch <= 32768, "nd4_qp3ls: extent out of range");
  const int64_t L = M < I ? M : I;
  Nd4WsScope scope(h);
  void* p = nullptr;
  ND4_TRY(nd4_ws_alloc(h, sizeof(double) * (size_t)(batch * (L * L + L * J)) + sizeof(int) * (size_t)batch, &p));
  double* Tm = static_cast<double*>(p);
  double* Z = Tm + batch * L * L;
  int* rank = rank_out ? rank_out : reinterpret_cast<int*>(Z + batch * L * J);
  ND4_TRY(nd4_qp3rank(h, batch, M, I, R, sR, rank));
  if (L > 0) {
    if (N == 0) ND4_HIP(hipMemsetAsync(Z, 0, sizeof(double) * (size_t)(batch * L * J), h->stream));
    else ND4_TRY(nd4_gemm(h, true, false, L, J, N, 1.0, Q, M, sQ, Y, J, sY, 0.0, Z, J, L * J, batch));   // (Q^T y)[0:L]  (:535-539)
    const int64_t wmax = L > J ? L : J;
    hipLaunchKernelGGL(qp3_mask, dim3((unsigned)((wmax + 255) / 256), (unsigned)(L < 1024 ? L : 1024), (unsigned)batch), dim3(256), 0,
                       h->stream, (int)L, (int)I, (int)J, R, (long)sR, rank, Tm, Z);
    ND4_HIP(hipGetLastError());
    ND4_TRY(nd4_trsm_ld(h, true, false, batch, L, J, Tm, L, L * L, Z, L * J));                       // _triu_solve (:541)
  }
  hipLaunchKernelGGL(qp3_unperm, dim3((unsigned)((J + 255) / 256), (unsigned)(I < 1024 ? I : 1024), (unsigned)batch), dim3(256), 0,
                     h->stream, (int)L, (int)I, (int)J, Z, P, (long)sP, X);
  ND4_HIP(hipGetLastError());
  return 0;
}
