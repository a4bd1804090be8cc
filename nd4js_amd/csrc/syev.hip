// eigen_sym / eigenvals_sym: the symmetric eigenproblem S = V diag(lambda) V^T on the device, composed from the pieces that are
// already here. The reference only plans these functions (src/la/eigen.js:28-30), so there is no reference
// algorithm to restate; the route is
//   1. syev_absmax_lower + syev_symm: W = 2^-e1 (lower triangle of S mirrored), e1 from max|s_ij| over the lower triangle. The
//      upper triangle of S is never read and S is never written. 64 x 64 tiles go through LDS so that both the straight and the
//      mirrored store are coalesced.
//   2. nd4_gehrd (hess.hip, unchanged): W = U H U^T. For symmetric W the Hessenberg form H is tridiagonal up to rounding:
//      d = diag(H), e = subdiag(H); what stands above the super-diagonal is rounding and is ignored.
//   3. syev_shift_chol, one wave per member: the Gershgorin bound g = max_i(|d_i| + |e_i-1| + |e_i|) >= rho(T), the exact power of
//      two 2^k that puts g in [1, 2), the shift c = g (1 + 2^-20), and the Cholesky recurrence of the positive definite
//      2^k T + c I = B^T B, B upper bidiagonal with diagonal p and super-diagonal q:
//         p_0 = sqrt(d_0 + c),  q_i = e_i / p_i,  p_i+1 = sqrt((d_i+1 + c) - q_i^2).
//      lambda_min(2^k T + c I) >= c - g = 2^-20 g, and every Schur complement of a positive definite matrix is at least its
//      smallest eigenvalue, so the exact radicand is >= 2^-20 and its computed value (three roundings of numbers <= 4.01) stays
//      above 2^-20 - 2^-49: no pivot of finite input can be non-positive. NaN or Inf in the lower triangle of S (max|s_ij| of
//      step 1 above DBL_MAX: the entrance check) or in d, e raises the call's flag word and the member gets the bidiagonal of
//      the identity, so the solver sees finite data whatever the input was. A member with e = 0 throughout (a diagonal T: the
//      identity, the zero matrix, a diagonal S) is marked: its eigenvalues are its d, which step 5 sorts instead of squaring and
//      subtracting, so they are exact.
//   4. nd4_bdsdc_rows (svd_dc.hip, unchanged): B = U2 diag(sv) V2, sv descending. B^T B = V2^T diag(sv^2) V2: the rows of V2 are
//      the eigenvectors of T.
//   5. syev_values: lambda_i = 2^(e1 - k) (sv_i^2 - c), descending because sv is (a marked member: 2^e1 d by descending rank, and
//      the unit vectors in that order for the rows of V2); V = U V2^T on the fp64 MFMA GEMM.
// The subtraction in 5 cancels: the error of lambda is absolute, a few eps g <= a few eps sqrt(3) ||S||_F, for every eigenvalue,
// small ones included. That is the bound of any backward stable symmetric solver, not more.
#include "syev_internal.h"
#include <climits>

namespace {

constexpr int SYEV_TILE = 64;
constexpr int SYEV_MAXN = 2048;            // the divide & conquer solver's limit; d and e of one member are staged in 32 KB of LDS
constexpr int SYEV_DIAG = INT_MIN;         // kexp of a member whose tridiagonal form is diagonal (e = 0): lambda = d, sorted

// mx[b] = bits of max |S[b, i, j]| over j <= i (the bit pattern of |x| orders like |x|; NaN sorts above Inf). grid (rows, batch)
__global__ __launch_bounds__(256) void syev_absmax_lower(const double* __restrict__ S, int N, u64* __restrict__ mx) {
  const double* s = S + (size_t)blockIdx.y * N * N;
  u64 m = 0;
  for (int r = blockIdx.x; r < N; r += gridDim.x)
    for (int c = threadIdx.x; c <= r; c += 256) {
      const u64 b = (u64)__double_as_longlong(fabs(s[(size_t)r * N + c]));
      m = b > m ? b : m;
    }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) { const u64 o = __shfl_xor(m, off); m = o > m ? o : m; }
  if ((threadIdx.x & 63) == 0 && m) atomicMax(mx + blockIdx.y, m);
}

// W[b] = 2^-e1 sym(lower(S[b])): the tile (ti, tj), tj <= ti, of the lower triangle is loaded once (rows of 64 consecutive words),
// stored straight at (ti, tj) and, through the 65-word pitch of the LDS tile, transposed at (tj, ti). A diagonal tile takes
// its upper half from its own lower half. grid (tiles, tiles, batch); blocks above the diagonal leave at once.
__global__ __launch_bounds__(256) void syev_symm(const double* __restrict__ S, double* __restrict__ W, int N, const u64* __restrict__ mx) {
  __shared__ double tile[SYEV_TILE][SYEV_TILE + 1];
  const int ti = blockIdx.y, tj = blockIdx.x;
  if (tj > ti) return;
  const int e1 = syev_exp(mx[blockIdx.z]);
  const double* s = S + (size_t)blockIdx.z * N * N;
  double* w = W + (size_t)blockIdx.z * N * N;
  const int i0 = ti * SYEV_TILE, j0 = tj * SYEV_TILE, c = threadIdx.x & 63;
  for (int r = threadIdx.x >> 6; r < SYEV_TILE; r += 4)
    if (i0 + r < N && j0 + c <= i0 + r) tile[r][c] = ldexp(s[(size_t)(i0 + r) * N + j0 + c], -e1);   // j0 + c <= i0 + r < N
  __syncthreads();
  for (int r = threadIdx.x >> 6; r < SYEV_TILE; r += 4) {
    if (i0 + r < N && j0 + c < N && (ti != tj || c <= r)) w[(size_t)(i0 + r) * N + j0 + c] = tile[r][c];
    // the mirrored element (j0 + r, i0 + c) = lower (i0 + c, j0 + r); on a diagonal tile only its strict upper half
    if (j0 + r < N && i0 + c < N && (ti != tj || c > r)) w[(size_t)(j0 + r) * N + i0 + c] = tile[c][r];
  }
}

// One wave per member. H [batch, N, N]: the Hessenberg form of a symmetric matrix. p [batch, N], q [batch, N-1]:
// the bidiagonal Cholesky factor of 2^k T + c I; cs [batch] = c; kexp [batch] = k, or SYEV_DIAG for a diagonal T. *flag: raised
// to 1 when a member is not finite: when mx[b], the bits of max|s_ij| over its lower triangle, lie above those of DBL_MAX (NaN
// or Inf anywhere in the triangle, also where the reduction leaves it below the subdiagonal of H: hess.hip finds a row that is
// already reduced with fmax, which drops NaN), or when d or e of H are not finite. The recurrence is serial (lane 0); its
// operands come from LDS. No contraction: the radicand is (d + c) - q q with each operation rounded once, as the bound in the
// head of this file assumes.
__global__ __launch_bounds__(64) void syev_shift_chol(const double* __restrict__ H, int N, const u64* __restrict__ mx, double* __restrict__ p,
                                                      double* __restrict__ q, double* __restrict__ cs, int* __restrict__ kexp, int* __restrict__ flag) {
#pragma clang fp contract(off)
  __shared__ double sd[SYEV_MAXN], se[SYEV_MAXN];
  const int b = blockIdx.x, lane = threadIdx.x;
  const double* h = H + (size_t)b * N * N;
  for (int i = lane; i < N; i += 64) {
    sd[i] = h[(size_t)i * N + i];
    se[i] = i + 1 < N ? h[(size_t)(i + 1) * N + i] : 0.0;
  }
  __syncthreads();
  double g = 0.0; int bad = mx[b] > SYEV_MAX_BITS, offdiag = 0;
  for (int i = lane; i < N; i += 64) {
    offdiag |= se[i] != 0.0;
    const double row = (fabs(sd[i]) + (i > 0 ? fabs(se[i - 1]) : 0.0)) + fabs(se[i]);
    bad |= !(row <= DBL_MAX);                                 // NaN or Inf (fmax below would drop a NaN)
    g = fmax(g, row);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) { g = fmax(g, __shfl_xor(g, off)); bad |= __shfl_xor(bad, off); offdiag |= __shfl_xor(offdiag, off); }
  double* pb = p + (size_t)b * N;
  double* qb = q + (size_t)b * (N - 1);
  if (bad || g == 0.0) {                                      // the identity's bidiagonal keeps the solver on finite data
    for (int i = lane; i < N; i += 64) { pb[i] = 1.0; if (i + 1 < N) qb[i] = 0.0; }
    if (lane == 0) { cs[b] = 0.0; kexp[b] = SYEV_DIAG; if (bad) atomicMax(flag, 1); }
    return;
  }
  int eg = 0;
  (void)frexp(g, &eg);                                        // g = m 2^eg, m in [0.5, 1)
  int k = 1 - eg;                                             // 2^k g in [1, 2)
  k = k > 1022 ? 1022 : (k < -1022 ? -1022 : k);              // 2^k itself stays a finite normal number
  const double c = ldexp(g, k) * (1.0 + 0x1p-20);
  if (lane != 0) return;
  cs[b] = c; kexp[b] = offdiag ? k : SYEV_DIAG;
  int fail = 0;
  double rad = ldexp(sd[0], k) + c;
  for (int i = 0; ; ++i) {
    const bool ok = rad > 0.0 && rad <= DBL_MAX;
    fail |= !ok;
    const double pi = ok ? sqrt(rad) : 1.0;                   // (unreachable for finite input; the solver still gets finite data)
    pb[i] = pi;
    if (i + 1 >= N) break;
    const double qi = ldexp(se[i], k) / pi;
    qb[i] = qi;
    rad = (ldexp(sd[i + 1], k) + c) - qi * qi;
  }
  if (fail) atomicMax(flag, 1);
}

// lambda = 2^(e1 - k) (sv^2 - c), one thread per value. A diagonal member (H [batch, N, N] holds its d): thread j writes
// 2^e1 d_j at its descending rank (ties by index) and, where the vectors are wanted (V2 != NULL), the unit vector e_j as row
// `rank` of V2 [batch, N, N] in place of the solver's. The solver's own rows are a permutation only up to rounding (its
// deflation rotates tied and near-zero pairs: entries like cos(pi/2) = 6.1e-17), and its order of the rounded roots
// sqrt(d + c) is the order of d only up to their ties; with e_j the pairs (2^e1 d_j, U e_j) of a diagonal T are exact.
__global__ __launch_bounds__(256) void syev_values(const double* __restrict__ sv, const double* __restrict__ H, int N, long total,
                                                   const double* __restrict__ cs, const int* __restrict__ kexp, const u64* __restrict__ mx,
                                                   double* __restrict__ lam, double* __restrict__ V2) {
#pragma clang fp contract(off)
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const long b = i / N;
  const int k = kexp[b], e1 = syev_exp(mx[b]);
  if (k == SYEV_DIAG) {
    const double* h = H + (size_t)b * N * N;
    const int j = (int)(i - b * N);
    const double dj = h[(size_t)j * N + j];
    int rank = 0;
    for (int m = 0; m < N; ++m) { const double dm = h[(size_t)m * N + m]; rank += dm > dj || (dm == dj && m < j); }
    lam[b * N + rank] = ldexp(dj, e1);                        // rank < N: at most N - 1 others precede j
    if (V2) {
      double* row = V2 + ((size_t)b * N + rank) * N;          // row rank < N of member b < batch
      for (int m = 0; m < N; ++m) row[m] = m == j ? 1.0 : 0.0;
    }
    return;
  }
  const double s = sv[i];
  lam[i] = ldexp(s * s - cs[b], e1 - k);
}

// N = 1: lambda = s_00
__global__ __launch_bounds__(256) void syev_copy(const double* __restrict__ S, long total, double* __restrict__ lam) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i < total) lam[i] = S[i];
}

template <class T> int syev_alloc(nd4hip_handle* h, size_t count, T** out) {
  void* p = nullptr;
  ND4_TRY(nd4_ws_alloc(h, sizeof(T) * count, &p));
  *out = static_cast<T*>(p);
  return 0;
}

// HIP-event time per stage while the profile is enabled (the events cost a few us each: off otherwise)
struct SyevStamps {
  nd4hip_handle* h; bool on; int n = 0;
  hipEvent_t ev[ND4HIP_SYEV_STAGES + 1] = {};
  explicit SyevStamps(nd4hip_handle* hh) : h(hh), on(hh->prof_on) {}
  void mark() {
    if (!on || n > ND4HIP_SYEV_STAGES) return;
    if (hipEventCreate(&ev[n]) != hipSuccess) { on = false; return; }
    (void)hipEventRecord(ev[n++], h->stream);
  }
  void collect() {                                            // after the call's synchronisation
    for (int i = 0; i < ND4HIP_SYEV_STAGES; ++i) {
      float ms = 0.f;
      h->syev_stage_ms[i] = on && i + 1 < n && hipEventElapsedTime(&ms, ev[i], ev[i + 1]) == hipSuccess ? ms : 0.0;
    }
  }
  ~SyevStamps() { for (int i = 0; i < n; ++i) (void)hipEventDestroy(ev[i]); }
};

}  // namespace

// step 1, shared with syevx.hip (syev_internal.h)
int nd4_syev_symm(nd4hip_handle* h, int64_t batch, int N, const double* S, double* W, u64* mx) {
  const unsigned tiles = (unsigned)((N + SYEV_TILE - 1) / SYEV_TILE);
  hipLaunchKernelGGL(syev_absmax_lower, dim3((unsigned)(N < 256 ? N : 256), (unsigned)batch), dim3(256), 0, h->stream, S, N, mx);
  hipLaunchKernelGGL(syev_symm, dim3(tiles, tiles, (unsigned)batch), dim3(256), 0, h->stream, S, W, N, mx);
  ND4_HIP(hipGetLastError());
  return 0;
}

// S [batch, N, N] -> lambda [batch, N] descending, V [batch, N, N] (columns = eigenvectors) or V = NULL for the values alone.
// batch <= 32768 (the grids' z axis), 1 <= N <= 2048. Synchronises: the solver reads its flag word back, then this call its own.
int nd4_syevd(nd4hip_handle* h, int64_t batch, int64_t N64, const double* S, double* lambda, double* V) {
  ND4_CHECK_ARG(N64 <= SYEV_MAXN, "nd4hip_dsyevd_batched: the divide & conquer solver takes N <= %d", SYEV_MAXN);
  ND4_CHECK_ARG(batch <= 32768, "nd4hip_dsyevd_batched: batch %lld exceeds 32768 per call", (long long)batch);
  const int N = (int)N64;
  if (N == 1) {                                               // no solver call: lambda = s_00, V = 1
    hipLaunchKernelGGL(syev_copy, dim3((unsigned)((batch + 255) / 256)), dim3(256), 0, h->stream, S, (long)batch, lambda);
    ND4_HIP(hipGetLastError());
    if (V) ND4_TRY(nd4_set_identity(h, 1, 1, V, 1, batch, 1));
    return 0;
  }
  Nd4WsScope scope(h);
  const size_t nn = (size_t)N * N;
  u64* mx = nullptr; int *kexp = nullptr, *flag = nullptr;
  double *W, *U, *U2, *V2, *p, *q, *sv, *cs;
  ND4_TRY(syev_alloc(h, (size_t)batch, &mx)); ND4_TRY(syev_alloc(h, (size_t)batch, &kexp)); ND4_TRY(syev_alloc(h, 1, &flag));
  ND4_TRY(syev_alloc(h, (size_t)batch, &cs));
  ND4_TRY(syev_alloc(h, (size_t)batch * N, &p)); ND4_TRY(syev_alloc(h, (size_t)batch * N, &q)); ND4_TRY(syev_alloc(h, (size_t)batch * N, &sv));
  ND4_TRY(syev_alloc(h, (size_t)batch * nn, &W)); ND4_TRY(syev_alloc(h, (size_t)batch * nn, &U));
  ND4_TRY(syev_alloc(h, (size_t)batch * nn, &U2)); ND4_TRY(syev_alloc(h, (size_t)batch * nn, &V2));
  ND4_HIP(hipMemsetAsync(mx, 0, sizeof(u64) * (size_t)batch, h->stream));
  ND4_HIP(hipMemsetAsync(flag, 0, sizeof(int), h->stream));
  SyevStamps st(h);
  st.mark();
  ND4_TRY(nd4_syev_symm(h, batch, N, S, W, mx));
  st.mark();
  ND4_TRY(nd4_gehrd(h, batch, N, W, U, W));                   // in place: H overwrites W
  st.mark();
  hipLaunchKernelGGL(syev_shift_chol, dim3((unsigned)batch), dim3(64), 0, h->stream, W, N, mx, p, q, cs, kexp, flag);
  ND4_HIP(hipGetLastError());
  st.mark();
  ND4_TRY(nd4_bdsdc_rows(h, batch, N, N, p, q, U2, sv, V2));  // synchronises
  st.mark();
  const long total = (long)batch * N;
  hipLaunchKernelGGL(syev_values, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, h->stream, sv, W, N, total, cs, kexp, mx, lambda,
                     V ? V2 : nullptr);
  ND4_HIP(hipGetLastError());
  if (V) ND4_TRY(nd4_gemm(h, false, true, N, N, N, 1.0, U, N, (int64_t)nn, V2, N, (int64_t)nn, 0.0, V, N, (int64_t)nn, batch));
  st.mark();
  void* hp = nullptr;
  ND4_TRY(nd4_pinned(h, sizeof(int), &hp));
  int* host = static_cast<int*>(hp);
  ND4_HIP(hipMemcpyAsync(host, flag, sizeof(int), hipMemcpyDeviceToHost, h->stream));
  ND4_HIP(hipStreamSynchronize(h->stream));
  st.collect();
  if (host[0] != 0) {
    nd4_set_error("eigen_sym(S): S contains NaN or Infinity in its lower triangle.");
    return ND4HIP_ERR_NOCONV;
  }
  return 0;
}

namespace {
// reduction='tridiag' only, one wave per member, before step 3: an off-diagonal entry of T = tridiag(d, e) on the diagonals of F
// with |e_i| <= eps g, g = max_i(|d_i| + |e_i-1| + |e_i|) the Gershgorin bound, becomes zero. The perturbation is at most eps g per
// entry, inside the error of the route (a few eps g). Why: nd4_sytrd works from the top, so a rank-deficient S leaves its rounding
// noise (d, e ~ 1e-16 g) in the trailing rows of T, and on such a tail the divide & conquer solver's own assertion (svd_dc.js:206, a
// child's values out of order) fails for about one input in seven; with the noise cut off, T splits there and none does
// (DESIGN.md 4.21). NaN or Inf: every comparison is false and nothing is written; the entrance word mx has flagged the member.
__global__ __launch_bounds__(64) void syev_tr_deflate(double* __restrict__ F, int N) {
  double* f = F + (size_t)blockIdx.x * N * N;
  const int lane = threadIdx.x;
  double g = 0.0;
  for (int i = lane; i < N; i += 64) {
    const double em = i > 0 ? fabs(f[(size_t)i * N + i - 1]) : 0.0, ep = i + 1 < N ? fabs(f[(size_t)(i + 1) * N + i]) : 0.0;
    g = fmax(g, (fabs(f[(size_t)i * N + i]) + em) + ep);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) g = fmax(g, __shfl_xor(g, off));
  for (int i = lane; i + 1 < N; i += 64)                      // (every read of e above is done: the shuffles are a wave barrier)
    if (fabs(f[(size_t)(i + 1) * N + i]) <= DBL_EPSILON * g) f[(size_t)(i + 1) * N + i] = 0.0;
}
}  // namespace

// The same with reduction='tridiag' (DESIGN.md 4.21): nd4_sytrd (sytrd.hip) runs straight on the lower triangle of S, so there is no
// symmetrised copy and no U; its scaled d and e stand on the diagonals of F, where steps 3-5 above read them (after
// syev_tr_deflate, above). The vectors are V = Q V2^T by nd4_ormtr on the transposed rows of V2; for the values alone neither
// runs. The symmetrise stage reads 0.
int nd4_syevd_tr(nd4hip_handle* h, int64_t batch, int64_t N64, const double* S, double* lambda, double* V) {
  ND4_CHECK_ARG(N64 <= SYEV_MAXN, "nd4hip_dsyevd_tr_batched: the divide & conquer solver takes N <= %d", SYEV_MAXN);
  ND4_CHECK_ARG(batch <= 32768, "nd4hip_dsyevd_tr_batched: batch %lld exceeds 32768 per call", (long long)batch);
  if (N64 == 1) return nd4_syevd(h, batch, N64, S, lambda, V);
  const int N = (int)N64;
  Nd4WsScope scope(h);
  const size_t nn = (size_t)N * N;
  u64* mx = nullptr; int *kexp = nullptr, *flag = nullptr;
  double *F, *tau, *U2, *V2, *p, *q, *sv, *cs;
  ND4_TRY(syev_alloc(h, (size_t)batch, &mx)); ND4_TRY(syev_alloc(h, (size_t)batch, &kexp)); ND4_TRY(syev_alloc(h, 1, &flag));
  ND4_TRY(syev_alloc(h, (size_t)batch, &cs)); ND4_TRY(syev_alloc(h, (size_t)batch * N, &tau));
  ND4_TRY(syev_alloc(h, (size_t)batch * N, &p)); ND4_TRY(syev_alloc(h, (size_t)batch * N, &q)); ND4_TRY(syev_alloc(h, (size_t)batch * N, &sv));
  ND4_TRY(syev_alloc(h, (size_t)batch * nn, &F));
  ND4_TRY(syev_alloc(h, (size_t)batch * nn, &U2)); ND4_TRY(syev_alloc(h, (size_t)batch * nn, &V2));
  ND4_HIP(hipMemsetAsync(mx, 0, sizeof(u64) * (size_t)batch, h->stream));
  ND4_HIP(hipMemsetAsync(flag, 0, sizeof(int), h->stream));
  SyevStamps st(h);
  st.mark(); st.mark();                                       // no symmetrisation
  ND4_TRY(nd4_sytrd(h, batch, N, S, F, tau, nullptr, nullptr, mx, false, flag));
  hipLaunchKernelGGL(syev_tr_deflate, dim3((unsigned)batch), dim3(64), 0, h->stream, F, N);
  st.mark();
  hipLaunchKernelGGL(syev_shift_chol, dim3((unsigned)batch), dim3(64), 0, h->stream, F, N, mx, p, q, cs, kexp, flag);
  ND4_HIP(hipGetLastError());
  st.mark();
  ND4_TRY(nd4_bdsdc_rows(h, batch, N, N, p, q, U2, sv, V2));  // synchronises
  st.mark();
  const long total = (long)batch * N;
  hipLaunchKernelGGL(syev_values, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, h->stream, sv, F, N, total, cs, kexp, mx, lambda,
                     V ? V2 : nullptr);
  ND4_HIP(hipGetLastError());
  if (V) {
    ND4_TRY(nd4_transpose(h, N, N, V2, N, V, N, batch, (int64_t)nn, (int64_t)nn));
    ND4_TRY(nd4_ormtr(h, batch, N, N, false, F, tau, V));
  }
  st.mark();
  void* hp = nullptr;
  ND4_TRY(nd4_pinned(h, sizeof(int), &hp));
  int* host = static_cast<int*>(hp);
  ND4_HIP(hipMemcpyAsync(host, flag, sizeof(int), hipMemcpyDeviceToHost, h->stream));
  ND4_HIP(hipStreamSynchronize(h->stream));
  st.collect();
  h->syev_stage_ms[0] = 0.0;                                  // (the time between two event records, not a stage)
  if (host[0] != 0) {
    nd4_set_error("eigen_sym(S): S contains NaN or Infinity in its lower triangle.");
    return ND4HIP_ERR_NOCONV;
  }
  return 0;
}

// eigen_herm / eigenvals_herm: the route of nd4_syevd_tr for a Hermitian H [batch, N, N] (complex128 as interleaved
// doubles). nd4_hetrd (hetrd.hip) leaves the real scaled d and e on the diagonals of the complex F; hetrd_diagonals copies them to
// the diagonals of a real N x N array, the layout steps 3-5 above read, so those kernels run unchanged. The vectors are
// V = Q V2^T: the rows of V2 transposed into the complex V, then nd4_zunmtr; for the values alone neither runs. lambda [batch, N]
// real descending, V [batch, N, N] complex (columns) or NULL. The symmetrise stage reads 0. Synchronises.
int nd4_zheevd(nd4hip_handle* h, int64_t batch, int64_t N64, const double* H, double* lambda, double* V) {
  ND4_CHECK_ARG(N64 >= 1 && N64 <= SYEV_MAXN, "nd4hip_zheevd_batched: the divide & conquer solver takes N <= %d", SYEV_MAXN);
  ND4_CHECK_ARG(batch <= 32768, "nd4hip_zheevd_batched: batch %lld exceeds 32768 per call", (long long)batch);
  if (N64 == 1) return nd4_hetrd_order_one(h, batch, H, lambda, V);
  const int N = (int)N64;
  Nd4WsScope scope(h);
  const size_t nn = (size_t)N * N;
  u64* mx = nullptr; int *kexp = nullptr, *flag = nullptr;
  double *F, *Tr, *tau, *U2, *V2, *p, *q, *sv, *cs;
  ND4_TRY(syev_alloc(h, (size_t)batch, &mx)); ND4_TRY(syev_alloc(h, (size_t)batch, &kexp)); ND4_TRY(syev_alloc(h, 1, &flag));
  ND4_TRY(syev_alloc(h, (size_t)batch, &cs)); ND4_TRY(syev_alloc(h, 2 * (size_t)batch * N, &tau));
  ND4_TRY(syev_alloc(h, (size_t)batch * N, &p)); ND4_TRY(syev_alloc(h, (size_t)batch * N, &q)); ND4_TRY(syev_alloc(h, (size_t)batch * N, &sv));
  ND4_TRY(syev_alloc(h, 2 * (size_t)batch * nn, &F)); ND4_TRY(syev_alloc(h, (size_t)batch * nn, &Tr));
  ND4_TRY(syev_alloc(h, (size_t)batch * nn, &U2)); ND4_TRY(syev_alloc(h, (size_t)batch * nn, &V2));
  ND4_HIP(hipMemsetAsync(mx, 0, sizeof(u64) * (size_t)batch, h->stream));
  ND4_HIP(hipMemsetAsync(flag, 0, sizeof(int), h->stream));
  SyevStamps st(h);
  st.mark(); st.mark();                                       // no symmetrisation
  ND4_TRY(nd4_hetrd(h, batch, N, H, F, tau, nullptr, nullptr, mx, false, flag));
  ND4_TRY(nd4_hetrd_diagonals(h, batch, N, F, Tr));
  hipLaunchKernelGGL(syev_tr_deflate, dim3((unsigned)batch), dim3(64), 0, h->stream, Tr, N);
  st.mark();
  hipLaunchKernelGGL(syev_shift_chol, dim3((unsigned)batch), dim3(64), 0, h->stream, Tr, N, mx, p, q, cs, kexp, flag);
  ND4_HIP(hipGetLastError());
  st.mark();
  ND4_TRY(nd4_bdsdc_rows(h, batch, N, N, p, q, U2, sv, V2));  // synchronises
  st.mark();
  const long total = (long)batch * N;
  hipLaunchKernelGGL(syev_values, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, h->stream, sv, Tr, N, total, cs, kexp, mx, lambda,
                     V ? V2 : nullptr);
  ND4_HIP(hipGetLastError());
  if (V) {
    ND4_TRY(nd4_hetrd_rows_to_columns(h, batch, N, N, V2, V));
    ND4_TRY(nd4_zunmtr(h, batch, N, N, false, F, tau, V));
  }
  st.mark();
  void* hp = nullptr;
  ND4_TRY(nd4_pinned(h, sizeof(int), &hp));
  int* host = static_cast<int*>(hp);
  ND4_HIP(hipMemcpyAsync(host, flag, sizeof(int), hipMemcpyDeviceToHost, h->stream));
  ND4_HIP(hipStreamSynchronize(h->stream));
  st.collect();
  h->syev_stage_ms[0] = 0.0;                                  // (the time between two event records, not a stage)
  if (host[0] != 0) {
    nd4_set_error("eigen_herm(H): H contains NaN or Infinity in its lower triangle.");
    return ND4HIP_ERR_NOCONV;
  }
  return 0;
}
