// Determinants and the Frobenius norm (src/la/det.js, src/la/norm.js) for gfx950.
//
//   det_tri / slogdet_tri (det.js:24-92): the diagonal's product / (sign product, log-sum) in index order. N <= DT_LANE_MAX: one
//       lane per matrix; larger N: one wave per matrix, whose lanes load and take the logs of 64 diagonal entries at a time, and
//       lane 0 multiplies / adds them in index order. A tree would change where the product overflows or underflows; the order
//       decides that bit for bit.
//   det / slogdet, square N <= 64 (det.js:95-106 = qr_decomp_full's elimination, qr.js:44-69, then det_tri): a Givens QR that
//       writes neither R nor Q, in the reference's operation order: blocked loops J, I, i, j with B = 8, the `0 === R_ij` and
//       `0 === s` skips, _giv_rot_qr and _giv_rot_rows (_giv_rot.js:22-37, :42-66). No contraction, and f64 `/` and `sqrt` are
//       correctly rounded on gfx950, so every operation is the reference's own.
//         N <= 8       : one lane per matrix, the matrix in registers with static indices only (template on N, fully unrolled;
//                        for N <= B the blocked order is the plain row order).
//         9 <= N <= 64 : one wave per matrix, the matrix in LDS; lane k owns column k, so a row rotation is one LDS
//                        read-modify-write per lane, and every lane computes c, s from two broadcast reads.
//       The reference's _giv_rot_qr asserts `0 <= norm` and throws 'Assertion failed: NaN' when a rotation meets NaN or
//       Infinity. Such a matrix gets DET_ASSERT_NAN (a NaN with its own payload) as its det / sign; the host forms turn it into
//       that error.
//   det / slogdet, N > 64 and every tall input: the R-only mode of nd4_geqrf_q_ex (qr_decomp's R with its sign convention, Q
//       never formed) into a workspace, then det_tri's kernel on its diagonal (nd4hip_api.hip).
//   norm 'fro' (norm.js:22-85): (2^e, s) pairs with s = sum (x / 2^e)^2, per workgroup over a fixed contiguous range, then one
//       ordered merge s = s1 (m1/m)^2 + s2 (m2/m)^2 with m = max(m1, m2). Powers of two make every rescaling exact, so 1e300
//       entries do not overflow and 1e-300 entries do not underflow. The grid depends on the size alone: two runs give the same
//       bits. Any Infinity gives +Infinity, otherwise any NaN gives NaN (norm.js:34-62).
#include "nd4hip_internal.h"
#include <cmath>

namespace {

constexpr int DT_LANE_MAX = 32;       // det_tri: one lane per matrix up to here, one wave per matrix beyond
constexpr int WAVE = 64;
constexpr int NRM_THREADS = 256;
constexpr int NRM_UNROLL = 8;         // elements per thread and step (coalesced: element k * 256 + tid of a 2048-element step)
constexpr int NRM_MAX_WG = 1024;

#pragma clang fp contract(off)

__device__ inline double js_sign(double x) { return x > 0.0 ? 1.0 : x < 0.0 ? -1.0 : x; }   // Math.sign: +-0 and NaN as they are
__device__ inline double js_max(double a, double b) { return (a != a || b != b) ? __longlong_as_double(0x7ff8000000000000ll) : (a < b ? b : a); }
__device__ inline double det_assert_nan() { return __longlong_as_double((long long)ND4HIP_DET_ASSERT_NAN_BITS); }

// _giv_rot_qr (_giv_rot.js:22-37): [c, s, norm]; false where the reference's assertion `0 <= norm` fails
__device__ inline bool giv_rot_qr(double a_ii, double a_ji, double& c, double& s, double& nrm) {
  const double mx = js_max(fabs(a_ii), fabs(a_ji));
  if (mx == 0.0) { c = 1.0; s = 0.0; nrm = 0.0; return true; }
  a_ii /= mx;
  a_ji /= mx;
  nrm = sqrt(a_ii * a_ii + a_ji * a_ji);
  c = a_ii / nrm;
  s = a_ji / nrm;
  nrm *= mx;
  return 0.0 <= nrm;
}

// ------------------------------------------------------------------------------------------------ det_tri / slogdet_tri
template <bool LOG>
__global__ __launch_bounds__(256) void det_tri_lane(int64_t batch, int N, const double* __restrict__ A, long sA, double* __restrict__ D,
                                                    double* __restrict__ L) {
  const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= batch) return;
  const double* a = A + b * sA;
  double d = 1.0, l = 0.0;
  for (int i = 0; i < N; i++) {
    const double x = a[(long)i * (N + 1)];
    if (LOG) { d *= js_sign(x); l += log(fabs(x)); }
    else d *= x;
  }
  D[b] = d;
  if (LOG) L[b] = l;
}

template <bool LOG>
__global__ __launch_bounds__(WAVE) void det_tri_wave(int N, const double* __restrict__ A, long sA, double* __restrict__ D,
                                                     double* __restrict__ L) {
  __shared__ double xs[WAVE], ls[WAVE];
  const int64_t b = blockIdx.x;
  const int lane = threadIdx.x;
  const double* a = A + b * sA;
  double d = 1.0, l = 0.0;                                  // lane 0's running product / log-sum
  for (int i0 = 0; i0 < N; i0 += WAVE) {
    const int i = i0 + lane, n = N - i0 < WAVE ? N - i0 : WAVE;
    if (i < N) {
      const double x = a[(long)i * (N + 1)];
      xs[lane] = LOG ? js_sign(x) : x;
      if (LOG) ls[lane] = log(fabs(x));
    }
    __syncthreads();
    if (lane == 0)
      for (int k = 0; k < n; k++) { d *= xs[k]; if (LOG) l += ls[k]; }
    __syncthreads();
  }
  if (lane == 0) { D[b] = d; if (LOG) L[b] = l; }
}

// ------------------------------------------------------------------------------------------------ det, N <= 8: a lane per matrix
template <int N, bool LOG>
__global__ __launch_bounds__(256) void det_givens_lane(int64_t batch, const double* __restrict__ A, double* __restrict__ D,
                                                       double* __restrict__ L) {
  const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= batch) return;
  double r[N * N > 0 ? N * N : 1];
  const double* a = A + b * (N * N);
#pragma unroll
  for (int k = 0; k < N * N; k++) r[k] = a[k];
  bool ok = true;
#pragma unroll
  for (int i = 1; i < N; i++) {
#pragma unroll
    for (int j = 0; j < i; j++) {
      const double rij = r[i * N + j];
      if (rij == 0.0) continue;
      double c, s, nrm;
      ok &= giv_rot_qr(r[j * N + j], rij, c, s, nrm);
      r[i * N + j] = 0.0;
      if (s == 0.0) continue;
      r[j * N + j] = nrm;
#pragma unroll
      for (int k = j + 1; k < N; k++) {
        const double wi = r[j * N + k], wj = r[i * N + k];
        r[j * N + k] = c * wi + s * wj;
        r[i * N + k] = c * wj - s * wi;
      }
    }
  }
  double d = 1.0, l = 0.0;
#pragma unroll
  for (int i = 0; i < N; i++) {
    if (LOG) { d *= js_sign(r[i * N + i]); l += log(fabs(r[i * N + i])); }
    else d *= r[i * N + i];
  }
  D[b] = ok ? d : det_assert_nan();
  if (LOG) L[b] = ok ? l : det_assert_nan();
}

// ------------------------------------------------------------------------------------------------ det, 9 <= N <= 64: a wave per matrix
template <bool LOG>
__global__ __launch_bounds__(WAVE) void det_givens_wave(int N, const double* __restrict__ A, double* __restrict__ D, double* __restrict__ L) {
  extern __shared__ double R[];                              // N x N, row-major
  const int64_t b = blockIdx.x;
  const int k = threadIdx.x;                                 // this lane's column
  const double* a = A + b * (long)N * N;
  for (int e = k; e < N * N; e += WAVE) R[e] = a[e];
  __syncthreads();
  constexpr int B = 8;                                       // qr.js:34 (float64)
  bool ok = true;
  for (int J = 0; J < N; J += B)
    for (int I = J; I < N; I += B)
      for (int i = I; i < I + B && i < N; i++)
        for (int j = J; j < J + B && j < N && j < i; j++) {
          const double rij = R[i * N + j];                    // broadcast reads: every lane takes the same decisions
          if (rij == 0.0) continue;
          const double rjj = R[j * N + j];
          double c, s, nrm;
          ok &= giv_rot_qr(rjj, rij, c, s, nrm);
          double wi = 0.0, wj = 0.0;
          if (k > j && k < N) { wi = R[j * N + k]; wj = R[i * N + k]; }
          __syncthreads();                                    // every lane has read R_ij, R_jj before they change
          if (k == 0) R[i * N + j] = 0.0;
          if (s != 0.0) {
            if (k == 0) R[j * N + j] = nrm;
            if (k > j && k < N) { R[j * N + k] = c * wi + s * wj; R[i * N + k] = c * wj - s * wi; }
          }
          __syncthreads();
        }
  if (k == 0) {
    double d = 1.0, l = 0.0;
    for (int i = 0; i < N; i++) {
      const double x = R[i * N + i];
      if (LOG) { d *= js_sign(x); l += log(fabs(x)); }
      else d *= x;
    }
    D[b] = ok ? d : det_assert_nan();
    if (LOG) L[b] = ok ? l : det_assert_nan();
  }
}

// ------------------------------------------------------------------------------------------------ norm 'fro'
struct NrmPair { int e; double s; int flags; };              // sum (x / 2^e)^2; flags: 1 = Infinity seen, 2 = NaN seen

__device__ inline void nrm_merge(NrmPair& p, const NrmPair& q) {
  p.flags |= q.flags;
  if (q.s == 0.0) return;
  if (p.s == 0.0) { p.e = q.e; p.s = q.s; return; }
  const int e = p.e > q.e ? p.e : q.e;
  p.s = ldexp(p.s, 2 * (p.e - e)) + ldexp(q.s, 2 * (q.e - e));
  p.e = e;
}

// per-thread pairs over its fixed elements, then a fixed tree over the workgroup; grid-stride over 2048-element steps
__device__ inline NrmPair nrm_block(NrmPair p, NrmPair* sh) {
  const int t = threadIdx.x;
  sh[t] = p;
  __syncthreads();
  for (int w = NRM_THREADS / 2; w > 0; w >>= 1) {
    if (t < w) { NrmPair x = sh[t]; nrm_merge(x, sh[t + w]); sh[t] = x; }
    __syncthreads();
  }
  return sh[0];
}

__global__ __launch_bounds__(NRM_THREADS) void nrm_partial(int64_t n, int64_t steps_per_wg, const double* __restrict__ A,
                                                           int* __restrict__ Pe, double* __restrict__ Ps, int* __restrict__ Pf) {
  __shared__ NrmPair sh[NRM_THREADS];
  NrmPair p{0, 0.0, 0};
  const int64_t step0 = (int64_t)blockIdx.x * steps_per_wg;
  for (int64_t st = step0; st < step0 + steps_per_wg; st++) {
    const int64_t base = st * (NRM_THREADS * NRM_UNROLL) + threadIdx.x;
    if (base >= n) break;
    double x[NRM_UNROLL];
#pragma unroll
    for (int u = 0; u < NRM_UNROLL; u++) { const int64_t i = base + (int64_t)u * NRM_THREADS; x[u] = i < n ? fabs(A[i]) : 0.0; }
    double m = 0.0;
#pragma unroll
    for (int u = 0; u < NRM_UNROLL; u++) {
      if (x[u] != x[u]) { p.flags |= 2; x[u] = 0.0; }
      else if (x[u] > 1.79769313486231570e308) { p.flags |= 1; x[u] = 0.0; }
      m = x[u] > m ? x[u] : m;
    }
    if (m == 0.0) continue;
    NrmPair q{ilogb(m), 0.0, 0};
#pragma unroll
    for (int u = 0; u < NRM_UNROLL; u++) { const double y = ldexp(x[u], -q.e); q.s += y * y; }
    nrm_merge(p, q);
  }
  const NrmPair r = nrm_block(p, sh);
  if (threadIdx.x == 0) { Pe[blockIdx.x] = r.e; Ps[blockIdx.x] = r.s; Pf[blockIdx.x] = r.flags; }
}

__global__ __launch_bounds__(NRM_THREADS) void nrm_final(int nwg, const int* __restrict__ Pe, const double* __restrict__ Ps,
                                                         const int* __restrict__ Pf, double* __restrict__ out) {
  __shared__ NrmPair sh[NRM_THREADS];
  NrmPair p{0, 0.0, 0};
  for (int w = threadIdx.x; w < nwg; w += NRM_THREADS) nrm_merge(p, NrmPair{Pe[w], Ps[w], Pf[w]});
  const NrmPair r = nrm_block(p, sh);
  if (threadIdx.x == 0)
    *out = (r.flags & 1) ? __longlong_as_double(0x7ff0000000000000ll) : (r.flags & 2) ? __longlong_as_double(0x7ff8000000000000ll)
         : r.s == 0.0 ? 0.0 : ldexp(sqrt(r.s), r.e);
}

template <bool LOG>
int launch_givens_small(nd4hip_handle* h, int64_t batch, int N, const double* A, double* D, double* L) {
  const dim3 g((unsigned)((batch + 255) / 256)), t(256);
  switch (N) {
    case 0: hipLaunchKernelGGL((det_givens_lane<0, LOG>), g, t, 0, h->stream, batch, A, D, L); break;
    case 1: hipLaunchKernelGGL((det_givens_lane<1, LOG>), g, t, 0, h->stream, batch, A, D, L); break;
    case 2: hipLaunchKernelGGL((det_givens_lane<2, LOG>), g, t, 0, h->stream, batch, A, D, L); break;
    case 3: hipLaunchKernelGGL((det_givens_lane<3, LOG>), g, t, 0, h->stream, batch, A, D, L); break;
    case 4: hipLaunchKernelGGL((det_givens_lane<4, LOG>), g, t, 0, h->stream, batch, A, D, L); break;
    case 5: hipLaunchKernelGGL((det_givens_lane<5, LOG>), g, t, 0, h->stream, batch, A, D, L); break;
    case 6: hipLaunchKernelGGL((det_givens_lane<6, LOG>), g, t, 0, h->stream, batch, A, D, L); break;
    case 7: hipLaunchKernelGGL((det_givens_lane<7, LOG>), g, t, 0, h->stream, batch, A, D, L); break;
    case 8: hipLaunchKernelGGL((det_givens_lane<8, LOG>), g, t, 0, h->stream, batch, A, D, L); break;
    default: hipLaunchKernelGGL((det_givens_wave<LOG>), dim3((unsigned)batch), dim3(WAVE), sizeof(double) * N * N, h->stream, N, A, D, L);
  }
  ND4_HIP(hipGetLastError());
  return 0;
}

}  // namespace

// the diagonal rule of det_tri / slogdet_tri on [batch] matrices of stride sA (elements); batch <= 65535 for N > DT_LANE_MAX
int nd4_dettri(nd4hip_handle* h, bool log_form, int64_t batch, int64_t N, const double* A, int64_t sA, double* D, double* L) {
  if (batch == 0) return 0;
  if (N <= DT_LANE_MAX) {
    const dim3 g((unsigned)((batch + 255) / 256));
    if (log_form) hipLaunchKernelGGL(det_tri_lane<true>, g, dim3(256), 0, h->stream, batch, (int)N, A, (long)sA, D, L);
    else          hipLaunchKernelGGL(det_tri_lane<false>, g, dim3(256), 0, h->stream, batch, (int)N, A, (long)sA, D, L);
  } else {
    if (log_form) hipLaunchKernelGGL(det_tri_wave<true>, dim3((unsigned)batch), dim3(WAVE), 0, h->stream, (int)N, A, (long)sA, D, L);
    else          hipLaunchKernelGGL(det_tri_wave<false>, dim3((unsigned)batch), dim3(WAVE), 0, h->stream, (int)N, A, (long)sA, D, L);
  }
  ND4_HIP(hipGetLastError());
  return 0;
}

// det / slogdet of [batch] matrices M x N (M >= N; batch <= 65535): the Givens tiers for square N <= 64 (unless force_qr), otherwise
// the R-only QR into a workspace and the diagonal rule on it
int nd4_det(nd4hip_handle* h, bool log_form, int64_t batch, int64_t M, int64_t N, const double* A, double* D, double* L, bool force_qr) {
  if (batch == 0) return 0;
  if (M == N && N <= 64 && !(force_qr && N > 0))
    return log_form ? launch_givens_small<true>(h, batch, (int)N, A, D, L) : launch_givens_small<false>(h, batch, (int)N, A, D, L);
  Nd4WsScope scope(h);
  void* p = nullptr;
  ND4_TRY(nd4_ws_alloc(h, sizeof(double) * (size_t)batch * N * N + 64, &p));
  double* R = static_cast<double*>(p);
  ND4_TRY(nd4_geqrf_q_ex(h, batch, M, N, A, nullptr, R, false));
  return nd4_dettri(h, log_form, batch, N, R, N * N, D, L);
}

// norm(A) 'fro' of n elements into out (device); n > 0
int nd4_nrmfro(nd4hip_handle* h, int64_t n, const double* A, double* out) {
  const int64_t steps = (n + NRM_THREADS * NRM_UNROLL - 1) / (NRM_THREADS * NRM_UNROLL);
  const int64_t per = (steps + NRM_MAX_WG - 1) / NRM_MAX_WG;
  const int nwg = (int)((steps + per - 1) / per);
  Nd4WsScope scope(h);
  void* p = nullptr;
  ND4_TRY(nd4_ws_alloc(h, (sizeof(double) + 2 * sizeof(int)) * (size_t)nwg + 64, &p));
  double* Ps = static_cast<double*>(p);
  int* Pe = reinterpret_cast<int*>(Ps + nwg);
  int* Pf = Pe + nwg;
  hipLaunchKernelGGL(nrm_partial, dim3((unsigned)nwg), dim3(NRM_THREADS), 0, h->stream, n, per, A, Pe, Ps, Pf);
  hipLaunchKernelGGL(nrm_final, dim3(1), dim3(NRM_THREADS), 0, h->stream, nwg, Pe, Ps, Pf, out);
  ND4_HIP(hipGetLastError());
  return 0;
}
