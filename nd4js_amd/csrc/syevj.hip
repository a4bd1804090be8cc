// eigen_sym / eigenvals_sym, algo = 'jacobi': cyclic two-sided Jacobi for stacks of small symmetric matrices (1 <= N <= 128),
// every member solved inside ONE launch. The default route (syev.hip) tridiagonalises, which costs a launch per
// reduction step and per solver level and loses the relative accuracy of small eigenvalues (lambda = sv^2 - c cancels). Here
//   1. the lower triangle of the member is read, checked for NaN / Inf, mirrored and scaled by the exact power of two that puts
//      max|s_ij| into [2^511, 2^512) (denormal input becomes normal; nothing in the iteration squares an entry, so nothing can
//      overflow). The upper triangle of S is never read, S is never written.
//   2. a sweep is the round-robin tournament over all pairs (nd4_rr_pair, p < q; odd N: the pair with index N is the bye). The
//      rotations of one round are disjoint. Pair (p, q) is rotated iff
//          s_pq != 0  and  |s_pq| > (eps sqrt|s_pp|) sqrt|s_qq|,   eps = 2^-52
//      (two square roots: their product cannot underflow). This RELATIVE rule is what gives every eigenvalue of a positive definite
//      S its own relative accuracy (Demmel & Veselic 1992): with A = D^-1 S D^-1, D = diag(sqrt s_ii),
//          |lambda^ - lambda| <= N eps kappa_2(A) lambda     for every eigenvalue,
//      however small lambda is against ||S||. There is no absolute threshold beside it.
//   3. the rotation (Rutishauser): theta = (s_qq - s_pp) / (2 s_pq), t = sign(theta) / (|theta| + sqrt(1 + theta^2)) (the smaller
//      root; theta^2 overflowing: t = 1 / (2 theta); theta = 0: t = 1), c = 1 / sqrt(1 + t^2), s = t c, tau = s / (1 + c);
//          s_pp -= t s_pq,  s_qq += t s_pq,  s_pq = 0 exactly,
//          x_p' = x_p - s (x_q + tau x_p),  x_q' = x_q + s (x_p - tau x_q)      for rows, columns and the rows of V^T:
//      1 - c = s tau is carried exactly, so the rotation stays orthogonal when c rounds to 1 (as jac_small, svd.hip).
//   4. one round = phase A (one thread per pair: the criterion, the rotation, the pair's own 2 x 2 block) | barrier | phase B (one
//      thread per 2 x 2 block (k, l), k > l, of the round's pairs: the row rotation of pair k, then the column rotation of pair l;
//      the result is written to (k, l) and mirrored to (l, k), so S stays exactly symmetric; and the rows p, q of V^T) | barrier.
//      There are no reductions in the arithmetic and the file is compiled without FMA contraction: every multiplication and
//      addition is rounded on its own, and tests/eigsym_jacobi_common.py restates the arithmetic in numpy, bit for bit.
//   5. a member is finished after a sweep that rotates nothing (cap: 60 sweeps, svd.hip's MAX_SWEEPS). lambda = the diagonal,
//      sorted descending (ties: ascending position), scaled back with ldexp; V follows the same permutation.
// Tiers, by shape alone: N <= 32 one wave per member, four members per workgroup (no workgroup barrier anywhere: the waves finish
// at different sweeps); 32 < N <= 64 one workgroup of 512 per member, S and V^T in LDS; 64 < N <= 128 one workgroup of 1024, S in
// LDS (150 KB), V^T in global memory. LDS rows have the odd pitch n2 + 1. No kernel waits on another workgroup; every loop is
// bounded by 60 (N + 1) rounds.
#include "nd4hip_internal.h"
#include "svd_internal.h"
#include <cfloat>
#include <cmath>

namespace {

typedef unsigned long long u64;

constexpr int SYEVJ_MAXN = 128;
constexpr int SYEVJ_MAX_SWEEPS = 60;       // svd.hip's MAX_SWEEPS
constexpr int SYEVJ_EXP = 512;             // max|s_ij| is scaled into [2^511, 2^512)
constexpr u64 SYEVJ_INF_BITS = 0x7FF0000000000000ull;

// where the pieces of one member lie in its LDS block (bytes); the same function sizes the launch
struct SyevjLayout {
  int n2, nb, LD, nblk;
  size_t off_v, off_sn, off_tau, off_mx, off_pair, off_blk, off_inv, off_ctl, bytes;
};
__host__ __device__ inline SyevjLayout syevj_layout(int N, bool v_in_lds) {
  SyevjLayout L;
  L.n2 = (N + 1) & ~1; L.nb = L.n2 / 2; L.LD = L.n2 + 1; L.nblk = L.nb * (L.nb - 1) / 2;
  size_t o = sizeof(double) * (size_t)L.n2 * L.LD;                 // S: n2 rows (odd N: a zero row and column for the bye)
  L.off_v = o;    o += v_in_lds ? sizeof(double) * (size_t)N * L.LD : 0;   // V^T: N rows
  L.off_sn = o;   o += sizeof(double) * L.nb;                      // s and tau of the round's pairs (s = 0: not rotated)
  L.off_tau = o;  o += sizeof(double) * L.nb;
  L.off_mx = o;   o += sizeof(u64);                                // bits of max|s_ij|
  L.off_pair = o; o += sizeof(unsigned short) * (size_t)(L.n2 - 1) * L.nb;   // the tournament: p | q << 8 per (round, slot)
  L.off_blk = o;  o += sizeof(unsigned short) * (size_t)L.nblk;    // the blocks k > l: k | l << 8
  L.off_inv = o;  o += sizeof(unsigned short) * (size_t)L.n2;      // position of the eigenvalue of each rank
  o = (o + 3) & ~(size_t)3;
  L.off_ctl = o;  o += sizeof(int);                                // "this sweep rotated"
  L.bytes = (o + 15) & ~(size_t)15;
  return L;
}

// all threads of a member meet here. One wave per member: the wave's LDS operations execute in order, so only the compiler has
// to be kept from moving them; a workgroup barrier would hang, the waves of a workgroup leave the sweep loop at different times
template <int T> __device__ __forceinline__ void syevj_sync() {
  if (T == 64) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  } else {
    __syncthreads();
  }
}

// T threads per member (64: one wave, four members per workgroup). VLDS: V^T lives in LDS, else in Vws [batch, N, N].
// V = NULL: the values alone, no V^T anywhere. flag: bit 0 = NaN / Inf in a lower triangle, bit 1 = a member hit the cap.
template <int T, bool VLDS>
__global__ __launch_bounds__(T == 64 ? 256 : T) void syevj_kernel(const double* __restrict__ S, int N, long batch, double* __restrict__ lam,
                                                                    double* __restrict__ V, double* __restrict__ Vws,
                                                                    int32_t* __restrict__ sweeps_out, int* __restrict__ flag, int max_sweeps) {
  static_assert(T == 64 || T == 512 || T == 1024, "one instantiation per tier");
  extern __shared__ __align__(16) unsigned char syevj_smem[];
  constexpr int MPW = T == 64 ? 4 : 1;
  const int t = threadIdx.x % T;
  const long mat = (long)blockIdx.x * MPW + threadIdx.x / T;
  if (mat >= batch) return;                                        // (whole waves of the last workgroup; no barrier follows for them)
  const bool vec = V != nullptr;
  const SyevjLayout L = syevj_layout(N, VLDS && vec);
  unsigned char* base = syevj_smem + (size_t)(threadIdx.x / T) * L.bytes;
  double* a = reinterpret_cast<double*>(base);
  double* vl = reinterpret_cast<double*>(base + L.off_v);
  double* s_sn = reinterpret_cast<double*>(base + L.off_sn);
  double* s_tau = reinterpret_cast<double*>(base + L.off_tau);
  u64* s_mx = reinterpret_cast<u64*>(base + L.off_mx);
  unsigned short* s_pair = reinterpret_cast<unsigned short*>(base + L.off_pair);
  unsigned short* s_blk = reinterpret_cast<unsigned short*>(base + L.off_blk);
  unsigned short* s_inv = reinterpret_cast<unsigned short*>(base + L.off_inv);
  int* s_ctl = reinterpret_cast<int*>(base + L.off_ctl);
  double* vg = Vws ? Vws + (size_t)mat * N * N : nullptr;          // (NULL when VLDS or !vec)
  const int n2 = L.n2, nb = L.nb, LD = L.LD, nblk = L.nblk, NN = N * N;
  const int ldv = VLDS ? LD : N;
  const double* s = S + (size_t)mat * NN;

  // ---- 1. load the lower triangle, max|s_ij|, tables
  if (t == 0) { *s_mx = 0; *s_ctl = 0; }
  syevj_sync<T>();
  u64 m = 0;
  for (int e = t; e < NN; e += T) {
    const int r = e / N, c = e - r * N;
    if (c <= r) {
      const double x = s[e];
      a[r * LD + c] = x;
      const u64 b = (u64)__double_as_longlong(fabs(x));           // the bits of |x| order like |x|; NaN above Inf
      m = b > m ? b : m;
    }
  }
  if (m) atomicMax(s_mx, m);
  for (int e = t; e < (n2 - 1) * nb; e += T) {
    int p, q;
    nd4_rr_pair(n2, e / nb, e % nb, p, q);
    s_pair[e] = (unsigned short)(p | (q << 8));                   // p < q <= 127
  }
  for (int k = 1 + t; k < nb; k += T)
    for (int l = 0; l < k; ++l) s_blk[k * (k - 1) / 2 + l] = (unsigned short)(k | (l << 8));
  syevj_sync<T>();
  const u64 mx = *s_mx;
  if (mx >= SYEVJ_INF_BITS) {                                      // uniform over the member: nothing is written for it
    if (t == 0) { atomicOr(flag, 1); if (sweeps_out) sweeps_out[mat] = 0; }
    return;
  }
  int sc = 0;
  if (mx) { int e1; (void)frexp(__longlong_as_double((long long)mx), &e1); sc = SYEVJ_EXP - e1; }
  for (int e = t; e < NN; e += T) {                                // (each thread rescales and mirrors what it stored itself)
    const int r = e / N, c = e - r * N;
    if (c <= r) { const double x = ldexp(a[r * LD + c], sc); a[r * LD + c] = x; a[c * LD + r] = x; }
    if (vec) {
      if (VLDS) vl[r * LD + c] = r == c ? 1.0 : 0.0; else vg[e] = r == c ? 1.0 : 0.0;
    }
  }
  if (n2 > N) for (int i = t; i < n2; i += T) { a[N * LD + i] = 0.0; a[i * LD + N] = 0.0; }
  syevj_sync<T>();

  // ---- 2.-4. sweeps
  int sweeps = 0;
  bool done = false;
  while (!done && sweeps < max_sweeps) {
    int my_rot = 0;
    for (int step = 0; step < n2 - 1; ++step) {
      const unsigned short* pairs = s_pair + step * nb;
      if (t < nb) {                                                // phase A: the pair's criterion, rotation and own 2 x 2 block
        const int p = pairs[t] & 255, q = pairs[t] >> 8;
        const double app = a[p * LD + p], aqq = a[q * LD + q], apq = a[q * LD + p];
        double sn = 0.0, tau = 0.0;
        if (apq != 0.0 && fabs(apq) > (0x1p-52 * sqrt(fabs(app))) * sqrt(fabs(aqq))) {
          const double theta = (aqq - app) / (2.0 * apq);
          const double at = fabs(theta), t2 = at * at;
          double tt = t2 <= DBL_MAX ? 1.0 / (at + sqrt(1.0 + t2)) : 0.5 / at;
          tt = copysign(tt, theta);
          const double c = 1.0 / sqrt(1.0 + tt * tt);
          sn = tt * c;
          tau = sn / (1.0 + c);
          const double hh = tt * apq;
          a[p * LD + p] = app - hh; a[q * LD + q] = aqq + hh;
          a[q * LD + p] = 0.0; a[p * LD + q] = 0.0;
          my_rot = 1;
        }
        s_sn[t] = sn; s_tau[t] = tau;
      }
      syevj_sync<T>();
      for (int idx = t; idx < nblk; idx += T) {                    // phase B: block (k, l), k > l
        const int k = s_blk[idx] & 255, l = s_blk[idx] >> 8;
        const double sk = s_sn[k], sl = s_sn[l];
        if (sk == 0.0 && sl == 0.0) continue;
        const int pk = pairs[k] & 255, qk = pairs[k] >> 8, pl = pairs[l] & 255, ql = pairs[l] >> 8;
        double x00 = a[pk * LD + pl], x01 = a[pk * LD + ql], x10 = a[qk * LD + pl], x11 = a[qk * LD + ql];
        if (sk != 0.0) {                                           // rows pk, qk
          const double tk = s_tau[k];
          const double n00 = x00 - sk * (x10 + tk * x00), n10 = x10 + sk * (x00 - tk * x10);
          const double n01 = x01 - sk * (x11 + tk * x01), n11 = x11 + sk * (x01 - tk * x11);
          x00 = n00; x10 = n10; x01 = n01; x11 = n11;
        }
        if (sl != 0.0) {                                           // columns pl, ql
          const double tl = s_tau[l];
          const double n00 = x00 - sl * (x01 + tl * x00), n01 = x01 + sl * (x00 - tl * x01);
          const double n10 = x10 - sl * (x11 + tl * x10), n11 = x11 + sl * (x10 - tl * x11);
          x00 = n00; x01 = n01; x10 = n10; x11 = n11;
        }
        a[pk * LD + pl] = x00; a[pk * LD + ql] = x01; a[qk * LD + pl] = x10; a[qk * LD + ql] = x11;
        a[pl * LD + pk] = x00; a[ql * LD + pk] = x01; a[pl * LD + qk] = x10; a[ql * LD + qk] = x11;
      }
      if (vec) {
        // rows p, q of V^T (a rotated pair has q < N): CW consecutive threads walk one pair's rows, T / CW pairs at a time
        constexpr int CW = T == 64 ? 32 : (T == 512 ? 64 : 128);
        const int j = t % CW;
        if (j < N) {
          for (int k = t / CW; k < nb; k += T / CW) {
            const double sk = s_sn[k];
            if (sk == 0.0) continue;
            const double tk = s_tau[k];
            const int p = pairs[k] & 255, q = pairs[k] >> 8;
            double* vp = (VLDS ? vl : vg) + p * ldv + j;
            double* vq = (VLDS ? vl : vg) + q * ldv + j;
            const double x = *vp, y = *vq;
            *vp = x - sk * (y + tk * x);
            *vq = y + sk * (x - tk * y);
          }
        }
      }
      syevj_sync<T>();
    }
    ++sweeps;
    if (my_rot) *s_ctl = 1;
    syevj_sync<T>();
    done = *s_ctl == 0;
    syevj_sync<T>();
    if (t == 0) *s_ctl = 0;                                        // (the next store to it is a whole sweep of barriers away)
  }

  // ---- 5. sort: descending, ties by ascending position
  for (int i = t; i < N; i += T) {
    const double di = a[i * LD + i];
    int rank = 0;
    for (int j = 0; j < N; ++j) { const double dj = a[j * LD + j]; rank += dj > di || (dj == di && j < i); }
    s_inv[rank] = (unsigned short)i;                               // rank < N: at most N - 1 others precede i
    lam[mat * N + rank] = ldexp(di, -sc);
  }
  syevj_sync<T>();
  if (vec) {
    double* v = V + (size_t)mat * NN;
    for (int e = t; e < NN; e += T) {
      const int r = e / N, j = e - r * N;
      v[e] = (VLDS ? vl : vg)[(int)s_inv[j] * ldv + r];
    }
  }
  if (t == 0) {
    if (sweeps_out) sweeps_out[mat] = sweeps;
    if (!done) atomicOr(flag, 2);
  }
}

template <int T, bool VLDS>
int syevj_launch(nd4hip_handle* h, int64_t batch, int N, const double* S, double* lambda, double* V, double* Vws, int32_t* sweeps, int* flag) {
  constexpr int MPW = T == 64 ? 4 : 1;
  const size_t lds = syevj_layout(N, VLDS && V != nullptr).bytes * MPW;
  ND4_CHECK_ARG(lds <= 160 * 1024, "nd4hip_dsyevj_batched: %zu bytes of LDS", lds);
  // above 64 KB the launch needs the function attribute (set every time: it is per device)
  if (lds > 64 * 1024)
    ND4_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&syevj_kernel<T, VLDS>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL((syevj_kernel<T, VLDS>), dim3((unsigned)((batch + MPW - 1) / MPW)), dim3(T == 64 ? 256 : T), lds, h->stream,
                     S, N, (long)batch, lambda, V, Vws, sweeps, flag, SYEVJ_MAX_SWEEPS);
  ND4_HIP(hipGetLastError());
  return 0;
}

}  // namespace

// S [batch, N, N] -> lambda [batch, N] descending, V [batch, N, N] (columns = eigenvectors) or V = NULL: the values alone (the same
// bits); sweeps [batch] or NULL. 1 <= N <= 128. One launch; synchronises to read the flag word back.
int nd4_syevj(nd4hip_handle* h, int64_t batch, int64_t N64, const double* S, double* lambda, double* V, int32_t* sweeps) {
  ND4_CHECK_ARG(N64 >= 1 && N64 <= SYEVJ_MAXN, "nd4hip_dsyevj_batched: the Jacobi route takes 1 <= N <= %d", SYEVJ_MAXN);
  ND4_CHECK_ARG(batch >= 1 && batch <= (int64_t)1 << 30, "nd4hip_dsyevj_batched: batch %lld out of range", (long long)batch);
  const int N = (int)N64;
  Nd4WsScope scope(h);
  void* p = nullptr;
  ND4_TRY(nd4_ws_alloc(h, sizeof(int), &p));
  int* flag = static_cast<int*>(p);
  ND4_HIP(hipMemsetAsync(flag, 0, sizeof(int), h->stream));
  if (N <= 32) ND4_TRY((syevj_launch<64, true>(h, batch, N, S, lambda, V, nullptr, sweeps, flag)));
  else if (N <= 64) ND4_TRY((syevj_launch<512, true>(h, batch, N, S, lambda, V, nullptr, sweeps, flag)));
  else {
    double* Vws = nullptr;
    if (V) { ND4_TRY(nd4_ws_alloc(h, sizeof(double) * (size_t)batch * N * N, &p)); Vws = static_cast<double*>(p); }
    ND4_TRY((syevj_launch<1024, false>(h, batch, N, S, lambda, V, Vws, sweeps, flag)));
  }
  void* hp = nullptr;
  ND4_TRY(nd4_pinned(h, sizeof(int), &hp));
  int* host = static_cast<int*>(hp);
  ND4_HIP(hipMemcpyAsync(host, flag, sizeof(int), hipMemcpyDeviceToHost, h->stream));
  ND4_HIP(hipStreamSynchronize(h->stream));
  if (host[0] & 1) {
    nd4_set_error("eigen_sym(S): S contains NaN or Infinity in its lower triangle.");
    return ND4HIP_ERR_NOCONV;
  }
  if (host[0] & 2) {
    nd4_set_error("eigen_sym(S, algo='jacobi'): no convergence after %d sweeps.", SYEVJ_MAX_SWEEPS);
    return ND4HIP_ERR_NOCONV;
  }
  return 0;
}
