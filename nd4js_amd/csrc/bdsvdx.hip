// Selected singular triplets of upper bidiagonal and dense matrices: bidiag_svd(d, e, subset=(i0, i1)), bidiag_svdvals(d, e),
// svd_decomp(A, subset), svd_vals(A). LAPACK's dbdsvdx restated on the kernels of syevx.hip: a singular value of
// B [K, J] (J = K or K + 1) is an eigenvalue of the Golub-Kahan matrix, the symmetric tridiagonal of order n = K + J with a zero
// diagonal and the off-diagonals b = (d0, e0, d1, e1, ...); its eigenvector for sigma is (v0, u0, v1, u1, ...) / sqrt(2). The
// descending spectrum is sigma_0 >= ... >= sigma_K-1 >= (0 for J = K + 1) >= -sigma_K-1 >= ...: index j < K of it is sigma_j.
// No workgroup waits for another, there is no spin loop and no atomic apart from raising flag words, and every loop has a bound
// computed from K, J, k or a constant.
//   1. bdx_prepare, one wave per member: stx_prepare with d = 0. The finite check on the bit patterns (a bad member becomes B = 0
//      and raises the call's flag word), the exact scale 2^-m, m the frexp exponent of max|b|; g = max_i(|b_i-1| + |b_i|); b^2; the
//      mark of B = 0, which is also that member's fallback flag. The zero diagonal is written once, for the vector stage only.
//   2. bdx_bisect: stx_bisect with q_0 = 0 - x, q_i = (0 - x) - b^2_i-1 / q_i-1. Only b^2 is staged: at most 4096 doubles, 32 KB,
//      for an order of up to 4097. sv = max(2^m midpoint, +0). A member with B = 0 gets zeros.
//   3. bdx_small, one lane per member: the fallback flag of a member with two or more selected scaled values below (1e-3 g) / 2.
//      Then +sigma_i and -sigma_j are closer than a cluster gap and nothing orthogonalises them against each other.
//   4. nd4_stx_vectors (syevx.hip, unchanged kernels): stx_clusters, three rounds of stx_factor_solve and stx_orth on rows of length
//      n, with the zero diagonal of step 1.
//   5. bdx_split, grid (k, batch): v = the even entries of z, u = the odd entries, each normalised on its own; both sums of squares
//      have a fixed order. What z holds of the partner for -sigma is (v, -u): it changes the two norms, not the directions. A
//      vector with min(|u|^2, |v|^2) < 1/8 (the ideal is 1/2) raises its member's fallback flag.
//   6. The flags are read back once. Flagged members are compacted and go through nd4_bdsdc_rows (svd_dc.hip, unchanged);
//      bdx_gather copies columns i0 .. i1 - 1 of U2 and rows i0 .. i1 - 1 of V2. sv stays the bisection's.
//   7 (dgesvdx): the scaling and nd4_gebrd of nd4_gesdd, steps 1-6 on the diagonals of B_b, U = U_b U2 and V = V2 V_b on the fp64
//      MFMA GEMM with k columns and rows.
// Arithmetic of 1-3 is + - * / and comparisons, each rounded once (the file is compiled without contraction): the device returns
// the bits of the numpy model in tests/svd_subset_common.py for the values and the flags of step 3.
#include "syev_internal.h"
#include "nd4hip_args.h"
#include <cstring>
#include <vector>

namespace {

constexpr int BDX_MAXOFF = 4096;            // off-diagonals of the Golub-Kahan matrix of K = 2048, J = 2049
constexpr int BDX_SPLIT_THREADS = 256;
constexpr int BDX_STAGES = ND4HIP_SVDX_STAGES;

struct BdxStamps : Nd4StageStamps<BDX_STAGES> {
  explicit BdxStamps(nd4hip_handle* hh) : Nd4StageStamps<BDX_STAGES>(hh, hh->svdx_stage_ms) {}
};

// off-diagonal i of the Golub-Kahan matrix: d_{i/2} for even i, e_{i/2} for odd i (i < K + J - 1, so e is read below J - 1)
__device__ __forceinline__ double bdx_off(const double* dm, long dinc, const double* em, long einc, int i) {
  return (i & 1) ? em[(size_t)(i >> 1) * einc] : dm[(size_t)(i >> 1) * dinc];
}

// zs (zeros), bs, b2 [batch, n] (bs, b2 [n-1] = 0), g, lexp, diag [batch]; fb [batch]: 1 for B = 0; *flag raised for NaN or Inf
__global__ __launch_bounds__(64) void bdx_prepare(const double* __restrict__ d, long dinc, long dstride, const double* __restrict__ e, long einc,
                                                  long estride, int n, double* __restrict__ zs, double* __restrict__ bs,
                                                  double* __restrict__ b2, double* __restrict__ g, int* __restrict__ lexp,
                                                  int* __restrict__ diag, int* __restrict__ fb, int* __restrict__ flag) {
  const int b = blockIdx.x, lane = threadIdx.x, no = n - 1;
  const double* dm = d + (size_t)b * dstride;
  const double* em = e ? e + (size_t)b * estride : nullptr;   // NULL only for K = J = 1: no odd i below n - 1 = 1
  double* zb = zs + (size_t)b * n; double* bb = bs + (size_t)b * n; double* qb = b2 + (size_t)b * n;
  u64 m = 0;
  for (int i = lane; i < no; i += 64) {
    const u64 w = (u64)__double_as_longlong(fabs(bdx_off(dm, dinc, em, einc, i)));
    m = w > m ? w : m;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) { const u64 o = __shfl_xor(m, off); m = o > m ? o : m; }
  if (m > SYEV_MAX_BITS) {                                    // NaN or Inf: B = 0 stands in, nothing is solved for it
    for (int i = lane; i < n; i += 64) { zb[i] = 0.0; bb[i] = 0.0; qb[i] = 0.0; }
    if (lane == 0) { g[b] = 1.0; lexp[b] = 0; diag[b] = 1; fb[b] = 0; atomicMax(flag, 1); }
    return;
  }
  int mm = 0;
  const double mv = __longlong_as_double((long long)m);
  if (mv > 0.0) (void)frexp(mv, &mm);
  double gg = 0.0; int nonzero = 0;
  for (int i = lane; i < n; i += 64) {
    const double bi = i < no ? ldexp(bdx_off(dm, dinc, em, einc, i), -mm) : 0.0;
    const double bp = i > 0 ? ldexp(bdx_off(dm, dinc, em, einc, i - 1), -mm) : 0.0;
    zb[i] = 0.0; bb[i] = bi; qb[i] = bi * bi;
    nonzero |= bi != 0.0;
    gg = fmax(gg, fabs(bp) + fabs(bi));
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) { gg = fmax(gg, __shfl_xor(gg, off)); nonzero |= __shfl_xor(nonzero, off); }
  if (lane == 0) { g[b] = gg; lexp[b] = mm; diag[b] = !nonzero; fb[b] = !nonzero; }
}

// #{i: q_i < 0} of the member whose squared off-diagonals are staged at s2: stx_negatives with d = 0
__device__ __forceinline__ int bdx_negatives(const double* s2, int n, double x) {
  double q = 0.0 - x;
  if (fabs(q) < STX_PIVMIN) q = -STX_PIVMIN;
  int c = q < 0.0;
  for (int i = 1; i < n; ++i) {
    q = (0.0 - x) - s2[i - 1] / q;
    if (fabs(q) < STX_PIVMIN) q = -STX_PIVMIN;
    c += q < 0.0;
  }
  return c;
}

// lams [batch, k] (scaled, as bisected) and sv [batch, k] = max(2^lexp lams, +0) for the indices i0 .. i0 + k - 1 of the descending
// singular values; grid (ceil(k / 256), batch)
__global__ __launch_bounds__(256) void bdx_bisect(const double* __restrict__ b2, const double* __restrict__ g, const int* __restrict__ lexp,
                                                  const int* __restrict__ diag, int n, int i0, int k, double* __restrict__ lams,
                                                  double* __restrict__ sv) {
  __shared__ double s2[BDX_MAXOFF];
  const int b = blockIdx.y, t = blockIdx.x * 256 + threadIdx.x;
  if (diag[b]) {                                              // the whole workgroup: B = 0
    if (t < k) { lams[(size_t)b * k + t] = 0.0; sv[(size_t)b * k + t] = 0.0; }
    return;
  }
  for (int i = threadIdx.x; i < n - 1; i += 256) s2[i] = b2[(size_t)b * n + i];   // n - 1 <= BDX_MAXOFF
  __syncthreads();
  if (t >= k) return;
  const double v = stx_bisect_value(g[b], i0 + t, n, [&](double x) { return bdx_negatives(s2, n, x); });
  const double s = ldexp(v, lexp[b]);
  lams[(size_t)b * k + t] = v;
  sv[(size_t)b * k + t] = s > 0.0 ? s : 0.0;
}

// fb [b] raised where two or more of the member's k scaled values lie below (1e-3 g) / 2. One lane per member.
__global__ __launch_bounds__(64) void bdx_small(const double* __restrict__ lams, const double* __restrict__ g, const int* __restrict__ diag,
                                                int batch, int k, int* __restrict__ fb) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= batch || diag[b]) return;
  const double thr = 0.5 * (1e-3 * g[b]);
  int c = 0;
  for (int j = 0; j < k; ++j) c += lams[(size_t)b * k + j] < thr;
  if (c >= 2) atomicMax(&fb[b], 1);
}

// sum over the workgroup in a fixed order: lanes by the xor butterfly, then the waves' sums in wave order
__device__ __forceinline__ double bdx_block_sum(double v, double* part) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  __syncthreads();                                             // part may still be read from the previous call
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = 0.0;
  for (int wv = 0; wv < BDX_SPLIT_THREADS / 64; ++wv) s += part[wv];
  return s;
}

// grid (k, batch): row jj of Z [batch, k, n] -> column jj of U2 [batch, K, k] (the odd entries) and row jj of V2 [batch, k, J] (the
// even entries), each divided by its own norm; fb [b] raised where min(|u|^2, |v|^2) < 1/8 (or is not a number)
__global__ __launch_bounds__(BDX_SPLIT_THREADS) void bdx_split(const double* __restrict__ Z, const int* __restrict__ diag, int K, int J, int k,
                                                               double* __restrict__ U2, double* __restrict__ V2, int* __restrict__ fb) {
  __shared__ double part[BDX_SPLIT_THREADS / 64];
  const int jj = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, n = K + J;
  if (diag[b]) return;                                        // the whole workgroup, before any barrier
  const double* z = Z + ((size_t)b * k + jj) * n;
  double su = 0.0, sv = 0.0;
  for (int i = tid; i < K; i += BDX_SPLIT_THREADS) { const double a = z[2 * i + 1]; su += a * a; }   // 2 i + 1 <= 2 K - 1 < n
  for (int i = tid; i < J; i += BDX_SPLIT_THREADS) { const double a = z[2 * i]; sv += a * a; }       // 2 i <= 2 J - 2 < n
  const double nu = bdx_block_sum(su, part), nv = bdx_block_sum(sv, part);
  if (tid == 0 && !(fmin(nu, nv) >= 0.125)) atomicMax(&fb[b], 1);
  const double ru = sqrt(nu), rv = sqrt(nv);
  const bool uok = nu > 0.0 && nu <= DBL_MAX, vok = nv > 0.0 && nv <= DBL_MAX;
  double* Ub = U2 + (size_t)b * K * k + jj;
  double* Vb = V2 + ((size_t)b * k + jj) * J;
  for (int i = tid; i < K; i += BDX_SPLIT_THREADS) Ub[(size_t)i * k] = uok ? z[2 * i + 1] / ru : z[2 * i + 1];
  for (int i = tid; i < J; i += BDX_SPLIT_THREADS) Vb[i] = vok ? z[2 * i] / rv : z[2 * i];
}

// the flagged members idx [nf] as dense d [nf, K], e [nf, J - 1] for the full solver; total = nf (K + J - 1)
__global__ __launch_bounds__(256) void bdx_compact(const double* __restrict__ d, long dinc, long dstride, const double* __restrict__ e, long einc,
                                                   long estride, const int* __restrict__ idx, int K, int J, long total,
                                                   double* __restrict__ dc, double* __restrict__ ec) {
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  if (t >= total) return;
  const int per = K + J - 1;
  const long m = t / per; const int i = (int)(t - m * per);
  const long b = idx[m];
  if (i < K) dc[m * K + i] = d[(size_t)b * dstride + (size_t)i * dinc];
  else ec[m * (J - 1) + (i - K)] = e[(size_t)b * estride + (size_t)(i - K) * einc];
}

// member idx [m] of U2 [batch, K, k] <- columns i0 .. i0 + k - 1 of Uf [nf, K, K]; of V2 [batch, k, J] <- rows i0 .. of Vf [nf, J, J];
// total = nf k (K + J)
__global__ __launch_bounds__(256) void bdx_gather(const double* __restrict__ Uf, const double* __restrict__ Vf, const int* __restrict__ idx, int K,
                                                  int J, int i0, int k, long total, double* __restrict__ U2, double* __restrict__ V2) {
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  if (t >= total) return;
  const long per = (long)k * (K + J), m = t / per, r = t - m * per;
  const long b = idx[m];
  if (r < (long)K * k) {                                      // U2 [i][jj]
    const long i = r / k, jj = r - i * k;
    U2[(size_t)b * K * k + r] = Uf[((size_t)m * K + i) * K + i0 + jj];
  } else {                                                    // V2 [jj][c]
    const long q = r - (long)K * k, jj = q / J, c = q - jj * J;
    V2[(size_t)b * k * J + q] = Vf[((size_t)m * J + i0 + jj) * J + c];
  }
}

__global__ __launch_bounds__(256) void bdx_copy_flags(const int* __restrict__ fb, int batch, int32_t* __restrict__ out) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b < batch) out[b] = fb[b];
}

// Steps 1-6 on the members given by (d, dinc, dstride), (e, einc, estride). sv [batch, k]; U2 [batch, K, k] and V2 [batch, k, J] or both
// NULL. Synchronises once (the flags); *bad = the call's flag word (NaN or Inf). st: marks after the values, the vectors, the fallback.
int bdx_run(nd4hip_handle* h, int64_t batch, int K, int J, int i0, int k, const double* d, long dinc, long dstride, const double* e, long einc,
            long estride, double* U2, double* sv, double* V2, int32_t* fallback, BdxStamps* st, int* bad) {
  static_assert(BDX_MAXOFF * sizeof(double) == 32768, "bdx_bisect stages the squares in the 32 KB stx_count uses");
  ND4_CHECK_ARG(nd4_bdx_offdiagonals(K, J) <= BDX_MAXOFF && nd4_bdx_lds_bytes(K, J) <= sizeof(double) * BDX_MAXOFF,
                "nd4hip_dbdsvdx_batched: extent out of range");
  const int n = (int)nd4_bdx_order(K, J);
  const size_t bn = (size_t)batch * n, bk = (size_t)batch * k;
  double *zs, *bs, *b2, *g, *lams; int *lexp, *diag, *fb;
  ND4_TRY(stx_alloc(h, bn, &zs)); ND4_TRY(stx_alloc(h, bn, &bs)); ND4_TRY(stx_alloc(h, bn, &b2));
  ND4_TRY(stx_alloc(h, (size_t)batch, &g)); ND4_TRY(stx_alloc(h, (size_t)batch, &lexp)); ND4_TRY(stx_alloc(h, (size_t)batch, &diag));
  ND4_TRY(stx_alloc(h, (size_t)batch + 1, &fb));             // fb [batch] is the call's flag word
  ND4_TRY(stx_alloc(h, bk, &lams));
  int* flag = fb + batch;
  ND4_HIP(hipMemsetAsync(flag, 0, sizeof(int), h->stream));
  hipLaunchKernelGGL(bdx_prepare, dim3((unsigned)batch), dim3(64), 0, h->stream, d, dinc, dstride, e, einc, estride, n, zs, bs, b2, g, lexp, diag, fb,
                     flag);
  hipLaunchKernelGGL(bdx_bisect, dim3((unsigned)nd4_stx_bisect_blocks(k), (unsigned)batch), dim3(256), 0, h->stream, b2, g, lexp, diag, n, i0, k, lams,
                     sv);
  hipLaunchKernelGGL(bdx_small, dim3((unsigned)((batch + 63) / 64)), dim3(64), 0, h->stream, lams, g, diag, (int)batch, k, fb);
  ND4_HIP(hipGetLastError());
  st->mark();
  if (U2) {
    double* Z = nullptr;                                      // with the four arrays of nd4_stx_vectors: nd4_bdx_vector_doubles
    ND4_TRY(stx_alloc(h, bk * n, &Z));
    ND4_TRY(nd4_stx_vectors(h, batch, n, i0, k, nullptr, zs, bs, g, diag, lams, Z));
    hipLaunchKernelGGL(bdx_split, dim3((unsigned)k, (unsigned)batch), dim3(BDX_SPLIT_THREADS), 0, h->stream, Z, diag, K, J, k, U2, V2, fb);
    ND4_HIP(hipGetLastError());
  }
  if (fallback) {
    hipLaunchKernelGGL(bdx_copy_flags, dim3((unsigned)((batch + 255) / 256)), dim3(256), 0, h->stream, fb, (int)batch, fallback);
    ND4_HIP(hipGetLastError());
  }
  st->mark();
  const int* host = nullptr;
  ND4_TRY(nd4_stx_read_flags(h, fb, (size_t)batch + 1, &host));
  *bad = host[batch];
  if (*bad || !U2) { st->mark(); return 0; }
  std::vector<int> idx;
  for (int64_t b = 0; b < batch; ++b) if (host[b]) idx.push_back((int)b);
  const int64_t nf = (int64_t)idx.size();
  if (nf == 0) { st->mark(); return 0; }
  int* didx = nullptr; double *dc, *ec, *Uf, *svf, *Vf;
  ND4_TRY(stx_alloc(h, (size_t)nf, &didx));
  ND4_TRY(stx_alloc(h, (size_t)nf * K, &dc)); ND4_TRY(stx_alloc(h, (size_t)nf * (J - 1), &ec));
  ND4_TRY(stx_alloc(h, (size_t)nf * K * K, &Uf)); ND4_TRY(stx_alloc(h, (size_t)nf * K, &svf)); ND4_TRY(stx_alloc(h, (size_t)nf * J * J, &Vf));
  void* hp = nullptr;
  ND4_TRY(nd4_pinned(h, sizeof(int) * (size_t)nf, &hp));
  memcpy(hp, idx.data(), sizeof(int) * (size_t)nf);
  ND4_HIP(hipMemcpyAsync(didx, hp, sizeof(int) * (size_t)nf, hipMemcpyHostToDevice, h->stream));
  ND4_HIP(hipStreamSynchronize(h->stream));                   // the full solver reuses the pinned buffer
  const long ctotal = (long)nf * (K + J - 1);
  hipLaunchKernelGGL(bdx_compact, dim3((unsigned)((ctotal + 255) / 256)), dim3(256), 0, h->stream, d, dinc, dstride, e, einc, estride, didx, K, J, ctotal,
                     dc, ec);
  ND4_HIP(hipGetLastError());
  ND4_TRY(nd4_bdsdc_rows(h, nf, K, J, dc, ec, Uf, svf, Vf));
  const long gtotal = (long)nf * k * (K + J);
  hipLaunchKernelGGL(bdx_gather, dim3((unsigned)((gtotal + 255) / 256)), dim3(256), 0, h->stream, Uf, Vf, didx, K, J, i0, k, gtotal, U2, V2);
  ND4_HIP(hipGetLastError());
  st->mark();
  return 0;
}

}  // namespace

int nd4_bdsvdx(nd4hip_handle* h, int64_t batch, int64_t K, int64_t J, int64_t i0, int64_t i1, const double* d, const double* e, double* U2,
               double* sv, double* V2, int32_t* fallback) {
  ND4_CHECK_ARG(K >= 1 && K <= 2048 && (J == K || J == K + 1) && batch >= 1 && batch <= 32768, "nd4hip_dbdsvdx_batched: extent out of range");
  Nd4WsScope scope(h);
  BdxStamps st(h);
  st.mark(); st.mark();                                       // no bidiagonalisation
  int bad = 0;
  ND4_TRY(bdx_run(h, batch, (int)K, (int)J, (int)i0, (int)(i1 - i0), d, 1, K, e, 1, J - 1, U2, sv, V2, fallback, &st, &bad));
  st.mark();                                                  // no products
  ND4_HIP(hipStreamSynchronize(h->stream));
  st.collect();
  h->svdx_stage_ms[0] = h->svdx_stage_ms[4] = 0.0;            // (the time between two event records, not a stage)
  if (bad) {
    nd4_set_error("bidiag_svd(d,e): d or e contains NaN or Infinity.");
    return ND4HIP_ERR_NOCONV;
  }
  return 0;
}

int nd4_gesvdx(nd4hip_handle* h, int64_t batch, int64_t M, int64_t N, int64_t i0, int64_t i1, const double* A, double* U, double* sv, double* V,
               int32_t* fallback) {
  const bool tall = M > N;
  const int64_t m = tall ? N : M, n = tall ? M : N, k = i1 - i0;   // the wide problem that is solved: m x n, m <= n
  ND4_CHECK_ARG(m >= 1 && m <= 2048 && batch >= 1 && batch <= 32768, "nd4hip_dgesvdx_batched: extent out of range");
  Nd4WsScope scope(h);
  BdxStamps st(h);
  const int64_t Jb = m < n ? m + 1 : m, sA = m * n;
  unsigned long long* mx = nullptr;
  double *As, *Ub, *Bb, *Vb, *U2 = nullptr, *V2 = nullptr, *Ut = nullptr, *Vt = nullptr;
  ND4_TRY(stx_alloc(h, (size_t)batch, &mx));
  ND4_TRY(stx_alloc(h, (size_t)batch * sA, &As)); ND4_TRY(stx_alloc(h, (size_t)batch * m * m, &Ub));
  ND4_TRY(stx_alloc(h, (size_t)batch * m * Jb, &Bb)); ND4_TRY(stx_alloc(h, (size_t)batch * Jb * n, &Vb));
  if (U) {
    ND4_TRY(stx_alloc(h, (size_t)batch * m * k, &U2)); ND4_TRY(stx_alloc(h, (size_t)batch * k * Jb, &V2));
    if (tall) { ND4_TRY(stx_alloc(h, (size_t)batch * m * k, &Ut)); ND4_TRY(stx_alloc(h, (size_t)batch * k * n, &Vt)); }
  }
  st.mark();
  // the scaling and the bidiagonalisation of nd4_gesdd (svd_dc.hip)
  ND4_TRY(nd4_svd_scale_begin(h, batch, M * N, A, mx));
  if (tall) { ND4_TRY(nd4_transpose(h, M, N, A, N, As, M, batch, sA, sA)); ND4_TRY(nd4_svd_scale_apply(h, batch, sA, As, As, mx)); }
  else ND4_TRY(nd4_svd_scale_apply(h, batch, sA, A, As, mx));
  ND4_TRY(nd4_gebrd(h, batch, m, n, As, Ub, Bb, Vb));
  st.mark();
  int bad = 0;
  ND4_TRY(bdx_run(h, batch, (int)m, (int)Jb, (int)i0, (int)k, Bb, Jb + 1, m * Jb, Bb + 1, Jb + 1, m * Jb, U2, sv, V2, fallback, &st, &bad));
  if (U && !bad) {
    double* Uo = tall ? Ut : U;                               // [m, k]
    double* Vo = tall ? Vt : V;                               // [k, n]
    ND4_TRY(nd4_gemm(h, false, false, m, k, m, 1.0, Ub, m, m * m, U2, k, m * k, 0.0, Uo, k, m * k, batch));
    ND4_TRY(nd4_gemm(h, false, false, k, n, Jb, 1.0, V2, Jb, k * Jb, Vb, n, Jb * n, 0.0, Vo, n, k * n, batch));
    if (tall) {                                               // U = V'^T [M, k], V = U'^T [k, N]
      ND4_TRY(nd4_transpose(h, k, n, Vt, n, U, k, batch, k * n, n * k));
      ND4_TRY(nd4_transpose(h, m, k, Ut, k, V, m, batch, m * k, k * m));
    }
  }
  ND4_TRY(nd4_svd_scale_undo(h, batch, k, sv, mx));
  st.mark();
  ND4_HIP(hipStreamSynchronize(h->stream));
  st.collect();
  ND4_TRY(nd4_xchg_check(h, "svd_subset"));
  if (bad) {
    nd4_set_error("svd_decomp(A): A contains NaN or Infinity.");
    return ND4HIP_ERR_NOCONV;
  }
  return 0;
}
