// Selected eigenpairs of symmetric tridiagonal and dense symmetric matrices: eigen_sym(S, subset=(i0, i1)), tridiag_eigen(d, e),
// tridiag_count(d, e, x). Bisection on Sturm counts for the values, inverse iteration for the vectors (LAPACK's
// dstebz + dstein, restated for one lane per eigenvalue and one lane per eigenvector). Every recurrence is serial in N and
// independent of every other, so k of them run side by side; no workgroup waits for another, there is no spin loop and no atomic
// apart from raising the call's flag word, and every loop has a bound computed from N, k or a constant.
//   1. stx_prepare, one wave per member: the finite check (the identity's d, e for a bad member and the flag raised, as
//      syev_shift_chol does), the exact scale 2^-m with m the frexp exponent of max(|d|, |e|), so that the scaled entries lie in
//      (-1, 1); g = max_i((|d_i| + |e_i-1|) + |e_i|) >= rho(T) of the scaled member; e^2; the mark of a diagonal member (e = 0).
//      pivmin is 2^-1022 for every member: the scaled e^2 are below 1.
//   2. stx_count: #{lambda > x} = N - #{i: q_i < 0}, q_0 = d_0 - x, q_i = (d_i - x) - e^2_i-1 / q_i-1, |q| < pivmin replaced by
//      -pivmin; one lane per (member, x), d and e^2 of the member in LDS (every lane reads the same word at each step).
//   3. stx_bisect: lambda_j, j the index in the descending spectrum, is the least x with #{lambda > x} <= j: bisection from
//      [-g', g'], g' = g (1 + 2^-20), until hi - lo <= 2 eps max(|lo|, |hi|) + eps g or the midpoint meets an end, at most 128
//      halvings; lambda = 2^m midpoint. stx_diag gives a diagonal member its d by descending rank (ties by index) and the unit
//      vectors, exactly as syev_values does.
//   4. stx_clusters, one lane per member: a cluster starts where the gap to the previous selected value exceeds 1e-3 g; inside a
//      cluster the shifts are kept 10 eps g apart (dstein's perturbation).
//   5. stx_factor_solve, one lane per vector: LU of T - shift with partial pivoting (dlagtf's scheme, a pivot below eps g in
//      magnitude replaced by +-eps g), the forward substitution fused into the elimination, then the back substitution. The
//      factors and the right-hand side live in a workspace laid out [row][vector]. Start vector u(seed, j N + i) of the project's
//      counter-based generator, j the index in the full spectrum; before each solve the iterate is scaled to N g eps / max|z|.
//   6. stx_orth, grid (k, batch): the workgroup of a cluster head walks its cluster: vector j is orthogonalised against the
//      cluster's earlier vectors by Gram-Schmidt applied twice, normalised and, in the last round, given the sign that makes its
//      first component of largest magnitude positive. Reductions have a fixed order: results are the same bits run to run.
//   Steps 5 and 6 run three times. 7 (dsyevx): steps 1-2 of syev.hip, then V = U Z^T on the fp64 MFMA GEMM.
//   The bisection loop (stx_bisect_value) and steps 4-6 as one launcher (nd4_stx_vectors) are declared in syev_internal.h: bdsvdx.hip
//   runs them on the Golub-Kahan form of a bidiagonal matrix.
// Arithmetic of 1-4 is + - * / and comparisons, each rounded once (the file is compiled without contraction): the device returns
// the bits of the numpy model in tests/eigsym_subset_common.py.
//   The interval forms select the eigenvalues in (lo, hi] of each member: after step 1 one stx_count launch with the
//   two probes (hi, lo) of every member writes its range (i0_b, i1_b) = (count(hi), count(lo)); the host reads the ranges back once,
//   for kmax = max_b(i1_b - i0_b) alone, which sizes the grids of steps 3-6. Those kernels then take each member's own range from
//   device memory (rng != NULL) in place of the call's uniform (i0, k): k is kmax there, the stride of the compact work arrays, and
//   lanes and workgroups past a member's k_b leave without work. stx_ragged moves the compact results into the caller's
//   [batch, kcap] and [batch, N, kcap] arrays: NaN and zero columns from k_b to kmax - 1, nothing from kmax on.
#include "syev_internal.h"
#include "nd4hip_args.h"
#include <climits>

namespace {

constexpr int STX_MAXN = 2048;             // d and e^2 of one member are staged in 2 x 16 KB of LDS
constexpr unsigned STX_SEED = 20480u;      // of the start vectors
constexpr int STX_ORTH_THREADS = 512;
constexpr int STX_STAGES = ND4HIP_SYEVX_STAGES;

__device__ __forceinline__ unsigned stx_fmix32(unsigned x) {
  x ^= x >> 16; x *= 0x85EBCA6Bu; x ^= x >> 13; x *= 0xC2B2AE35u; x ^= x >> 16;
  return x;
}
// u(seed, idx) of nd4js_amd/rng.py, s = fmix32(seed)
__device__ __forceinline__ double stx_uniform(unsigned s, unsigned idx) {
  const unsigned hi = stx_fmix32(idx ^ s);
  const unsigned lo = stx_fmix32(hi + 0x9E3779B9u + idx);
  const double m = (double)(hi >> 5) * 67108864.0 + (double)(lo >> 6);
  return m * 0x1p-52 - 1.0;
}

// member b's slice of the descending spectrum, (first index, number of values): the call's (i0, k), or, in the interval forms,
// (i0_b, i1_b - i0_b) of rng [batch, 2] and never more than k, the stride of the work arrays
__device__ __forceinline__ void stx_range(const int* __restrict__ rng, long b, int i0, int k, int* first, int* kb) {
  if (!rng) { *first = i0; *kb = k; return; }
  const int a = rng[2 * b], n = rng[2 * b + 1] - a;
  *first = a; *kb = n < k ? n : k;
}

// d (elements dinc apart, members dstride apart) and e (likewise; NULL for N = 1) -> ds, es, e2 [batch, N] (es, e2 [N-1] = 0),
// g [batch], lexp [batch] = m + e1 (e1 from mx, 0 without), diag [batch]. mx (may be NULL): syev_absmax_lower's word of the member.
__global__ __launch_bounds__(64) void stx_prepare(const double* __restrict__ d, long dinc, long dstride, const double* __restrict__ e, long einc,
                                                  long estride, int N, const u64* __restrict__ mx, double* __restrict__ ds,
                                                  double* __restrict__ es, double* __restrict__ e2, double* __restrict__ g,
                                                  int* __restrict__ lexp, int* __restrict__ diag, int* __restrict__ flag) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const double* dm = d + (size_t)b * dstride;
  const double* em = N > 1 ? e + (size_t)b * estride : nullptr;
  double* dsb = ds + (size_t)b * N; double* esb = es + (size_t)b * N; double* e2b = e2 + (size_t)b * N;
  u64 m = 0;
  for (int i = lane; i < N; i += 64) {
    u64 w = (u64)__double_as_longlong(fabs(dm[(size_t)i * dinc]));
    m = w > m ? w : m;
    if (i + 1 < N) { w = (u64)__double_as_longlong(fabs(em[(size_t)i * einc])); m = w > m ? w : m; }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) { const u64 o = __shfl_xor(m, off); m = o > m ? o : m; }
  if (m > SYEV_MAX_BITS || (mx && mx[b] > SYEV_MAX_BITS)) {   // NaN or Inf: the identity stands in
    for (int i = lane; i < N; i += 64) { dsb[i] = 1.0; esb[i] = 0.0; e2b[i] = 0.0; }
    if (lane == 0) { g[b] = 1.0; lexp[b] = 0; diag[b] = 1; atomicMax(flag, 1); }
    return;
  }
  int mm = 0;
  const double mv = __longlong_as_double((long long)m);
  if (mv > 0.0) (void)frexp(mv, &mm);
  double gg = 0.0; int offdiag = 0;
  for (int i = lane; i < N; i += 64) {
    const double di = ldexp(dm[(size_t)i * dinc], -mm);
    const double ei = i + 1 < N ? ldexp(em[(size_t)i * einc], -mm) : 0.0;
    const double ep = i > 0 ? ldexp(em[(size_t)(i - 1) * einc], -mm) : 0.0;
    dsb[i] = di; esb[i] = ei; e2b[i] = ei * ei;
    offdiag |= ei != 0.0;
    gg = fmax(gg, (fabs(di) + fabs(ep)) + fabs(ei));
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) { gg = fmax(gg, __shfl_xor(gg, off)); offdiag |= __shfl_xor(offdiag, off); }
  if (lane == 0) { g[b] = gg; lexp[b] = mm + (mx ? syev_exp(mx[b]) : 0); diag[b] = !offdiag; }
}

// #{i: q_i < 0} of the member staged at sd, s2
__device__ __forceinline__ int stx_negatives(const double* sd, const double* s2, int N, double x) {
  double q = sd[0] - x;
  if (fabs(q) < STX_PIVMIN) q = -STX_PIVMIN;
  int c = q < 0.0;
  for (int i = 1; i < N; ++i) {
    q = (sd[i] - x) - s2[i - 1] / q;
    if (fabs(q) < STX_PIVMIN) q = -STX_PIVMIN;
    c += q < 0.0;
  }
  return c;
}

// count [batch, M] = #{lambda > x} of the member; grid (ceil(M / 256), batch). reversed: count[t] belongs to x[M - 1 - t], so that
// the bounds (lo, hi) of an interval give the range (count(hi), count(lo))
__global__ __launch_bounds__(256) void stx_count(const double* __restrict__ ds, const double* __restrict__ e2, const int* __restrict__ lexp, int N,
                                                 long M, const double* __restrict__ x, int* __restrict__ count, int reversed) {
  __shared__ double sd[STX_MAXN], s2[STX_MAXN];
  const int b = blockIdx.y;
  for (int i = threadIdx.x; i < N; i += 256) { sd[i] = ds[(size_t)b * N + i]; s2[i] = e2[(size_t)b * N + i]; }
  __syncthreads();
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  if (t >= M) return;
  const double xs = ldexp(x[(size_t)b * M + (reversed ? M - 1 - t : t)], -lexp[b]);
  count[(size_t)b * M + t] = N - stx_negatives(sd, s2, N, xs);
}

// lams [batch, k] (scaled) and lam [batch, k] = 2^lexp lams for the indices i0 .. i0 + k - 1 of the descending spectrum (rng: the
// member's own, see stx_range); grid (ceil(k / 256), batch). A diagonal member is left to stx_diag.
__global__ __launch_bounds__(256) void stx_bisect(const double* __restrict__ ds, const double* __restrict__ e2, const double* __restrict__ g,
                                                  const int* __restrict__ lexp, const int* __restrict__ diag, int N, int i0, int k,
                                                  const int* __restrict__ rng, double* __restrict__ lams, double* __restrict__ lam) {
  __shared__ double sd[STX_MAXN], s2[STX_MAXN];
  const int b = blockIdx.y;
  int first, kb;
  stx_range(rng, b, i0, k, &first, &kb);
  if (diag[b] || (int)blockIdx.x * 256 >= kb) return;         // the whole workgroup: nobody waits at the barrier below
  for (int i = threadIdx.x; i < N; i += 256) { sd[i] = ds[(size_t)b * N + i]; s2[i] = e2[(size_t)b * N + i]; }
  __syncthreads();
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= kb) return;
  const int j = first + t;
  const double v = stx_bisect_value(g[b], j, N, [&](double x) { return stx_negatives(sd, s2, N, x); });
  lams[(size_t)b * k + t] = v;
  lam[(size_t)b * k + t] = ldexp(v, lexp[b]);
}

// a diagonal member: thread (b, r) writes d_r at its descending rank (ties by index) if that rank is selected, and, where the
// vectors are wanted (Z != NULL), the unit vector e_r as that row of Z [batch, k, N]
__global__ __launch_bounds__(256) void stx_diag(const double* __restrict__ ds, const int* __restrict__ lexp, const int* __restrict__ diag, int N,
                                                long total, int i0, int k, const int* __restrict__ rng, double* __restrict__ lams,
                                                double* __restrict__ lam, double* __restrict__ Z) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const long b = i / N;
  if (!diag[b]) return;
  const int r = (int)(i - b * N);
  const double* db = ds + (size_t)b * N;
  const double dr = db[r];
  int rank = 0;
  for (int m = 0; m < N; ++m) { const double dm = db[m]; rank += dm > dr || (dm == dr && m < r); }
  int first, kb;
  stx_range(rng, b, i0, k, &first, &kb);
  if (rank < first || rank >= first + kb) return;
  const size_t o = (size_t)b * k + (rank - first);            // rank - first < kb <= k
  lams[o] = dr;
  lam[o] = ldexp(dr, lexp[b]);
  if (Z) {
    double* row = Z + o * N;
    for (int m = 0; m < N; ++m) row[m] = m == r ? 1.0 : 0.0;
  }
}

// head [batch, k]: the index (in the subset) of the first vector of the cluster each vector belongs to; shift [batch, k]: the
// value, moved where needed so that the shifts of one cluster are at least 10 eps g apart. One lane per member.
__global__ __launch_bounds__(64) void stx_clusters(const double* __restrict__ lams, const double* __restrict__ g, const int* __restrict__ diag,
                                                   int batch, int k, const int* __restrict__ rng, int* __restrict__ head,
                                                   double* __restrict__ shift) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= batch || diag[b]) return;
  int first, kb;
  stx_range(rng, b, 0, k, &first, &kb);
  if (kb <= 0) return;                                        // an empty interval: nothing was bisected
  const double* l = lams + (size_t)b * k;
  int* hd = head + (size_t)b * k;
  double* sh = shift + (size_t)b * k;
  const double ctol = 1e-3 * g[b], pert = (10.0 * STX_EPS) * g[b];
  int cur = 0; double prev = l[0];
  hd[0] = 0; sh[0] = prev;
  for (int j = 1; j < kb; ++j) {                              // a cluster never extends past the member's own values
    double s = l[j];
    if (l[j - 1] - s > ctol) cur = j;
    else if (prev - s < pert) s = prev - pert;
    hd[j] = cur; sh[j] = s;
    prev = s;
  }
}

__device__ __forceinline__ double stx_guard(double p, double tiny) { return fabs(p) < tiny ? copysign(tiny, p) : p; }

// One lane per (member, vector): (T - shift) x = scale z, z the start vector (round 0) or row j of Z; x overwrites that row.
// u0, u1, u2, y [batch, N, k]: the rows of U and the eliminated right-hand side.
__global__ __launch_bounds__(64) void stx_factor_solve(const double* __restrict__ ds, const double* __restrict__ es, const double* __restrict__ g,
                                                       const int* __restrict__ diag, const double* __restrict__ shift, int N, int i0, int k,
                                                       const int* __restrict__ rng, long total, int round, double* __restrict__ u0, double* __restrict__ u1,
                                                       double* __restrict__ u2, double* __restrict__ y, double* __restrict__ Z) {
  const long t = (long)blockIdx.x * 64 + threadIdx.x;
  if (t >= total) return;
  const long b = t / k;
  if (diag[b]) return;
  const int jj = (int)(t - b * k);
  int first, kb;
  stx_range(rng, b, i0, k, &first, &kb);
  if (jj >= kb) return;
  const double* D = ds + (size_t)b * N;
  const double* E = es + (size_t)b * N;
  double* z = Z + (size_t)t * N;                               // row jj of member b: t = b k + jj < batch k
  const size_t w = (size_t)b * N * k + jj;                     // row i of the workspace: w + i k < batch N k
  const double gg = g[b], tiny = STX_EPS * gg, sigma = shift[t];
  const unsigned s = stx_fmix32(STX_SEED), base = (unsigned)(first + jj) * (unsigned)N;
  double zmax = 0.0;
  for (int i = 0; i < N; ++i) zmax = fmax(zmax, fabs(round == 0 ? stx_uniform(s, base + i) : z[i]));
  const double scale = zmax > 0.0 && zmax <= DBL_MAX ? (((double)N * gg) * STX_EPS) / zmax : 1.0;
#define STX_SRC(i) ((round == 0 ? stx_uniform(s, base + (i)) : z[i]) * scale)
  double p = D[0] - sigma, sup = N > 1 ? E[0] : 0.0, yi = STX_SRC(0);
  for (int i = 0; i + 1 < N; ++i) {
    const double l = E[i], dd = D[i + 1] - sigma, ee = i + 2 < N ? E[i + 1] : 0.0, zn = STX_SRC(i + 1);
    const size_t o = w + (size_t)i * k;
    if (fabs(p) >= fabs(l)) {
      const double piv = stx_guard(p, tiny), mult = l / piv;
      u0[o] = piv; u1[o] = sup; u2[o] = 0.0; y[o] = yi;
      p = dd - mult * sup; sup = ee; yi = zn - mult * yi;
    } else {                                                   // rows i and i + 1 change places
      const double piv = stx_guard(l, tiny), mult = p / piv;
      u0[o] = piv; u1[o] = dd; u2[o] = ee; y[o] = zn;
      p = sup - mult * dd; sup = -(mult * ee); yi = yi - mult * zn;
    }
  }
#undef STX_SRC
  double x1 = yi / stx_guard(p, tiny), x2 = 0.0;
  z[N - 1] = x1;
  for (int i = N - 2; i >= 0; --i) {
    const size_t o = w + (size_t)i * k;
    const double x = ((y[o] - u1[o] * x1) - u2[o] * x2) / u0[o];
    z[i] = x; x2 = x1; x1 = x;
  }
}

// sum over the workgroup in a fixed order: lanes by the xor butterfly, then the waves' sums in wave order
__device__ __forceinline__ double stx_block_sum(double v, double* part) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  __syncthreads();                                             // part may still be read from the previous call
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = 0.0;
  for (int wv = 0; wv < STX_ORTH_THREADS / 64; ++wv) s += part[wv];
  return s;
}

// grid (k, batch), STX_ORTH_THREADS threads: see step 6 in the head of this file. Z [batch, k, N], rows = vectors, in place.
__global__ __launch_bounds__(STX_ORTH_THREADS) void stx_orth(double* __restrict__ Z, const int* __restrict__ head, const int* __restrict__ diag,
                                                             int N, int k, const int* __restrict__ rng, int last) {
  __shared__ double dots[STX_MAXN];
  __shared__ double part[STX_ORTH_THREADS / 64];
  __shared__ double pmax[STX_ORTH_THREADS / 64];
  __shared__ int pidx[STX_ORTH_THREADS / 64];
  const int jj = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int* hd = head + (size_t)b * k;
  int first, kb;
  stx_range(rng, b, 0, k, &first, &kb);
  if (diag[b] || jj >= kb || hd[jj] != jj) return;            // the whole workgroup, before any barrier
  int c = 1;
  while (jj + c < kb && hd[jj + c] == jj) ++c;                // at most kb - jj steps
  double* Zc = Z + ((size_t)b * k + jj) * N;                  // the cluster's rows: jj + c <= kb <= k
  for (int v = 0; v < c; ++v) {
    double* zv = Zc + (size_t)v * N;
    for (int pass = 0; pass < 2 && v > 0; ++pass) {
      for (int t = wave; t < v; t += STX_ORTH_THREADS / 64) { // all dots of the pass, one wave each
        const double* zt = Zc + (size_t)t * N;
        double s = 0.0;
        for (int i = lane; i < N; i += 64) s += zt[i] * zv[i];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
        if (lane == 0) dots[t] = s;                           // t < v < c <= k <= STX_MAXN
      }
      __syncthreads();
      for (int i = tid; i < N; i += STX_ORTH_THREADS) {
        double a = zv[i];
        for (int t = 0; t < v; ++t) a -= dots[t] * Zc[(size_t)t * N + i];
        zv[i] = a;
      }
      __syncthreads();
    }
    double ss = 0.0, am = -1.0; int ai = INT_MAX;
    for (int i = tid; i < N; i += STX_ORTH_THREADS) {
      const double a = zv[i];
      ss += a * a;
      if (fabs(a) > am) { am = fabs(a); ai = i; }             // ascending i: the first of equal magnitudes stays
    }
    const double nrm = sqrt(stx_block_sum(ss, part));
    double sign = 1.0;
    if (last) {
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) {
        const double om = __shfl_xor(am, off); const int oi = __shfl_xor(ai, off);
        if (om > am || (om == am && oi < ai)) { am = om; ai = oi; }
      }
      if (lane == 0) { pmax[wave] = am; pidx[wave] = ai; }
      __syncthreads();
      for (int wv = 0; wv < STX_ORTH_THREADS / 64; ++wv)
        if (pmax[wv] > am || (pmax[wv] == am && pidx[wv] < ai)) { am = pmax[wv]; ai = pidx[wv]; }
      if (ai < N && zv[ai] < 0.0) sign = -1.0;
      __syncthreads();                                        // everybody has read zv[ai] before it is rewritten
    }
    if (nrm > 0.0 && nrm <= DBL_MAX)
      for (int i = tid; i < N; i += STX_ORTH_THREADS) zv[i] = sign * (zv[i] / nrm);
    __syncthreads();                                          // the next vector of the cluster reads this one
  }
}

// HIP-event time per stage while the profile is enabled
struct StxStamps : Nd4StageStamps<STX_STAGES> {
  explicit StxStamps(nd4hip_handle* hh) : Nd4StageStamps<STX_STAGES>(hh, hh->syevx_stage_ms) {}
};

struct StxPrepared { double *ds, *es, *e2, *g; int *lexp, *diag, *flag; };

// step 1 into the caller's workspace scope
int stx_prepare_run(nd4hip_handle* h, int64_t batch, int N, const double* d, long dinc, long dstride, const double* e, long einc, long estride,
                    const u64* mx, StxPrepared* w) {
  const size_t bn = (size_t)batch * N;
  ND4_TRY(stx_alloc(h, bn, &w->ds)); ND4_TRY(stx_alloc(h, bn, &w->es)); ND4_TRY(stx_alloc(h, bn, &w->e2));
  ND4_TRY(stx_alloc(h, (size_t)batch, &w->g)); ND4_TRY(stx_alloc(h, (size_t)batch, &w->lexp)); ND4_TRY(stx_alloc(h, (size_t)batch, &w->diag));
  ND4_TRY(stx_alloc(h, 1, &w->flag));
  ND4_HIP(hipMemsetAsync(w->flag, 0, sizeof(int), h->stream));
  hipLaunchKernelGGL(stx_prepare, dim3((unsigned)batch), dim3(64), 0, h->stream, d, dinc, dstride, e, einc, estride, N, mx, w->ds, w->es, w->e2,
                     w->g, w->lexp, w->diag, w->flag);
  ND4_HIP(hipGetLastError());
  return 0;
}

// steps 1-6 for the tridiagonal members given by (d, dinc, dstride), (e, einc, estride): lambda [batch, k], Z [batch, k, N] or NULL.
// Enqueues only; *flag is the call's flag word for the caller to read back. st: marks after the values and after the vectors.
int stx_solve(nd4hip_handle* h, int64_t batch, int N, int i0, int k, const int* rng, const StxPrepared& w, double* lambda, double* Z,
              StxStamps* st);
int stx_run(nd4hip_handle* h, int64_t batch, int N, int i0, int k, const double* d, long dinc, long dstride, const double* e, long einc,
            long estride, const u64* mx, double* lambda, double* Z, StxStamps* st, int** flag) {
  StxPrepared w;
  ND4_TRY(stx_prepare_run(h, batch, N, d, dinc, dstride, e, einc, estride, mx, &w));
  *flag = w.flag;
  return stx_solve(h, batch, N, i0, k, nullptr, w, lambda, Z, st);
}

// steps 3-6 on prepared members. rng = NULL: the indices i0 .. i0 + k - 1 of every member; else rng [batch, 2] on the device holds
// each member's own range, i0 is not used and k is the largest k_b: lambda [batch, k] and Z [batch, k, N] are then written in a
// member's first k_b entries and rows only
int stx_solve(nd4hip_handle* h, int64_t batch, int N, int i0, int k, const int* rng, const StxPrepared& w, double* lambda, double* Z,
              StxStamps* st) {
  const size_t bk = (size_t)batch * k;
  double* lams = nullptr;
  ND4_TRY(stx_alloc(h, bk, &lams));
  const long total = (long)batch * N;
  hipLaunchKernelGGL(stx_diag, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, h->stream, w.ds, w.lexp, w.diag, N, total, i0, k, rng, lams,
                     lambda, Z);
  hipLaunchKernelGGL(stx_bisect, dim3((unsigned)nd4_stx_bisect_blocks(k), (unsigned)batch), dim3(256), 0, h->stream, w.ds, w.e2, w.g, w.lexp, w.diag, N, i0,
                     k, rng, lams, lambda);
  ND4_HIP(hipGetLastError());
  st->mark();
  if (Z) ND4_TRY(nd4_stx_vectors(h, batch, N, i0, k, rng, w.ds, w.es, w.g, w.diag, lams, Z));
  st->mark();
  return 0;
}

// The selection of the interval forms: range [batch, 2] (device) = (count(hi), count(lo)) of bounds [batch, 2] = (lo, hi) by one
// stx_count launch, read back once for *kmax = max_b(i1_b - i0_b) (nd4_interval_kmax refuses lo > hi); kcap < kmax is refused here,
// before anything else is launched. Synchronises.
int stx_select(nd4hip_handle* h, const char* op, int64_t batch, int N, const StxPrepared& w, const double* bounds, int64_t kcap, int32_t* range,
               int* kmax) {
  hipLaunchKernelGGL(stx_count, dim3(1, (unsigned)batch), dim3(256), 0, h->stream, w.ds, w.e2, w.lexp, N, 2L, bounds, range, 1);
  ND4_HIP(hipGetLastError());
  void* hp = nullptr;
  const size_t bytes = sizeof(int32_t) * 2 * (size_t)batch;
  ND4_TRY(nd4_pinned(h, bytes, &hp));
  ND4_HIP(hipMemcpyAsync(hp, range, bytes, hipMemcpyDeviceToHost, h->stream));
  ND4_HIP(hipStreamSynchronize(h->stream));
  int64_t km = 0;
  ND4_TRY(nd4_interval_kmax(op, batch, N, static_cast<const int32_t*>(hp), &km));
  ND4_TRY(nd4_args_kcap(op, kcap, km));
  *kmax = (int)km;
  return 0;
}

// out [batch, rows, kcap] <- src [batch, rows, k] in a member's first k_b columns (src = NULL: they stay), `fill` in the columns
// k_b .. k - 1; by_rows: the selected index is the row, out [batch, kcap, rows] <- src [batch, k, rows]. total = batch rows k.
__global__ __launch_bounds__(256) void stx_ragged(const double* __restrict__ src, const int* __restrict__ rng, long rows, int k, long kcap,
                                                  long total, int by_rows, double fill, double* __restrict__ out) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const long per = rows * k, b = i / per, r = i - b * per;    // r: (row, j) or, by_rows, (j, row) of the compact member
  const int j = (int)(by_rows ? r / rows : r % k);            // j < k <= kcap
  const long o = by_rows ? b * rows * kcap + r : b * rows * kcap + (r / k) * kcap + j;
  const int kb = rng[2 * b + 1] - rng[2 * b];
  if (j >= kb) out[o] = fill;
  else if (src) out[o] = src[i];
}
int stx_ragged_run(nd4hip_handle* h, int64_t batch, int64_t rows, int k, int64_t kcap, bool by_rows, double fill, const double* src,
                   const int32_t* range, double* out) {
  const long total = (long)batch * rows * k;
  if (total <= 0) return 0;
  hipLaunchKernelGGL(stx_ragged, dim3((unsigned)nd4_stx_ragged_blocks(batch, rows, k)), dim3(256), 0, h->stream, src, range, (long)rows, k, (long)kcap, total,
                     by_rows ? 1 : 0, fill, out);
  ND4_HIP(hipGetLastError());
  return 0;
}
constexpr double STX_NAN = __builtin_nan("");

int stx_read_flag(nd4hip_handle* h, const int* flag, int* value) {
  const int* host = nullptr;
  ND4_TRY(nd4_stx_read_flags(h, flag, 1, &host));
  *value = host[0];
  return 0;
}

}  // namespace

int nd4_stx_read_flags(nd4hip_handle* h, const int* flags, size_t count, const int** host) {
  void* hp = nullptr;
  ND4_TRY(nd4_pinned(h, sizeof(int) * count, &hp));
  ND4_HIP(hipMemcpyAsync(hp, flags, sizeof(int) * count, hipMemcpyDeviceToHost, h->stream));
  ND4_HIP(hipStreamSynchronize(h->stream));
  *host = static_cast<const int*>(hp);
  return 0;
}

// steps 4-6 (declared in syev_internal.h: bdsvdx.hip runs them on the Golub-Kahan form of a bidiagonal matrix)
int nd4_stx_vectors(nd4hip_handle* h, int64_t batch, int N, int i0, int k, const int* rng, const double* ds, const double* es, const double* g,
                    const int* diag, const double* lams, double* Z) {
  const size_t bk = (size_t)batch * k;
  int* head = nullptr; double *shift, *u0, *u1, *u2, *y;
  ND4_TRY(stx_alloc(h, bk, &head)); ND4_TRY(stx_alloc(h, bk, &shift));
  ND4_TRY(stx_alloc(h, bk * N, &u0)); ND4_TRY(stx_alloc(h, bk * N, &u1)); ND4_TRY(stx_alloc(h, bk * N, &u2)); ND4_TRY(stx_alloc(h, bk * N, &y));
  hipLaunchKernelGGL(stx_clusters, dim3((unsigned)((batch + 63) / 64)), dim3(64), 0, h->stream, lams, g, diag, (int)batch, k, rng, head, shift);
  for (int round = 0; round < 3; ++round) {
    hipLaunchKernelGGL(stx_factor_solve, dim3((unsigned)nd4_stx_solve_blocks(batch, k)), dim3(64), 0, h->stream, ds, es, g, diag, shift, N, i0, k, rng,
                       (long)bk, round, u0, u1, u2, y, Z);
    hipLaunchKernelGGL(stx_orth, dim3((unsigned)k, (unsigned)batch), dim3(STX_ORTH_THREADS), 0, h->stream, Z, head, diag, N, k, rng, round == 2);
  }
  ND4_HIP(hipGetLastError());
  return 0;
}

// count [batch, M] = #{lambda > x [batch, M]} of tridiag(d [batch, N], e [batch, N-1]); batch <= 32768, 1 <= N <= 2048. Enqueues only.
int nd4_stcnt(nd4hip_handle* h, int64_t batch, int64_t N64, int64_t M, const double* d, const double* e, const double* x, int32_t* count) {
  ND4_CHECK_ARG(N64 <= STX_MAXN && batch <= 32768 && M <= (int64_t)INT32_MAX, "nd4hip_dstcnt_batched: extent out of range");
  const int N = (int)N64;
  Nd4WsScope scope(h);
  StxPrepared w;
  ND4_TRY(stx_prepare_run(h, batch, N, d, 1, N, e, 1, N - 1, nullptr, &w));
  hipLaunchKernelGGL(stx_count, dim3((unsigned)((M + 255) / 256), (unsigned)batch), dim3(256), 0, h->stream, w.ds, w.e2, w.lexp, N, (long)M, x, count, 0);
  ND4_HIP(hipGetLastError());
  return 0;
}

// lambda [batch, k] = the eigenvalues i0 .. i1 - 1 of the descending spectrum of tridiag(d, e), Z [batch, k, N] (rows = vectors) or
// NULL; batch <= 32768, 1 <= N <= 2048, 0 <= i0 < i1 <= N. Synchronises.
int nd4_stevx(nd4hip_handle* h, int64_t batch, int64_t N64, int64_t i0, int64_t i1, const double* d, const double* e, double* lambda, double* Z) {
  ND4_CHECK_ARG(N64 <= STX_MAXN && batch <= 32768, "nd4hip_dstevx_batched: extent out of range");
  const int N = (int)N64;
  Nd4WsScope scope(h);
  StxStamps st(h);
  st.mark(); st.mark(); st.mark();                            // no symmetrisation, no reduction
  int* flag = nullptr; int bad = 0;
  ND4_TRY(stx_run(h, batch, N, (int)i0, (int)(i1 - i0), d, 1, N, e, 1, N - 1, nullptr, lambda, Z, &st, &flag));
  st.mark();
  ND4_TRY(stx_read_flag(h, flag, &bad));
  st.collect();
  h->syevx_stage_ms[0] = h->syevx_stage_ms[1] = 0.0;          // (the time between two event records, not a stage)
  if (bad) {
    nd4_set_error("tridiag_eigen(d,e): d or e contains NaN or Infinity.");
    return ND4HIP_ERR_NOCONV;
  }
  return 0;
}

// the same for the lower triangle of S [batch, N, N]: V [batch, N, k] (columns = eigenvectors) or NULL. Synchronises.
int nd4_syevx(nd4hip_handle* h, int64_t batch, int64_t N64, int64_t i0, int64_t i1, const double* S, double* lambda, double* V) {
  ND4_CHECK_ARG(N64 <= STX_MAXN && batch <= 32768, "nd4hip_dsyevx_batched: extent out of range");
  const int N = (int)N64, k = (int)(i1 - i0);
  Nd4WsScope scope(h);
  StxStamps st(h);
  int* flag = nullptr; int bad = 0;
  st.mark();
  if (N == 1) {                                               // T = S; Z [batch, 1, 1] is V
    st.mark(); st.mark();
    ND4_TRY(stx_run(h, batch, 1, (int)i0, k, S, 1, 1, nullptr, 1, 0, nullptr, lambda, V, &st, &flag));
  } else {
    const size_t nn = (size_t)N * N;
    u64* mx = nullptr; double *W, *U, *Z = nullptr;
    ND4_TRY(stx_alloc(h, (size_t)batch, &mx)); ND4_TRY(stx_alloc(h, (size_t)batch * nn, &W)); ND4_TRY(stx_alloc(h, (size_t)batch * nn, &U));
    if (V) ND4_TRY(stx_alloc(h, (size_t)batch * k * N, &Z));
    ND4_HIP(hipMemsetAsync(mx, 0, sizeof(u64) * (size_t)batch, h->stream));
    ND4_TRY(nd4_syev_symm(h, batch, N, S, W, mx));
    st.mark();
    ND4_TRY(nd4_gehrd(h, batch, N, W, U, W));                 // in place: H overwrites W; d = diag(H), e = subdiag(H)
    st.mark();
    ND4_TRY(stx_run(h, batch, N, (int)i0, k, W, N + 1, (long)nn, W + N, N + 1, (long)nn, mx, lambda, Z, &st, &flag));
    if (V) ND4_TRY(nd4_gemm(h, false, true, N, k, N, 1.0, U, N, (int64_t)nn, Z, N, (int64_t)k * N, 0.0, V, k, (int64_t)N * k, batch));
  }
  st.mark();
  ND4_TRY(stx_read_flag(h, flag, &bad));
  st.collect();
  if (bad) {
    nd4_set_error("eigen_sym(S): S contains NaN or Infinity in its lower triangle.");
    return ND4HIP_ERR_NOCONV;
  }
  return 0;
}

// The same with reduction='tridiag' (DESIGN.md 4.21): nd4_sytrd (sytrd.hip) in place of the symmetrised copy and nd4_gehrd; the
// scaled d and e stand on the diagonals of F, where stx_prepare reads them. V = Q Z^T by nd4_ormtr on the k transposed rows of Z:
// 2 N^2 k flops, no U. The symmetrise stage reads 0.
int nd4_syevx_tr(nd4hip_handle* h, int64_t batch, int64_t N64, int64_t i0, int64_t i1, const double* S, double* lambda, double* V) {
  ND4_CHECK_ARG(N64 <= STX_MAXN && batch <= 32768, "nd4hip_dsyevx_tr_batched: extent out of range");
  if (N64 == 1) return nd4_syevx(h, batch, N64, i0, i1, S, lambda, V);
  const int N = (int)N64, k = (int)(i1 - i0);
  Nd4WsScope scope(h);
  StxStamps st(h);
  int *flag = nullptr, *flag0 = nullptr; int bad = 0;         // flag0: stx_prepare raises its own word from mx as well
  const size_t nn = (size_t)N * N;
  u64* mx = nullptr; double *F, *tau, *Z = nullptr;
  ND4_TRY(stx_alloc(h, (size_t)batch, &mx)); ND4_TRY(stx_alloc(h, 1, &flag0));
  ND4_TRY(stx_alloc(h, (size_t)batch * nn, &F)); ND4_TRY(stx_alloc(h, (size_t)batch * N, &tau));
  if (V) ND4_TRY(stx_alloc(h, (size_t)batch * k * N, &Z));
  ND4_HIP(hipMemsetAsync(mx, 0, sizeof(u64) * (size_t)batch, h->stream));
  ND4_HIP(hipMemsetAsync(flag0, 0, sizeof(int), h->stream));
  st.mark(); st.mark();                                       // no symmetrisation
  ND4_TRY(nd4_sytrd(h, batch, N, S, F, tau, nullptr, nullptr, mx, false, flag0));
  st.mark();
  ND4_TRY(stx_run(h, batch, N, (int)i0, k, F, N + 1, (long)nn, F + N, N + 1, (long)nn, mx, lambda, Z, &st, &flag));
  if (V) {
    ND4_TRY(nd4_transpose(h, k, N, Z, N, V, k, batch, (int64_t)k * N, (int64_t)N * k));
    ND4_TRY(nd4_ormtr(h, batch, N, k, false, F, tau, V));
  }
  st.mark();
  ND4_TRY(stx_read_flag(h, flag, &bad));
  st.collect();
  h->syevx_stage_ms[0] = 0.0;                                 // (the time between two event records, not a stage)
  if (bad) {
    nd4_set_error("eigen_sym(S): S contains NaN or Infinity in its lower triangle.");
    return ND4HIP_ERR_NOCONV;
  }
  return 0;
}

namespace {

// Steps 2-6 of an interval form on prepared members: *kmax, range [batch, 2] and lambda [batch, kcap] are final; the compact vectors
// *Zc [batch, kmax, N] (wanted: vectors), zero in the rows past a member's k_b, are left for the caller's back-transformation.
// kmax = 0: nothing is launched after the read-back and *Zc stays NULL.
int stx_interval(nd4hip_handle* h, const char* op, int64_t batch, int N, const StxPrepared& w, const double* bounds, int64_t kcap, bool vectors,
                 double* lambda, int32_t* range, int* kmax, double** Zc, StxStamps* st) {
  *Zc = nullptr;
  ND4_TRY(stx_select(h, op, batch, N, w, bounds, kcap, range, kmax));
  const int k = *kmax;
  if (k == 0) { st->mark(); st->mark(); return 0; }
  double* lc = nullptr;
  ND4_TRY(stx_alloc(h, (size_t)batch * k, &lc));
  if (vectors) {
    ND4_TRY(stx_alloc(h, (size_t)batch * k * N, Zc));
    ND4_HIP(hipMemsetAsync(*Zc, 0, sizeof(double) * (size_t)batch * k * N, h->stream));
  }
  ND4_TRY(stx_solve(h, batch, N, 0, k, range, w, lc, *Zc, st));
  return stx_ragged_run(h, batch, 1, k, kcap, false, STX_NAN, lc, range, lambda);
}

}  // namespace

// The interval forms: the eigenvalues in (lo, hi] of every member, bounds [batch, 2] = (lo, hi) on the device.
// range [batch, 2] (device) = (i0_b, i1_b), *kmax (host) = max_b k_b; lambda [batch, kcap], Z [batch, kcap, N] (rows = vectors) or
// NULL: a member's k_b results first, then NaN / zero rows up to kmax - 1, nothing from kmax on. kcap < kmax: ND4HIP_ERR_ARG after
// the count. Arguments already checked, batch in 1 .. 32768, 1 <= N <= 2048, kcap >= 0. Synchronises.
int nd4_stevxv(nd4hip_handle* h, int64_t batch, int64_t N64, int64_t kcap, const double* bounds, const double* d, const double* e, double* lambda,
               double* Z, int32_t* range, int64_t* kmax) {
  ND4_CHECK_ARG(N64 <= STX_MAXN && batch <= 32768, "nd4hip_dstevxv_batched: extent out of range");
  const int N = (int)N64;
  Nd4WsScope scope(h);
  StxStamps st(h);
  st.mark(); st.mark(); st.mark();                            // no symmetrisation, no reduction
  StxPrepared w; int km = 0, bad = 0; double* Zc = nullptr;
  ND4_TRY(stx_prepare_run(h, batch, N, d, 1, N, e, 1, N - 1, nullptr, &w));
  ND4_TRY(stx_interval(h, "dstevxv_batched", batch, N, w, bounds, kcap, Z != nullptr, lambda, range, &km, &Zc, &st));
  *kmax = km;
  if (Zc) ND4_TRY(stx_ragged_run(h, batch, N, km, kcap, true, 0.0, Zc, range, Z));
  st.mark();
  ND4_TRY(stx_read_flag(h, w.flag, &bad));
  st.collect();
  h->syevx_stage_ms[0] = h->syevx_stage_ms[1] = 0.0;          // (the time between two event records, not a stage)
  if (bad) {
    nd4_set_error("tridiag_eigen(d,e): d or e contains NaN or Infinity.");
    return ND4HIP_ERR_NOCONV;
  }
  return 0;
}

// the same for the lower triangle of S [batch, N, N], by either reduction (tridiag: nd4_sytrd and nd4_ormtr, as nd4_syevx_tr):
// V [batch, N, kcap] (columns = eigenvectors) or NULL. The back-transformation runs on kmax columns.
int nd4_syevxv(nd4hip_handle* h, bool tridiag, int64_t batch, int64_t N64, int64_t kcap, const double* bounds, const double* S, double* lambda,
               double* V, int32_t* range, int64_t* kmax) {
  const char* op = tridiag ? "dsyevxv_tr_batched" : "dsyevxv_batched";
  ND4_CHECK_ARG(N64 <= STX_MAXN && batch <= 32768, "nd4hip_%s: extent out of range", op);
  const int N = (int)N64;
  Nd4WsScope scope(h);
  StxStamps st(h);
  StxPrepared w; int km = 0, bad = 0; double* Zc = nullptr;
  st.mark();
  if (N == 1) {                                               // T = S; Z [batch, kcap, 1] is V
    st.mark(); st.mark();
    ND4_TRY(stx_prepare_run(h, batch, 1, S, 1, 1, nullptr, 1, 0, nullptr, &w));
    ND4_TRY(stx_interval(h, op, batch, 1, w, bounds, kcap, V != nullptr, lambda, range, &km, &Zc, &st));
    if (Zc) ND4_TRY(stx_ragged_run(h, batch, 1, km, kcap, true, 0.0, Zc, range, V));
  } else {
    const size_t nn = (size_t)N * N;
    u64* mx = nullptr; double *W = nullptr, *U = nullptr, *tau = nullptr, *Vc = nullptr; int* flag0 = nullptr;
    ND4_TRY(stx_alloc(h, (size_t)batch, &mx)); ND4_TRY(stx_alloc(h, (size_t)batch * nn, &W));
    ND4_HIP(hipMemsetAsync(mx, 0, sizeof(u64) * (size_t)batch, h->stream));
    if (tridiag) {                                            // W is F: d and e on its diagonals
      ND4_TRY(stx_alloc(h, 1, &flag0)); ND4_TRY(stx_alloc(h, (size_t)batch * N, &tau));
      ND4_HIP(hipMemsetAsync(flag0, 0, sizeof(int), h->stream));
      st.mark();                                              // no symmetrisation
      ND4_TRY(nd4_sytrd(h, batch, N, S, W, tau, nullptr, nullptr, mx, false, flag0));
    } else {
      ND4_TRY(stx_alloc(h, (size_t)batch * nn, &U));
      ND4_TRY(nd4_syev_symm(h, batch, N, S, W, mx));
      st.mark();
      ND4_TRY(nd4_gehrd(h, batch, N, W, U, W));               // in place: H overwrites W; d = diag(H), e = subdiag(H)
    }
    st.mark();
    ND4_TRY(stx_prepare_run(h, batch, N, W, N + 1, (long)nn, W + N, N + 1, (long)nn, mx, &w));
    ND4_TRY(stx_interval(h, op, batch, N, w, bounds, kcap, V != nullptr, lambda, range, &km, &Zc, &st));
    if (Zc && tridiag) {                                      // nd4_ormtr works in place on dense [N, kmax] members
      ND4_TRY(stx_alloc(h, (size_t)batch * N * km, &Vc));
      ND4_TRY(nd4_transpose(h, km, N, Zc, N, Vc, km, batch, (int64_t)km * N, (int64_t)N * km));
      ND4_TRY(nd4_ormtr(h, batch, N, km, false, W, tau, Vc));
      ND4_TRY(stx_ragged_run(h, batch, N, km, kcap, false, 0.0, Vc, range, V));
    } else if (Zc) {                                          // the GEMM writes the kmax columns of V itself, rows kcap apart
      ND4_TRY(nd4_gemm(h, false, true, N, km, N, 1.0, U, N, (int64_t)nn, Zc, N, (int64_t)km * N, 0.0, V, kcap, (int64_t)N * kcap, batch));
      ND4_TRY(stx_ragged_run(h, batch, N, km, kcap, false, 0.0, nullptr, range, V));   // exact zeros past a member's k_b
    }
  }
  *kmax = km;
  st.mark();
  ND4_TRY(stx_read_flag(h, w.flag, &bad));
  st.collect();
  if (tridiag || N == 1) h->syevx_stage_ms[0] = 0.0;          // (the time between two event records, not a stage)
  if (N == 1) h->syevx_stage_ms[1] = 0.0;
  if (bad) {
    nd4_set_error("eigen_sym(S): S contains NaN or Infinity in its lower triangle.");
    return ND4HIP_ERR_NOCONV;
  }
  return 0;
}

// NaN (lambda) and zeros (vectors; by_rows: Z [batch, kcap, N], else V [batch, N, kcap]) in the columns k_b .. kmax - 1 of every
// member: what the entry points run when the chunks of a large batch found different kmax. Enqueues only.
int nd4_stxv_pad(nd4hip_handle* h, int64_t batch, int64_t N, int64_t kcap, int64_t kmax, const int32_t* range, double* lambda, double* vectors,
                 bool by_rows) {
  for (int64_t b0 = 0; b0 < batch; b0 += 32768) {
    const int64_t nb = batch - b0 < 32768 ? batch - b0 : 32768;
    ND4_TRY(stx_ragged_run(h, nb, 1, (int)kmax, kcap, false, STX_NAN, nullptr, range + 2 * b0, lambda + b0 * kcap));
    if (vectors) ND4_TRY(stx_ragged_run(h, nb, N, (int)kmax, kcap, by_rows, 0.0, nullptr, range + 2 * b0, vectors + b0 * N * kcap));
  }
  return 0;
}
