// The direct parts of the nonsymmetric eigenproblem (src/la/schur.js:31-370, src/la/eigen.js:91-270) for gfx950: eigenvalues and
// eigenvectors of a real Schur form, and balancing before / after. The Francis iteration (schur_decomp) is in schur.hip.
//
//   schur_eigenvals (schur.js:31-87): one lane per matrix walks the diagonal right to left with the reference's block test
//       (1x1 iff j == 0 or T[j,j-1] == 0) and its 2x2 formula; it also records each row's block type for the eigenvector kernel.
//       A 2x2 block with real eigenvalues (sqr >= 0) raises bit EV_FLAG_REAL2X2 of the matrix's flag word.
//   schur_eigen (schur.js:90-370): the reference overwrites V = T column by column from the right, but a later column reads an
//       earlier one only through a product with an exact zero (the k = J+1 term of a 1x1 column), so given the original T the
//       columns are independent: one lane per eigenvector column runs computeVec (:170-247) in the reference's own order: k
//       descending, separate real and imaginary updates, the same divisions, no contraction. The column lives in the output
//       buffer (lane c owns column c: neighbouring lanes touch neighbouring addresses).
//         N <= EV_LDS_MAX : one workgroup (one wave) per matrix, T staged in LDS. The lane's column stays in the output buffer
//                           (global memory, L2-resident): T (32 KiB at N = 64) and 64 columns of 64 complex values (64 KiB)
//                           do not fit the 64 KiB of LDS together beyond N = 45, and one path for all N <= 64 was preferred.
//         larger N        : the blocked tier, a multi-shift blocked back-substitution with row blocks of EV_NB = 64 rows that
//                           start at multiples of EV_NB (one row earlier where a 2x2 block would be split), walked from the
//                           bottom. Per block [j0, j1): evb_diag solves the block's rows for ALL columns c >= j0 at once, one
//                           lane per column with its own shift (the TOL branches and the 2x2 solves included), reading what
//                           the rows below have accumulated into X; then one real GEMM on the 2(N - j0) wide real view,
//                           X[0:j0, c >= j0] -= T[0:j0, j0:j1] X[j0:j1, c >= j0], moves the block's contribution to the rows
//                           above. A column that RESTARTS at row j is cleared by evb_diag itself, in the same pass: its rows
//                           below j (in the block and below it) and every row above j, where contributions of the discarded
//                           vector had already been accumulated; the block's GEMM then starts from the new e_j. The blocks of
//                           each matrix follow its own 2x2 structure, so the block types are read back once per call and the
//                           launches are issued per matrix. Sums run in another order than the reference's (the rows below a
//                           block first), so this tier is within rounding of the reference, not bit-identical.
//       TOL = sqrt(eps) ||T||_F (:254-269) is a block reduction of (max, sum) pairs, so it may differ from the reference's
//       left-to-right sum in the last bits; it only enters `<= TOL` tests. A NaN TOL or a zero 2x2 determinant (:233, :270) raises
//       EV_FLAG_ASSERT. Column norms (:338-363) are one lane per column in the reference's order, so they are its bits; then
//       Q V runs as the real GEMM on the N x 2N view of V.
//   eigen_balance_pre (eigen.js:91-226): one workgroup per matrix, Gauss-Seidel over i as the reference: block-reduced scaled
//       p-norms of the off-diagonal row and column, lane 0 takes the reference's decisions, the block scales row i and column i.
//   eigen_balance_post (eigen.js:229-270): V[i,:] *= D[i], then the same column-norm kernel as schur_eigen.
#include "nd4hip_internal.h"
#include <cmath>
#include <vector>

namespace {

constexpr int WAVE = 64;
constexpr int EV_LDS_MAX = 64;        // T in LDS up to here (32 KiB), one wave per matrix; the blocked tier beyond
constexpr int BAL_MAX_SWEEPS = 1024;  // a guard for the shared device, documented in nd4hip.h: the reference loops until a sweep changes nothing
constexpr int EV_NB = 64;             // row-block height of the blocked tier
constexpr int RED_THREADS = 256;

#pragma clang fp contract(off)

struct Cx { double re, im; };
__device__ inline Cx cmul(Cx a, Cx b) { return Cx{a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re}; }       // '= c0*c1'
__device__ inline void cmsub(Cx& x, Cx a, Cx b) { x.re -= a.re * b.re - a.im * b.im; x.im -= a.re * b.im + a.im * b.re; }   // '-= c0*c1'
__device__ inline void cdiv(Cx& x, double re, double im) {                                                        // '/=' (mutable_complex.js:31-48)
  if (im == 0.0) { x.re /= re; x.im /= re; return; }
  const double xr = x.re;
  if (fabs(re) >= fabs(im)) { const double R = im / re; x.re = (xr + x.im * R) / (re + im * R); x.im = (x.im - xr * R) / (re + im * R); }
  else                      { const double R = re / im; x.re = (xr * R + x.im) / (re * R + im); x.im = (x.im * R - xr) / (re * R + im); }
}

// ------------------------------------------------------------------------------------------------ schur_eigenvals
__global__ __launch_bounds__(256) void ev_vals(int64_t batch, int N, const double* __restrict__ T, double* __restrict__ Lam,
                                               int* __restrict__ blk, int* __restrict__ flags) {
  const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= batch) return;
  const double* t = T + b * N * N;
  double* lam = Lam + 2 * b * N;
  int flag = 0;
  for (int j = N - 1; j >= 0; j--) {
    const int i = j - 1;
    if (j == 0 || t[(long)j * N + i] == 0.0) {
      lam[2 * j] = t[(long)j * N + j]; lam[2 * j + 1] = 0.0;
      if (blk) blk[b * N + j] = 0;
    } else {
      const double Tii = t[(long)i * N + i], Tij = t[(long)i * N + j], Tji = t[(long)j * N + i], Tjj = t[(long)j * N + j];
      const double diag = Tii - Tjj, tr = Tii + Tjj, sqr = diag * diag + (4.0 * Tij) * Tji;
      if (sqr >= 0.0) flag |= ND4HIP_EV_FLAG_REAL2X2;
      const double s = 0.5 * sqrt((fabs(sqr) - sqr) * 0.5), half = 0.5 * tr;      // Complex.sqrt of (sqr, 0), sqr < 0: (0, sqrt(|sqr|))
      lam[2 * i] = half; lam[2 * i + 1] = s;
      lam[2 * j] = half; lam[2 * j + 1] = 0.0 - s;
      if (blk) { blk[b * N + i] = 1; blk[b * N + j] = 2; }
      j--;
    }
  }
  flags[b] = flag;
}

// ------------------------------------------------------------------------------------------------ TOL = sqrt(eps) ||T||_F
__device__ inline void fro_merge(double& m, double& s, double m2, double s2) {
  if (m2 > m)        { const double q = m / m2; s = s * (q * q) + s2; m = m2; }
  else if (m > 0.0)  { const double q = m2 / m; s = s + s2 * (q * q); }
  else s += s2;                                                                   // both maxima 0 (or NaN sums, which stay NaN)
}

__global__ __launch_bounds__(RED_THREADS) void ev_tol(int N, const double* __restrict__ T, double* __restrict__ tol, int* __restrict__ flags) {
  __shared__ double shm[RED_THREADS], shs[RED_THREADS];
  const int64_t b = blockIdx.x;
  const double* t = T + b * N * N;
  const long n = (long)N * N;
  double sum = 0.0, mx = 0.0;
  for (long e = threadIdx.x; e < n; e += RED_THREADS) {
    const double elem = fabs(t[e]);
    if (elem != 0.0) {                                                            // NaN makes the sum NaN
      if (elem > mx) { const double q = mx / elem; sum *= q * q; mx = elem; }
      const double q = elem / mx; sum += q * q;
    }
  }
  shm[threadIdx.x] = mx; shs[threadIdx.x] = sum;
  __syncthreads();
  for (int w = RED_THREADS / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) { double m = shm[threadIdx.x], s = shs[threadIdx.x]; fro_merge(m, s, shm[threadIdx.x + w], shs[threadIdx.x + w]); shm[threadIdx.x] = m; shs[threadIdx.x] = s; }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const double TOL = 1.4901161193847656e-08 * (sqrt(shs[0]) * shm[0]);           // sqrt(Number.EPSILON) = 2^-26
    tol[b] = TOL;
    if (!(TOL >= 0.0)) flags[b] |= ND4HIP_EV_FLAG_ASSERT;
  }
}

// ------------------------------------------------------------------------------------------------ eigenvectors of T, unnormalised
// X [batch, N, N] complex; lane c of the grid's x axis owns column c. computeVec (schur.js:170-247) per column.
__global__ __launch_bounds__(WAVE) void ev_vecs(int N, const double* __restrict__ T, const double* __restrict__ Lam, const int* __restrict__ blk,
                                                const double* __restrict__ tolp, double* __restrict__ X, int* __restrict__ flags) {
  extern __shared__ double sh[];
  const int64_t b = blockIdx.y;
  const int c = blockIdx.x * WAVE + threadIdx.x;
  const double* tg = T + b * N * N;
  for (int e = threadIdx.x; e < N * N; e += WAVE) sh[e] = tg[e];
  __syncthreads();
  const double* t = sh;
  if (c >= N) return;
  double* v = X + 2 * (b * N * N + c);
  const long vs = 2L * N;                                                         // doubles between rows of one column
  const double tol = tolp[b];
  const int type = blk[b * N + c];
  const Cx lam{Lam[2 * (b * N + c)], Lam[2 * (b * N + c) + 1]};
  const double Z = 0.0;                                                           // the imaginary part of every entry of T
  int J, K;                                                                       // rows < J are solved for; rows >= K are never read
  if (type == 0) {                                                                // 1x1 block: e_c
    J = c; K = c + 1;
    for (int r = 0; r < N; r++) {
      const double x = r < c ? 0.0 : r == c ? 1.0 : r == c + 1 ? 0.0 : tg[(long)r * N + c];   // below: what the reference leaves of T
      v[r * vs] = x; v[r * vs + 1] = 0.0;
    }
  } else {                                                                        // 2x2 block (i, j): the 2-vector of schur.js:318-323
    const int i = type == 1 ? c : c - 1, j = i + 1;
    J = i; K = j + 1;
    for (int r = 0; r < N; r++) { v[r * vs] = r <= j ? 0.0 : tg[(long)r * N + c]; v[r * vs + 1] = 0.0; }
    const double Tii = t[i * N + i], Tij = t[i * N + j], Tji = t[j * N + i], Tjj = t[j * N + j];
    if (fabs(Tij) >= fabs(Tji)) { v[i * vs] = Tij; v[j * vs] = lam.re - Tii; v[j * vs + 1] = lam.im; }
    else                        { v[j * vs] = Tji; v[i * vs] = lam.re - Tjj; v[i * vs + 1] = lam.im; }
  }
  bool bad = false;
  for (int j = J; j-- > 0;) {
    Cx vj{0.0, 0.0};
    for (int k = K; --k > j;) cmsub(vj, Cx{v[k * vs], v[k * vs + 1]}, Cx{t[j * N + k], Z});
    if (j == 0 || t[j * N + j - 1] == 0.0) {                                      // 1x1 pivot
      const double dre = t[j * N + j] - lam.re, dim = Z - lam.im;
      if (hypot(dre, dim) <= tol) {
        if (hypot(vj.re, vj.im) <= tol) vj = Cx{0.0, 0.0};                        // already an eigenvector
        else {                                                                    // restart at row j
          vj = Cx{1.0, 0.0};
          for (int k = j + 1; k < K; k++) { v[k * vs] = 0.0; v[k * vs + 1] = 0.0; }
        }
      } else cdiv(vj, dre, dim);
      v[j * vs] = vj.re; v[j * vs + 1] = vj.im;
    } else {                                                                      // 2x2 pivot: complex Cramer (schur.js:221-243)
      const int i = j - 1;
      Cx vi{0.0, 0.0};
      for (int k = K; --k > j;) cmsub(vi, Cx{v[k * vs], v[k * vs + 1]}, Cx{t[i * N + k], Z});
      const Cx Tii{t[i * N + i] - lam.re, Z - lam.im}, Tjj{t[j * N + j] - lam.re, Z - lam.im}, Tij{t[i * N + j], Z}, Tji{t[j * N + i], Z};
      Cx det = cmul(Tii, Tjj);
      cmsub(det, Tij, Tji);
      if (det.re == 0.0 && det.im == 0.0) bad = true;
      Cx nj = cmul(Tii, vj); cmsub(nj, Tji, vi); cdiv(nj, det.re, det.im);
      Cx ni = cmul(Tjj, vi); cmsub(ni, Tij, vj); cdiv(ni, det.re, det.im);
      v[i * vs] = ni.re; v[i * vs + 1] = ni.im;
      v[j * vs] = nj.re; v[j * vs + 1] = nj.im;
      j--;
    }
  }
  if (bad) atomicOr(&flags[b], ND4HIP_EV_FLAG_ASSERT);
}

// ------------------------------------------------------------------------------------------------ the blocked tier (N > EV_LDS_MAX)
// One matrix per launch in y = 0 form: T, Lam, blk, X, flags point at the matrix. Start vectors of all columns, zero elsewhere
// (the GEMMs multiply the rows below a column's start, so they must be zero, not what the reference leaves of T there).
__global__ __launch_bounds__(WAVE) void evb_init(int N, const double* __restrict__ T, const double* __restrict__ Lam, const int* __restrict__ blk,
                                                 double* __restrict__ X) {
  const int64_t b = blockIdx.y;
  const int c = blockIdx.x * WAVE + threadIdx.x;
  if (c >= N) return;
  const double* t = T + b * N * N;
  double* v = X + 2 * (b * N * N + c);
  const long vs = 2L * N;
  for (int r = 0; r < N; r++) { v[r * vs] = 0.0; v[r * vs + 1] = 0.0; }
  const int type = blk[b * N + c];
  if (type == 0) { v[c * vs] = 1.0; return; }
  const int i = type == 1 ? c : c - 1, j = i + 1;
  const double lre = Lam[2 * (b * N + c)], lim = Lam[2 * (b * N + c) + 1];
  const double Tii = t[(long)i * N + i], Tij = t[(long)i * N + j], Tji = t[(long)j * N + i], Tjj = t[(long)j * N + j];
  if (fabs(Tij) >= fabs(Tji)) { v[i * vs] = Tij; v[j * vs] = lre - Tii; v[j * vs + 1] = lim; }
  else                        { v[j * vs] = Tji; v[i * vs] = lre - Tjj; v[i * vs + 1] = lim; }
}

// rows [j0, j1) of every column c >= j0 of ONE matrix: X[j, c] holds minus the sum over the rows k >= j1 already (the GEMMs of the
// blocks below); the in-block part of the sum and the pivot solves are computeVec's, per lane with its own shift
__global__ __launch_bounds__(WAVE) void evb_diag(int N, int j0, int j1, const double* __restrict__ t, const double* __restrict__ Lam,
                                                 const int* __restrict__ blk, const double* __restrict__ tolp, double* __restrict__ X,
                                                 int* __restrict__ flag) {
  const int c = j0 + blockIdx.x * WAVE + threadIdx.x;
  if (c >= N) return;
  const int type = blk[c];
  const int J = type == 2 ? c - 1 : c, K = type == 0 ? c + 1 : J + 2;            // rows < J are solved for; rows >= K are zero
  const int jtop = J < j1 ? J : j1, kin = K < j1 ? K : j1;
  if (jtop <= j0) return;
  double* v = X + 2 * (long)c;
  const long vs = 2L * N;
  const double tol = *tolp, Z = 0.0;
  const Cx lam{Lam[2 * c], Lam[2 * c + 1]};
  bool bad = false;
  for (int j = jtop; j-- > j0;) {
    Cx vj{v[j * vs], v[j * vs + 1]};
    for (int k = kin; --k > j;) cmsub(vj, Cx{v[k * vs], v[k * vs + 1]}, Cx{t[(long)j * N + k], Z});
    if (j == 0 || t[(long)j * N + j - 1] == 0.0) {
      const double dre = t[(long)j * N + j] - lam.re, dim = Z - lam.im;
      if (hypot(dre, dim) <= tol) {
        if (hypot(vj.re, vj.im) <= tol) vj = Cx{0.0, 0.0};
        else {                                                                    // restart at row j: e_j, and nothing of the old vector stays
          vj = Cx{1.0, 0.0};
          for (int k = j + 1; k < K; k++) { v[k * vs] = 0.0; v[k * vs + 1] = 0.0; }
          for (int r = 0; r < j; r++) { v[r * vs] = 0.0; v[r * vs + 1] = 0.0; }   // accumulated from the discarded vector (rows < j0 too)
        }
      } else cdiv(vj, dre, dim);
      v[j * vs] = vj.re; v[j * vs + 1] = vj.im;
    } else {
      const int i = j - 1;
      Cx vi{v[i * vs], v[i * vs + 1]};
      for (int k = kin; --k > j;) cmsub(vi, Cx{v[k * vs], v[k * vs + 1]}, Cx{t[(long)i * N + k], Z});
      const Cx Tii{t[(long)i * N + i] - lam.re, Z - lam.im}, Tjj{t[(long)j * N + j] - lam.re, Z - lam.im}, Tij{t[(long)i * N + j], Z}, Tji{t[(long)j * N + i], Z};
      Cx det = cmul(Tii, Tjj);
      cmsub(det, Tij, Tji);
      if (det.re == 0.0 && det.im == 0.0) bad = true;
      Cx nj = cmul(Tii, vj); cmsub(nj, Tji, vi); cdiv(nj, det.re, det.im);
      Cx ni = cmul(Tjj, vi); cmsub(ni, Tij, vj); cdiv(ni, det.re, det.im);
      v[i * vs] = ni.re; v[i * vs + 1] = ni.im;
      v[j * vs] = nj.re; v[j * vs + 1] = nj.im;
      j--;
    }
  }
  if (bad) atomicOr(flag, ND4HIP_EV_FLAG_ASSERT);
}

// ------------------------------------------------------------------------------------------------ column norms (schur.js:338-363)
// X [batch, N, N] complex, in place: every column divided by its scaled 2-norm over the 2N real parts, in the reference's order
__global__ __launch_bounds__(WAVE) void ev_colnorm(int N, double* __restrict__ X) {
  const int64_t b = blockIdx.y;
  const int c = blockIdx.x * WAVE + threadIdx.x;
  if (c >= N) return;
  double* v = X + 2 * (b * N * N + c);
  const long vs = 2L * N;
  double sum = 0.0, mx = 0.0;
  for (int i = 0; i < N; i++)
    for (int part = 0; part < 2; part++) {
      const double a = fabs(v[i * vs + part]);
      if (a > 0.0) {
        if (a > mx) { const double scale = mx / a; mx = a; sum *= scale * scale; }
        const double ratio = a / mx;
        sum += ratio * ratio;
      }
    }
  const double norm = isfinite(mx) ? sqrt(sum) * mx : mx;
  for (int i = 0; i < N; i++) { v[i * vs] /= norm; v[i * vs + 1] /= norm; }
}

// ------------------------------------------------------------------------------------------------ eigen_balance_pre
__device__ inline double js_max(double a, double b) { return (a != a || b != b) ? __longlong_as_double(0x7ff8000000000000ll) : (a < b ? b : a); }
__device__ inline double powp(double x, double p) { return p == 2.0 ? x * x : p == 1.0 ? x : pow(x, p); }
__device__ inline double rootp(double x, double p) { return p == 2.0 ? sqrt(x) : p == 1.0 ? x : pow(x, 1.0 / p); }

// (max, sum of (|x| / max)^p) pairs; INF: the max alone
template <bool INF>
__device__ inline void bal_add(double& m, double& s, double a, double p) {
  if (INF) { m = js_max(m, a); return; }
  if (a > 0.0) {
    if (a > m) { const double scale = m / a; m = a; s *= powp(scale, p); }
    const double ratio = a / m;
    s += powp(ratio, p);
  }
}
template <bool INF>
__device__ inline void bal_merge(double& m, double& s, double m2, double s2, double p) {
  if (INF) { m = js_max(m, m2); return; }
  if (m2 > m)       { s = s * powp(m / m2, p) + s2; m = m2; }
  else if (m > 0.0) { s = s + s2 * powp(m2 / m, p); }
  else s += s2;
}

template <bool INF>
__global__ __launch_bounds__(RED_THREADS) void bal_pre(int N, double p, double TOL, const double* __restrict__ A, double* __restrict__ D,
                                                       double* __restrict__ B, int* __restrict__ flags) {
  __shared__ double rm[RED_THREADS], rs[RED_THREADS], cm[RED_THREADS], cs[RED_THREADS];
  __shared__ double s_scale;
  __shared__ int s_act, s_done;                                                   // s_act: 0 skip, 1 scale, 2 the reference throws
  const int64_t bi = blockIdx.x;
  const int tid = threadIdx.x;
  const double* a = A + bi * N * N;
  double* bm = B + bi * N * N;
  double* d = D + bi * N;
  for (long e = tid; e < (long)N * N; e += RED_THREADS) bm[e] = a[e];
  for (int e = tid; e < N; e += RED_THREADS) d[e] = 1.0;
  __syncthreads();
  for (int sweep = 0;; sweep++) {
    if (sweep == BAL_MAX_SWEEPS) { if (tid == 0) flags[bi] |= ND4HIP_EV_FLAG_SWEEPS; return; }
    if (tid == 0) s_done = 1;
    for (int i = 0; i < N; i++) {
      double r_max = 0.0, r = 0.0, c_max = 0.0, c = 0.0;
      for (int j = tid; j < N; j += RED_THREADS)
        if (j != i) {
          bal_add<INF>(r_max, r, fabs(bm[(long)i * N + j]), p);
          bal_add<INF>(c_max, c, fabs(bm[(long)j * N + i]), p);
        }
      rm[tid] = r_max; rs[tid] = r; cm[tid] = c_max; cs[tid] = c;
      __syncthreads();
      for (int w = RED_THREADS / 2; w > 0; w >>= 1) {
        if (tid < w) {
          double m = rm[tid], s = rs[tid]; bal_merge<INF>(m, s, rm[tid + w], rs[tid + w], p); rm[tid] = m; rs[tid] = s;
          m = cm[tid]; s = cs[tid];        bal_merge<INF>(m, s, cm[tid + w], cs[tid + w], p); cm[tid] = m; cs[tid] = s;
        }
        __syncthreads();
      }
      if (tid == 0) {
        int act = 0;
        double scale = 1.0;
        if (INF) {
          r = rm[0]; c = cm[0];
          if (!(r * c == 0.0)) {
            const double old_norm = js_max(c, r);
            if (!isfinite(old_norm)) act = 2;
            else {
              while (r >= c * 2) { c *= 2; r /= 2; scale *= 2; }
              while (c >= r * 2) { c /= 2; r *= 2; scale /= 2; }
              if (!(js_max(c, r) >= old_norm)) act = 1;
            }
          }
        } else {
          r = !isfinite(rs[0]) ? rs[0] : rootp(rs[0], p) * rm[0];
          c = !isfinite(cs[0]) ? cs[0] : rootp(cs[0], p) * cm[0];
          if (!(r * c == 0.0)) {
            if (!isfinite(r * c)) act = 2;
            else {
              const double old_norm = c >= r ? rootp(1 + powp(r / c, p), p) * c : rootp(1 + powp(c / r, p), p) * r;
              while (r >= c * 2) { c *= 2; r /= 2; scale *= 2; }
              while (c >= r * 2) { c /= 2; r *= 2; scale /= 2; }
              const double new_norm = c >= r ? rootp(1 + powp(r / c, p), p) * c : rootp(1 + powp(c / r, p), p) * r;
              if (!(new_norm >= TOL * old_norm)) act = 1;
            }
          }
        }
        s_act = act; s_scale = scale;
        if (act == 1) { s_done = 0; d[i] *= scale; }
      }
      __syncthreads();
      const int act = s_act;
      if (act == 2) { if (tid == 0) flags[bi] |= ND4HIP_EV_FLAG_NAN; return; }
      if (act == 1) {
        const double scale = s_scale;
        for (int j = tid; j < N; j += RED_THREADS) {
          bm[(long)i * N + j] /= scale;
          bm[(long)j * N + i] *= scale;
        }
      }
      __syncthreads();
    }
    const int done = s_done;
    __syncthreads();
    if (done) return;
  }
}

// ------------------------------------------------------------------------------------------------ eigen_balance_post: W = diag(D) V
__global__ __launch_bounds__(256) void bal_post_scale(int N, const double* __restrict__ D, const double* __restrict__ V, double* __restrict__ W) {
  const int64_t b = blockIdx.y;
  const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (long)N * N) return;
  const double dd = D[b * N + e / N], re = V[2 * (b * N * N + e)], im = V[2 * (b * N * N + e) + 1];
  W[2 * (b * N * N + e)] = re * dd - im * 0.0;                                    // Complex.mul(D, 0)
  W[2 * (b * N * N + e) + 1] = re * 0.0 + im * dd;
}

}  // namespace

// schur_eigenvals of [batch] matrices T [N, N] (any batch here; nd4_trevc calls it per chunk): Lam [batch, N] complex, blk
// [batch, N] (may be NULL) the block type of every row (0: 1x1, 1 / 2: first / second row of a 2x2 block), flags [batch] overwritten
int nd4_trevals(nd4hip_handle* h, int64_t batch, int64_t N, const double* T, double* Lam, int* blk, int* flags) {
  if (batch == 0) return 0;
  hipLaunchKernelGGL(ev_vals, dim3((unsigned)((batch + 255) / 256)), dim3(256), 0, h->stream, batch, (int)N, T, Lam, blk, flags);
  ND4_HIP(hipGetLastError());
  return 0;
}

// schur_eigen: Lam [batch, N], V = Q X [batch, N, N] complex, X the normalised eigenvectors of T; flags [batch] overwritten.
// batch <= 65535 (the grids' y axis): the entry points call this per chunk of ND4_CHUNK = 32768 matrices. N > EV_LDS_MAX synchronises once.
int nd4_trevc(nd4hip_handle* h, int64_t batch, int64_t N, const double* Q, const double* T, double* Lam, double* V, int* flags) {
  if (batch == 0) return 0;
  if (N == 0) { ND4_HIP(hipMemsetAsync(flags, 0, sizeof(int) * (size_t)batch, h->stream)); return 0; }
  Nd4WsScope scope(h);
  void *px = nullptr, *pt = nullptr, *pb = nullptr;
  ND4_TRY(nd4_ws_alloc(h, 2 * sizeof(double) * (size_t)batch * N * N, &px));
  ND4_TRY(nd4_ws_alloc(h, sizeof(double) * (size_t)batch, &pt));
  ND4_TRY(nd4_ws_alloc(h, sizeof(int) * (size_t)batch * N, &pb));
  double* X = static_cast<double*>(px);
  double* tol = static_cast<double*>(pt);
  int* blk = static_cast<int*>(pb);
  ND4_TRY(nd4_trevals(h, batch, N, T, Lam, blk, flags));
  hipLaunchKernelGGL(ev_tol, dim3((unsigned)batch), dim3(RED_THREADS), 0, h->stream, (int)N, T, tol, flags);
  ND4_HIP(hipGetLastError());
  const dim3 grid((unsigned)((N + WAVE - 1) / WAVE), (unsigned)batch);
  if (N <= EV_LDS_MAX) {
    hipLaunchKernelGGL(ev_vecs, grid, dim3(WAVE), sizeof(double) * N * N, h->stream, (int)N, T, Lam, blk, tol, X, flags);
    ND4_HIP(hipGetLastError());
  } else {
    // the row blocks follow each matrix's own 2x2 structure: one small read-back of the block types, then launches per matrix
    std::vector<int> hb((size_t)batch * N);
    ND4_HIP(hipMemcpyAsync(hb.data(), blk, sizeof(int) * hb.size(), hipMemcpyDeviceToHost, h->stream));
    ND4_HIP(hipStreamSynchronize(h->stream));
    hipLaunchKernelGGL(evb_init, grid, dim3(WAVE), 0, h->stream, (int)N, T, Lam, blk, X);
    ND4_HIP(hipGetLastError());
    for (int64_t b = 0; b < batch; b++) {
      const double* t = T + b * N * N;
      double* x = X + 2 * b * N * N;
      for (int64_t j1 = N, j0; j1 > 0; j1 = j0) {
        j0 = (j1 - 1) / EV_NB * EV_NB;
        if (j0 > 0 && hb[(size_t)(b * N + j0)] == 2) j0--;                        // never split a 2x2 block
        hipLaunchKernelGGL(evb_diag, dim3((unsigned)((N - j0 + WAVE - 1) / WAVE)), dim3(WAVE), 0, h->stream, (int)N, (int)j0, (int)j1, t,
                           Lam + 2 * b * N, blk + b * N, tol + b, x, flags + b);
        ND4_HIP(hipGetLastError());
        if (j0 > 0)   // X[0:j0, c >= j0] -= T[0:j0, j0:j1] X[j0:j1, c >= j0] on the real view (the RC form: real GEMM, 2J columns)
          ND4_TRY(nd4_gemm(h, false, false, j0, 2 * (N - j0), j1 - j0, -1.0, t + j0, N, 0, x + 2 * (j0 * N + j0), 2 * N, 0,
                           1.0, x + 2 * j0, 2 * N, 0, 1));
      }
    }
  }
  hipLaunchKernelGGL(ev_colnorm, grid, dim3(WAVE), 0, h->stream, (int)N, X);
  ND4_HIP(hipGetLastError());
  // Q (N x N real) times the N x 2N real view of X
  return nd4_gemm(h, false, false, N, 2 * N, N, 1.0, Q, N, N * N, X, 2 * N, 2 * N * N, 0.0, V, 2 * N, 2 * N * N, batch);
}

// eigen_balance_pre: D [batch, N], B [batch, N, N]; p >= 1 or +Infinity (the max-norm variant); flags [batch] must be zero on entry
int nd4_gebal(nd4hip_handle* h, int64_t batch, int64_t N, double p, const double* A, double* D, double* B, int* flags) {
  if (batch == 0 || N == 0) return 0;
  const dim3 grid((unsigned)batch), block(RED_THREADS);
  if (p > 1.79769313486231570e308) hipLaunchKernelGGL(bal_pre<true>, grid, block, 0, h->stream, (int)N, p, 1.0, A, D, B, flags);
  else hipLaunchKernelGGL(bal_pre<false>, grid, block, 0, h->stream, (int)N, p, std::pow(0.95, 1.0 / p), A, D, B, flags);
  ND4_HIP(hipGetLastError());
  return 0;
}

// eigen_balance_post: W = diag(D) V with unit columns; V, W [batch, N, N] complex, distinct
int nd4_gebak(nd4hip_handle* h, int64_t batch, int64_t N, const double* D, const double* V, double* W) {
  if (batch == 0 || N == 0) return 0;
  hipLaunchKernelGGL(bal_post_scale, dim3((unsigned)((N * N + 255) / 256), (unsigned)batch), dim3(256), 0, h->stream, (int)N, D, V, W);
  hipLaunchKernelGGL(ev_colnorm, dim3((unsigned)((N + WAVE - 1) / WAVE), (unsigned)batch), dim3(WAVE), 0, h->stream, (int)N, W);
  ND4_HIP(hipGetLastError());
  return 0;
}
