// Strong rank-revealing QR (srrqr_decomp_full, src/la/srrqr.js:58-802): Gu-Eisenstat column swaps under a binary search over
// the rank.
//
// The decision pass decides P and the rank r only. ONE workgroup per matrix runs the reference's whole state machine (the
// binary-search bounds k0 / k / K, the search for the best swap, the cyclic shift and retriangulation, the eliminations) on a
// column-major workspace of the scaled A; the batch is the grid. Nothing waits on another workgroup, and every loop has a static
// bound: a matrix that hits the cap stops with rank -2 (the host form turns that into ND4HIP_ERR_NOCONV).
//   * R lives in W (column j of R at W + cm[j] M): the column swaps and cyclic shifts of the reference move the index map cm,
//     not the data. The rows a shift would move below the diagonal are zero, so the map is the same matrix.
//   * inv(A_k) and A_k \ B_k are kept in AB / AB0 exactly as the reference keeps them (its update, downdate, cycle and
//     Givens steps, :236-281, :400-412, :670-782), so every F_ij is computed from the same quantities.
//   * The eliminations (piv_elim, swap_elim) use a Householder reflector where the reference uses Givens rotations: row k of R
//     and the trailing block then differ by signs and an orthogonal transform of rows > k, to which the column norms, the
//     A \ B quotients and the inverse row norms (everything a decision reads) are invariant. A column whose part below the
//     diagonal is exactly zero is left untouched, as the reference's rotations leave it.
// Reductions are fixed: a butterfly inside a wave, then the waves in index order in one thread; no atomics. Q and R are the
// full QR (dgeqrf_full) of A[:, P]; R[r:, r:] is therefore triangular where the reference leaves it untriangularised.
#include "nd4hip_internal.h"
#include <climits>
#include <algorithm>
#include <cmath>

namespace {

constexpr int WAVE = 64;
constexpr int NT = 1024;              // threads per matrix
constexpr int NW = NT / WAVE;

__device__ inline double wave_sum(double x) {
  for (int o = WAVE / 2; o > 0; o >>= 1) x += __shfl_xor(x, o, WAVE);
  return x;
}
__device__ inline double nan_max(double a, double b) { return (a != a) ? a : ((b != b) ? b : (a > b ? a : b)); }
__device__ inline double wave_max(double x) {
  for (int o = WAVE / 2; o > 0; o >>= 1) x = nan_max(x, __shfl_xor(x, o, WAVE));
  return x;
}
__device__ inline int norm_exp(double mx) { return (mx > 0.0 && mx <= 1.79769313486231570e308) ? ilogb(mx) : 0; }
__device__ inline double norm_finish(double mx, double s, int e) {
  if (!(mx <= 1.79769313486231570e308)) return mx;
  if (mx == 0.0) return 0.0;
  return ldexp(sqrt(s), e);
}

struct Shared {
  double red[NW];
  int ired[NW];
  double bc[4];
  int ibc[4];
};

// ||x|| over x(t), t in [0, n), the whole block; every thread returns the same value
template <class F>
__device__ double block_norm(Shared& sh, int n, F x) {
  const int t = threadIdx.x, lane = t & (WAVE - 1), wv = t >> 6;
  double mx = 0.0;
  for (int i = t; i < n; i += NT) mx = nan_max(mx, fabs(x(i)));
  mx = wave_max(mx);
  if (lane == 0) sh.red[wv] = mx;
  __syncthreads();
  mx = sh.red[0];
  for (int w = 1; w < NW; w++) mx = nan_max(mx, sh.red[w]);
  __syncthreads();
  const int ex = norm_exp(mx);
  double s = 0.0;
  for (int i = t; i < n; i += NT) { const double y = ldexp(x(i), -ex); s += y * y; }
  s = wave_sum(s);
  if (lane == 0) sh.red[wv] = s;
  __syncthreads();
  s = 0.0;
  for (int w = 0; w < NW; w++) s += sh.red[w];
  __syncthreads();
  return norm_finish(mx, s, ex);
}

// first maximum (strict <, an earlier index wins a tie, NaN never wins) of v(t), t in [0, n); returns the index or -1
template <class F>
__device__ int block_first_max(Shared& sh, int n, F v, double* best_out) {
  const int t = threadIdx.x, lane = t & (WAVE - 1), wv = t >> 6;
  double best = -INFINITY; int idx = INT_MAX;
  for (int i = t; i < n; i += NT) { const double f = v(i); if (best < f) { best = f; idx = i; } }
  for (int o = WAVE / 2; o > 0; o >>= 1) {
    const double ob = __shfl_xor(best, o, WAVE); const int oi = __shfl_xor(idx, o, WAVE);
    if (ob > best || (ob == best && oi < idx)) { best = ob; idx = oi; }
  }
  if (lane == 0) { sh.red[wv] = best; sh.ired[wv] = idx; }
  __syncthreads();
  best = sh.red[0]; idx = sh.ired[0];
  for (int w = 1; w < NW; w++)
    if (sh.red[w] > best || (sh.red[w] == best && sh.ired[w] < idx)) { best = sh.red[w]; idx = sh.ired[w]; }
  __syncthreads();
  *best_out = best;
  return idx == INT_MAX ? -1 : idx;
}

// _giv_rot_qr (the reference's _giv_rot.js:22-37)
__device__ inline void giv_rot_qr(double a, double b, double& c, double& s, double& nrm) {
  const double mx = fmax(fabs(a), fabs(b));
  if (mx == 0.0) { c = 1.0; s = 0.0; nrm = 0.0; return; }
  a /= mx; b /= mx;
  double n = sqrt(a * a + b * b);
  c = a / n; s = b / n; nrm = n * mx;
}

struct Mat {
  int M, N;
  double* W;       // [N][M] physical columns
  int* cm;         // logical column -> physical column
  double* AB;      // [N][M]: AB[i + j M]
  double* AB0;
  double* nrm;     // column norms of C (index >= k)
  double* rn;      // row norms of inv(A_k)
  double* v;       // Householder vector [M]
  int32_t* P;
  __device__ double& R(int i, int j) const { return W[(long)cm[j] * M + i]; }
  __device__ double* col(int j) const { return W + (long)cm[j] * M; }
};

// nrm[j] = ||R[r0:, j]|| for j in [c0, N): one wave per column
__device__ void col_norms(const Mat& m, int r0, int c0) {
  const int lane = threadIdx.x & (WAVE - 1), wv = threadIdx.x >> 6;
  for (int j = c0 + wv; j < m.N; j += NW) {
    const double* c = m.col(j);
    double mx = 0.0;
    for (int i = r0 + lane; i < m.M; i += WAVE) mx = nan_max(mx, fabs(c[i]));
    mx = wave_max(mx);
    const int ex = norm_exp(mx);
    double s = 0.0;
    for (int i = r0 + lane; i < m.M; i += WAVE) { const double y = ldexp(c[i], -ex); s += y * y; }
    s = wave_sum(s);
    if (lane == 0) m.nrm[j] = norm_finish(mx, s, ex);
  }
  __syncthreads();
}

// update (:236-257): inv(A_k) and A_k \ B_k from those of A_{k-1}
__device__ void ab_update(const Mat& m, double* AB, int k) {
  const int M = m.M, N = m.N, t = threadIdx.x;
  const double Rkk = -m.R(k, k);
  for (int i = t; i <= k; i += NT) {
    if (i == k) AB[k + (long)k * M] = -1 / Rkk;
    else AB[i + (long)k * M] /= Rkk;
  }
  __syncthreads();
  const long n = (long)(k + 1) * (N - k - 1);
  for (long e = t; e < n; e += NT) {
    const int i = (int)(e % (k + 1)), j = k + 1 + (int)(e / (k + 1));
    AB[i + (long)j * M] += AB[i + (long)k * M] * m.R(k, j);
  }
  __syncthreads();
}

// downdate (:263-281)
__device__ void ab_downdate(const Mat& m, double* AB, int k) {
  const int M = m.M, N = m.N, t = threadIdx.x;
  const long n = (long)(k + 1) * (N - k - 1);
  for (long e = t; e < n; e += NT) {
    const int i = (int)(e % (k + 1)), j = k + 1 + (int)(e / (k + 1));
    if (i == k) AB[k + (long)j * M] = 0.0;
    else AB[i + (long)j * M] -= AB[i + (long)k * M] * m.R(k, j);
  }
  __syncthreads();
  const double Rkk = -m.R(k, k);
  for (int i = t; i <= k; i += NT) {
    if (i == k) AB[k + (long)k * M] = 0.0;
    else AB[i + (long)k * M] *= Rkk;
  }
  __syncthreads();
}

// copy (:393-399): rows < k of every column
__device__ void ab_copy(const Mat& m, const double* src, double* dst, int k) {
  if (k > 0) {
    const long n = (long)k * m.N;
    for (long e = threadIdx.x; e < n; e += NT) {
      const int i = (int)(e % k), j = (int)(e / k);
      dst[i + (long)j * m.M] = src[i + (long)j * m.M];
    }
  }
  __syncthreads();
}

// cycle (:446-451): the row permutation of inv(A) and A \ B that matches moving column p of R to k
__device__ void ab_cycle(const Mat& m, double* AB, int p, int k) {
  const int M = m.M;
  for (int j = p + (int)threadIdx.x; j < m.N; j += NT) {
    double* a = AB + (long)j * M;
    const double apj = a[p];
    if (j < k) { for (int i = p; i < j; i++) a[i] = a[i + 1]; a[j] = 0.0; }
    else for (int i = p; i < k; i++) a[i] = a[i + 1];
    a[k] = apj;
  }
  __syncthreads();
}

// R: logical column p moves to k, p+1..k move one left (the reference's column cycle, rows <= k); P likewise
__device__ void r_cycle(const Mat& m, int p, int k) {
  if (threadIdx.x == 0) {
    const int cp = m.cm[p]; const int32_t pp = m.P[p];
    for (int j = p; j < k; j++) { m.cm[j] = m.cm[j + 1]; m.P[j] = m.P[j + 1]; }
    m.cm[k] = cp; m.P[k] = pp;
  }
  __syncthreads();
}

// retriangulate rows p..k of R after a cycle to k (:697-723 / :752-775); AB1 (and AB2 when not NULL) get the same rotations
__device__ void retri(Shared& sh, const Mat& m, int p, int k, double* AB1, double* AB2) {
  const int M = m.M, N = m.N, t = threadIdx.x;
  for (int i = p; i < k; i++) {
    if (t == 0) {
      int rot = 0; double c = 1.0, s = 0.0;
      const double Rji = m.R(i + 1, i);
      if (Rji != 0.0) {
        double nr;
        giv_rot_qr(m.R(i, i), Rji, c, s, nr);
        m.R(i + 1, i) = 0.0;
        if (s != 0.0) { m.R(i, i) = nr; rot = 1; }
      }
      sh.bc[0] = c; sh.bc[1] = s; sh.ibc[0] = rot;
    }
    __syncthreads();
    const double c = sh.bc[0], s = sh.bc[1];
    const int rot = sh.ibc[0];
    if (rot) {
      for (int j = i + 1 + t; j < N; j += NT) {        // R rows i, i+1 right of the diagonal
        double* cj = m.col(j);
        const double x = cj[i], y = cj[i + 1];
        cj[i] = c * x + s * y; cj[i + 1] = c * y - s * x;
      }
      for (int r = t; r <= i; r += NT) {                // columns i, i+1 of inv(A), rows 0..i
        double* a = AB1 + (long)i * M; double* b = AB1 + (long)(i + 1) * M;
        const double x = a[r], y = b[r];
        a[r] = c * x + s * y; b[r] = c * y - s * x;
        if (AB2) {
          double* a2 = AB2 + (long)i * M; double* b2 = AB2 + (long)(i + 1) * M;
          const double x2 = a2[r], y2 = b2[r];
          a2[r] = c * x2 + s * y2; b2[r] = c * y2 - s * x2;
        }
      }
    }
    if (t == NT - 1) {                                  // row k of inv(A) (the moved row), then zero its entry in column i
      if (rot) AB1[k + (long)(i + 1) * M] = -s * AB1[k + (long)i * M] + c * AB1[k + (long)(i + 1) * M];
      AB1[k + (long)i * M] = 0.0;
      if (AB2) {
        if (rot) AB2[k + (long)(i + 1) * M] = -s * AB2[k + (long)i * M] + c * AB2[k + (long)(i + 1) * M];
        AB2[k + (long)i * M] = 0.0;
      }
    }
    __syncthreads();
  }
}

// swap_elim (:285-336): swap columns k and p, then eliminate column k below the diagonal; nrm[j > k] = ||R[k+1:, j]||
__device__ void swap_elim(Shared& sh, const Mat& m, int k, int p) {
  const int M = m.M, N = m.N, t = threadIdx.x, lane = t & (WAVE - 1), wv = t >> 6;
  if (p != k) {
    for (int j = t; j < k; j += NT) {
      double x = m.AB0[j + (long)k * M]; m.AB0[j + (long)k * M] = m.AB0[j + (long)p * M]; m.AB0[j + (long)p * M] = x;
      x = m.AB[j + (long)k * M]; m.AB[j + (long)k * M] = m.AB[j + (long)p * M]; m.AB[j + (long)p * M] = x;
    }
    if (t == 0) {
      const int c = m.cm[k]; m.cm[k] = m.cm[p]; m.cm[p] = c;
      const int32_t q = m.P[k]; m.P[k] = m.P[p]; m.P[p] = q;
    }
    __syncthreads();
  }
  double* x = m.col(k);
  const double sub = block_norm(sh, M - k - 1, [&](int i) { return x[k + 1 + i]; });
  const bool apply = sub != 0.0;                        // all zero below the diagonal: the reference rotates nothing
  if (apply) {
    const double alpha = x[k];
    const double full = block_norm(sh, M - k, [&](int i) { return x[k + i]; });
    const double beta = -copysign(full, alpha), den = alpha - beta, tau = (beta - alpha) / beta;
    for (int i = k + t; i < M; i += NT) {
      m.v[i] = i == k ? 1.0 : x[i] / den;
      x[i] = i == k ? beta : 0.0;
    }
    __syncthreads();
    for (int j = k + 1 + wv; j < N; j += NW) {
      double* c = m.col(j);
      double d = 0.0;
      for (int i = k + lane; i < M; i += WAVE) d += m.v[i] * c[i];
      const double w = tau * wave_sum(d);
      for (int i = k + lane; i < M; i += WAVE) c[i] -= w * m.v[i];
    }
    __syncthreads();
  }
  col_norms(m, k + 1, k + 1);
}

__device__ double norm_C(Shared& sh, const Mat& m, int k) {
  return block_norm(sh, m.N - k, [&](int i) { return m.nrm[k + i]; });
}

__device__ void piv_elim(Shared& sh, const Mat& m, int k) {
  double best;
  int p = block_first_max(sh, m.N - k, [&](int i) { return m.nrm[k + i]; }, &best);
  swap_elim(sh, m, k, p < 0 ? k : k + p);
}

// W [batch][N][M] holds A column-major on entry; AB / AB0 are zero; P, rank out. ztol < 0: the reference default (:201-210).
__global__ __launch_bounds__(NT) void srrqr_decide(int M, int N, double* __restrict__ Wg, int* __restrict__ cmg,
                                                   double* __restrict__ ABg, double* __restrict__ AB0g, double* __restrict__ nrmg,
                                                   double* __restrict__ rng, double* __restrict__ vg, int32_t* __restrict__ Pg,
                                                   int32_t* __restrict__ rank, double dtol, double ztol_opt) {
  __shared__ Shared sh;
  const long b = blockIdx.x;
  const long MN = (long)M * N;
  Mat m{M, N, Wg + b * MN, cmg + b * N, ABg + b * MN, AB0g + b * MN, nrmg + b * N, rng + b * N, vg + b * M, Pg + b * N};
  const int t = threadIdx.x;
  const int L = M < N ? M : N;
  for (int j = t; j < N; j += NT) { m.cm[j] = j; m.P[j] = j; }
  __syncthreads();

  // scale by ||A||_F (:586-594); a zero matrix keeps scale 1
  double* W = m.W;
  double scale = block_norm(sh, (int)MN, [&](int i) { return W[i]; });
  if (!(scale <= 1.79769313486231570e308)) { if (t == 0) rank[b] = scale != scale ? -3 : -1; return; }   // 'Assertion failed: ' + SCALE
  if (scale == 0.0) scale = 1.0;
  if (scale != 1.0) {
    for (long i = t; i < MN; i += NT) W[i] /= scale;
    __syncthreads();
  }
  const double ztol = ztol_opt >= 0.0
      ? ztol_opt
      : 1.4901161193847656e-08 * block_norm(sh, (int)MN, [&](int i) { return W[i]; }) * (double)(M > N ? M : N);

  int k0 = 0, k = 0, K = L;
  col_norms(m, 0, 0);                                                     // update_col_norms (:457-462) at k = 0

  // adjust_k (:491-549)
  long inner = 0;
  const long inner_cap = (long)(L + 2) * (L + 2) + 64;
  auto adjust_k = [&](bool increase) {
    if (increase) {
      piv_elim(sh, m, k);
      ab_update(m, m.AB, k); k++;
      ab_copy(m, m.AB, m.AB0, k);
      k0 = k;
    } else {
      ab_copy(m, m.AB0, m.AB, k);
      k = k0;
      col_norms(m, k, k);
    }
    int mid = (k0 + K) >> 1;
    while (k < mid && ++inner < inner_cap) {
      if (norm_C(sh, m, k) <= ztol) {
        K = k;
        if (k0 < k) {
          ab_copy(m, m.AB0, m.AB, k);
          k = k0;
          col_norms(m, k, k);
          mid = (k0 + K) >> 1;
          increase = false;
          continue;
        }
        break;
      }
      if (increase) piv_elim(sh, m, k);
      ab_update(m, m.AB, k); k++;
      if (!increase) col_norms(m, k, k);
    }
  };

  const long cap = 4l * N + 2l * L + 64;
  long it = 0;
  for (; it < cap && inner < inner_cap; it++) {
    if (norm_C(sh, m, k) <= ztol) {
      K = k;
      if (k0 < k) adjust_k(false);
      else if (k == N) break;
    }
    // the best swap (:633-660): F_ij = hypot((A\B)_ij, ||row i of inv(A)|| ||column j of C||), first maximum row-major
    {
      const int lane = t & (WAVE - 1), wv = t >> 6;
      for (int i = wv; i < k; i += NW) {
        double mx = 0.0;
        for (int j = i + lane; j < k; j += WAVE) mx = nan_max(mx, fabs(m.AB[i + (long)j * M]));
        mx = wave_max(mx);
        const int ex = norm_exp(mx);
        double s = 0.0;
        for (int j = i + lane; j < k; j += WAVE) { const double y = ldexp(m.AB[i + (long)j * M], -ex); s += y * y; }
        s = wave_sum(s);
        if (lane == 0) m.rn[i] = norm_finish(mx, s, ex);
      }
      __syncthreads();
    }
    const int nc = N - k;
    double F;
    const long nF = (long)k * nc;
    const int f = nF > 0 ? block_first_max(sh, (int)nF, [&](int e) {
      const int i = e / nc, j = k + e % nc;
      return hypot(m.AB[i + (long)j * M], m.rn[i] * m.nrm[j]);
    }, &F) : -1;
    if (f < 0) F = -INFINITY;
    if (!(F > dtol)) {
      if (k0 >= K) break;
      adjust_k(true);
      continue;
    }
    int p = f / nc, q = k + f % nc;
    if (p < k0) {                                                         // inv(A0) is affected (:669-727)
      --k0;
      r_cycle(m, p, k0);
      ab_cycle(m, m.AB, p, k0);
      ab_cycle(m, m.AB0, p, k0);
      retri(sh, m, p, k0, m.AB, m.AB0);
      ab_downdate(m, m.AB0, k0);
      p = k0++;
    }
    --k;
    r_cycle(m, p, k);
    ab_cycle(m, m.AB, p, k);
    for (int i = t; i < k0; i += NT) {                                    // cycle the columns of inv(A0) (:739-742)
      const double x = m.AB0[i + (long)p * M];
      for (int j = p; j < k; j++) m.AB0[i + (long)j * M] = m.AB0[i + (long)(j + 1) * M];
      m.AB0[i + (long)k * M] = x;
    }
    __syncthreads();
    retri(sh, m, p, k, m.AB, nullptr);
    ab_downdate(m, m.AB, k);
    swap_elim(sh, m, k, q);
    if (p < k0) ab_update(m, m.AB0, p);
    ab_update(m, m.AB, k); k++;
  }
  if (t == 0) rank[b] = (it >= cap || inner >= inner_cap) ? -2 : k;
}

// Ap[b][r][c] = A[b][r][P[b][c]]
__global__ void srrqr_gather(int M, int N, const double* __restrict__ A, const int32_t* __restrict__ P, double* __restrict__ Ap) {
  const long b = blockIdx.z;
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= N) return;
  const int pc = P[b * (long)N + c];
  const double* a = A + b * (long)M * N;
  double* o = Ap + b * (long)M * N;
  for (int r = blockIdx.y; r < M; r += gridDim.y) o[(long)r * N + c] = a[(long)r * N + pc];
}

__global__ void srrqr_empty(int N, int32_t* __restrict__ P, int32_t* __restrict__ rank) {
  const long b = blockIdx.y;
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j < N) P[b * (long)N + j] = j;
  if (j == 0) rank[b] = 0;
}


// ---- URV (urv.js:30-135) -------------------------------------------------------------------------------------------------------
// The r x N trapezoid R1 = R[:r, :] is reduced from the right through the QR of X' [N, L] (row-major), X'[i][j] = R1[r-1-j][N-1-i]
// for j < r, 0 otherwise: X'[:, :r] = Q' [S'; 0] gives R1 = T V1 with T = J S'^T J upper triangular and V1 = J Q'^T[:r] J_N.
__global__ void urv_pack(int M, int N, int L, const double* __restrict__ R, const int32_t* __restrict__ rank, double* __restrict__ X) {
  const long b = blockIdx.z;
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= L) return;
  const int r = rank[b] < 0 ? 0 : rank[b];
  const double* Rb = R + b * (long)M * N;
  double* Xb = X + b * (long)N * L;
  for (int i = blockIdx.y; i < N; i += gridDim.y) Xb[(long)i * L + j] = j < r ? Rb[(long)(r - 1 - j) * N + (N - 1 - i)] : 0.0;
}

// R <- [[T, 0], [0, 0]] (exact zeros outside T), V [N, N] with A = U R V: V[a][P[c]] = Vf[a][c], Vf = [J Q'^T[:r] J_N; Q'^T[r:] J_N].
// r == N: T is R[:N, :] itself and Vf = I (the reference's pure permutation, urv.js:47-52).
__global__ void urv_unpack(int M, int N, int L, double* __restrict__ R, const int32_t* __restrict__ rank, const int32_t* __restrict__ P,
                           const double* __restrict__ Qp, const double* __restrict__ Rp, double* __restrict__ V) {
  const long b = blockIdx.z;
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= N) return;
  const int r = rank[b] < 0 ? 0 : rank[b];
  double* Rb = R + b * (long)M * N;
  double* Vb = V + b * (long)N * N;
  const double* Q = Qp + b * (long)N * N;
  const double* S = Rp + b * (long)N * L;
  const int pc = P[b * (long)N + c];
  for (int a = blockIdx.y; a < N; a += gridDim.y) {
    double v;
    if (r == N || !Q) v = a == c ? 1.0 : 0.0;                      // (Q == NULL: M == 0, nothing to rotate)
    else v = a < r ? Q[(long)(N - 1 - c) * N + (r - 1 - a)] : Q[(long)(N - 1 - c) * N + a];
    Vb[(long)a * N + pc] = v;
  }
  if (r < N)
    for (int a = blockIdx.y; a < M; a += gridDim.y)
      Rb[(long)a * N + c] = (a < r && c < r && c >= a) ? S[(long)(r - 1 - c) * L + (r - 1 - a)] : 0.0;
}

// urv_lstsq: Tm [Lr, Lr] = R[:r, :r] (row stride K), identity outside; Z rows >= r zeroed
__global__ void urv_mask(int Lr, int K, int Jc, const double* __restrict__ R, long sR, const int32_t* __restrict__ rank, long sRank,
                         double* __restrict__ Tm, double* __restrict__ Z) {
  const long b = blockIdx.z;
  int r = rank[b * sRank];
  r = r < 0 ? 0 : (r > Lr ? Lr : r);
  const int c = blockIdx.x * 256 + threadIdx.x;
  const double* Rb = R + b * sR;
  double* T = Tm + b * (long)Lr * Lr;
  double* z = Z + b * (long)Lr * Jc;
  for (int row = blockIdx.y; row < Lr; row += gridDim.y) {
    if (c < Lr) T[(long)row * Lr + c] = (row < r && c < r) ? Rb[(long)row * K + c] : (row == c ? 1.0 : 0.0);
    if (c < Jc && row >= r) z[(long)row * Jc + c] = 0.0;
  }
}
}  // namespace

// Q [batch,M,M], R [batch,M,N], P [batch,N], rank [batch] (-1 / -3: ||A||_F is Infinity / NaN, -2: the swap cap was hit); batch <= 32768
int nd4_srrqr(nd4hip_handle* h, int64_t batch, int64_t M64, int64_t N64, const double* A, double dtol, double ztol, double* Q, double* R,
              int32_t* P, int32_t* rank) {
  ND4_CHECK_ARG(M64 < (1ll << 30) && N64 < (1ll << 30) && M64 * N64 < (1ll << 31) && batch <= 32768, "nd4_srrqr: extent out of range");
  const int M = (int)M64, N = (int)N64;
  if (batch == 0) return 0;
  if (M == 0 || N == 0) {
    hipLaunchKernelGGL(srrqr_empty, dim3((unsigned)((N + 255) / 256 + 1), (unsigned)batch), dim3(256), 0, h->stream, N, P, rank);
    ND4_HIP(hipGetLastError());
    if (M > 0) ND4_TRY(nd4_set_identity(h, M, M, Q, M, batch, M64 * M64));
    return 0;
  }
  const int64_t per_ws = (int64_t)M * N;
  int64_t step = ((int64_t)1 << 27) / (3 * per_ws + 2 * N + M + N);
  if (step < 1) step = 1;
  if (step > batch) step = batch;
  for (int64_t b0 = 0; b0 < batch; b0 += step) {
    const int nb = (int)(batch - b0 < step ? batch - b0 : step);
    const double* Ab = A + b0 * per_ws;
    Nd4WsScope scope(h);
    void* p = nullptr;
    ND4_TRY(nd4_ws_alloc(h, sizeof(double) * (size_t)nb * (size_t)(3 * per_ws + 2 * N + M) + sizeof(int) * (size_t)nb * N, &p));
    double* W = static_cast<double*>(p);
    double* AB = W + (size_t)nb * per_ws;
    double* AB0 = AB + (size_t)nb * per_ws;
    double* nrm = AB0 + (size_t)nb * per_ws;
    double* rn = nrm + (size_t)nb * N;
    double* v = rn + (size_t)nb * N;
    int* cm = reinterpret_cast<int*>(v + (size_t)nb * M);
    ND4_HIP(hipMemsetAsync(AB, 0, sizeof(double) * (size_t)nb * 2 * per_ws, h->stream));
    ND4_TRY(nd4_transpose(h, M, N, Ab, N, W, M, nb, per_ws, per_ws));           // column j of A -> row j of W
    hipLaunchKernelGGL(srrqr_decide, dim3((unsigned)nb), dim3(NT), 0, h->stream, M, N, W, cm, AB, AB0, nrm, rn, v, P + b0 * N,
                       rank + b0, dtol, ztol);
    ND4_HIP(hipGetLastError());
    const dim3 g((unsigned)((N + 255) / 256), (unsigned)(M < 1024 ? M : 1024), (unsigned)nb);
    hipLaunchKernelGGL(srrqr_gather, g, dim3(256), 0, h->stream, M, N, Ab, P + b0 * N, W);
    ND4_HIP(hipGetLastError());
    ND4_TRY(nd4_geqrf_q_ex(h, nb, M, N, W, Q + b0 * M64 * M64, R + b0 * M64 * N64, true));
  }
  return 0;
}

// urv_decomp_full (urv.js:100-135): U [batch,M,M], R [batch,M,N] <- [[T,0],[0,0]], V [batch,N,N] with A = U R V, rank [batch]
int nd4_urv(nd4hip_handle* h, int64_t batch, int64_t M64, int64_t N64, const double* A, double* U, double* R, double* V, int32_t* rank) {
  ND4_CHECK_ARG(M64 < (1ll << 30) && N64 < (1ll << 30) && M64 * N64 < (1ll << 31) && N64 * N64 < (1ll << 31) && batch <= 32768,
                "nd4_urv: extent out of range");
  const int M = (int)M64, N = (int)N64, L = M < N ? M : N;
  if (batch == 0 || N == 0) return 0;
  Nd4WsScope scope(h);
  void* p = nullptr;
  ND4_TRY(nd4_ws_alloc(h, sizeof(int32_t) * (size_t)(batch * N), &p));
  int32_t* P = static_cast<int32_t*>(p);
  ND4_TRY(nd4_srrqr(h, batch, M, N, A, 1.01, -1.0, U, R, P, rank));
  if (M == 0) {
    ND4_HIP(hipMemsetAsync(V, 0, sizeof(double) * (size_t)(batch * N * N), h->stream));
    const dim3 g((unsigned)((N + 255) / 256), (unsigned)(N < 1024 ? N : 1024), (unsigned)batch);
    hipLaunchKernelGGL(urv_unpack, g, dim3(256), 0, h->stream, M, N, L, R, rank, P, (const double*)nullptr, (const double*)nullptr, V);
    ND4_HIP(hipGetLastError());
    return 0;
  }
  const int64_t step = std::max<int64_t>(1, std::min<int64_t>(batch, ((int64_t)1 << 27) / ((int64_t)N * N + 2 * (int64_t)N * L)));
  for (int64_t b0 = 0; b0 < batch; b0 += step) {
    const int64_t nb = batch - b0 < step ? batch - b0 : step;
    Nd4WsScope s2(h);
    void* q = nullptr;
    ND4_TRY(nd4_ws_alloc(h, sizeof(double) * (size_t)(nb * ((int64_t)N * N + 2 * (int64_t)N * L)), &q));
    double* X = static_cast<double*>(q);
    double* Qp = X + nb * N * L;
    double* Rp = Qp + nb * N * N;
    double* Rb = R + b0 * M64 * N64;
    const int32_t* rk = rank + b0;
    hipLaunchKernelGGL(urv_pack, dim3((unsigned)((L + 255) / 256), (unsigned)(N < 1024 ? N : 1024), (unsigned)nb), dim3(256), 0, h->stream,
                       M, N, L, Rb, rk, X);
    ND4_HIP(hipGetLastError());
    ND4_TRY(nd4_geqrf_q_ex(h, nb, N, L, X, Qp, Rp, true));
    const int rows = M > N ? M : N;
    hipLaunchKernelGGL(urv_unpack, dim3((unsigned)((N + 255) / 256), (unsigned)(rows < 1024 ? rows : 1024), (unsigned)nb), dim3(256), 0,
                       h->stream, M, N, L, Rb, rk, P + b0 * N, Qp, Rp, V + b0 * N64 * N64);
    ND4_HIP(hipGetLastError());
  }
  return 0;
}

// urv_lstsq (urv.js:138-323): U [I,J], R [J,K], V [K,Lv], rank (stride sRank: 0 or 1), Y [I,Jc] -> X [Lv,Jc] = V[:r]^T T^-1 (U^T Y)[:r]
int nd4_urvls(nd4hip_handle* h, int64_t batch, int64_t I, int64_t J, int64_t K, int64_t Lv, int64_t Jc, const double* U, int64_t sU,
              const double* R, int64_t sR, const double* V, int64_t sV, const int32_t* rank, int64_t sRank, const double* Y, int64_t sY,
              double* X) {
  ND4_CHECK_ARG(I < (1ll << 30) && J < (1ll << 30) && K < (1ll << 30) && Lv < (1ll << 30) && Jc < (1ll << 30) && batch <= 32768,
                "nd4_urvls: extent out of range");
  const int64_t Lr = J < K ? J : K;
  if (batch == 0 || Lv == 0 || Jc == 0) return 0;
  if (Lr == 0 || I == 0) { ND4_HIP(hipMemsetAsync(X, 0, sizeof(double) * (size_t)(batch * Lv * Jc), h->stream)); return 0; }
  Nd4WsScope scope(h);
  void* p = nullptr;
  ND4_TRY(nd4_ws_alloc(h, sizeof(double) * (size_t)(batch * (Lr * Lr + Lr * Jc)), &p));
  double* Tm = static_cast<double*>(p);
  double* Z = Tm + batch * Lr * Lr;
  ND4_TRY(nd4_gemm(h, true, false, Lr, Jc, I, 1.0, U, J, sU, Y, Jc, sY, 0.0, Z, Jc, Lr * Jc, batch));     // (U^T Y)[0:Lr]
  const int64_t wmax = Lr > Jc ? Lr : Jc;
  hipLaunchKernelGGL(urv_mask, dim3((unsigned)((wmax + 255) / 256), (unsigned)(Lr < 1024 ? Lr : 1024), (unsigned)batch), dim3(256), 0,
                     h->stream, (int)Lr, (int)K, (int)Jc, R, (long)sR, rank, (long)sRank, Tm, Z);
  ND4_HIP(hipGetLastError());
  ND4_TRY(nd4_trsm_ld(h, true, false, batch, Lr, Jc, Tm, Lr, Lr * Lr, Z, Lr * Jc));
  ND4_TRY(nd4_gemm(h, true, false, Lv, Jc, Lr, 1.0, V, Lv, sV, Z, Jc, Lr * Jc, 0.0, X, Jc, Lv * Jc, batch));   // V[0:Lr]^T Z
  return 0;
}
