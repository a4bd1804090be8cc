// Hermitian Cholesky, complex lower triangular solves and the generalised Hermitian-definite eigenproblem A x = lambda B x on the
// device: herm_cholesky_decomp / herm_cholesky_solve / ztril_solve / herm_gen_reduce / eigen_herm_gen. The complex
// twin of sygv.hip on top of hetrd.hip's eigen routes. complex128 operands are interleaved (re, im) doubles. The route is LAPACK's
// zhegvd, itype 1, lower:
//   1. L = chol(B) (zpotrf)            2. C = L^-1 A L^-H (zhegst; lower triangle, real diagonal)
//   3. (lambda, Y) of C by nd4_zheevd or nd4_zheevx, unchanged
//   4. X = L^-H Y                      so that A X = B X diag(lambda) and X^H B X = I.
//
// One order of operations for every N. Every entry is a chain that starts from the matrix entry and subtracts its products one at a
// time, each operation rounded on its own (the file is built without FMA contraction), in the order in which the unknowns become
// known: ascending k in the factorisation and in L X = Y, descending k in L^H X = Y,
//   l_jj = sqrt(Re h_jj - sum_k |l_jk|^2),   l_ij = (h_ij - sum_{k<j} l_ik conj(l_jk)) / l_jj
//   x_ic = (y_ic - sum_{k<i} l_ik x_kc) / l_ii,   x_ic = (y_ic - sum_{k>i} conj(l_ki) x_kc) / conj(l_ii)
// with the one product form hegv_nmsc below (s - a conj(b): Re (s_re - a_re b_re) - a_im b_im, Im (s_im - a_im b_re) + a_re b_im; the
// other forms negate an imaginary part first, which is exact) and the one division hegv_div (by the real part alone where the
// imaginary part is zero, else Smith's form). The kernels are right-looking: a finished column or row is subtracted from everything
// that waits for it, by all threads of the workgroup, so an entry sees its products in exactly that order whatever the tier and the
// block size, and the device returns the bits of the numpy model in tests/hegv_common.py at every N. No atomics on doubles, no
// synchronisation but __syncthreads() and the kernel boundary.
//
// Small tier, N <= 64: one workgroup of four waves per member, member index in blockIdx.x, tiles in LDS at pitch N | 1 in 16-byte
// elements (the layout hetrd_small shows to be conflict-free for ds_read_b128 row and column walks). eigen_herm_gen fuses the
// factorisation of a member's own B into hegst_small up to N = 32 (measured); above it runs zpotrf_small first.
//   zpotrf_small  the lower triangle of H (Im h_ii dropped) -> L in place.
//   hegst_small   two tiles: the Hermitian mirror of A's lower triangle and L (given, or factorised here from a member's own B).
//                 W = L^-1 A in place, the tile is conjugate-transposed in place, C = L^-1 W^H in place. 2 N (N | 1) 16 bytes of LDS:
//                 133 120 at N = 64 (the function attribute is set above 64 KiB).
//   ztrsm_small   L X = Y, L^H X = Y or both in turn on a tile of 64 right-hand sides; step 4 is its L^H form on the k selected columns.
// Large tier, 64 < N <= 2048, blocks of 64: zpotrf_diag (one workgroup factorises the diagonal block in LDS), zpotrf_panel (the rows
// below it), hegv_update (the trailing update, and the updates of the blocked substitutions: 64 x 64 tiles of C -= a conj(b)^T from
// LDS, 4 x 4 entries per thread), ztrsm_diag (a diagonal block against 64 right-hand sides in LDS), hegv_load_lower (Hermitian
// mirror), hegv_conj_transpose, hegv_finish_c (zeros above the diagonal, a real diagonal, the finiteness flag).
// Flags: [0] the OR over the members of a pass, [1 + member]; bit 1 a radicand that is not a finite number > 0, bit 2 a non-finite
// entry in C's lower triangle. The host reads the one OR word per pass before the solver starts.
#include "nd4hip_internal.h"
#include <cfloat>
#include <cmath>

namespace {

typedef double2 cd;

constexpr int HEGV_MAXN = 2048;
constexpr int HEGV_SMALL_N = 64;               // every operation: one member per workgroup in LDS up to here
constexpr int HEGV_FUSED_N = 32;               // eigen_herm_gen: factorisation and reduction in one launch up to here (measured)
constexpr int HEGV_NB = 64;                     // block of the large tier, right-hand sides per workgroup
constexpr int HEGV_T = 256;                     // threads per workgroup
constexpr int64_t HEGV_CHUNK = 32768;           // members per pass (the eigen routes take batch <= 32768)
constexpr int64_t HEGV_WS_ELEMS = 1ll << 26;    // a pass's L, W and C take at most 1 GiB each
constexpr int HEGV_BAD_B = 1, HEGV_BAD_C = 2;

__device__ __forceinline__ cd hz(double re, double im) { cd r; r.x = re; r.y = im; return r; }
__device__ __forceinline__ cd hconj(cd a) { return hz(a.x, -a.y); }
// s - a conj(b), the one order of the four real products
__device__ __forceinline__ cd hegv_nmsc(cd s, cd a, cd b) { return hz((s.x - a.x * b.x) - a.y * b.y, (s.y - a.y * b.x) + a.x * b.y); }
// x / d: true divisions; Smith's form for a complex d
__device__ __forceinline__ cd hegv_div(cd x, cd d) {
  if (d.y == 0.0) return hz(x.x / d.x, x.y / d.x);
  if (fabs(d.x) >= fabs(d.y)) {
    const double r = d.y / d.x, den = d.x + d.y * r;
    return hz((x.x + x.y * r) / den, (x.y - x.x * r) / den);
  }
  const double r = d.x / d.y, den = d.x * r + d.y;
  return hz((x.x * r + x.y) / den, (x.y * r - x.x) / den);
}
__device__ __forceinline__ bool hegv_finite(cd v) { return fabs(v.x) <= DBL_MAX && fabs(v.y) <= DBL_MAX; }

inline int hegv_ld(int n) { return n | 1; }

// ---- the substitutions on LDS tiles, by all HEGV_T threads; each ends behind a barrier ---------------------------------------------
// Ls [n][ld]: the lower triangle of a Hermitian matrix (Im of the diagonal is not read) -> L in place; true: a radicand was bad
__device__ bool hegv_chol_lds(cd* Ls, int n, int ld) {
  const int t = threadIdx.x;
  bool bad = false;
  for (int j = 0; j < n; ++j) {
    const double s = Ls[j * ld + j].x;
    if (!(s > 0.0 && s <= DBL_MAX)) bad = true;
    const double d = sqrt(s);
    for (int i = j + 1 + t; i < n; i += HEGV_T) { const cd v = Ls[i * ld + j]; Ls[i * ld + j] = hz(v.x / d, v.y / d); }
    __syncthreads();
    const int m = n - j - 1;
    for (int e = t; e < m * m; e += HEGV_T) {
      const int i = j + 1 + e / m, c = j + 1 + e % m;
      if (c <= i) Ls[i * ld + c] = hegv_nmsc(Ls[i * ld + c], Ls[i * ld + j], Ls[c * ld + j]);
    }
    __syncthreads();
  }
  for (int j = t; j < n; j += HEGV_T) Ls[j * ld + j] = hz(sqrt(Ls[j * ld + j].x), 0.0);
  __syncthreads();
  return bad;
}

// X [n][ldx], k columns: L X = Y in place
__device__ void hegv_fwd_lds(const cd* Ls, int ldl, cd* X, int ldx, int n, int k) {
  const int t = threadIdx.x;
  for (int i = 0; i < n; ++i) {
    const cd d = Ls[i * ldl + i];
    for (int c = t; c < k; c += HEGV_T) X[i * ldx + c] = hegv_div(X[i * ldx + c], d);
    __syncthreads();
    const int m = n - i - 1;
    for (int e = t; e < m * k; e += HEGV_T) {
      const int r = i + 1 + e / k, c = e % k;
      X[r * ldx + c] = hegv_nmsc(X[r * ldx + c], Ls[r * ldl + i], hconj(X[i * ldx + c]));
    }
    __syncthreads();
  }
}

// L^H X = Y in place
__device__ void hegv_bwd_lds(const cd* Ls, int ldl, cd* X, int ldx, int n, int k) {
  const int t = threadIdx.x;
  for (int i = n - 1; i >= 0; --i) {
    const cd d = hconj(Ls[i * ldl + i]);
    for (int c = t; c < k; c += HEGV_T) X[i * ldx + c] = hegv_div(X[i * ldx + c], d);
    __syncthreads();
    for (int e = t; e < i * k; e += HEGV_T) {
      const int r = e / k, c = e % k;
      X[r * ldx + c] = hegv_nmsc(X[r * ldx + c], hconj(Ls[i * ldl + r]), hconj(X[i * ldx + c]));
    }
    __syncthreads();
  }
}

// P [rows][ldp], nb columns: P Ld^H = the panel, in place (the rows below a factorised diagonal block Ld, whose diagonal is real)
__device__ void hegv_panel_lds(const cd* Ld, int ldl, cd* P, int ldp, int rows, int nb) {
  const int t = threadIdx.x;
  for (int c = 0; c < nb; ++c) {
    const double d = Ld[c * ldl + c].x;
    for (int r = t; r < rows; r += HEGV_T) { const cd v = P[r * ldp + c]; P[r * ldp + c] = hz(v.x / d, v.y / d); }
    __syncthreads();
    const int m = nb - c - 1;
    for (int e = t; e < rows * m; e += HEGV_T) {
      const int r = e / m, c2 = c + 1 + e % m;
      P[r * ldp + c2] = hegv_nmsc(P[r * ldp + c2], P[r * ldp + c], Ld[c2 * ldl + c]);
    }
    __syncthreads();
  }
}

// the lower triangle of src [N][N] into the tile: Im of the diagonal dropped; above it the conjugate mirror, or zeros
__device__ __forceinline__ void hegv_load_tile(const cd* __restrict__ src, cd* tile, int N, int ld, bool mirror) {
  for (int e = threadIdx.x; e < N * N; e += HEGV_T) {
    const int i = e / N, j = e - i * N;
    if (j < i) {
      const cd v = src[e];
      tile[i * ld + j] = v;
      if (mirror) tile[j * ld + i] = hconj(v);
    } else if (j == i) tile[i * ld + i] = hz(src[e].x, 0.0);
    else if (!mirror) tile[i * ld + j] = hz(0.0, 0.0);
  }
}

// ---- small tier -----------------------------------------------------------------------------------------------------------------
// flags NULL: no verdict wanted
__global__ __launch_bounds__(HEGV_T) void zpotrf_small(const cd* __restrict__ H, cd* __restrict__ L, int* __restrict__ flags, int N) {
  extern __shared__ __attribute__((aligned(16))) char hegv_smem[];
  cd* Ls = reinterpret_cast<cd*>(hegv_smem);
  const int ld = N | 1;
  const long mat = blockIdx.x;
  hegv_load_tile(H + mat * N * N, Ls, N, ld, false);
  __syncthreads();
  const bool bad = hegv_chol_lds(Ls, N, ld);
  for (int e = threadIdx.x; e < N * N; e += HEGV_T) { const int i = e / N, j = e - i * N; L[mat * N * N + e] = Ls[i * ld + j]; }
  if (flags && threadIdx.x == 0 && bad) { flags[1 + mat] = HEGV_BAD_B; atomicOr(&flags[0], HEGV_BAD_B); }
}

// have_L: T holds L (stride sT, 0 = one for all), else B. Lout may be NULL. C: lower triangle, real diagonal, zeros above
__global__ __launch_bounds__(HEGV_T) void hegst_small(const cd* __restrict__ A, const cd* __restrict__ T, long sT, int have_L, cd* __restrict__ Lout,
                                                      cd* __restrict__ C, int* __restrict__ flags, int N) {
  extern __shared__ __attribute__((aligned(16))) char hegv_smem[];
  const int ld = N | 1, t = threadIdx.x;
  const long mat = blockIdx.x;
  cd* As = reinterpret_cast<cd*>(hegv_smem);
  cd* Ls = As + N * ld;
  hegv_load_tile(A + mat * N * N, As, N, ld, true);
  if (have_L) {
    const cd* Lg = T + mat * sT;
    for (int e = t; e < N * N; e += HEGV_T) { const int i = e / N, j = e - i * N; Ls[i * ld + j] = j <= i ? Lg[e] : hz(0.0, 0.0); }
  } else hegv_load_tile(T + mat * sT, Ls, N, ld, false);
  __syncthreads();
  bool bad = false;
  if (!have_L) bad = hegv_chol_lds(Ls, N, ld);
  if (Lout)
    for (int e = t; e < N * N; e += HEGV_T) { const int i = e / N, j = e - i * N; Lout[mat * N * N + e] = Ls[i * ld + j]; }
  hegv_fwd_lds(Ls, ld, As, ld, N, N);                         // W = L^-1 A
  for (int e = t; e < N * N; e += HEGV_T) {                   // W^H in place: one thread per pair
    const int i = e / N, j = e - i * N;
    if (j < i) { const cd a = As[i * ld + j], b = As[j * ld + i]; As[i * ld + j] = hconj(b); As[j * ld + i] = hconj(a); }
    else if (j == i) As[i * ld + i] = hconj(As[i * ld + i]);
  }
  __syncthreads();
  hegv_fwd_lds(Ls, ld, As, ld, N, N);                         // C = L^-1 W^H
  int nonfinite = 0;
  for (int e = t; e < N * N; e += HEGV_T) {
    const int i = e / N, j = e - i * N;
    cd v = hz(0.0, 0.0);
    if (j <= i) { v = As[i * ld + j]; if (j == i) v.y = 0.0; if (!hegv_finite(v)) nonfinite = 1; }
    C[mat * N * N + e] = v;
  }
  nonfinite = __syncthreads_or(nonfinite);
  if (flags) {
    const int f = (bad ? HEGV_BAD_B : 0) | (nonfinite ? HEGV_BAD_C : 0);
    if (t == 0 && f) { flags[1 + mat] = f; atomicOr(&flags[0], f); }
  }
}

// X [members][N][ldx], columns blockIdx.y * 64 .. of the first K: mode 0 L X = Y, 1 L^H X = Y, 2 both in turn (L L^H X = Y)
__global__ __launch_bounds__(HEGV_T) void ztrsm_small(const cd* __restrict__ L, long sL, cd* __restrict__ X, int N, int K, long ldx, int mode) {
  extern __shared__ __attribute__((aligned(16))) char hegv_smem[];
  const int ld = N | 1, ldx_s = HEGV_NB + 1, t = threadIdx.x;
  const long mat = blockIdx.x;
  const int c0 = blockIdx.y * HEGV_NB, k = K - c0 < HEGV_NB ? K - c0 : HEGV_NB;
  cd* Ls = reinterpret_cast<cd*>(hegv_smem);
  cd* Xs = Ls + N * ld;
  cd* Xg = X + mat * N * ldx + c0;
  const cd* Lg = L + mat * sL;
  for (int e = t; e < N * N; e += HEGV_T) { const int i = e / N, j = e - i * N; Ls[i * ld + j] = j <= i ? Lg[e] : hz(0.0, 0.0); }
  for (int e = t; e < N * k; e += HEGV_T) { const int i = e / k, j = e - i * k; Xs[i * ldx_s + j] = Xg[i * ldx + j]; }
  __syncthreads();
  if (mode != 1) hegv_fwd_lds(Ls, ld, Xs, ldx_s, N, k);
  if (mode != 0) hegv_bwd_lds(Ls, ld, Xs, ldx_s, N, k);
  for (int e = t; e < N * k; e += HEGV_T) { const int i = e / k, j = e - i * k; Xg[i * ldx + j] = Xs[i * ldx_s + j]; }
}

// N = 1: lambda = Re a / Re b, X = 1 / sqrt(Re b) (X may be NULL); grid over the members
__global__ __launch_bounds__(256) void hegv_order_one(const cd* __restrict__ A, const cd* __restrict__ B, long sB, long total, double* __restrict__ lam,
                                                      cd* __restrict__ X, int* __restrict__ flags) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const double b = B[i * sB].x, v = A[i].x / b;
  int f = 0;
  if (!(b > 0.0 && b <= DBL_MAX)) f = HEGV_BAD_B;
  else if (!(fabs(v) <= DBL_MAX)) f = HEGV_BAD_C;
  lam[i] = v;
  if (X) X[i] = hz(1.0 / sqrt(b), 0.0);
  if (f) { flags[1 + i] = f; atomicOr(&flags[0], f); }
}

// ---- large tier -----------------------------------------------------------------------------------------------------------------
// dst = the lower triangle of src, Im of the diagonal dropped; above: the conjugate mirror, or zeros. grid (tiles of 256, members)
__global__ __launch_bounds__(256) void hegv_load_lower(const cd* __restrict__ src, cd* __restrict__ dst, int N, int mirror) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= (long)N * N) return;
  const long off = (long)blockIdx.y * N * N;
  const int i = (int)(e / N), j = (int)(e - (long)i * N);
  cd v;
  if (j < i) v = src[off + e];
  else if (j == i) v = hz(src[off + e].x, 0.0);
  else v = mirror ? hconj(src[off + (long)j * N + i]) : hz(0.0, 0.0);
  dst[off + e] = v;
}

// the diagonal block j0 .. j0 + nb - 1 of every member of L [members][N][N], in place; grid (members)
__global__ __launch_bounds__(HEGV_T) void zpotrf_diag(cd* __restrict__ L, int* __restrict__ flags, int N, int j0, int nb) {
  extern __shared__ __attribute__((aligned(16))) char hegv_smem[];
  cd* Ls = reinterpret_cast<cd*>(hegv_smem);
  const int ld = nb | 1, t = threadIdx.x;
  const long mat = blockIdx.x;
  cd* g = L + mat * N * N + (long)j0 * N + j0;
  for (int e = t; e < nb * nb; e += HEGV_T) { const int i = e / nb, j = e - i * nb; if (j <= i) Ls[i * ld + j] = g[(long)i * N + j]; }
  __syncthreads();
  const bool bad = hegv_chol_lds(Ls, nb, ld);
  for (int e = t; e < nb * nb; e += HEGV_T) { const int i = e / nb, j = e - i * nb; if (j <= i) g[(long)i * N + j] = Ls[i * ld + j]; }
  if (flags && t == 0 && bad) { atomicOr(&flags[1 + mat], HEGV_BAD_B); atomicOr(&flags[0], HEGV_BAD_B); }
}

// the rows j0 + nb + 64 blockIdx.x .. below the diagonal block; grid (row tiles, members)
__global__ __launch_bounds__(HEGV_T) void zpotrf_panel(cd* __restrict__ L, int N, int j0, int nb) {
  extern __shared__ __attribute__((aligned(16))) char hegv_smem[];
  const int ld = HEGV_NB + 1, t = threadIdx.x;
  cd* Ld = reinterpret_cast<cd*>(hegv_smem);
  cd* Ps = Ld + HEGV_NB * ld;
  cd* m = L + (long)blockIdx.y * N * N;
  const int r0 = j0 + nb + blockIdx.x * HEGV_NB, rows = N - r0 < HEGV_NB ? N - r0 : HEGV_NB;
  for (int e = t; e < nb * nb; e += HEGV_T) { const int i = e / nb, j = e - i * nb; if (j <= i) Ld[i * ld + j] = m[(long)(j0 + i) * N + j0 + j]; }
  for (int e = t; e < rows * nb; e += HEGV_T) { const int i = e / nb, j = e - i * nb; Ps[i * ld + j] = m[(long)(r0 + i) * N + j0 + j]; }
  __syncthreads();
  hegv_panel_lds(Ld, ld, Ps, ld, rows, nb);
  for (int e = t; e < rows * nb; e += HEGV_T) { const int i = e / nb, j = e - i * nb; m[(long)(r0 + i) * N + j0 + j] = Ps[i * ld + j]; }
}

// C [rows][cols] (row pitch ldc) -= sum_l a(i, l) conj(b(j, l)), one product at a time, l = 0 .. kb - 1 (rev: kb - 1 .. 0);
// a(i, l) = A[i ai + l al] (ca: conjugated), b(j, l) = B[j bj + l bl] (cb: conjugated). lower: only j <= i (rows = cols). The three
// arrays do not overlap in what is read and written. grid (column tiles, row tiles, members); 64 x 64 per workgroup, 16 l at a time
struct HegvUpd {
  const cd* A; long ai, al, sA; int ca;
  const cd* B; long bj, bl, sB; int cb;
  cd* C; long ldc, sC;
  int rows, cols, kb, lower, rev;
};
__global__ __launch_bounds__(HEGV_T) void hegv_update(HegvUpd u) {
  __shared__ cd As[16][HEGV_NB], Bs[16][HEGV_NB];
  const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
  const int i0 = blockIdx.y * HEGV_NB, j0 = blockIdx.x * HEGV_NB;
  if (u.lower && j0 > i0 + HEGV_NB - 1) return;               // (the whole workgroup)
  const cd* A = u.A + (long)blockIdx.z * u.sA;
  const cd* B = u.B + (long)blockIdx.z * u.sB;
  cd* C = u.C + (long)blockIdx.z * u.sC;
  cd acc[4][4];
#pragma unroll
  for (int p = 0; p < 4; ++p)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int i = i0 + ty + 16 * p, j = j0 + tx + 16 * q;
      acc[p][q] = (i < u.rows && j < u.cols) ? C[(long)i * u.ldc + j] : hz(0.0, 0.0);
    }
  const int nchunks = (u.kb + 15) / 16;
  for (int ch = 0; ch < nchunks; ++ch) {
    const int l0 = (u.rev ? nchunks - 1 - ch : ch) * 16, len = u.kb - l0 < 16 ? u.kb - l0 : 16;
    __syncthreads();
    for (int e = t; e < 16 * HEGV_NB; e += HEGV_T) {
      int l, i;
      if (u.al == 1) { l = e & 15; i = e >> 4; } else { i = e & 63; l = e >> 6; }
      cd v = hz(0.0, 0.0);
      if (i0 + i < u.rows && l < len) { v = A[(long)(i0 + i) * u.ai + (long)(l0 + l) * u.al]; if (u.ca) v.y = -v.y; }
      As[l][i] = v;
      if (u.bl == 1) { l = e & 15; i = e >> 4; } else { i = e & 63; l = e >> 6; }
      v = hz(0.0, 0.0);
      if (j0 + i < u.cols && l < len) { v = B[(long)(j0 + i) * u.bj + (long)(l0 + l) * u.bl]; if (u.cb) v.y = -v.y; }
      Bs[l][i] = v;
    }
    __syncthreads();
    for (int s = 0; s < len; ++s) {
      const int l = u.rev ? len - 1 - s : s;
      cd a[4], b[4];
#pragma unroll
      for (int p = 0; p < 4; ++p) { a[p] = As[l][ty + 16 * p]; b[p] = Bs[l][tx + 16 * p]; }
#pragma unroll
      for (int p = 0; p < 4; ++p)
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[p][q] = hegv_nmsc(acc[p][q], a[p], b[q]);
    }
  }
#pragma unroll
  for (int p = 0; p < 4; ++p)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int i = i0 + ty + 16 * p, j = j0 + tx + 16 * q;
      if (i < u.rows && j < u.cols && (!u.lower || j <= i)) C[(long)i * u.ldc + j] = acc[p][q];
    }
}

// rows j0 .. j0 + nb - 1 of X [members][N][K] against the diagonal block of L: L_d X = Y or L_d^H X = Y; grid (members, column tiles)
__global__ __launch_bounds__(HEGV_T) void ztrsm_diag(const cd* __restrict__ L, long sL, cd* __restrict__ X, int N, int K, int j0, int nb, int adjoint) {
  extern __shared__ __attribute__((aligned(16))) char hegv_smem[];
  const int ld = HEGV_NB + 1, t = threadIdx.x;
  cd* Ld = reinterpret_cast<cd*>(hegv_smem);
  cd* Xs = Ld + HEGV_NB * ld;
  const long mat = blockIdx.x;
  const int c0 = blockIdx.y * HEGV_NB, k = K - c0 < HEGV_NB ? K - c0 : HEGV_NB;
  const cd* g = L + mat * sL + (long)j0 * N + j0;
  cd* x = X + mat * N * K + (long)j0 * K + c0;
  for (int e = t; e < nb * nb; e += HEGV_T) { const int i = e / nb, j = e - i * nb; if (j <= i) Ld[i * ld + j] = g[(long)i * N + j]; }
  for (int e = t; e < nb * k; e += HEGV_T) { const int i = e / k, j = e - i * k; Xs[i * ld + j] = x[(long)i * K + j]; }
  __syncthreads();
  if (adjoint) hegv_bwd_lds(Ld, ld, Xs, ld, nb, k);
  else hegv_fwd_lds(Ld, ld, Xs, ld, nb, k);
  for (int e = t; e < nb * k; e += HEGV_T) { const int i = e / k, j = e - i * k; x[(long)i * K + j] = Xs[i * ld + j]; }
}

// C = W^H per member; grid (N / 32, N / 32, members), 256 threads
__global__ __launch_bounds__(256) void hegv_conj_transpose(const cd* __restrict__ W, cd* __restrict__ C, int N) {
  __shared__ cd tile[32][33];
  const long off = (long)blockIdx.z * N * N;
  const int bx = blockIdx.x * 32, by = blockIdx.y * 32, tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (int r = ty; r < 32; r += 8)
    if (by + r < N && bx + tx < N) tile[r][tx] = W[off + (long)(by + r) * N + bx + tx];
  __syncthreads();
  for (int r = ty; r < 32; r += 8)
    if (bx + r < N && by + tx < N) C[off + (long)(bx + r) * N + by + tx] = hconj(tile[tx][r]);
}

// zeros above the diagonal, Im c_ii = 0, bit 2 for a non-finite entry of the lower triangle; grid (tiles of 256, members)
__global__ __launch_bounds__(256) void hegv_finish_c(cd* __restrict__ C, int* __restrict__ flags, int N) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= (long)N * N) return;
  const long off = (long)blockIdx.y * N * N;
  const int i = (int)(e / N), j = (int)(e - (long)i * N);
  if (j > i) { C[off + e] = hz(0.0, 0.0); return; }
  cd v = C[off + e];
  if (j == i) { v.y = 0.0; C[off + e] = v; }
  if (flags && !hegv_finite(v)) { atomicOr(&flags[1 + blockIdx.y], HEGV_BAD_C); atomicOr(&flags[0], HEGV_BAD_C); }
}

// ---- host side ------------------------------------------------------------------------------------------------------------------
inline const cd* ccd(const double* p) { return reinterpret_cast<const cd*>(p); }
inline cd* mcd(double* p) { return reinterpret_cast<cd*>(p); }

int hegv_attr(const void* fn, size_t lds) {
  // above 64 KiB the launch needs the function attribute (set every time: it is per device)
  if (lds > 64 * 1024) ND4_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  return 0;
}
inline size_t hegv_tile_bytes(int n) { return sizeof(cd) * (size_t)n * hegv_ld(n); }
constexpr size_t HEGV_BLOCK_LDS = sizeof(cd) * 2 * HEGV_NB * (HEGV_NB + 1);   // a diagonal block and 64 rows or right-hand sides

// L [nb, N, N] = chol(H [nb, N, N]); flags [1 + nb] zero on entry, or NULL
int hegv_factor(nd4hip_handle* h, int64_t nb, int N, const cd* H, cd* L, int* flags) {
  if (N <= HEGV_SMALL_N) {
    const size_t lds = hegv_tile_bytes(N);
    ND4_TRY(hegv_attr(reinterpret_cast<const void*>(&zpotrf_small), lds));
    hipLaunchKernelGGL(zpotrf_small, dim3((unsigned)nb), dim3(HEGV_T), lds, h->stream, H, L, flags, N);
    ND4_HIP(hipGetLastError());
    return 0;
  }
  const int64_t nn = (int64_t)N * N;
  hipLaunchKernelGGL(hegv_load_lower, dim3((unsigned)((nn + 255) / 256), (unsigned)nb), dim3(256), 0, h->stream, H, L, N, 0);
  ND4_HIP(hipGetLastError());
  ND4_TRY(hegv_attr(reinterpret_cast<const void*>(&zpotrf_diag), hegv_tile_bytes(HEGV_NB)));
  ND4_TRY(hegv_attr(reinterpret_cast<const void*>(&zpotrf_panel), HEGV_BLOCK_LDS));
  for (int j0 = 0; j0 < N; j0 += HEGV_NB) {
    const int kb = N - j0 < HEGV_NB ? N - j0 : HEGV_NB, j1 = j0 + kb, rest = N - j1;
    hipLaunchKernelGGL(zpotrf_diag, dim3((unsigned)nb), dim3(HEGV_T), hegv_tile_bytes(kb), h->stream, L, flags, N, j0, kb);
    ND4_HIP(hipGetLastError());
    if (rest == 0) break;
    const unsigned tiles = (unsigned)((rest + HEGV_NB - 1) / HEGV_NB);
    hipLaunchKernelGGL(zpotrf_panel, dim3(tiles, (unsigned)nb), dim3(HEGV_T), HEGV_BLOCK_LDS, h->stream, L, N, j0, kb);
    ND4_HIP(hipGetLastError());
    const cd* P = L + (int64_t)j1 * N + j0;
    const HegvUpd u{P, N, 1, nn, 0, P, N, 1, nn, 0, L + (int64_t)j1 * N + j1, N, nn, rest, rest, kb, 1, 0};
    hipLaunchKernelGGL(hegv_update, dim3(tiles, tiles, (unsigned)nb), dim3(HEGV_T), 0, h->stream, u);
    ND4_HIP(hipGetLastError());
  }
  return 0;
}

// X [nb, N, K] in place: mode 0 L X = Y, 1 L^H X = Y, 2 L L^H X = Y; L stride sL (0 = one for all)
int hegv_solve(nd4hip_handle* h, int64_t nb, int N, int64_t K64, int mode, const cd* L, int64_t sL, cd* X) {
  const int64_t tiles64 = (K64 + HEGV_NB - 1) / HEGV_NB;
  ND4_CHECK_ARG(K64 < (1ll << 30) && tiles64 <= 65535, "nd4hip_ztrsm_batched: K exceeds 4 193 280 right-hand sides");
  const int K = (int)K64;
  const unsigned tiles = (unsigned)tiles64;
  if (N <= HEGV_SMALL_N) {
    const size_t lds = hegv_tile_bytes(N) + sizeof(cd) * (size_t)N * (HEGV_NB + 1);
    ND4_TRY(hegv_attr(reinterpret_cast<const void*>(&ztrsm_small), lds));
    hipLaunchKernelGGL(ztrsm_small, dim3((unsigned)nb, tiles), dim3(HEGV_T), lds, h->stream, L, (long)sL, X, N, K, (long)K, mode);
    ND4_HIP(hipGetLastError());
    return 0;
  }
  ND4_TRY(hegv_attr(reinterpret_cast<const void*>(&ztrsm_diag), HEGV_BLOCK_LDS));
  const int64_t nk = (int64_t)N * K;
  const int nblocks = (N + HEGV_NB - 1) / HEGV_NB;
  if (mode != 1)
    for (int s = 0; s < nblocks; ++s) {
      const int j0 = s * HEGV_NB, kb = N - j0 < HEGV_NB ? N - j0 : HEGV_NB, j1 = j0 + kb, rest = N - j1;
      hipLaunchKernelGGL(ztrsm_diag, dim3((unsigned)nb, tiles), dim3(HEGV_T), HEGV_BLOCK_LDS, h->stream, L, (long)sL, X, N, K, j0, kb, 0);
      ND4_HIP(hipGetLastError());
      if (rest == 0) break;
      const HegvUpd u{L + (int64_t)j1 * N + j0, N, 1, sL, 0, X + (int64_t)j0 * K, 1, K, nk, 1, X + (int64_t)j1 * K, K, nk, rest, K, kb, 0, 0};
      hipLaunchKernelGGL(hegv_update, dim3(tiles, (unsigned)((rest + HEGV_NB - 1) / HEGV_NB), (unsigned)nb), dim3(HEGV_T), 0, h->stream, u);
      ND4_HIP(hipGetLastError());
    }
  if (mode != 0)
    for (int s = nblocks - 1; s >= 0; --s) {
      const int j0 = s * HEGV_NB, kb = N - j0 < HEGV_NB ? N - j0 : HEGV_NB;
      hipLaunchKernelGGL(ztrsm_diag, dim3((unsigned)nb, tiles), dim3(HEGV_T), HEGV_BLOCK_LDS, h->stream, L, (long)sL, X, N, K, j0, kb, 1);
      ND4_HIP(hipGetLastError());
      if (j0 == 0) break;
      const HegvUpd u{L + (int64_t)j0 * N, 1, N, sL, 1, X + (int64_t)j0 * K, 1, K, nk, 1, X, K, nk, j0, K, kb, 0, 1};
      hipLaunchKernelGGL(hegv_update, dim3(tiles, (unsigned)(j0 / HEGV_NB), (unsigned)nb), dim3(HEGV_T), 0, h->stream, u);
      ND4_HIP(hipGetLastError());
    }
  return 0;
}

int hegst_small_launch(nd4hip_handle* h, int64_t nb, int N, const cd* A, const cd* T, int64_t sT, bool have_L, cd* Lout, cd* C, int* flags) {
  const size_t lds = 2 * hegv_tile_bytes(N);
  ND4_TRY(hegv_attr(reinterpret_cast<const void*>(&hegst_small), lds));
  hipLaunchKernelGGL(hegst_small, dim3((unsigned)nb), dim3(HEGV_T), lds, h->stream, A, T, (long)sT, have_L ? 1 : 0, Lout, C, flags, N);
  ND4_HIP(hipGetLastError());
  return 0;
}

// C [nb, N, N] = L^-1 A L^-H; W [nb, N, N] scratch; N > 64
int hegst_large(nd4hip_handle* h, int64_t nb, int N, const cd* A, const cd* L, int64_t sL, cd* W, cd* C, int* flags) {
  const int64_t nn = (int64_t)N * N;
  const dim3 grid((unsigned)((nn + 255) / 256), (unsigned)nb);
  const unsigned t32 = (unsigned)((N + 31) / 32);
  hipLaunchKernelGGL(hegv_load_lower, grid, dim3(256), 0, h->stream, A, W, N, 1);
  ND4_HIP(hipGetLastError());
  ND4_TRY(hegv_solve(h, nb, N, N, 0, L, sL, W));              // W = L^-1 A
  hipLaunchKernelGGL(hegv_conj_transpose, dim3(t32, t32, (unsigned)nb), dim3(256), 0, h->stream, W, C, N);   // C = W^H = A L^-H
  ND4_HIP(hipGetLastError());
  ND4_TRY(hegv_solve(h, nb, N, N, 0, L, sL, C));              // C = L^-1 A L^-H
  hipLaunchKernelGGL(hegv_finish_c, grid, dim3(256), 0, h->stream, C, flags, N);
  ND4_HIP(hipGetLastError());
  return 0;
}

// one read-back of the OR word; the member flags follow only when it is raised
int hegv_verdict(nd4hip_handle* h, const int* flags, int64_t nb, int64_t member0, const char* who) {
  void* hp = nullptr;
  ND4_TRY(nd4_pinned(h, sizeof(int) * (size_t)(nb + 1), &hp));
  int* host = static_cast<int*>(hp);
  ND4_HIP(hipMemcpyAsync(host, flags, sizeof(int), hipMemcpyDeviceToHost, h->stream));
  ND4_HIP(hipStreamSynchronize(h->stream));
  if (host[0] == 0) return 0;
  if (host[0] & HEGV_BAD_B) {
    ND4_HIP(hipMemcpyAsync(host, flags, sizeof(int) * (size_t)(nb + 1), hipMemcpyDeviceToHost, h->stream));
    ND4_HIP(hipStreamSynchronize(h->stream));
    int64_t b = 0;
    while (b < nb - 1 && !(host[1 + b] & HEGV_BAD_B)) ++b;
    nd4_set_error("%s is not positive definite. (matrix %lld)", who, (long long)(member0 + b));
    return ND4HIP_ERR_SINGULAR;
  }
  nd4_set_error("eigen_herm_gen(A,B): L^-1 A L^-H is not finite (NaN or Infinity in the lower triangle of A, or overflow).");
  return ND4HIP_ERR_NOCONV;
}

template <class T> int hegv_alloc(nd4hip_handle* h, size_t n, T** out) {
  void* p = nullptr;
  ND4_TRY(nd4_ws_alloc(h, sizeof(T) * n, &p));
  *out = static_cast<T*>(p);
  return 0;
}

constexpr const char* HEGV_WHO = "eigen_herm_gen(A,B): B";

}  // namespace

// ---- the host-side arithmetic of the tiers (tools/hegv_host_check.hip) ----
int nd4_hegv_tier(int64_t N) { return N <= HEGV_SMALL_N ? 0 : 1; }
// the largest dynamic LDS request of any kernel that runs at this N
size_t nd4_hegv_lds(int64_t N) {
  if (nd4_hegv_tier(N) == 0)                   // ztrsm_small: L and 64 right-hand sides at pitch 65, never less than hegst_small's two tiles
    return hegv_tile_bytes((int)N) + sizeof(cd) * (size_t)N * (HEGV_NB + 1);
  return HEGV_BLOCK_LDS;
}
// members per pass: L, W and C are N^2 complex elements per member each, at most 1 GiB each (32 768 members up to N = 45)
int64_t nd4_hegv_chunk(int64_t batch, int64_t N) {
  int64_t c = HEGV_CHUNK;
  if (HEGV_WS_ELEMS / (N * N) < c) c = HEGV_WS_ELEMS / (N * N);
  if (c < 1) c = 1;
  return batch < c ? batch : c;
}

// herm_cholesky_decomp: L [batch, N, N] = chol(H). Arguments already checked, batch >= 1, 1 <= N <= 2048. Synchronises (one flag word per pass)
int nd4_zpotrf(nd4hip_handle* h, int64_t batch, int64_t N64, const double* H, double* L, int64_t member0) {
  const int N = (int)N64;
  const int64_t nn = N64 * N64, chunk = nd4_hegv_chunk(batch, N64);
  Nd4WsScope scope(h);
  int* flags = nullptr;
  ND4_TRY(hegv_alloc(h, (size_t)(chunk + 1), &flags));
  for (int64_t b0 = 0; b0 < batch; b0 += chunk) {
    const int64_t nb = batch - b0 < chunk ? batch - b0 : chunk;
    ND4_HIP(hipMemsetAsync(flags, 0, sizeof(int) * (size_t)(nb + 1), h->stream));
    ND4_TRY(hegv_factor(h, nb, N, ccd(H) + b0 * nn, mcd(L) + b0 * nn, flags));
    ND4_TRY(hegv_verdict(h, flags, nb, member0 + b0, "herm_cholesky_decomp(H): H"));
  }
  return 0;
}

// ztril_solve / herm_cholesky_solve: X [batch, N, K] in place; mode 0 L X = Y, 1 L^H X = Y, 2 L L^H X = Y. Enqueues only
int nd4_ztrsm(nd4hip_handle* h, int mode, int64_t batch, int64_t N64, int64_t K, const double* L, int64_t sL, double* X) {
  const int64_t chunk = nd4_hegv_chunk(batch, N64);
  for (int64_t b0 = 0; b0 < batch; b0 += chunk) {
    const int64_t nb = batch - b0 < chunk ? batch - b0 : chunk;
    ND4_TRY(hegv_solve(h, nb, (int)N64, K, mode, ccd(L) + b0 * sL, sL, mcd(X) + b0 * N64 * K));
  }
  return 0;
}

// herm_gen_reduce: C [batch, N, N] = L^-1 A L^-H from a given L (stride sL, 0 = one L). Enqueues only
int nd4_zhegst(nd4hip_handle* h, int64_t batch, int64_t N64, const double* A, const double* L, int64_t sL, double* C) {
  const int N = (int)N64;
  const int64_t nn = N64 * N64, chunk = nd4_hegv_chunk(batch, N64);
  const bool small = N <= HEGV_SMALL_N;
  Nd4WsScope scope(h);
  cd* Ww = nullptr;
  if (!small) ND4_TRY(hegv_alloc(h, (size_t)(chunk * nn), &Ww));
  for (int64_t b0 = 0; b0 < batch; b0 += chunk) {
    const int64_t nb = batch - b0 < chunk ? batch - b0 : chunk;
    if (small) ND4_TRY(hegst_small_launch(h, nb, N, ccd(A) + b0 * nn, ccd(L) + b0 * sL, sL, true, nullptr, mcd(C) + b0 * nn, nullptr));
    else       ND4_TRY(hegst_large(h, nb, N, ccd(A) + b0 * nn, ccd(L) + b0 * sL, sL, Ww, mcd(C) + b0 * nn, nullptr));
  }
  return 0;
}

// eigen_herm_gen / eigenvals_herm_gen: A [batch, N, N], B [batch (stride sB = N*N, or 0: one B), N, N] -> lambda [batch, K] descending,
// X [batch, N, K] or NULL; every eigenpair (all, K = N) or the subset i0 <= i < i1 (K = i1 - i0). member0: the index of the first
// member in the caller's batch, for the error text. Synchronises.
int nd4_zhegvx(nd4hip_handle* h, bool all, int64_t i0, int64_t i1, int64_t batch, int64_t N64, const double* Am, const double* Bm, int64_t sB,
               double* lambda, double* Xm, int64_t member0) {
  const int N = (int)N64;
  const int64_t K = all ? N64 : i1 - i0, nn = N64 * N64;
  const bool small = N <= HEGV_FUSED_N, shared = sB == 0;   // (the factorisation and the solves choose their own tier by N)
  const int64_t chunk = nd4_hegv_chunk(batch, N64);
  const cd *A = ccd(Am), *B = ccd(Bm);
  cd* X = Xm ? mcd(Xm) : nullptr;
  // one request for the flags, L, C and W: a call's first request reuses a cached block of the arena, later ones may not
  Nd4WsScope scope(h);
  const size_t fbytes = (sizeof(int) * (size_t)(chunk + 1) + 255) & ~size_t(255);
  const size_t lelems = N == 1 ? 0 : (size_t)((shared ? 1 : chunk) * nn), celems = N == 1 ? 0 : (size_t)(chunk * nn);
  char* ws = nullptr;
  ND4_TRY(hegv_alloc(h, fbytes + sizeof(cd) * (lelems + celems * (small ? 1 : 2)), &ws));
  int* flags = reinterpret_cast<int*>(ws);
  if (N == 1) {
    for (int64_t b0 = 0; b0 < batch; b0 += chunk) {
      const int64_t nb = batch - b0 < chunk ? batch - b0 : chunk;
      ND4_HIP(hipMemsetAsync(flags, 0, sizeof(int) * (size_t)(nb + 1), h->stream));
      if (K > 0) {
        hipLaunchKernelGGL(hegv_order_one, dim3((unsigned)((nb + 255) / 256)), dim3(256), 0, h->stream, A + b0, B + b0 * sB, (long)sB, (long)nb,
                           lambda + b0, X ? X + b0 : nullptr, flags);
        ND4_HIP(hipGetLastError());
      }
      ND4_TRY(hegv_verdict(h, flags, nb, member0 + b0, HEGV_WHO));
    }
    return 0;
  }
  cd* Lw = reinterpret_cast<cd*>(ws + fbytes);
  cd *Cw = Lw + lelems, *Ww = small ? nullptr : Cw + celems;
  if (shared) {                                 // one B: factorised once, before the passes over the members
    ND4_HIP(hipMemsetAsync(flags, 0, sizeof(int) * 2, h->stream));
    ND4_TRY(hegv_factor(h, 1, N, B, Lw, flags));
    ND4_TRY(hegv_verdict(h, flags, 1, member0, HEGV_WHO));
  }
  for (int64_t b0 = 0; b0 < batch; b0 += chunk) {
    const int64_t nb = batch - b0 < chunk ? batch - b0 : chunk;
    const cd* Ab = A + b0 * nn;
    double* lam = lambda + b0 * K;
    cd* Xb = X ? X + b0 * N64 * K : nullptr;
    ND4_HIP(hipMemsetAsync(flags, 0, sizeof(int) * (size_t)(nb + 1), h->stream));
    if (small) {
      ND4_TRY(hegst_small_launch(h, nb, N, Ab, shared ? Lw : B + b0 * sB, sB, shared, (shared || !X) ? nullptr : Lw, Cw, flags));
    } else {
      if (!shared) ND4_TRY(hegv_factor(h, nb, N, B + b0 * sB, Lw, flags));
      ND4_TRY(hegst_large(h, nb, N, Ab, Lw, shared ? 0 : nn, Ww, Cw, flags));
    }
    ND4_TRY(hegv_verdict(h, flags, nb, member0 + b0, HEGV_WHO));
    if (K == 0) continue;
    if (all) ND4_TRY(nd4_zheevd(h, nb, N, reinterpret_cast<const double*>(Cw), lam, reinterpret_cast<double*>(Xb)));
    else     ND4_TRY(nd4_zheevx(h, nb, N, i0, i1, reinterpret_cast<const double*>(Cw), lam, reinterpret_cast<double*>(Xb)));
    if (Xb) ND4_TRY(hegv_solve(h, nb, N, K, 1, Lw, shared ? 0 : nn, Xb));
  }
  ND4_HIP(hipStreamSynchronize(h->stream));
  return 0;
}
