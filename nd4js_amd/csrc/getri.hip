// Matrix inverses on the device: inv / tril_inv / triu_inv / cholesky_inv. float64, row-major members, 1 <= N <= 2048.
//
// inv is LAPACK's getri on lu_decomp's factorisation: X = U^-1 (L^-1 P) from a partial-pivoting LU, never Gauss-Jordan on [A | I]. Pivot
// of column j: the first row i >= j with the largest |a_ij|; a later row wins only by strict >, a NaN never wins unless it is the start
// row (gi_key turns that rule into a total order, so a tree reduction gives the scalar scan's answer). Every division is a true division.
// A pivot that is zero or not finite sets the member's flag to 1 + its column (the first such column); the member's X is then all NaN.
// The triangular inverses are substitutions with true divisions that never read the other triangle and leave +0 in it.
//
// Register tier, N <= 16 (getri_reg<NP>, NP = 4, 8, 16 the padded order): a member occupies one DPP row of 16 lanes, a wave holds four
//   members, a workgroup sixteen. Lane i of the row holds row i of A and row i of Z. The column loops are expanded at compile time (folds
//   over integer sequences), so every register index is static. Arg-max by DPP inside the row; the pivot row and the substitution rows
//   are broadcast inside the row of 16 lanes by __shfl(., src, 16), because the pivot differs per member. Z = the permuted identity (row i
//   is e_P[i]), then the unit lower sweep (rows below i subtract l_ri Z_i), then the upper sweep from the bottom (row i is divided by
//   u_ii, rows above subtract u_ri Z_i). No LDS and no barrier.
// LDS tier, 16 < N <= 128 where the tile fits the device's LDS limit for a workgroup (getri_lds, trtri_lds): one workgroup of 256 threads per member, one tile at
//   pitch N | 1 and one N-vector. LU in place, then getri's in-place form: U is inverted in place row by row from the bottom (the row of U
//   is saved in the vector, every thread owns a column), then X L = U^-1 from the last column to the first with the column of L saved in
//   the vector; the columns are un-permuted on the way out. trtri_lds is the same substitution on the named triangle; for cholesky_inv
//   the product W^T W of W = L^-1 follows in the same launch, each (i, j), i >= j, computed once and stored to both places.
// Blocked tier, blocks of 64:
//   trtri_diag     every 64 x 64 diagonal block inverted by substitution in LDS, one workgroup per block; it also clears the blocks of
//                  its block column that lie in the other triangle.
//   trtri_trmm     C = -T B with T triangular, on v_mfma_f64_16x16x4_f64: a workgroup owns 64 rows of C, a wave 16 of them and four
//                  16 x 16 accumulators; the K loop of a row tile covers only the tiles of T on its side of the diagonal, and the
//                  loads mask the other triangle, so it is neither read nor multiplied. Block column j of U^-1 above the diagonal is
//                  -X[0:j, 0:j] (U[0:j, j] X_jj): the small right factor on the GEMM, the triangular product here.
//   getri_rsolve   X[:, j] <- X[:, j] L_jj^-1 against the 64 x 64 unit lower block, 32 rows of X per workgroup in LDS.
//   inv: nd4_getrf into workspace, getri_flags (the first unusable diagonal entry of U), trtri_diag + trtri_trmm for U^-1, then getri's
//   sweep from the last block column to the first, X[:, j] <- (U^-1[:, j] - X[:, j+1:] L[j+1:, j]) L_jj^-1 with the rectangular update
//   on the GEMM, the column un-permutation by struct.hip's kernel, and getri_poison for the flagged members.
//   tril_inv / triu_inv: trtri_diag + trtri_trmm, then trtri_poison: after a row whose diagonal entry is zero or NaN every row is NaN in
//   its triangle, as in tril_solve(L, I), where that row's 0 / 0 in the other triangle reaches every later row (gi_trtri_tile does the
//   same inside a tile).
//   cholesky_inv: W = L^-1 as above, X = W^T W on the GEMM, getri_mirror copies the lower triangle onto the upper.
// No atomics on doubles, no synchronisation but __syncthreads(), wave shuffles / DPP and the kernel boundary.
// Flags: [0] the OR over the members of a pass, [1 + member] = 1 + the first column with an unusable pivot.
#include "nd4hip_internal.h"
#include "dpp.h"
#include <cfloat>
#include <climits>
#include <cmath>
#include <utility>

namespace {

typedef double d4 __attribute__((ext_vector_type(4)));

constexpr int GI_REG_N = 16;                    // four members per wave in registers up to here
constexpr int GI_LDS_N = 128;                   // one member per workgroup in LDS up to here (if the tile fits)
constexpr int GI_NB = 64;                       // block of the blocked tier
constexpr int GI_T = 256;                       // threads per workgroup
constexpr int GI_BK = 32;                       // K step of trtri_trmm
constexpr int GI_RS = 32;                       // rows of X per workgroup of getri_rsolve
constexpr int64_t GI_CHUNK = 32768;             // members per pass
constexpr int64_t GI_WS_ELEMS = 1ll << 27;      // blocked tier: a pass's workspace takes at most 1 GiB

__device__ __forceinline__ double gi_key(double v, bool start) {
  const double m = fabs(v);
  return m != m ? (start ? INFINITY : -1.0) : m;
}
__device__ __forceinline__ bool gi_better(double m, int i, double bm, int bi) { return m > bm || (m == bm && i < bi); }
__device__ __forceinline__ bool gi_bad_pivot(double p) { const double m = fabs(p); return !(m > 0.0 && m <= DBL_MAX); }

// ---- register tier ----------------------------------------------------------------------------------------------------------------
#define GI_DPP_STEP(X)                                                     \
  do { const double om = nd4dpp::X(m); const int oi = nd4dpp::X(idx);      \
       if (gi_better(om, oi, m, idx)) { m = om; idx = oi; } } while (0)

// column J of the LU of the member that this row of 16 lanes holds: a[c] = row `sub`, column c; orig: the row's index in A
template <int NP, int J>
__device__ __forceinline__ void gi_reg_lu(double (&a)[NP], int& orig, int& flag, int sub, int N) {
  if (J >= N) return;                                          // (the whole wave)
  double m = -2.0;
  int idx = INT_MAX;
  if (sub >= J && sub < N) { m = gi_key(a[J], sub == J); idx = sub; }
  GI_DPP_STEP(xor1); GI_DPP_STEP(xor2); GI_DPP_STEP(xor4); GI_DPP_STEP(xor8);   // every lane: the best of its row of 16 lanes
  const int piv = idx;
  // rows J and piv change places: each of the two lanes reads the other's row
  const int src = sub == J ? piv : (sub == piv ? J : sub);
#pragma unroll
  for (int c = 0; c < NP; ++c) a[c] = __shfl(a[c], src, 16);
  orig = __shfl(orig, src, 16);
  const double p = __shfl(a[J], J, 16);
  const bool bad = gi_bad_pivot(p);
  if (bad && !flag) flag = J + 1;
  const bool below = sub > J && sub < N;
  double l = a[J];
  if (below && !bad) { l = l / p; a[J] = l; }
#pragma unroll
  for (int c = J + 1; c < NP; ++c) {
    const double u = __shfl(a[c], J, 16);
    if (below) a[c] -= l * u;
  }
}
// L Z = Z, L unit lower: the rows below I subtract l_rI Z_I
template <int NP, int I>
__device__ __forceinline__ void gi_reg_fwd(const double (&a)[NP], double (&z)[NP], int sub, int N) {
  if (I + 1 >= N) return;
#pragma unroll
  for (int c = 0; c < NP; ++c) {
    const double zi = __shfl(z[c], I, 16);
    if (sub > I && sub < N) z[c] -= a[I] * zi;
  }
}
// U Z = Z from the bottom: row I = NP - 1 - R is divided by u_II, the rows above subtract u_rI Z_I
template <int NP, int R>
__device__ __forceinline__ void gi_reg_bwd(const double (&a)[NP], double (&z)[NP], int sub, int N) {
  constexpr int I = NP - 1 - R;
  if (I >= N) return;
  if (sub == I) {
#pragma unroll
    for (int c = 0; c < NP; ++c) z[c] = z[c] / a[I];
  }
#pragma unroll
  for (int c = 0; c < NP; ++c) {
    const double zi = __shfl(z[c], I, 16);
    if (sub < I) z[c] -= a[I] * zi;
  }
}
template <int NP, int... J>
__device__ __forceinline__ void gi_reg_all(std::integer_sequence<int, J...>, double (&a)[NP], double (&z)[NP], int& orig, int& flag, int sub, int N) {
  (gi_reg_lu<NP, J>(a, orig, flag, sub, N), ...);
#pragma unroll
  for (int c = 0; c < NP; ++c) z[c] = c == orig ? 1.0 : 0.0;   // row i of the permuted identity is e_P[i]
  (gi_reg_fwd<NP, J>(a, z, sub, N), ...);
  (gi_reg_bwd<NP, J>(a, z, sub, N), ...);
}

// N <= NP <= 16; grid (ceil(members / 16)), 256 threads: the row of 16 lanes q of workgroup b holds member 16 b + q
template <int NP>
__global__ __launch_bounds__(GI_T) void getri_reg(const double* __restrict__ A, double* __restrict__ X, int* __restrict__ flags, int N, long members) {
  const int sub = threadIdx.x & 15;
  const long mat = (long)blockIdx.x * 16 + (threadIdx.x >> 4);
  if (mat >= members) return;                                  // (whole rows of 16 lanes)
  const double* g = A + mat * N * N + (long)sub * N;
  double a[NP], z[NP];
#pragma unroll
  for (int c = 0; c < NP; ++c) a[c] = (sub < N && c < N) ? g[c] : 0.0;
  int orig = sub, flag = 0;
  gi_reg_all<NP>(std::make_integer_sequence<int, NP>{}, a, z, orig, flag, sub, N);
  if (sub < N) {
    double* o = X + mat * N * N + (long)sub * N;
#pragma unroll
    for (int c = 0; c < NP; ++c)
      if (c < N) o[c] = flag ? NAN : z[c];
  }
  if (sub == 0 && flag) { flags[1 + mat] = flag; atomicOr(&flags[0], 1); }
}

// ---- substitution on an LDS tile by all GI_T threads; ends behind a barrier ---------------------------------------------------------
// S [n][ld] <- the inverse of its upper (lower) triangle in place; the other triangle is neither read nor written. Row by row, from the
// bottom (top): the row of the operand goes to vec [n], then the thread of column c forms (delta_ic - sum_k t_ik x_kc) / t_ii.
// The result holds the inf / NaN of the substitution on the whole identity (tril_solve(L, I)): there a zero or NaN t_ii leaves 0 / t_ii
// = NaN in the other triangle of row i, which every later row multiplies into all its entries, so after such a row every row is NaN
__device__ void gi_trtri_tile(double* S, int ld, double* vec, int n, bool upper) {
  const int t = threadIdx.x;
  bool dead = false;                                           // (the whole workgroup)
  for (int s = 0; s < n; ++s) {
    const int i = upper ? n - 1 - s : s;
    const bool mine = t < n && (upper ? t >= i : t <= i);
    if (mine) vec[t] = S[i * ld + t];
    __syncthreads();
    const double d = vec[i];
    if (mine) {
      double x = t == i ? 1.0 : 0.0;
      if (upper) for (int k = i + 1; k <= t; ++k) x -= vec[k] * S[k * ld + t];
      else       for (int k = t; k < i; ++k) x -= vec[k] * S[k * ld + t];
      S[i * ld + t] = dead ? NAN : x / d;
    }
    dead = dead || d == 0.0 || d != d;
    __syncthreads();
  }
}

// ---- LDS tier ---------------------------------------------------------------------------------------------------------------------
inline size_t gi_lds_bytes(int n) { return sizeof(double) * ((size_t)n * (n | 1) + n); }

__device__ __forceinline__ void gi_wave_argmax(double& bm, int& bi) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const double om = __shfl_xor(bm, off);
    const int oi = __shfl_xor(bi, off);
    if (gi_better(om, oi, bm, bi)) { bm = om; bi = oi; }
  }
}

// 16 < N <= 128; grid (members); dynamic LDS gi_lds_bytes(N)
__global__ __launch_bounds__(GI_T) void getri_lds(const double* __restrict__ A, double* __restrict__ X, int* __restrict__ flags, int N) {
  extern __shared__ __attribute__((aligned(16))) double gi_smem[];
  __shared__ int perm[GI_LDS_N];
  __shared__ int s_piv, s_flag;
  double* S = gi_smem;
  const int ld = N | 1, t = threadIdx.x;
  double* vec = S + N * ld;
  const long mat = blockIdx.x;
  for (int e = t; e < N * N; e += GI_T) { const int i = e / N, j = e - i * N; S[i * ld + j] = A[mat * N * N + e]; }
  if (t < N) perm[t] = t;
  if (t == 0) s_flag = 0;
  __syncthreads();
  for (int j = 0; j < N; ++j) {
    if (t < 64) {                                              // wave 0: lane l looks at the rows j + l, j + l + 64
      double bm = -2.0;
      int bi = INT_MAX;
      for (int row = j + t; row < N; row += 64) {
        const double m = gi_key(S[row * ld + j], row == j);
        if (gi_better(m, row, bm, bi)) { bm = m; bi = row; }
      }
      gi_wave_argmax(bm, bi);
      if (t == 0) s_piv = bi;
    }
    __syncthreads();
    const int piv = s_piv;
    if (piv != j) {
      if (t < N) { const double a = S[j * ld + t]; S[j * ld + t] = S[piv * ld + t]; S[piv * ld + t] = a; }
      if (t == GI_T - 1) { const int a = perm[j]; perm[j] = perm[piv]; perm[piv] = a; }
    }
    __syncthreads();
    const double p = S[j * ld + j];
    const bool bad = gi_bad_pivot(p);
    if (t == 0 && bad && !s_flag) s_flag = j + 1;
    if (!bad)
      for (int i = j + 1 + t; i < N; i += GI_T) S[i * ld + j] = S[i * ld + j] / p;
    __syncthreads();
    const int m = N - j - 1;
    for (int e = t; e < m * m; e += GI_T) {
      const int i = j + 1 + e / m, c = j + 1 + e % m;
      S[i * ld + c] -= S[i * ld + j] * S[j * ld + c];
    }
    __syncthreads();
  }
  const int flag = s_flag;
  if (flag) {                                                  // (the whole workgroup)
    for (int e = t; e < N * N; e += GI_T) X[mat * N * N + e] = NAN;
    if (t == 0) { flags[1 + mat] = flag; atomicOr(&flags[0], 1); }
    return;
  }
  gi_trtri_tile(S, ld, vec, N, true);                          // U^-1 in place of U
  // X L = U^-1 from the last column to the first: column j of L goes to vec and leaves zeros, then every row subtracts
  for (int j = N - 2; j >= 0; --j) {
    if (t > j && t < N) { vec[t] = S[t * ld + j]; S[t * ld + j] = 0.0; }
    __syncthreads();
    if (t < N) {
      double x = S[t * ld + j];
      for (int k = j + 1; k < N; ++k) x -= S[t * ld + k] * vec[k];
      S[t * ld + j] = x;
    }
    __syncthreads();
  }
  for (int e = t; e < N * N; e += GI_T) { const int i = e / N, j = e - i * N; X[mat * N * N + (long)i * N + perm[j]] = S[i * ld + j]; }
}

// mode 0: X = the inverse of the lower triangle of T, 1: of the upper triangle, 2: X = W^T W for W = the inverse of the lower triangle.
// N <= 128; grid (members); dynamic LDS gi_lds_bytes(N)
__global__ __launch_bounds__(GI_T) void trtri_lds(const double* __restrict__ T, double* __restrict__ X, int N, int mode) {
  extern __shared__ __attribute__((aligned(16))) double gi_smem[];
  double* S = gi_smem;
  const int ld = N | 1, t = threadIdx.x;
  double* vec = S + N * ld;
  const long mat = blockIdx.x;
  const bool upper = mode == 1;
  for (int e = t; e < N * N; e += GI_T) {
    const int i = e / N, j = e - i * N;
    S[i * ld + j] = (upper ? j >= i : j <= i) ? T[mat * N * N + e] : 0.0;
  }
  __syncthreads();
  gi_trtri_tile(S, ld, vec, N, upper);
  double* x = X + mat * N * N;
  if (mode != 2) {
    for (int e = t; e < N * N; e += GI_T) { const int i = e / N, j = e - i * N; x[e] = S[i * ld + j]; }
    return;
  }
  for (int e = t; e < N * N; e += GI_T) {
    const int i = e / N, j = e - i * N;
    if (j > i) continue;
    double s = 0.0;
    for (int k = i; k < N; ++k) s += S[k * ld + i] * S[k * ld + j];
    x[(long)i * N + j] = s;
    x[(long)j * N + i] = s;
  }
}

// ---- blocked tier -------------------------------------------------------------------------------------------------------------------
// the diagonal block blockIdx.x of every member: dst block = the inverse of the named triangle of the src block (zeros in the other
// triangle); the blocks of the block column in the other triangle of dst are cleared. Row pitch N, members sS / sD apart. grid (blocks, members)
__global__ __launch_bounds__(GI_T) void trtri_diag(const double* __restrict__ src, long sS, double* __restrict__ dst, long sD, int N, int upper) {
  __shared__ double Ts[GI_NB * (GI_NB + 1)], vec[GI_NB];
  const int ld = GI_NB + 1, t = threadIdx.x;
  const int j0 = blockIdx.x * GI_NB, kb = N - j0 < GI_NB ? N - j0 : GI_NB, j1 = j0 + kb;
  const double* g = src + blockIdx.y * sS + (long)j0 * N + j0;
  double* d = dst + blockIdx.y * sD;
  for (int e = t; e < kb * kb; e += GI_T) {
    const int i = e / kb, j = e - i * kb;
    Ts[i * ld + j] = (upper ? j >= i : j <= i) ? g[(long)i * N + j] : 0.0;
  }
  __syncthreads();
  gi_trtri_tile(Ts, ld, vec, kb, upper != 0);
  for (int e = t; e < kb * kb; e += GI_T) { const int i = e / kb, j = e - i * kb; d[(long)(j0 + i) * N + j0 + j] = Ts[i * ld + j]; }
  const int r0 = upper ? j1 : 0, rows = upper ? N - j1 : j0;
  for (int e = t; e < rows * kb; e += GI_T) { const int i = e / kb, j = e - i * kb; d[(long)(r0 + i) * N + j0 + j] = 0.0; }
}

// C [M][nc] (row pitch ldc) = -T B for T [M][M] (lda) upper or lower triangular and B [M][nc] (ldb), nc <= 64, on the fp64 MFMA. Only the
// named triangle of T is read. C does not overlap what is read of T and B. grid (row tiles of 64, members), members sT / sB / sC apart
struct GiTrmm {
  const double* T; long lda, sT;
  const double* B; long ldb, sB;
  double* C; long ldc, sC;
  int M, nc, upper;
};
__global__ __launch_bounds__(GI_T) void trtri_trmm(GiTrmm g) {
  __shared__ double sa[GI_NB * (GI_BK + 1)], sb[GI_BK * (GI_NB + 1)];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, fx = lane & 15, fk = lane >> 4;
  const int m0 = blockIdx.x * GI_NB;
  const double* T = g.T + blockIdx.y * g.sT;
  const double* B = g.B + blockIdx.y * g.sB;
  double* C = g.C + blockIdx.y * g.sC;
  // the columns of T that meet the rows m0 .. m0 + 63 on the named side of the diagonal
  const int klo = g.upper ? m0 : 0, khi = g.upper ? g.M : (m0 + GI_NB < g.M ? m0 + GI_NB : g.M);
  d4 acc[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) acc[j] = d4{0.0, 0.0, 0.0, 0.0};
  for (int k0 = klo; k0 < khi; k0 += GI_BK) {
    for (int e = t; e < GI_NB * GI_BK; e += GI_T) {
      const int i = e / GI_BK, k = e - i * GI_BK, row = m0 + i, col = k0 + k;
      const bool in = row < g.M && col < khi && (g.upper ? col >= row : col <= row);
      sa[i * (GI_BK + 1) + k] = in ? T[(long)row * g.lda + col] : 0.0;
    }
    for (int e = t; e < GI_BK * GI_NB; e += GI_T) {
      const int k = e / GI_NB, j = e - k * GI_NB, row = k0 + k;
      sb[k * (GI_NB + 1) + j] = (row < khi && j < g.nc) ? B[(long)row * g.ldb + j] : 0.0;
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < GI_BK / 4; ++kk) {
      const double a = sa[(wave * 16 + fx) * (GI_BK + 1) + kk * 4 + fk];
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, sb[(kk * 4 + fk) * (GI_NB + 1) + j * 16 + fx], acc[j], 0, 0, 0);
    }
    __syncthreads();
  }
  // lane holds C[row = (lane >> 4) + 4 r][col = lane & 15] of each 16 x 16 tile
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = m0 + wave * 16 + fk + 4 * r, col = j * 16 + fx;
      if (row < g.M && col < g.nc) C[(long)row * g.ldc + col] = -acc[j][r];
    }
}

// X[:, j0 .. j0 + kb - 1] <- X[:, j0 ..] L^-1 for the unit lower kb x kb block L of LU at (j0, j0) (its diagonal is not read): 32 rows of
// X per workgroup (with the block of L 50 KB of LDS). Row pitch N, members N N apart. grid (row tiles of 32, members)
__global__ __launch_bounds__(GI_T) void getri_rsolve(double* __restrict__ X, const double* __restrict__ LU, int N, int j0, int kb) {
  __shared__ double Ls[GI_NB * (GI_NB + 1)], Xs[GI_RS * (GI_NB + 1)];
  const int ld = GI_NB + 1, t = threadIdx.x;
  const int r0 = blockIdx.x * GI_RS, rows = N - r0 < GI_RS ? N - r0 : GI_RS;
  const double* l = LU + (long)blockIdx.y * N * N + (long)j0 * N + j0;
  double* x = X + (long)blockIdx.y * N * N + (long)r0 * N + j0;
  for (int e = t; e < kb * kb; e += GI_T) { const int i = e / kb, j = e - i * kb; Ls[i * ld + j] = l[(long)i * N + j]; }
  for (int e = t; e < rows * kb; e += GI_T) { const int i = e / kb, j = e - i * kb; Xs[i * ld + j] = x[(long)i * N + j]; }
  __syncthreads();
  for (int k = kb - 1; k >= 1; --k) {                          // column k is final: the columns left of it subtract x_rk l_kc
    for (int e = t; e < rows * k; e += GI_T) { const int i = e / k, c = e - i * k; Xs[i * ld + c] -= Xs[i * ld + k] * Ls[k * ld + c]; }
    __syncthreads();
  }
  for (int e = t; e < rows * kb; e += GI_T) { const int i = e / kb, j = e - i * kb; x[(long)i * N + j] = Xs[i * ld + j]; }
}

// the first diagonal entry of U that is zero or not finite; grid (members)
__global__ __launch_bounds__(GI_T) void getri_flags(const double* __restrict__ LU, int N, int* __restrict__ flags) {
  __shared__ int first;
  if (threadIdx.x == 0) first = INT_MAX;
  __syncthreads();
  const double* m = LU + (long)blockIdx.x * N * N;
  int mine = INT_MAX;
  for (int j = threadIdx.x; j < N; j += GI_T)
    if (gi_bad_pivot(m[(long)j * N + j]) && j < mine) mine = j;
  if (mine != INT_MAX) atomicMin(&first, mine);
  __syncthreads();
  if (threadIdx.x == 0 && first != INT_MAX) { flags[1 + blockIdx.x] = first + 1; atomicOr(&flags[0], 1); }
}

// NaN into every element of the flagged members; grid (tiles, members)
__global__ __launch_bounds__(GI_T) void getri_poison(double* __restrict__ X, long nn, const int* __restrict__ flags) {
  if (flags[1 + blockIdx.y] == 0) return;
  double* x = X + blockIdx.y * nn;
  for (long e = (long)blockIdx.x * GI_T + threadIdx.x; e < nn; e += (long)gridDim.x * GI_T) x[e] = NAN;
}

// the lower triangle onto the upper; grid (tiles, members)
__global__ __launch_bounds__(GI_T) void getri_mirror(double* __restrict__ X, int N) {
  double* x = X + (long)blockIdx.y * N * N;
  for (long e = (long)blockIdx.x * GI_T + threadIdx.x; e < (long)N * N; e += (long)gridDim.x * GI_T) {
    const int i = (int)(e / N), j = (int)(e - (long)i * N);
    if (j > i) x[e] = x[(long)j * N + i];
  }
}

// gi_trtri_tile's rule across the blocks: NaN into the named triangle of every row of X behind the first zero or NaN on the diagonal of
// T (below it: lower, above it: upper). Every workgroup finds that row itself; grid (tiles, members)
__global__ __launch_bounds__(GI_T) void trtri_poison(const double* __restrict__ T, double* __restrict__ X, int N, int upper) {
  __shared__ int first;
  if (threadIdx.x == 0) first = upper ? -1 : INT_MAX;
  __syncthreads();
  const double* m = T + (long)blockIdx.y * N * N;
  for (int j = threadIdx.x; j < N; j += GI_T) {
    const double d = m[(long)j * N + j];
    if (d == 0.0 || d != d) { if (upper) atomicMax(&first, j); else atomicMin(&first, j); }
  }
  __syncthreads();
  const int f = first;
  if (upper ? f < 0 : f == INT_MAX) return;                    // (the whole workgroup)
  double* x = X + (long)blockIdx.y * N * N;
  for (long e = (long)blockIdx.x * GI_T + threadIdx.x; e < (long)N * N; e += (long)gridDim.x * GI_T) {
    const int i = (int)(e / N), j = (int)(e - (long)i * N);
    if (upper ? (i < f && j >= i) : (i > f && j <= i)) x[e] = NAN;
  }
}

// ---- host side ----------------------------------------------------------------------------------------------------------------------
template <class T> int gi_alloc(nd4hip_handle* h, size_t n, T** out) {
  void* p = nullptr;
  ND4_TRY(nd4_ws_alloc(h, sizeof(T) * n, &p));
  *out = static_cast<T*>(p);
  return 0;
}
inline unsigned gi_tiles(int64_t n) { const int64_t t = (n + GI_T - 1) / GI_T; return (unsigned)(t < 1024 ? t : 1024); }

// the largest order of the LDS tier on this device: the tile, the vector and getri_lds's static LDS (perm, s_piv, s_flag) within the
// device's limit for a workgroup; an order that does not fit goes to the blocked tier
constexpr size_t GI_LDS_STATIC = sizeof(int) * (GI_LDS_N + 2) + 16;
int gi_lds_max_n(const nd4hip_handle* h, int* out) {
  int attr = 0;
  ND4_HIP(hipDeviceGetAttribute(&attr, hipDeviceAttributeMaxSharedMemoryPerBlock, h->device));
  const size_t lim = (size_t)(attr > 0 ? attr : 0);
  int n = GI_LDS_N;
  while (n > GI_REG_N && gi_lds_bytes(n) + GI_LDS_STATIC > lim) --n;
  *out = n;
  return 0;
}
int gi_attr(const void* fn, size_t lds) {
  // above 64 KiB the launch needs the function attribute (set every time: it is per device)
  if (lds > 64 * 1024) ND4_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  return 0;
}
// members per pass; ws: doubles of workspace per member
int64_t gi_chunk(int64_t batch, int64_t ws) {
  int64_t c = GI_CHUNK;
  if (ws > 0 && GI_WS_ELEMS / ws < c) c = GI_WS_ELEMS / ws;
  if (c < 1) c = 1;
  return batch < c ? batch : c;
}

int gi_trmm(nd4hip_handle* h, int64_t nb, const GiTrmm& g) {
  hipLaunchKernelGGL(trtri_trmm, dim3((unsigned)((g.M + GI_NB - 1) / GI_NB), (unsigned)nb), dim3(GI_T), 0, h->stream, g);
  ND4_HIP(hipGetLastError());
  return 0;
}

// blocked tier: dst [nb, N, N] = the inverse of the named triangle of src [nb, N, N], +0 in the other triangle; tmp [nb, N, 64]
int gi_trtri_blocked(nd4hip_handle* h, int64_t nb, int N, bool upper, const double* src, double* dst, double* tmp) {
  const int64_t nn = (int64_t)N * N, nt = (int64_t)N * GI_NB;
  const int nblk = (N + GI_NB - 1) / GI_NB;
  hipLaunchKernelGGL(trtri_diag, dim3((unsigned)nblk, (unsigned)nb), dim3(GI_T), 0, h->stream, src, (long)nn, dst, (long)nn, N, upper ? 1 : 0);
  ND4_HIP(hipGetLastError());
  for (int s = 1; s < nblk; ++s) {
    const int jb = upper ? s : nblk - 1 - s;                   // upper: left to right; lower: right to left
    const int j0 = jb * GI_NB, kb = N - j0 < GI_NB ? N - j0 : GI_NB, j1 = j0 + kb;
    const int r0 = upper ? 0 : j1, M = upper ? j0 : N - j1;    // the rows of the block column outside its diagonal block
    // tmp = T[rows, block] X_jj (the small factor), then X[rows, block] = -X[rows, rows] tmp
    ND4_TRY(nd4_gemm_member_order(h, false, false, M, kb, kb, 1.0, src + (int64_t)r0 * N + j0, N, nn, dst + (int64_t)j0 * N + j0, N, nn, 0.0, tmp, GI_NB, nt, nb));
    ND4_TRY(gi_trmm(h, nb, GiTrmm{dst + (int64_t)r0 * N + r0, N, (long)nn, tmp, GI_NB, (long)nt, dst + (int64_t)r0 * N + j0, N, (long)nn, M, kb, upper ? 1 : 0}));
  }
  return 0;
}

// X [nb, N, N] from A; flags [nb + 2] zero on entry (the last word: scratch of the column un-permutation)
int gi_inv_pass(nd4hip_handle* h, int64_t nb, int N, int tier, const double* A, double* X, int* flags) {
  if (tier == 0) {
    const dim3 grid((unsigned)((nb + 15) / 16)), block(GI_T);
    if (N <= 4)      hipLaunchKernelGGL(getri_reg<4>, grid, block, 0, h->stream, A, X, flags, N, (long)nb);
    else if (N <= 8) hipLaunchKernelGGL(getri_reg<8>, grid, block, 0, h->stream, A, X, flags, N, (long)nb);
    else             hipLaunchKernelGGL(getri_reg<16>, grid, block, 0, h->stream, A, X, flags, N, (long)nb);
    ND4_HIP(hipGetLastError());
    return 0;
  }
  if (tier == 1) {
    const size_t lds = gi_lds_bytes(N);
    ND4_TRY(gi_attr(reinterpret_cast<const void*>(&getri_lds), lds));
    hipLaunchKernelGGL(getri_lds, dim3((unsigned)nb), dim3(GI_T), lds, h->stream, A, X, flags, N);
    ND4_HIP(hipGetLastError());
    return 0;
  }
  const int64_t nn = (int64_t)N * N;
  const int nblk = (N + GI_NB - 1) / GI_NB;
  Nd4WsScope scope(h);
  double *LU = nullptr, *W = nullptr, *tmp = nullptr;
  int* P = nullptr;
  ND4_TRY(gi_alloc(h, (size_t)(nb * nn), &LU));
  ND4_TRY(gi_alloc(h, (size_t)(nb * nn), &W));
  ND4_TRY(gi_alloc(h, (size_t)(nb * N * GI_NB), &tmp));
  ND4_TRY(gi_alloc(h, (size_t)(nb * N), &P));
  ND4_TRY(nd4_getrf(h, nb, N, A, LU, P));
  hipLaunchKernelGGL(getri_flags, dim3((unsigned)nb), dim3(GI_T), 0, h->stream, LU, N, flags);
  ND4_HIP(hipGetLastError());
  ND4_TRY(gi_trtri_blocked(h, nb, N, true, LU, W, tmp));       // W = U^-1, zeros below
  for (int jb = nblk - 1; jb >= 0; --jb) {
    const int j0 = jb * GI_NB, kb = N - j0 < GI_NB ? N - j0 : GI_NB, j1 = j0 + kb;
    if (j1 < N) ND4_TRY(nd4_gemm_member_order(h, false, false, N, kb, N - j1, -1.0, W + j1, N, nn, LU + (int64_t)j1 * N + j0, N, nn, 1.0, W + j0, N, nn, nb));
    hipLaunchKernelGGL(getri_rsolve, dim3((unsigned)((N + GI_RS - 1) / GI_RS), (unsigned)nb), dim3(GI_T), 0, h->stream, W, LU, N, j0, kb);
    ND4_HIP(hipGetLastError());
  }
  ND4_TRY(nd4_permute_enqueue(h, 1, 1, nb, N, N, W, nn, P, N, X, flags + nb + 1));   // X[:, P[i]] = W[:, i]
  hipLaunchKernelGGL(getri_poison, dim3(gi_tiles(nn), (unsigned)nb), dim3(GI_T), 0, h->stream, X, (long)nn, flags);
  ND4_HIP(hipGetLastError());
  return 0;
}

int gi_tier(const nd4hip_handle* h, int N, bool reg_tier, int* tier) {
  int lds_n = 0;
  ND4_TRY(gi_lds_max_n(h, &lds_n));
  *tier = (reg_tier && N <= GI_REG_N) ? 0 : (N <= lds_n ? 1 : 2);
  return 0;
}

}  // namespace

// inv: X [batch, N, N] with A X = I. info (device, int32 [batch]) receives the members' flags and the call only enqueues; info = NULL: one
// flag word per pass is read back, the members' flags only when it is raised: ND4HIP_ERR_SINGULAR with the lowest flagged member (member0:
// the index of the first member in the caller's batch), also in *first_bad (may be NULL). Arguments already checked
int nd4_getri(nd4hip_handle* h, int64_t batch, int64_t N64, const double* A, double* X, int32_t* info, int64_t member0, int64_t* first_bad) {
  const int N = (int)N64;
  const int64_t nn = N64 * N64;
  int tier = 0;
  ND4_TRY(gi_tier(h, N, true, &tier));
  const int64_t chunk = gi_chunk(batch, tier == 2 ? 2 * nn + N64 * GI_NB + N64 : 0);
  Nd4WsScope scope(h);
  int* flags = nullptr;
  ND4_TRY(gi_alloc(h, (size_t)(chunk + 2), &flags));
  int* host = nullptr;
  if (!info) {
    void* hp = nullptr;
    ND4_TRY(nd4_pinned(h, sizeof(int) * (size_t)(chunk + 1), &hp));
    host = static_cast<int*>(hp);
  }
  for (int64_t b0 = 0; b0 < batch; b0 += chunk) {
    const int64_t nb = batch - b0 < chunk ? batch - b0 : chunk;
    ND4_HIP(hipMemsetAsync(flags, 0, sizeof(int) * (size_t)(nb + 2), h->stream));
    ND4_TRY(gi_inv_pass(h, nb, N, tier, A + b0 * nn, X + b0 * nn, flags));
    if (info) {
      ND4_HIP(hipMemcpyAsync(info + b0, flags + 1, sizeof(int) * (size_t)nb, hipMemcpyDeviceToDevice, h->stream));
      continue;
    }
    ND4_HIP(hipMemcpyAsync(host, flags, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    ND4_HIP(hipStreamSynchronize(h->stream));
    if (host[0] == 0) continue;
    ND4_HIP(hipMemcpyAsync(host, flags, sizeof(int) * (size_t)(nb + 1), hipMemcpyDeviceToHost, h->stream));
    ND4_HIP(hipStreamSynchronize(h->stream));
    int64_t b = 0;
    while (b < nb - 1 && host[1 + b] == 0) ++b;
    if (first_bad) *first_bad = member0 + b0 + b;
    nd4_set_error("inv(A): A is singular. (matrix %lld)", (long long)(member0 + b0 + b));
    return ND4HIP_ERR_SINGULAR;
  }
  return 0;
}

// tril_inv / triu_inv: X [batch, N, N] = the inverse of the named triangle of T, +0 in the other triangle. Enqueues only
int nd4_trtri(nd4hip_handle* h, bool upper, int64_t batch, int64_t N64, const double* T, double* X) {
  const int N = (int)N64;
  const int64_t nn = N64 * N64;
  int tier = 0;
  ND4_TRY(gi_tier(h, N, false, &tier));
  const int64_t chunk = gi_chunk(batch, tier == 2 ? N64 * GI_NB : 0);
  Nd4WsScope scope(h);
  double* tmp = nullptr;
  if (tier == 2) ND4_TRY(gi_alloc(h, (size_t)(chunk * N64 * GI_NB), &tmp));
  for (int64_t b0 = 0; b0 < batch; b0 += chunk) {
    const int64_t nb = batch - b0 < chunk ? batch - b0 : chunk;
    if (tier == 2) {
      ND4_TRY(gi_trtri_blocked(h, nb, N, upper, T + b0 * nn, X + b0 * nn, tmp));
      hipLaunchKernelGGL(trtri_poison, dim3(gi_tiles(nn), (unsigned)nb), dim3(GI_T), 0, h->stream, T + b0 * nn, X + b0 * nn, N, upper ? 1 : 0);
      ND4_HIP(hipGetLastError());
      continue;
    }
    const size_t lds = gi_lds_bytes(N);
    ND4_TRY(gi_attr(reinterpret_cast<const void*>(&trtri_lds), lds));
    hipLaunchKernelGGL(trtri_lds, dim3((unsigned)nb), dim3(GI_T), lds, h->stream, T + b0 * nn, X + b0 * nn, N, upper ? 1 : 0);
    ND4_HIP(hipGetLastError());
  }
  return 0;
}

// cholesky_inv: X [batch, N, N] = L^-T L^-1 from the lower triangle of L, both triangles with identical bits. Enqueues only
int nd4_potri(nd4hip_handle* h, int64_t batch, int64_t N64, const double* L, double* X) {
  const int N = (int)N64;
  const int64_t nn = N64 * N64;
  int tier = 0;
  ND4_TRY(gi_tier(h, N, false, &tier));
  const int64_t chunk = gi_chunk(batch, tier == 2 ? nn + N64 * GI_NB : 0);
  Nd4WsScope scope(h);
  double *W = nullptr, *tmp = nullptr;
  if (tier == 2) {
    ND4_TRY(gi_alloc(h, (size_t)(chunk * nn), &W));
    ND4_TRY(gi_alloc(h, (size_t)(chunk * N64 * GI_NB), &tmp));
  }
  for (int64_t b0 = 0; b0 < batch; b0 += chunk) {
    const int64_t nb = batch - b0 < chunk ? batch - b0 : chunk;
    double* x = X + b0 * nn;
    if (tier == 2) {
      ND4_TRY(gi_trtri_blocked(h, nb, N, false, L + b0 * nn, W, tmp));
      ND4_TRY(nd4_gemm_member_order(h, true, false, N, N, N, 1.0, W, N, nn, W, N, nn, 0.0, x, N, nn, nb));
      hipLaunchKernelGGL(getri_mirror, dim3(gi_tiles(nn), (unsigned)nb), dim3(GI_T), 0, h->stream, x, N);
      ND4_HIP(hipGetLastError());
      continue;
    }
    const size_t lds = gi_lds_bytes(N);
    ND4_TRY(gi_attr(reinterpret_cast<const void*>(&trtri_lds), lds));
    hipLaunchKernelGGL(trtri_lds, dim3((unsigned)nb), dim3(GI_T), lds, h->stream, L + b0 * nn, x, N, 2);
    ND4_HIP(hipGetLastError());
  }
  return 0;
}
