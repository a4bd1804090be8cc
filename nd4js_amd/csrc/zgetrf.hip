// General complex128 LU with partial pivoting and its solves on the device: zlu_decomp / zlu_solve / zsolve. The
// complex twin of lu.hip, LAPACK's zgetrf / zgetrs with the reference's lu_decomp conventions: (L U)[i, :] = A[P[i], :], L unit lower
// below the diagonal of LU, U on and above it. complex128 operands are interleaved (re, im) doubles, strides in complex elements.
//
// Pivot of column j: the first row i >= j with the largest |Re a_ij| + |Im a_ij| (izamax); a later row wins only by strict >, a NaN
// never wins unless it is the start row (zlu_key turns that rule into a total order, so a tree reduction gives the scalar scan's
// answer). l_ij = a_ij / a_jj is a true division (zlu_div: Smith's form). A pivot whose |Re| + |Im| is zero or not finite sets the
// member's flag to 1 + its column (LAPACK's info, the first such column), leaves the column unscaled and goes on.
//
// Register tier, N <= 16 (zgetrf_reg<NP>, NP = 8, 16 the padded order): one wave per member, four members per workgroup, lane i
//   holds row i (at most 16 complex: 32 doubles). The column loop is expanded at compile time (a fold over an integer sequence), so
//   every register index is static. Arg-max by DPP inside the row of 16 lanes, ties to the lowest lane; the pivot row is broadcast
//   by lane reads, the row swap is a select on two lanes. No LDS and no barrier. (At 32 rows the tier lost to the LDS tier:
//   DESIGN.md 4.26.)
// LDS tier, 16 < N <= 64 (zgetrf_small; zgetrs_small for every N <= 64): one workgroup of four waves per member, the tile in LDS at
//   pitch N | 1 in 16-byte elements, right-looking, four barriers per column.
// Both: one product form (zlu_nms), one order, the file is built without FMA contraction: the bits of tests/zlu_common.py.
// Blocked tier, 64 < N <= 2048, outer blocks of 16 columns (64 lost 1.2 - 1.6 x to it):
//   zgetrf_panel<R, IB>  one workgroup of 512 threads per member factorises the block's columns in inner panels of IB columns held in
//                    registers (thread t holds the rows j0 + t + 512 s, s < R): 16 columns up to 512 rows (R = 1), 8 columns above
//                    (R = 2, 4; 4 x 16 complex would be 256 VGPRs, the whole budget of a wave at 512 threads, and 2 x 16 spilled 92
//                    bytes per lane in the compiler's report), two barriers per column:
//                    arg-max by a wave reduction and one LDS round, then the pivot row and the start row change places through LDS.
//                    After an inner panel its interchanges, the unit lower solve and the rank-IB update are applied to the other
//                    columns of the outer block only.
//   zlu_laswp        the block's interchanges on the columns left and right of it, one thread per column.
//   zlu_u12          U12 = L11^-1 A12, L11 (unit lower) and 64 columns in LDS per workgroup.
//   zlu_update       A22 -= L21 U12 on v_mfma_f64_16x16x4_f64: macro tile 128 x 64 complex, four waves as 2 x 2, the accumulators
//                    are loaded from C and the four chains run with negated A fragments (Re -= Ar Br - Ai Bi, Im -= Ar Bi + Ai Br),
//                    so C is read once and written once. Staging and LDS images are zgemm.hip's (zgemm_stage.h).
//   solves           zlu_gather (X = Y[P]), zgetrs_diag (a diagonal block against 64 right-hand sides in LDS), zlu_update for the
//                    rows below (forward) or above (backward).
// No atomics on doubles, no synchronisation but __syncthreads(), wave shuffles and the kernel boundary.
// Flags: [0] the OR over the members of a pass, [1 + member] = 1 + the first column with an unusable pivot.
#include "nd4hip_internal.h"
#include "zgemm_stage.h"
#include "dpp.h"
#include <cfloat>
#include <climits>
#include <cmath>
#include <utility>

namespace {

typedef double2 cd;

constexpr int ZLU_MAXN = 2048;
constexpr int ZLU_REG_N = 16;                   // one member per wave in registers up to here
constexpr int ZLU_SMALL_N = 64;                 // one member per workgroup in LDS up to here
constexpr int ZLU_OB = 16;                      // outer block of the factorisation (measured against 64)
constexpr int ZLU_NB = 64;                      // block of the solves, columns or right-hand sides per workgroup
constexpr int ZLU_T = 256;                      // threads per workgroup (all kernels but the panel)
constexpr int ZLU_PT = 512;                     // threads of the panel kernel
constexpr int64_t ZLU_CHUNK = 32768;            // members per pass
constexpr int64_t ZLU_WS_ELEMS = 1ll << 26;     // zsolve: a pass's LU takes at most 1 GiB

__device__ __forceinline__ cd zz(double re, double im) { cd r; r.x = re; r.y = im; return r; }
// s - a b, the one order of the four real products
__device__ __forceinline__ cd zlu_nms(cd s, cd a, cd b) { return zz((s.x - a.x * b.x) + a.y * b.y, (s.y - a.x * b.y) - a.y * b.x); }
// x / d: true divisions; by the real part alone where the imaginary part is zero, else Smith's form
__device__ __forceinline__ cd zlu_div(cd x, cd d) {
  if (d.y == 0.0) return zz(x.x / d.x, x.y / d.x);
  if (fabs(d.x) >= fabs(d.y)) {
    const double r = d.y / d.x, den = d.x + d.y * r;
    return zz((x.x + x.y * r) / den, (x.y - x.x * r) / den);
  }
  const double r = d.x / d.y, den = d.x * r + d.y;
  return zz((x.x * r + x.y) / den, (x.y * r - x.x) / den);
}
__device__ __forceinline__ double zlu_mag(cd v) { return fabs(v.x) + fabs(v.y); }
// the arg-max key: a NaN in the start row beats everything that follows (nothing is > NaN in the scalar scan), elsewhere it never wins
__device__ __forceinline__ double zlu_key(cd v, bool start) {
  const double m = zlu_mag(v);
  return m != m ? (start ? INFINITY : -1.0) : m;
}
__device__ __forceinline__ bool zlu_better(double m, int i, double bm, int bi) { return m > bm || (m == bm && i < bi); }
__device__ __forceinline__ bool zlu_bad_pivot(cd p) { const double m = zlu_mag(p); return !(m > 0.0 && m <= DBL_MAX); }
__device__ __forceinline__ void zlu_wave_argmax(double& bm, int& bi) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const double om = __shfl_xor(bm, off);
    const int oi = __shfl_xor(bi, off);
    if (zlu_better(om, oi, bm, bi)) { bm = om; bi = oi; }
  }
}

inline int zlu_ld(int n) { return n | 1; }

// ---- substitutions on LDS tiles by all ZLU_T threads; each ends behind a barrier -----------------------------------------------------
// X [n][ldx], k columns: L X = Y in place, L unit lower (its diagonal is not read)
__device__ void zlu_fwd_lds(const cd* Ls, int ldl, cd* X, int ldx, int n, int k) {
  const int t = threadIdx.x;
  for (int i = 0; i + 1 < n; ++i) {
    const int m = n - i - 1;
    for (int e = t; e < m * k; e += ZLU_T) {
      const int r = i + 1 + e / k, c = e % k;
      X[r * ldx + c] = zlu_nms(X[r * ldx + c], Ls[r * ldl + i], X[i * ldx + c]);
    }
    __syncthreads();
  }
}
// U X = Y in place, U upper
__device__ void zlu_bwd_lds(const cd* Us, int ldu, cd* X, int ldx, int n, int k) {
  const int t = threadIdx.x;
  for (int i = n - 1; i >= 0; --i) {
    const cd d = Us[i * ldu + i];
    for (int c = t; c < k; c += ZLU_T) X[i * ldx + c] = zlu_div(X[i * ldx + c], d);
    __syncthreads();
    for (int e = t; e < i * k; e += ZLU_T) {
      const int r = e / k, c = e % k;
      X[r * ldx + c] = zlu_nms(X[r * ldx + c], Us[r * ldu + i], X[i * ldx + c]);
    }
    __syncthreads();
  }
}

// ---- register tier ----------------------------------------------------------------------------------------------------------------
// one step of the DPP arg-max: the better of a lane's pair and its partner's
#define ZLU_DPP_STEP(X)                                                    \
  do { const double om = nd4dpp::X(m); const int oi = nd4dpp::X(idx);      \
       if (zlu_better(om, oi, m, idx)) { m = om; idx = oi; } } while (0)

// column J of the member that this wave holds: ar / ai [c] = row `lane`, column c; orig: the row's index in A; flag: wave-uniform
template <int NP, int J>
__device__ __forceinline__ void zlu_reg_col(double (&ar)[NP], double (&ai)[NP], int& orig, int& flag, int lane, int N) {
  if (J >= N) return;                                          // (the whole wave)
  double m = -2.0;
  int idx = INT_MAX;
  if (lane >= J && lane < N) { m = zlu_key(zz(ar[J], ai[J]), lane == J); idx = lane; }
  ZLU_DPP_STEP(xor1); ZLU_DPP_STEP(xor2); ZLU_DPP_STEP(xor4); ZLU_DPP_STEP(xor8);   // every lane: the best of its row of 16 lanes
  const int piv = __builtin_amdgcn_readfirstlane(__builtin_amdgcn_readlane(idx, 0));   // (N <= 16: the rows are one row of lanes)
  if (piv != J) {                                              // rows J and piv change places: a select on two lanes
#pragma unroll
    for (int c = 0; c < NP; ++c) {
      const double pr = nd4dpp::rl_d(ar[c], piv), pi = nd4dpp::rl_d(ai[c], piv), dr = nd4dpp::rl_d(ar[c], J), di = nd4dpp::rl_d(ai[c], J);
      if (lane == piv) { ar[c] = dr; ai[c] = di; }
      if (lane == J) { ar[c] = pr; ai[c] = pi; }
    }
    const int po = __builtin_amdgcn_readlane(orig, piv), jo = __builtin_amdgcn_readlane(orig, J);
    if (lane == piv) orig = jo;
    if (lane == J) orig = po;
  }
  const cd p = zz(nd4dpp::rl_d(ar[J], J), nd4dpp::rl_d(ai[J], J));
  const bool bad = zlu_bad_pivot(p);
  if (bad && !flag) flag = J + 1;
  const bool below = lane > J && lane < N;
  cd l = zz(ar[J], ai[J]);
  if (below && !bad) { l = zlu_div(l, p); ar[J] = l.x; ai[J] = l.y; }
#pragma unroll
  for (int c = J + 1; c < NP; ++c) {
    const cd u = zz(nd4dpp::rl_d(ar[c], J), nd4dpp::rl_d(ai[c], J));
    if (below) { const cd v = zlu_nms(zz(ar[c], ai[c]), l, u); ar[c] = v.x; ai[c] = v.y; }
  }
}
template <int NP, int... J>
__device__ __forceinline__ void zlu_reg_cols(std::integer_sequence<int, J...>, double (&ar)[NP], double (&ai)[NP], int& orig, int& flag, int lane, int N) {
  (zlu_reg_col<NP, J>(ar, ai, orig, flag, lane, N), ...);
}

// N <= NP; grid (ceil(members / 4)), 256 threads: wave w of workgroup b holds member 4 b + w
template <int NP>
__global__ __launch_bounds__(ZLU_T) void zgetrf_reg(const cd* __restrict__ A, cd* __restrict__ LU, int* __restrict__ P, int* __restrict__ flags, int N,
                                                    long members) {
  const int lane = threadIdx.x & 63;
  const long mat = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (mat >= members) return;                                  // (the whole wave)
  const cd* a = A + mat * N * N + (long)lane * N;
  double ar[NP], ai[NP];
#pragma unroll
  for (int c = 0; c < NP; ++c) {
    cd v = zz(0.0, 0.0);
    if (lane < N && c < N) v = a[c];
    ar[c] = v.x; ai[c] = v.y;
  }
  int orig = lane, flag = 0;
  zlu_reg_cols<NP>(std::make_integer_sequence<int, NP>{}, ar, ai, orig, flag, lane, N);
  if (lane < N) {
    cd* o = LU + mat * N * N + (long)lane * N;
#pragma unroll
    for (int c = 0; c < NP; ++c)
      if (c < N) o[c] = zz(ar[c], ai[c]);
    P[mat * N + lane] = orig;
  }
  if (lane == 0 && flag) { flags[1 + mat] = flag; atomicOr(&flags[0], 1); }
}

// ---- LDS tier -------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(ZLU_T) void zgetrf_small(const cd* __restrict__ A, cd* __restrict__ LU, int* __restrict__ P, int* __restrict__ flags, int N) {
  extern __shared__ __attribute__((aligned(16))) char zlu_smem[];
  __shared__ int perm[ZLU_SMALL_N];
  __shared__ int s_piv;
  cd* S = reinterpret_cast<cd*>(zlu_smem);
  const int ld = N | 1, t = threadIdx.x;
  const long mat = blockIdx.x;
  for (int e = t; e < N * N; e += ZLU_T) { const int i = e / N, j = e - i * N; S[i * ld + j] = A[mat * N * N + e]; }
  if (t < N) perm[t] = t;
  __syncthreads();
  int flag = 0;                                                // (thread 0)
  for (int j = 0; j < N; ++j) {
    if (t < 64) {                                              // wave 0: lane l looks at row j + l
      const int row = j + t;
      double bm = -2.0;
      int bi = INT_MAX;
      if (row < N) { bm = zlu_key(S[row * ld + j], t == 0); bi = row; }
      zlu_wave_argmax(bm, bi);
      if (t == 0) s_piv = bi;
    }
    __syncthreads();
    const int piv = s_piv;
    if (piv != j) {
      if (t < N) { const cd a = S[j * ld + t]; S[j * ld + t] = S[piv * ld + t]; S[piv * ld + t] = a; }
      if (t == ZLU_T - 1) { const int a = perm[j]; perm[j] = perm[piv]; perm[piv] = a; }
    }
    __syncthreads();
    const cd p = S[j * ld + j];
    const bool bad = zlu_bad_pivot(p);
    if (t == 0 && bad && !flag) flag = j + 1;
    if (!bad)
      for (int i = j + 1 + t; i < N; i += ZLU_T) S[i * ld + j] = zlu_div(S[i * ld + j], p);
    __syncthreads();
    const int m = N - j - 1;
    for (int e = t; e < m * m; e += ZLU_T) {
      const int i = j + 1 + e / m, c = j + 1 + e % m;
      S[i * ld + c] = zlu_nms(S[i * ld + c], S[i * ld + j], S[j * ld + c]);
    }
    __syncthreads();
  }
  for (int e = t; e < N * N; e += ZLU_T) { const int i = e / N, j = e - i * N; LU[mat * N * N + e] = S[i * ld + j]; }
  if (t < N) P[mat * N + t] = perm[t];
  if (t == 0 && flag) { flags[1 + mat] = flag; atomicOr(&flags[0], 1); }
}

// a row index of P that is not one: the right-hand side loads as NaN instead of reading out of bounds
__device__ __forceinline__ cd zlu_row_of(const cd* __restrict__ Y, int p, int N, long K, long c) {
  return (unsigned)p < (unsigned)N ? Y[(long)p * K + c] : zz(NAN, NAN);
}

// X [members][N][K], columns blockIdx.y * 64 ..: the rows of Y gathered through P, L X = Y[P], U X = that
__global__ __launch_bounds__(ZLU_T) void zgetrs_small(const cd* __restrict__ LU, long sLU, const int* __restrict__ P, long sP, const cd* __restrict__ Y,
                                                      long sY, cd* __restrict__ X, int N, int K) {
  extern __shared__ __attribute__((aligned(16))) char zlu_smem[];
  const int ld = N | 1, ldx = ZLU_NB + 1, t = threadIdx.x;
  const long mat = blockIdx.x;
  const int c0 = blockIdx.y * ZLU_NB, k = K - c0 < ZLU_NB ? K - c0 : ZLU_NB;
  cd* S = reinterpret_cast<cd*>(zlu_smem);
  cd* Xs = S + N * ld;
  const cd* g = LU + mat * sLU;
  const int* p = P + mat * sP;
  const cd* y = Y + mat * sY;
  for (int e = t; e < N * N; e += ZLU_T) { const int i = e / N, j = e - i * N; S[i * ld + j] = g[e]; }
  for (int e = t; e < N * k; e += ZLU_T) { const int i = e / k, j = e - i * k; Xs[i * ldx + j] = zlu_row_of(y, p[i], N, K, c0 + j); }
  __syncthreads();
  zlu_fwd_lds(S, ld, Xs, ldx, N, k);
  zlu_bwd_lds(S, ld, Xs, ldx, N, k);
  for (int e = t; e < N * k; e += ZLU_T) { const int i = e / k, j = e - i * k; X[mat * N * K + (long)i * K + c0 + j] = Xs[i * ldx + j]; }
}

// ---- blocked tier ---------------------------------------------------------------------------------------------------------------
// The columns j0 .. j0 + nb - 1 (nb <= ZLU_OB) and rows j0 .. N - 1 of every member of LU, in place. P [members][N]: the rows' indices in A
// (identity before the first block). ipiv [members][N]: row j changed places with row ipiv[j], for zlu_laswp. grid (members)
template <int R, int IB>
__global__ __launch_bounds__(ZLU_PT) void zgetrf_panel(cd* __restrict__ LU, int* __restrict__ P, int* __restrict__ ipiv, int* __restrict__ flags,
                                                       int N, int j0, int nb) {
  __shared__ cd bufP[IB], bufD[IB], sL[IB][IB + 1], Us[IB][ZLU_NB + 1];
  __shared__ double redm[ZLU_PT / 64];
  __shared__ int redi[ZLU_PT / 64], spiv[ZLU_OB], bufPi, bufDi;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  cd* M = LU + (long)blockIdx.x * N * N;
  int* Pm = P + (long)blockIdx.x * N;
  int orig[R];
#pragma unroll
  for (int s = 0; s < R; ++s) {
    const int row = j0 + t + ZLU_PT * s;
    orig[s] = row < N ? (j0 == 0 ? row : Pm[row]) : -1;
  }
  int flag = 0;                                                // (thread 0)
  for (int c0 = j0; c0 < j0 + nb; c0 += IB) {
    const int w = j0 + nb - c0 < IB ? j0 + nb - c0 : IB;
    cd a[R][IB];
#pragma unroll
    for (int s = 0; s < R; ++s) {
      const int row = j0 + t + ZLU_PT * s;
#pragma unroll
      for (int c = 0; c < IB; ++c) a[s][c] = (row >= c0 && row < N && c < w) ? M[(long)row * N + c0 + c] : zz(0.0, 0.0);
    }
#pragma unroll
    for (int jj = 0; jj < IB; ++jj) {
      if (jj < w) {                                            // (the whole workgroup)
        const int gc = c0 + jj;
        double bm = -2.0;
        int bi = INT_MAX;
#pragma unroll
        for (int s = 0; s < R; ++s) {
          const int row = j0 + t + ZLU_PT * s;
          if (row >= gc && row < N) {
            const double m = zlu_key(a[s][jj], row == gc);
            if (zlu_better(m, row, bm, bi)) { bm = m; bi = row; }
          }
        }
        zlu_wave_argmax(bm, bi);
        if (lane == 0) { redm[wave] = bm; redi[wave] = bi; }
        __syncthreads();
        bm = redm[0]; bi = redi[0];
#pragma unroll
        for (int q = 1; q < ZLU_PT / 64; ++q)
          if (zlu_better(redm[q], redi[q], bm, bi)) { bm = redm[q]; bi = redi[q]; }
        const int piv = bi;
        // the pivot row and the start row change places through LDS; everyone reads the pivot row
#pragma unroll
        for (int s = 0; s < R; ++s) {
          const int row = j0 + t + ZLU_PT * s;
          if (row == piv) {
#pragma unroll
            for (int c = 0; c < IB; ++c) bufP[c] = a[s][c];
            bufPi = orig[s];
          }
          if (row == gc) {
#pragma unroll
            for (int c = 0; c < IB; ++c) bufD[c] = a[s][c];
            bufDi = orig[s];
          }
        }
        __syncthreads();
#pragma unroll
        for (int s = 0; s < R; ++s) {
          const int row = j0 + t + ZLU_PT * s;
          if (row == piv) {
#pragma unroll
            for (int c = 0; c < IB; ++c) a[s][c] = bufD[c];
            orig[s] = bufDi;
          }
          if (row == gc) {
#pragma unroll
            for (int c = 0; c < IB; ++c) a[s][c] = bufP[c];
            orig[s] = bufPi;
          }
        }
        cd u[IB];
#pragma unroll
        for (int c = 0; c < IB; ++c) u[c] = bufP[c];
        const cd p = u[jj];
        const bool bad = zlu_bad_pivot(p);
        if (t == 0) { spiv[gc - j0] = piv; if (bad && !flag) flag = gc + 1; }
#pragma unroll
        for (int s = 0; s < R; ++s) {
          const int row = j0 + t + ZLU_PT * s;
          if (row > gc && row < N) {
            const cd l = bad ? a[s][jj] : zlu_div(a[s][jj], p);
            a[s][jj] = l;
#pragma unroll
            for (int c = jj + 1; c < IB; ++c) a[s][c] = zlu_nms(a[s][c], l, u[c]);
          }
        }
      }
    }
    // the finished inner panel goes back; its top w rows (L11 below their diagonal) also to LDS
#pragma unroll
    for (int s = 0; s < R; ++s) {
      const int row = j0 + t + ZLU_PT * s;
      if (row >= c0 && row < N) {
#pragma unroll
        for (int c = 0; c < IB; ++c)
          if (c < w) M[(long)row * N + c0 + c] = a[s][c];
        if (row < c0 + w) {
#pragma unroll
          for (int c = 0; c < IB; ++c) sL[row - c0][c] = a[s][c];
        }
      }
    }
    __syncthreads();
    // the other columns of the outer block, one thread each: the interchanges; right of the panel also U = L11^-1 (that column)
    if (t < nb) {
      const int col = j0 + t;
      if (col < c0 || col >= c0 + w) {
        for (int jj = 0; jj < w; ++jj) {
          const int r1 = c0 + jj, r2 = spiv[r1 - j0];
          if (r1 != r2) { const cd x = M[(long)r1 * N + col]; M[(long)r1 * N + col] = M[(long)r2 * N + col]; M[(long)r2 * N + col] = x; }
        }
        if (col >= c0 + w) {                                   // (w = IB here: only the last inner panel is narrower)
          cd x[IB];
#pragma unroll
          for (int k = 0; k < IB; ++k) x[k] = M[(long)(c0 + k) * N + col];
#pragma unroll
          for (int k = 0; k < IB; ++k)
#pragma unroll
            for (int i = k + 1; i < IB; ++i) x[i] = zlu_nms(x[i], sL[i][k], x[k]);
#pragma unroll
          for (int k = 0; k < IB; ++k) { M[(long)(c0 + k) * N + col] = x[k]; Us[k][t] = x[k]; }
        }
      }
    }
    __syncthreads();
    // rank-IB update of the block's columns right of the panel, every thread on its own rows (l_ik is still in registers)
    const int right = j0 + nb - (c0 + w);
    if (right > 0) {
#pragma unroll
      for (int s = 0; s < R; ++s) {
        const int row = j0 + t + ZLU_PT * s;
        if (row >= c0 + w && row < N)
          for (int cc = 0; cc < right; ++cc) {
            const int col = c0 + w + cc;
            cd v = M[(long)row * N + col];
#pragma unroll
            for (int k = 0; k < IB; ++k) v = zlu_nms(v, a[s][k], Us[k][col - j0]);
            M[(long)row * N + col] = v;
          }
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int s = 0; s < R; ++s) {
    const int row = j0 + t + ZLU_PT * s;
    if (row < N) Pm[row] = orig[s];
  }
  if (t < nb) ipiv[(long)blockIdx.x * N + j0 + t] = spiv[t];
  if (t == 0 && flag && flags[1 + blockIdx.x] == 0) { flags[1 + blockIdx.x] = flag; atomicOr(&flags[0], 1); }
}

// the interchanges of the block j0 .. j0 + nb - 1 on the columns outside it, one thread per column; grid (tiles of 256 columns, members)
__global__ __launch_bounds__(ZLU_T) void zlu_laswp(cd* __restrict__ LU, const int* __restrict__ ipiv, int N, int j0, int nb) {
  const int e = blockIdx.x * ZLU_T + threadIdx.x;
  const int col = e < j0 ? e : e + nb;
  if (col >= N) return;
  cd* M = LU + (long)blockIdx.y * N * N;
  const int* ip = ipiv + (long)blockIdx.y * N;
  for (int r1 = j0; r1 < j0 + nb; ++r1) {
    const int r2 = ip[r1];
    if (r1 != r2) { const cd x = M[(long)r1 * N + col]; M[(long)r1 * N + col] = M[(long)r2 * N + col]; M[(long)r2 * N + col] = x; }
  }
}

// U12 = L11^-1 A12: rows j0 .. j0 + nb - 1, columns j0 + nb + 64 blockIdx.x ..; grid (column tiles, members)
__global__ __launch_bounds__(ZLU_T) void zlu_u12(cd* __restrict__ LU, int N, int j0, int nb) {
  extern __shared__ __attribute__((aligned(16))) char zlu_smem[];
  const int ld = ZLU_NB + 1, t = threadIdx.x;
  cd* Ld = reinterpret_cast<cd*>(zlu_smem);
  cd* Xs = Ld + nb * ld;
  cd* M = LU + (long)blockIdx.y * N * N;
  const int c0 = j0 + nb + blockIdx.x * ZLU_NB, k = N - c0 < ZLU_NB ? N - c0 : ZLU_NB;
  for (int e = t; e < nb * nb; e += ZLU_T) { const int i = e / nb, j = e - i * nb; Ld[i * ld + j] = M[(long)(j0 + i) * N + j0 + j]; }
  for (int e = t; e < nb * k; e += ZLU_T) { const int i = e / k, j = e - i * k; Xs[i * ld + j] = M[(long)(j0 + i) * N + c0 + j]; }
  __syncthreads();
  zlu_fwd_lds(Ld, ld, Xs, ld, nb, k);
  for (int e = t; e < nb * k; e += ZLU_T) { const int i = e / k, j = e - i * k; M[(long)(j0 + i) * N + c0 + j] = Xs[i * ld + j]; }
}

// C [M][N] (row pitch ldc) -= A [M][K] (lda) B [K][N] (ldb) on the fp64 MFMA; the three do not overlap in what is read and written,
// every base is 16-byte aligned. grid (column tiles of 64, row tiles of 128, members); strides 0: one operand for all
// (struct ZluUpd: nd4hip_internal.h)
__global__ __launch_bounds__(256, 2) void zlu_update(ZluUpd g) {
  __shared__ __attribute__((aligned(16))) double lds[2 * ZBUF];   // [buf][A | B]
  const int m0 = blockIdx.y * ZBM, n0 = blockIdx.x * ZBN;
  const long bz = blockIdx.z;
  const double* __restrict__ A = g.A + 2 * bz * g.sA;
  const double* __restrict__ B = g.B + 2 * bz * g.sB;
  double* __restrict__ C = g.C + 2 * bz * g.sC;
  const int K = g.K;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int wm = (wave >> 1) * 64, wn = (wave & 1) * 32;
  const int fx = lane & 15, fk = lane >> 4;

  // the accumulators start from C: lane holds C[row = (lane >> 4) + 4 r][col = lane & 15] of each 16 x 16 tile
  d4 re[4][2], im[4][2];
#pragma unroll
  for (int i = 0; i < 4; i++)
#pragma unroll
    for (int j = 0; j < 2; j++) {
      const int col = n0 + wn + j * 16 + fx;
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const int row = m0 + wm + i * 16 + fk + 4 * r;
        d2 v = {0.0, 0.0};
        if (row < g.M && col < g.N) v = *reinterpret_cast<const d2*>(C + 2 * ((long)row * g.ldc + col));
        re[i][j][r] = v.x; im[i][j][r] = v.y;
      }
    }

  d2 ra[4], rb[2];
  auto gload = [&](int k0) {
    zload_a<true, false>(ra, A, g.lda, m0, g.M, k0, K, t);
    zload_b<true, true, false>(rb, B, g.ldb, n0, g.N, k0, K, t);
  };
  auto sstore = [&](int buf) {
    double* sa = lds + buf * ZBUF;
    zstore_a(sa, ra, t);
    zstore_b<true>(sa + ZTA, rb, t);
  };

  const int nk = (K + ZBK - 1) / ZBK;
  gload(0);
  sstore(0);
  __syncthreads();
  for (int kt = 0; kt < nk; kt++) {
    const int cur = kt & 1;
    if (kt + 1 < nk) gload((kt + 1) * ZBK);        // in flight during the MFMAs below
    const double* sa = lds + cur * ZBUF;
    const double* sb = sa + ZTA;
#pragma unroll
    for (int kk = 0; kk < ZBK / 4; kk++) {
      double ai[4], nar[4], nai[4], br[2], bi[2];
#pragma unroll
      for (int i = 0; i < 4; i++) {
        const double* p = sa + (wm + i * 16 + fx) * ZLDA + kk * 4 + fk;
        nar[i] = -p[0]; ai[i] = p[ZBK]; nai[i] = -ai[i];
      }
#pragma unroll
      for (int j = 0; j < 2; j++) {
        const double* p = sb + (kk * 4 + fk) * ZLDB + wn + j * 16 + fx;
        br[j] = p[0]; bi[j] = p[ZBN];
      }
      if (kk == ZBK / 4 - 1 && kt + 1 < nk) {
        sstore(cur ^ 1);                             // the next tile into the other buffer before the last MFMAs of this step
        __builtin_amdgcn_sched_barrier(0);
      }
      __builtin_amdgcn_s_setprio(1);
      // Re += (-Ar) Br + Ai Bi, Im += (-Ar) Bi + (-Ai) Br; between two MFMAs on one accumulator lie 15 others
#pragma unroll
      for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 2; j++) {
          re[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(nar[i], br[j], re[i][j], 0, 0, 0);
          im[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(nar[i], bi[j], im[i][j], 0, 0, 0);
        }
#pragma unroll
      for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 2; j++) {
          re[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(ai[i], bi[j], re[i][j], 0, 0, 0);
          im[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(nai[i], br[j], im[i][j], 0, 0, 0);
        }
      __builtin_amdgcn_s_setprio(0);
    }
    __syncthreads();
  }

#pragma unroll
  for (int i = 0; i < 4; i++)
#pragma unroll
    for (int j = 0; j < 2; j++) {
      const int col = n0 + wn + j * 16 + fx;
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const int row = m0 + wm + i * 16 + fk + 4 * r;
        if (row < g.M && col < g.N) *reinterpret_cast<d2*>(C + 2 * ((long)row * g.ldc + col)) = d2{re[i][j][r], im[i][j][r]};
      }
    }
}

// X [members][N][K] = the rows of Y gathered through P; grid (tiles of 256 over N K, members)
__global__ __launch_bounds__(ZLU_T) void zlu_gather(const cd* __restrict__ Y, long sY, const int* __restrict__ P, long sP, cd* __restrict__ X, int N, int K) {
  const long e = (long)blockIdx.x * ZLU_T + threadIdx.x;
  if (e >= (long)N * K) return;
  const long mat = blockIdx.y;
  const int i = (int)(e / K);
  X[mat * N * K + e] = zlu_row_of(Y + mat * sY, P[mat * sP + i], N, K, e - (long)i * K);
}

// rows j0 .. j0 + nb - 1 of X [members][N][K] against the diagonal block of LU: its unit lower part, or (upper) its upper part;
// grid (members, column tiles)
__global__ __launch_bounds__(ZLU_T) void zgetrs_diag(const cd* __restrict__ LU, long sLU, cd* __restrict__ X, int N, int K, int j0, int nb, int upper) {
  extern __shared__ __attribute__((aligned(16))) char zlu_smem[];
  const int ld = ZLU_NB + 1, t = threadIdx.x;
  cd* Ld = reinterpret_cast<cd*>(zlu_smem);
  cd* Xs = Ld + ZLU_NB * ld;
  const long mat = blockIdx.x;
  const int c0 = blockIdx.y * ZLU_NB, k = K - c0 < ZLU_NB ? K - c0 : ZLU_NB;
  const cd* g = LU + mat * sLU + (long)j0 * N + j0;
  cd* x = X + mat * N * K + (long)j0 * K + c0;
  for (int e = t; e < nb * nb; e += ZLU_T) { const int i = e / nb, j = e - i * nb; Ld[i * ld + j] = g[(long)i * N + j]; }
  for (int e = t; e < nb * k; e += ZLU_T) { const int i = e / k, j = e - i * k; Xs[i * ld + j] = x[(long)i * K + j]; }
  __syncthreads();
  if (upper) zlu_bwd_lds(Ld, ld, Xs, ld, nb, k);
  else zlu_fwd_lds(Ld, ld, Xs, ld, nb, k);
  for (int e = t; e < nb * k; e += ZLU_T) { const int i = e / k, j = e - i * k; x[(long)i * K + j] = Xs[i * ld + j]; }
}

// ---- host side ------------------------------------------------------------------------------------------------------------------
inline const cd* ccd(const double* p) { return reinterpret_cast<const cd*>(p); }
inline cd* mcd(double* p) { return reinterpret_cast<cd*>(p); }

int zlu_attr(const void* fn, size_t lds) {
  // above 64 KiB the launch needs the function attribute (set every time: it is per device)
  if (lds > 64 * 1024) ND4_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  return 0;
}
inline size_t zlu_tile_bytes(int n) { return sizeof(cd) * (size_t)n * zlu_ld(n); }
constexpr size_t ZLU_BLOCK_LDS = sizeof(cd) * 2 * ZLU_NB * (ZLU_NB + 1);   // the solves: a diagonal block and 64 right-hand sides
inline size_t zlu_u12_lds(int nb) { return sizeof(cd) * 2 * (size_t)nb * (ZLU_NB + 1); }   // L11 (nb rows) and nb rows of 64 columns: 33 280 B

template <class T> int zlu_alloc(nd4hip_handle* h, size_t n, T** out) {
  void* p = nullptr;
  ND4_TRY(nd4_ws_alloc(h, sizeof(T) * n, &p));
  *out = static_cast<T*>(p);
  return 0;
}

// LU, P [nb members] from A; flags [1 + nb] zero on entry; ipiv [nb][N] scratch of the blocked tier
int zlu_factor(nd4hip_handle* h, int64_t nb, int N, const cd* A, cd* LU, int* P, int* flags, int* ipiv) {
  if (N <= ZLU_REG_N) {
    const dim3 grid((unsigned)((nb + 3) / 4)), block(ZLU_T);
    if (N <= 8) hipLaunchKernelGGL(zgetrf_reg<8>, grid, block, 0, h->stream, A, LU, P, flags, N, (long)nb);
    else        hipLaunchKernelGGL(zgetrf_reg<16>, grid, block, 0, h->stream, A, LU, P, flags, N, (long)nb);
    ND4_HIP(hipGetLastError());
    return 0;
  }
  if (N <= ZLU_SMALL_N) {
    const size_t lds = zlu_tile_bytes(N);
    ND4_TRY(zlu_attr(reinterpret_cast<const void*>(&zgetrf_small), lds));
    hipLaunchKernelGGL(zgetrf_small, dim3((unsigned)nb), dim3(ZLU_T), lds, h->stream, A, LU, P, flags, N);
    ND4_HIP(hipGetLastError());
    return 0;
  }
  const int64_t nn = (int64_t)N * N;
  ND4_HIP(hipMemcpyAsync(LU, A, sizeof(cd) * (size_t)(nb * nn), hipMemcpyDeviceToDevice, h->stream));
  for (int j0 = 0; j0 < N; j0 += ZLU_OB) {
    const int kb = N - j0 < ZLU_OB ? N - j0 : ZLU_OB, j1 = j0 + kb, rest = N - j1, rows = N - j0;
    const dim3 grid((unsigned)nb), block(ZLU_PT);
    if (rows <= ZLU_PT)          hipLaunchKernelGGL((zgetrf_panel<1, 16>), grid, block, 0, h->stream, LU, P, ipiv, flags, N, j0, kb);
    else if (rows <= 2 * ZLU_PT) hipLaunchKernelGGL((zgetrf_panel<2, 8>), grid, block, 0, h->stream, LU, P, ipiv, flags, N, j0, kb);
    else                         hipLaunchKernelGGL((zgetrf_panel<4, 8>), grid, block, 0, h->stream, LU, P, ipiv, flags, N, j0, kb);
    ND4_HIP(hipGetLastError());
    hipLaunchKernelGGL(zlu_laswp, dim3((unsigned)((N - kb + ZLU_T - 1) / ZLU_T), (unsigned)nb), dim3(ZLU_T), 0, h->stream, LU, ipiv, N, j0, kb);
    ND4_HIP(hipGetLastError());
    if (rest == 0) break;
    hipLaunchKernelGGL(zlu_u12, dim3((unsigned)((rest + ZLU_NB - 1) / ZLU_NB), (unsigned)nb), dim3(ZLU_T), zlu_u12_lds(kb), h->stream, LU, N, j0, kb);
    ND4_HIP(hipGetLastError());
    double* m = reinterpret_cast<double*>(LU);
    const ZluUpd u{m + 2 * ((int64_t)j1 * N + j0), N, nn, m + 2 * ((int64_t)j0 * N + j1), N, nn, m + 2 * ((int64_t)j1 * N + j1), N, nn, rest, rest, kb};
    ND4_TRY(zlu_update_launch(h, nb, u));
  }
  return 0;
}

// X [nb, N, K] from LU (stride sLU), P (sP), Y (sY); 0 strides: one for all
int zlu_solve(nd4hip_handle* h, int64_t nb, int N, int64_t K64, const cd* LU, int64_t sLU, const int* P, int64_t sP, const cd* Y, int64_t sY, cd* X) {
  const int64_t tiles64 = (K64 + ZLU_NB - 1) / ZLU_NB;
  ND4_CHECK_ARG(K64 < (1ll << 30) && tiles64 <= 65535, "nd4hip_zgetrs_batched: K exceeds 4 194 240 right-hand sides");
  const int K = (int)K64;
  const unsigned tiles = (unsigned)tiles64;
  if (N <= ZLU_SMALL_N) {
    const size_t lds = zlu_tile_bytes(N) + sizeof(cd) * (size_t)N * (ZLU_NB + 1);
    ND4_TRY(zlu_attr(reinterpret_cast<const void*>(&zgetrs_small), lds));
    hipLaunchKernelGGL(zgetrs_small, dim3((unsigned)nb, tiles), dim3(ZLU_T), lds, h->stream, LU, (long)sLU, P, (long)sP, Y, (long)sY, X, N, K);
    ND4_HIP(hipGetLastError());
    return 0;
  }
  const int64_t nk = (int64_t)N * K;
  hipLaunchKernelGGL(zlu_gather, dim3((unsigned)((nk + ZLU_T - 1) / ZLU_T), (unsigned)nb), dim3(ZLU_T), 0, h->stream, Y, (long)sY, P, (long)sP, X, N, K);
  ND4_HIP(hipGetLastError());
  ND4_TRY(zlu_attr(reinterpret_cast<const void*>(&zgetrs_diag), ZLU_BLOCK_LDS));
  const double* lu = reinterpret_cast<const double*>(LU);
  double* x = reinterpret_cast<double*>(X);
  const int nblocks = (N + ZLU_NB - 1) / ZLU_NB;
  for (int s = 0; s < nblocks; ++s) {                          // L (unit) X = Y[P]
    const int j0 = s * ZLU_NB, kb = N - j0 < ZLU_NB ? N - j0 : ZLU_NB, j1 = j0 + kb, rest = N - j1;
    hipLaunchKernelGGL(zgetrs_diag, dim3((unsigned)nb, tiles), dim3(ZLU_T), ZLU_BLOCK_LDS, h->stream, LU, (long)sLU, X, N, K, j0, kb, 0);
    ND4_HIP(hipGetLastError());
    if (rest == 0) break;
    const ZluUpd u{lu + 2 * ((int64_t)j1 * N + j0), N, sLU, x + 2 * (int64_t)j0 * K, K, nk, x + 2 * (int64_t)j1 * K, K, nk, rest, K, kb};
    ND4_TRY(zlu_update_launch(h, nb, u));
  }
  return nd4_zgetrs_upper(h, nb, N, K, lu, sLU, x);            // U X = that
}

inline bool zlu_al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

int zlu_update_launch(nd4hip_handle* h, int64_t nb, const ZluUpd& u) {
  const dim3 grid((unsigned)((u.N + ZBN - 1) / ZBN), (unsigned)((u.M + ZBM - 1) / ZBM), (unsigned)nb);
  hipLaunchKernelGGL(zlu_update, grid, dim3(256), 0, h->stream, u);
  ND4_HIP(hipGetLastError());
  return 0;
}

// the upper sweep of the blocked solve, U X = X in place: X [nb, N, K] dense, U the upper triangle of LU (row pitch N, members sLU
// apart, 0: one for all), blocks of 64 from the last: zgetrs_diag, then zlu_update on the rows above. K <= 4 194 240. Enqueues only
int nd4_zgetrs_upper(nd4hip_handle* h, int64_t nb, int N, int K, const double* lu, int64_t sLU, double* x) {
  const unsigned tiles = (unsigned)((K + ZLU_NB - 1) / ZLU_NB);
  const int64_t nk = (int64_t)N * K;
  const int nblocks = (N + ZLU_NB - 1) / ZLU_NB;
  ND4_TRY(zlu_attr(reinterpret_cast<const void*>(&zgetrs_diag), ZLU_BLOCK_LDS));
  for (int s = nblocks - 1; s >= 0; --s) {
    const int j0 = s * ZLU_NB, kb = N - j0 < ZLU_NB ? N - j0 : ZLU_NB;
    hipLaunchKernelGGL(zgetrs_diag, dim3((unsigned)nb, tiles), dim3(ZLU_T), ZLU_BLOCK_LDS, h->stream, ccd(lu), (long)sLU, mcd(x), N, K, j0, kb, 1);
    ND4_HIP(hipGetLastError());
    if (j0 == 0) break;
    const ZluUpd u{lu + 2 * (int64_t)j0, N, sLU, x + 2 * (int64_t)j0 * K, K, nk, x, K, nk, j0, K, kb};
    ND4_TRY(zlu_update_launch(h, nb, u));
  }
  return 0;
}

// ---- the host-side arithmetic of the tiers (tools/zlu_host_check.hip) ----
int nd4_zgetrf_tier(int64_t N) { return N <= ZLU_REG_N ? 0 : N <= ZLU_SMALL_N ? 1 : 2; }
// the largest dynamic LDS request of any kernel that runs at this N
size_t nd4_zgetrf_lds(int64_t N) {
  if (nd4_zgetrf_tier(N) <= 1) return zlu_tile_bytes((int)N) + sizeof(cd) * (size_t)N * (ZLU_NB + 1);   // zgetrs_small
  return ZLU_BLOCK_LDS;
}
// members per pass; with_lu: LU lives in workspace (zsolve), N^2 complex elements per member, at most 1 GiB
int64_t nd4_zgetrf_chunk(int64_t batch, int64_t N, bool with_lu) {
  int64_t c = ZLU_CHUNK;
  if (with_lu && ZLU_WS_ELEMS / (N * N) < c) c = ZLU_WS_ELEMS / (N * N);
  if (c < 1) c = 1;
  return batch < c ? batch : c;
}

// zlu_decomp: LU [batch, N, N], P [batch, N] from A; info (device, int32 [batch], may be NULL) receives the members' flags. Arguments
// already checked, batch >= 1, 1 <= N <= 2048. Enqueues only: a singular member is no error here
int nd4_zgetrf(nd4hip_handle* h, int64_t batch, int64_t N64, const double* A, double* LU, int32_t* P, int32_t* info) {
  ND4_CHECK_ARG(N64 >= 1 && N64 <= ZLU_MAXN, "nd4hip_zgetrf_batched: N <= 2048");
  ND4_CHECK_ARG(zlu_al16(A) && zlu_al16(LU), "nd4hip_zgetrf_batched: complex operands must be 16-byte aligned");
  const int N = (int)N64;
  const int64_t nn = N64 * N64, chunk = nd4_zgetrf_chunk(batch, N64, false);
  Nd4WsScope scope(h);
  int *flags = nullptr, *ipiv = nullptr;
  ND4_TRY(zlu_alloc(h, (size_t)(chunk + 1), &flags));
  if (nd4_zgetrf_tier(N64) == 2) ND4_TRY(zlu_alloc(h, (size_t)(chunk * N64), &ipiv));
  for (int64_t b0 = 0; b0 < batch; b0 += chunk) {
    const int64_t nb = batch - b0 < chunk ? batch - b0 : chunk;
    ND4_HIP(hipMemsetAsync(flags, 0, sizeof(int) * (size_t)(nb + 1), h->stream));
    ND4_TRY(zlu_factor(h, nb, N, ccd(A) + b0 * nn, mcd(LU) + b0 * nn, P + b0 * N64, flags, ipiv));
    if (info) ND4_HIP(hipMemcpyAsync(info + b0, flags + 1, sizeof(int) * (size_t)nb, hipMemcpyDeviceToDevice, h->stream));
  }
  return 0;
}

// zlu_solve: X [batch, N, K] with A X = Y from LU, P; strides in complex elements (ints for P), 0 = one for all. Enqueues only
int nd4_zgetrs(nd4hip_handle* h, int64_t batch, int64_t N64, int64_t K, const double* LU, int64_t sLU, const int32_t* P, int64_t sP,
               const double* Y, int64_t sY, double* X) {
  ND4_CHECK_ARG(N64 >= 1 && N64 <= ZLU_MAXN, "nd4hip_zgetrs_batched: N <= 2048");
  ND4_CHECK_ARG(zlu_al16(LU) && zlu_al16(Y) && zlu_al16(X), "nd4hip_zgetrs_batched: complex operands must be 16-byte aligned");
  const int64_t chunk = nd4_zgetrf_chunk(batch, N64, false);
  for (int64_t b0 = 0; b0 < batch; b0 += chunk) {
    const int64_t nb = batch - b0 < chunk ? batch - b0 : chunk;
    ND4_TRY(zlu_solve(h, nb, (int)N64, K, ccd(LU) + b0 * sLU, sLU, P + b0 * sP, sP, ccd(Y) + b0 * sY, sY, mcd(X) + b0 * N64 * K));
  }
  return 0;
}

// zsolve: X [batch, N, K] with A X = Y, LU and P in workspace, both steps back to back on the stream. One flag word per pass is read
// back; the members' flags only when it is raised: ND4HIP_ERR_SINGULAR with the lowest flagged member (member0: the index of the
// first member in the caller's batch), also in *first_bad (may be NULL). Synchronises
int nd4_zgesv(nd4hip_handle* h, int64_t batch, int64_t N64, int64_t K, const double* A, const double* Y, double* X, int64_t member0, int64_t* first_bad) {
  ND4_CHECK_ARG(N64 >= 1 && N64 <= ZLU_MAXN, "nd4hip_zgesv_batched: N <= 2048");
  ND4_CHECK_ARG(zlu_al16(A) && zlu_al16(Y) && zlu_al16(X), "nd4hip_zgesv_batched: complex operands must be 16-byte aligned");
  const int N = (int)N64;
  const int64_t nn = N64 * N64, nk = N64 * K, chunk = nd4_zgetrf_chunk(batch, N64, true);
  Nd4WsScope scope(h);
  // one request for the flags, the pivots, P and LU: a call's first request reuses a cached block of the arena
  const size_t ibytes = (sizeof(int) * (size_t)(chunk + 1 + 2 * chunk * N64) + 255) & ~size_t(255);
  char* ws = nullptr;
  ND4_TRY(zlu_alloc(h, ibytes + sizeof(cd) * (size_t)(chunk * nn), &ws));
  int* flags = reinterpret_cast<int*>(ws);
  int *Pw = flags + chunk + 1, *ipiv = Pw + chunk * N64;
  cd* LUw = reinterpret_cast<cd*>(ws + ibytes);
  void* hp = nullptr;
  ND4_TRY(nd4_pinned(h, sizeof(int) * (size_t)(chunk + 1), &hp));
  int* host = static_cast<int*>(hp);
  for (int64_t b0 = 0; b0 < batch; b0 += chunk) {
    const int64_t nb = batch - b0 < chunk ? batch - b0 : chunk;
    ND4_HIP(hipMemsetAsync(flags, 0, sizeof(int) * (size_t)(nb + 1), h->stream));
    ND4_TRY(zlu_factor(h, nb, N, ccd(A) + b0 * nn, LUw, Pw, flags, ipiv));
    ND4_TRY(zlu_solve(h, nb, N, K, LUw, nn, Pw, N64, ccd(Y) + b0 * nk, nk, mcd(X) + b0 * nk));
    ND4_HIP(hipMemcpyAsync(host, flags, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    ND4_HIP(hipStreamSynchronize(h->stream));
    if (host[0] == 0) continue;
    ND4_HIP(hipMemcpyAsync(host, flags, sizeof(int) * (size_t)(nb + 1), hipMemcpyDeviceToHost, h->stream));
    ND4_HIP(hipStreamSynchronize(h->stream));
    int64_t b = 0;
    while (b < nb - 1 && host[1 + b] == 0) ++b;
    if (first_bad) *first_bad = member0 + b0 + b;
    nd4_set_error("zsolve(A,Y): A is singular. (matrix %lld)", (long long)(member0 + b0 + b));
    return ND4HIP_ERR_SINGULAR;
  }
  return 0;
}
