// Sylvester and Lyapunov equations on the device: schur_sylvester / sylvester_solve / lyapunov_solve. float64,
// row-major members, 1 <= M, N <= 2048.
//
// dtrsyl is LAPACK's trsyl without its scaling: TA Y + Y op(TB) = C for upper quasi-triangular TA [M, M] and TB [N, N] (Bartels-Stewart's
// triangular stage). A nonzero T[i+1][i] joins rows i and i + 1 into a 2 x 2 diagonal block; nothing below the first subdiagonal is
// read. Cell (p, q) of the block grid, the pair (block p of TA, block q of TB), is a Kronecker system of order 1, 2 or 4:
//   A_pp Y_pq + Y_pq op(B)_qq = C_pq - sum_{k > p} A_pk Y_kq - sum_{k < q} Y_pk B_kq          (op = transpose: sum_{k > q} Y_pk B_qk^T)
// so a cell waits for the cells below it in its column and left (transposed: right) of it in its row, and the cells of one
// anti-diagonal of the grid are independent.
//
// trsyl_tile   one workgroup of 256 threads solves one tile pair, at most 64 x 64, with TA's tile, TB's tile and the right-hand side in
//              LDS: 3 x 64 x 65 doubles = 99 840 bytes of the CU's 160 KB (pitch 65 against bank conflicts of the column reads; three
//              tiles of 81 would still fit, 64 is kept because it is also the MFMA tile of the update below). Waves 0 and 1 find the
//              block starts of the two subdiagonals by a ballot and a population count (the prefix scan). Then the anti-diagonals of
//              the cell grid, one barrier each: the nc <= 64 cells of an anti-diagonal get G = min(64, 256 / nc rounded down to a
//              power of two) >= 4 lanes each, lane l of a cell forms entry l & 3 of the 2 x 2 right-hand side over the terms
//              l >> 2, l >> 2 + G / 4, ... of its dot products (first the TA row against the solved part of the column, then the
//              solved part of the row against TB), a butterfly over the G / 4 slices adds them, and the cell solves its padded 4 x 4
//              system in registers by Gaussian elimination with complete pivoting. G depends only on the member's own block
//              structure, so does every sum's order. A pivot that is zero or not finite raises the member's flag.
// Orders up to 64 are one tile; above, the tiles start at 63 k, moved to 63 k + 1 where T[63k][63k-1] != 0 (a 2 x 2 block is never
// cut), so no tile exceeds 64; every kernel reads that entry itself, the host never sees the structure.
// trsyl_update after the tile pairs of a tile anti-diagonal are solved (one launch over members x pairs), one launch over members x all
//              tile pairs: an unsolved pair (I', J') subtracts TA[I', I] Y[I, J'] of the pair just solved in its column and
//              Y[I', J] op(TB)[J, J'] of the pair just solved in its row, both into the same accumulators of
//              v_mfma_f64_16x16x4_f64 (a wave owns 16 rows and four 16 x 16 accumulators), the column product first. Every other
//              workgroup leaves at once. Launches per call: 2 (tiles of M + tiles of N) - 3 and a copy, whatever the number of pairs.
// dgesyl       the Schur forms by dgees (twice; once for the Lyapunov form B = A^T, which takes op = transpose on the same T),
//              F = QA^T C QB and X = QA Y QB^T on the GEMM that never splits K.
// No atomics on doubles, no synchronisation but __syncthreads(), wave shuffles and the kernel boundary.
// Flags: [0] the OR over the members of a pass, [1 + member] = 1 for a member with an unusable pivot.
#include "nd4hip_internal.h"
#include <cfloat>
#include <cmath>

namespace {

typedef double d4 __attribute__((ext_vector_type(4)));

constexpr int TS_N = 64;                        // the largest tile, and the largest order that is one tile
constexpr int TS_STEP = 63;                     // nominal tile start distance above TS_N (a start may move up by one)
constexpr int TS_LD = TS_N + 1;                 // LDS pitch
constexpr int TS_T = 256;                       // threads per workgroup
constexpr int TS_BK = 32;                       // K step of trsyl_update
constexpr int64_t TS_CHUNK = 32768;             // members per pass
constexpr int64_t TS_WS_ELEMS = 1ll << 27;      // dgesyl: a pass's workspace takes at most 1 GiB
constexpr size_t TS_LDS_BYTES = sizeof(double) * 3 * TS_N * TS_LD;

struct TsArgs {
  const double* TA; const double* TB;           // members M M and N N apart
  const double* C; double* X;                   // members M N apart; C == X in the tiled tier
  int* flags;
  int M, N, ntA, ntB, w, trans;                 // w: the tile anti-diagonal
};

inline int ts_nt(int n) { return n <= TS_N ? 1 : (n + TS_STEP - 1) / TS_STEP; }

// the first row of tile k of T [n][n], k in [0, nt]; a tile may be empty (n = 63 j + 1 with a 2 x 2 block at its end)
__device__ __forceinline__ int ts_bound(const double* T, int n, int nt, int k) {
  if (k <= 0) return 0;
  if (k >= nt) return n;
  const int b = TS_STEP * k;
  return b + (T[(long)b * n + b - 1] != 0.0 ? 1 : 0);
}
// the pair of tile anti-diagonal w with number c: a = ntA - 1 - I counts the tile rows from the bottom, w - a the tile columns from
// the side the sweep starts at
__device__ __forceinline__ void ts_pair(const TsArgs& g, int c, int& I, int& J) {
  const int alo = g.w - (g.ntB - 1) > 0 ? g.w - (g.ntB - 1) : 0;
  const int a = alo + c, qq = g.w - a;
  I = g.ntA - 1 - a;
  J = g.trans ? g.ntB - 1 - qq : qq;
}

// K y = r of order 4 in registers, complete pivoting (the first largest |k_ij| in row-major order; a NaN is never preferred); true if a
// pivot is zero or not finite. Rows of an absent unknown are unit rows, so blocks of order 1 and 2 take the same code
__device__ __forceinline__ bool ts_solve4(double (&K)[4][4], double (&r)[4], double (&y)[4]) {
  int cp[4] = {0, 1, 2, 3};
  bool bad = false;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    double best = fabs(K[k][k]);
    int bi = k, bj = k;
#pragma unroll
    for (int i = k; i < 4; ++i)
#pragma unroll
      for (int j = k; j < 4; ++j) {
        const double m = fabs(K[i][j]);
        if (m > best) { best = m; bi = i; bj = j; }
      }
#pragma unroll
    for (int i = k + 1; i < 4; ++i)
      if (i == bi) {
#pragma unroll
        for (int j = 0; j < 4; ++j) { const double s = K[k][j]; K[k][j] = K[i][j]; K[i][j] = s; }
        const double s = r[k]; r[k] = r[i]; r[i] = s;
      }
#pragma unroll
    for (int j = k + 1; j < 4; ++j)
      if (j == bj) {
#pragma unroll
        for (int i = 0; i < 4; ++i) { const double s = K[i][k]; K[i][k] = K[i][j]; K[i][j] = s; }
        const int s = cp[k]; cp[k] = cp[j]; cp[j] = s;
      }
    const double piv = K[k][k], mag = fabs(piv);
    bad = bad || !(mag > 0.0 && mag <= DBL_MAX);
#pragma unroll
    for (int i = k + 1; i < 4; ++i) {
      const double l = K[i][k] / piv;
      if (l != 0.0) {                                          // (a unit row never meets an overflowed right-hand side)
#pragma unroll
        for (int j = k + 1; j < 4; ++j) K[i][j] -= l * K[k][j];
        r[i] -= l * r[k];
      }
    }
  }
  double z[4];
#pragma unroll
  for (int k = 3; k >= 0; --k) {
    double s = r[k];
#pragma unroll
    for (int j = k + 1; j < 4; ++j) s -= K[k][j] * z[j];
    z[k] = s / K[k][k];
  }
#pragma unroll
  for (int k = 0; k < 4; ++k)
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (cp[k] == e) y[e] = z[k];
  return bad;
}

// block starts of the m rows of the tile S from its subdiagonal, by one wave: blk[p] = first row of block p, blk[count] = m. Row i
// continues a block only if S[i][i-1] != 0 and S[i-1][i-2] == 0, so no block has more than two rows whatever S holds
__device__ __forceinline__ void ts_blocks(const double* S, int m, int lane, int* blk, int* count) {
  const bool sub1 = lane >= 1 && lane < m && S[lane * TS_LD + lane - 1] != 0.0;
  const bool sub2 = lane >= 2 && lane < m && S[(lane - 1) * TS_LD + lane - 2] != 0.0;
  const bool start = lane < m && (!sub1 || sub2);
  const unsigned long long mask = __ballot(start);
  const int idx = __popcll(mask & ((2ull << lane) - 1ull)) - 1;
  if (start) blk[idx] = lane;
  if (lane == 0) { const int n = __popcll(mask); blk[n] = m; *count = n; }
}

// one tile pair of anti-diagonal g.w per workgroup; grid (pairs, members); dynamic LDS TS_LDS_BYTES
__global__ __launch_bounds__(TS_T) void trsyl_tile(TsArgs g) {
  extern __shared__ __attribute__((aligned(16))) double ts_smem[];
  __shared__ int blkA[TS_N + 1], blkB[TS_N + 1], s_nb[2];
  double *SA = ts_smem, *SB = SA + TS_N * TS_LD, *SC = SB + TS_N * TS_LD;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const long mat = blockIdx.y;
  const double* TA = g.TA + mat * g.M * g.M;
  const double* TB = g.TB + mat * g.N * g.N;
  int I, J;
  ts_pair(g, blockIdx.x, I, J);
  const int i0 = ts_bound(TA, g.M, g.ntA, I), m = ts_bound(TA, g.M, g.ntA, I + 1) - i0;
  const int j0 = ts_bound(TB, g.N, g.ntB, J), n = ts_bound(TB, g.N, g.ntB, J + 1) - j0;
  if (m <= 0 || n <= 0) return;                                // (the whole workgroup)
  for (int e = t; e < m * m; e += TS_T) { const int i = e / m, j = e - i * m; SA[i * TS_LD + j] = j >= i - 1 ? TA[(long)(i0 + i) * g.M + i0 + j] : 0.0; }
  for (int e = t; e < n * n; e += TS_T) { const int i = e / n, j = e - i * n; SB[i * TS_LD + j] = j >= i - 1 ? TB[(long)(j0 + i) * g.N + j0 + j] : 0.0; }
  const double* c = g.C + mat * g.M * g.N + (long)i0 * g.N + j0;
  for (int e = t; e < m * n; e += TS_T) { const int i = e / n, j = e - i * n; SC[i * TS_LD + j] = c[(long)i * g.N + j]; }
  __syncthreads();
  if (wave == 0) ts_blocks(SA, m, lane, blkA, &s_nb[0]);
  if (wave == 1) ts_blocks(SB, n, lane, blkB, &s_nb[1]);
  __syncthreads();
  const int nbA = s_nb[0], nbB = s_nb[1];
  bool raised = false;
  for (int w = 0; w < nbA + nbB - 1; ++w) {
    const int alo = w - (nbB - 1) > 0 ? w - (nbB - 1) : 0, ahi = w < nbA - 1 ? w : nbA - 1, nc = ahi - alo + 1;
    int G = 64;
    while (G > 4 && G * nc > TS_T) G >>= 1;
    const int grp = t / G, li = t & (G - 1), e = li & 3, di = e >> 1, dj = e & 1;
    const bool active = grp < nc;
    int r0 = 0, ra = 0, c0 = 0, cb = 0;
    if (active) {
      const int a = alo + grp, p = nbA - 1 - a, qq = w - a, q = g.trans ? nbB - 1 - qq : qq;
      r0 = blkA[p]; ra = blkA[p + 1] - r0;
      c0 = blkB[q]; cb = blkB[q + 1] - c0;
    }
    const bool has = di < ra && dj < cb;
    const int i = r0 + di, j = c0 + dj;
    double sum = 0.0;
    if (has) {
      const int kA = r0 + ra, La = m - kA, kB = g.trans ? c0 + cb : 0, Lb = g.trans ? n - kB : c0;
      for (int s = li >> 2; s < La + Lb; s += G >> 2) {
        if (s < La) sum += SA[i * TS_LD + kA + s] * SC[(kA + s) * TS_LD + j];
        else if (g.trans) sum += SC[i * TS_LD + kB + s - La] * SB[j * TS_LD + kB + s - La];
        else sum += SC[i * TS_LD + s - La] * SB[(s - La) * TS_LD + j];
      }
    }
    for (int off = 4; off < G; off <<= 1) sum += __shfl_xor(sum, off);
    const double rv = has ? SC[i * TS_LD + j] - sum : 0.0;
    const int base = lane & ~(G - 1);
    double r[4], y[4], K[4][4];
#pragma unroll
    for (int k = 0; k < 4; ++k) r[k] = __shfl(rv, base + k);
    // unknown 2 i + j is y_ij; row (i, j): sum_k a_ik y_kj + sum_l y_il b'_lj with b' = op(B)
    double a00 = 0.0, a01 = 0.0, a10 = 0.0, a11 = 0.0, b00 = 0.0, b01 = 0.0, b10 = 0.0, b11 = 0.0;
    if (active) {
      a00 = SA[r0 * TS_LD + r0]; b00 = SB[c0 * TS_LD + c0];
      if (ra == 2) { a01 = SA[r0 * TS_LD + r0 + 1]; a10 = SA[(r0 + 1) * TS_LD + r0]; a11 = SA[(r0 + 1) * TS_LD + r0 + 1]; }
      if (cb == 2) {
        const double u = SB[c0 * TS_LD + c0 + 1], l = SB[(c0 + 1) * TS_LD + c0];
        b01 = g.trans ? l : u; b10 = g.trans ? u : l; b11 = SB[(c0 + 1) * TS_LD + c0 + 1];
      }
    }
    K[0][0] = a00 + b00; K[0][1] = b10;       K[0][2] = a01;       K[0][3] = 0.0;
    K[1][0] = b01;       K[1][1] = a00 + b11; K[1][2] = 0.0;       K[1][3] = a01;
    K[2][0] = a10;       K[2][1] = 0.0;       K[2][2] = a11 + b00; K[2][3] = b10;
    K[3][0] = 0.0;       K[3][1] = a10;       K[3][2] = b01;       K[3][3] = a11 + b11;
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (!((k >> 1) < ra && (k & 1) < cb)) {
#pragma unroll
        for (int l = 0; l < 4; ++l) K[k][l] = k == l ? 1.0 : 0.0;
        r[k] = 0.0;
      }
    const bool bad = ts_solve4(K, r, y);
    if (has && li < 4) SC[i * TS_LD + j] = y[e];
    raised = raised || (bad && active && li == 0);
    __syncthreads();
  }
  if (raised) { atomicOr(&g.flags[1 + mat], 1); atomicOr(&g.flags[0], 1); }
  double* x = g.X + mat * g.M * g.N + (long)i0 * g.N + j0;
  for (int e = t; e < m * n; e += TS_T) { const int i = e / n, j = e - i * n; x[(long)i * g.N + j] = SC[i * TS_LD + j]; }
}

// acc += P Q on the fp64 MFMA: P(r, k) = Pp[r ldp + k], r < rows; Q(k, c) = tq ? Qp[c ldq + k] : Qp[k ldq + c], c < cols; k < K.
// All 256 threads; a wave owns rows 16 wave .. 16 wave + 15 of the 64 x 64 product; ends behind a barrier
__device__ void ts_mma(d4 (&acc)[4], double* sa, double* sb, const double* Pp, long ldp, int rows, const double* Qp, long ldq, bool tq, int K, int cols) {
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, fx = lane & 15, fk = lane >> 4;
  for (int k0 = 0; k0 < K; k0 += TS_BK) {
    for (int e = t; e < TS_N * TS_BK; e += TS_T) {
      const int i = e / TS_BK, k = e - i * TS_BK;
      sa[i * (TS_BK + 1) + k] = (i < rows && k0 + k < K) ? Pp[(long)i * ldp + k0 + k] : 0.0;
    }
    for (int e = t; e < TS_BK * TS_N; e += TS_T) {
      const int k = tq ? e % TS_BK : e / TS_N, j = tq ? e / TS_BK : e % TS_N;
      sb[k * TS_LD + j] = (k0 + k < K && j < cols) ? (tq ? Qp[(long)j * ldq + k0 + k] : Qp[(long)(k0 + k) * ldq + j]) : 0.0;
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < TS_BK / 4; ++kk) {
      const double a = sa[(wave * 16 + fx) * (TS_BK + 1) + kk * 4 + fk];
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, sb[(kk * 4 + fk) * TS_LD + j * 16 + fx], acc[j], 0, 0, 0);
    }
    __syncthreads();
  }
}

// after anti-diagonal g.w: the pair blockIdx.x = I' ntB + J', if unsolved, subtracts the products with the two pairs just solved in its
// column and in its row; grid (ntA ntB, members)
__global__ __launch_bounds__(TS_T) void trsyl_update(TsArgs g) {
  __shared__ double sa[TS_N * (TS_BK + 1)], sb[TS_BK * TS_LD];
  const int Ip = blockIdx.x / g.ntB, Jp = blockIdx.x - Ip * g.ntB;
  const int ap = g.ntA - 1 - Ip, qp = g.trans ? g.ntB - 1 - Jp : Jp;
  const int a = g.w - qp, I = g.ntA - 1 - a;                   // the solved pair of column J' is (I, J')
  const int qq = g.w - ap, J = g.trans ? g.ntB - 1 - qq : qq;  // the solved pair of row I' is (I', J)
  const bool col = a >= 0 && a < ap, row = qq >= 0 && qq < qp;
  if (!col && !row) return;                                    // (the whole workgroup)
  const long mat = blockIdx.y;
  const double* TA = g.TA + mat * g.M * g.M;
  const double* TB = g.TB + mat * g.N * g.N;
  double* X = g.X + mat * g.M * g.N;
  const int i0 = ts_bound(TA, g.M, g.ntA, Ip), m = ts_bound(TA, g.M, g.ntA, Ip + 1) - i0;
  const int j0 = ts_bound(TB, g.N, g.ntB, Jp), n = ts_bound(TB, g.N, g.ntB, Jp + 1) - j0;
  if (m <= 0 || n <= 0) return;
  d4 acc[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) acc[j] = d4{0.0, 0.0, 0.0, 0.0};
  if (col) {
    const int k0 = ts_bound(TA, g.M, g.ntA, I), K = ts_bound(TA, g.M, g.ntA, I + 1) - k0;
    ts_mma(acc, sa, sb, TA + (long)i0 * g.M + k0, g.M, m, X + (long)k0 * g.N + j0, g.N, false, K, n);
  }
  if (row) {
    const int k0 = ts_bound(TB, g.N, g.ntB, J), K = ts_bound(TB, g.N, g.ntB, J + 1) - k0;
    if (g.trans) ts_mma(acc, sa, sb, X + (long)i0 * g.N + k0, g.N, m, TB + (long)j0 * g.N + k0, g.N, true, K, n);
    else         ts_mma(acc, sa, sb, X + (long)i0 * g.N + k0, g.N, m, TB + (long)k0 * g.N + j0, g.N, false, K, n);
  }
  // lane holds row (lane >> 4) + 4 r, column lane & 15 of each 16 x 16 tile
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, fx = lane & 15, fk = lane >> 4;
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int rr = wave * 16 + fk + 4 * r, cc = j * 16 + fx;
      if (rr < m && cc < n) X[(long)(i0 + rr) * g.N + j0 + cc] -= acc[j][r];
    }
}

// NaN into every element of the flagged members; grid (tiles, members)
__global__ __launch_bounds__(TS_T) void trsyl_poison(double* __restrict__ X, long mn, const int* __restrict__ flags) {
  if (flags[1 + blockIdx.y] == 0) return;
  double* x = X + blockIdx.y * mn;
  for (long e = (long)blockIdx.x * TS_T + threadIdx.x; e < mn; e += (long)gridDim.x * TS_T) x[e] = NAN;
}
__global__ void trsyl_clear(int* __restrict__ flags, long n) {
  const long e = (long)blockIdx.x * TS_T + threadIdx.x;
  if (e < n) flags[e] = 0;
}

// ---- host side ----------------------------------------------------------------------------------------------------------------------
template <class T> int ts_alloc(nd4hip_handle* h, size_t n, T** out) {
  void* p = nullptr;
  ND4_TRY(nd4_ws_alloc(h, sizeof(T) * n, &p));
  *out = static_cast<T*>(p);
  return 0;
}

// Y [nb, M, N] into X from TA, TB, C (none of them X); flags [nb + 1] are cleared here
int ts_pass(nd4hip_handle* h, int64_t nb, int M, int N, bool trans, const double* TA, const double* TB, const double* C, double* X, int* flags) {
  const int64_t mn = (int64_t)M * N;
  hipLaunchKernelGGL(trsyl_clear, dim3((unsigned)((nb + 1 + TS_T - 1) / TS_T)), dim3(TS_T), 0, h->stream, flags, (long)(nb + 1));
  ND4_HIP(hipGetLastError());
  ND4_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&trsyl_tile), hipFuncAttributeMaxDynamicSharedMemorySize, (int)TS_LDS_BYTES));
  TsArgs g{TA, TB, C, X, flags, M, N, ts_nt(M), ts_nt(N), 0, trans ? 1 : 0};
  const int nw = g.ntA + g.ntB - 1;
  if (nw > 1) {                                                // the tiled tier works in place in X
    ND4_HIP(hipMemcpyAsync(X, C, sizeof(double) * (size_t)(nb * mn), hipMemcpyDeviceToDevice, h->stream));
    g.C = X;
  }
  for (int w = 0; w < nw; ++w) {
    g.w = w;
    const int alo = w - (g.ntB - 1) > 0 ? w - (g.ntB - 1) : 0, ahi = w < g.ntA - 1 ? w : g.ntA - 1;
    hipLaunchKernelGGL(trsyl_tile, dim3((unsigned)(ahi - alo + 1), (unsigned)nb), dim3(TS_T), TS_LDS_BYTES, h->stream, g);
    ND4_HIP(hipGetLastError());
    if (w + 1 == nw) break;
    hipLaunchKernelGGL(trsyl_update, dim3((unsigned)(g.ntA * g.ntB), (unsigned)nb), dim3(TS_T), 0, h->stream, g);
    ND4_HIP(hipGetLastError());
  }
  const int64_t tiles = (mn + TS_T - 1) / TS_T;
  hipLaunchKernelGGL(trsyl_poison, dim3((unsigned)(tiles < 1024 ? tiles : 1024), (unsigned)nb), dim3(TS_T), 0, h->stream, X, (long)mn, flags);
  ND4_HIP(hipGetLastError());
  return 0;
}

// a pass's flags: into info, or one word read back and, if it is raised, the members' words: the lowest flagged member
int ts_verdict(nd4hip_handle* h, int64_t nb, const int* flags, int32_t* info, int64_t first, const char* what, int64_t* first_bad) {
  if (info) {
    ND4_HIP(hipMemcpyAsync(info, flags + 1, sizeof(int) * (size_t)nb, hipMemcpyDeviceToDevice, h->stream));
    return 0;
  }
  void* hp = nullptr;                                          // (taken here: dgees's own read-back may have moved the pinned block)
  ND4_TRY(nd4_pinned(h, sizeof(int) * (size_t)(nb + 1), &hp));
  int* host = static_cast<int*>(hp);
  ND4_HIP(hipMemcpyAsync(host, flags, sizeof(int), hipMemcpyDeviceToHost, h->stream));
  ND4_HIP(hipStreamSynchronize(h->stream));
  if (host[0] == 0) return 0;
  ND4_HIP(hipMemcpyAsync(host, flags, sizeof(int) * (size_t)(nb + 1), hipMemcpyDeviceToHost, h->stream));
  ND4_HIP(hipStreamSynchronize(h->stream));
  int64_t b = 0;
  while (b < nb - 1 && host[1 + b] == 0) ++b;
  if (first_bad) *first_bad = first + b;
  nd4_set_error("%s: the equation is singular. (matrix %lld)", what, (long long)(first + b));
  return ND4HIP_ERR_SINGULAR;
}

}  // namespace

// schur_sylvester: Y [batch, M, N] with TA Y + Y op(TB) = C. info (device, int32 [batch]) receives the members' flags and the call only
// enqueues; info = NULL: one flag word per pass is read back, ND4HIP_ERR_SINGULAR names the lowest flagged member (counted from member0,
// also in *first_bad, may be NULL). Arguments already checked
int nd4_trsyl(nd4hip_handle* h, bool trans_b, int64_t batch, int64_t M, int64_t N, const double* TA, const double* TB, const double* C, double* X,
              int32_t* info, int64_t member0, int64_t* first_bad) {
  const int64_t chunk = batch < TS_CHUNK ? batch : TS_CHUNK;
  Nd4WsScope scope(h);
  int* flags = nullptr;
  ND4_TRY(ts_alloc(h, (size_t)(chunk + 1), &flags));
  for (int64_t b0 = 0; b0 < batch; b0 += chunk) {
    const int64_t nb = batch - b0 < chunk ? batch - b0 : chunk;
    ND4_TRY(ts_pass(h, nb, (int)M, (int)N, trans_b, TA + b0 * M * M, TB + b0 * N * N, C + b0 * M * N, X + b0 * M * N, flags));
    ND4_TRY(ts_verdict(h, nb, flags, info ? info + b0 : nullptr, member0 + b0, "schur_sylvester(TA,TB,C)", first_bad));
  }
  return 0;
}

// sylvester_solve: X with A X + X B = C; B = NULL (M == N): lyapunov_solve, A X + X A^T = C. info, member0, first_bad as nd4_trsyl;
// dgees synchronises in either case. Arguments already checked
int nd4_gesyl(nd4hip_handle* h, int64_t batch, int64_t M, int64_t N, const double* A, const double* B, const double* C, double* X,
              int32_t* info, int64_t member0, int64_t* first_bad) {
  const int64_t mm = M * M, nn = N * N, mn = M * N;
  const int64_t per = 2 * mm + (B ? 2 * nn : 0) + 2 * mn;
  int64_t chunk = TS_WS_ELEMS / per < TS_CHUNK ? TS_WS_ELEMS / per : TS_CHUNK;
  if (chunk < 1) chunk = 1;
  if (batch < chunk) chunk = batch;
  const char* what = B ? "sylvester_solve(A,B,C)" : "lyapunov_solve(A,Q)";
  Nd4WsScope scope(h);
  double *QA = nullptr, *SA = nullptr, *QB = nullptr, *SB = nullptr, *F = nullptr, *W = nullptr;
  int* flags = nullptr;
  ND4_TRY(ts_alloc(h, (size_t)(chunk * mm), &QA));
  ND4_TRY(ts_alloc(h, (size_t)(chunk * mm), &SA));
  if (B) {
    ND4_TRY(ts_alloc(h, (size_t)(chunk * nn), &QB));
    ND4_TRY(ts_alloc(h, (size_t)(chunk * nn), &SB));
  } else {
    QB = QA; SB = SA;
  }
  ND4_TRY(ts_alloc(h, (size_t)(chunk * mn), &F));
  ND4_TRY(ts_alloc(h, (size_t)(chunk * mn), &W));
  ND4_TRY(ts_alloc(h, (size_t)(chunk + 1), &flags));
  for (int64_t b0 = 0; b0 < batch; b0 += chunk) {
    const int64_t nb = batch - b0 < chunk ? batch - b0 : chunk;
    ND4_TRY(nd4hip_dgees_batched_dev(h, nb, M, A + b0 * mm, QA, SA, nullptr));
    if (B) ND4_TRY(nd4hip_dgees_batched_dev(h, nb, N, B + b0 * nn, QB, SB, nullptr));
    // F = QA^T C QB, Y (in W) from the triangular stage, X = QA Y QB^T
    ND4_TRY(nd4_gemm_member_order(h, true, false, M, N, M, 1.0, QA, M, mm, C + b0 * mn, N, mn, 0.0, W, N, mn, nb));
    ND4_TRY(nd4_gemm_member_order(h, false, false, M, N, N, 1.0, W, N, mn, QB, N, nn, 0.0, F, N, mn, nb));
    ND4_TRY(ts_pass(h, nb, (int)M, (int)N, !B, SA, SB, F, W, flags));
    ND4_TRY(nd4_gemm_member_order(h, false, false, M, N, M, 1.0, QA, M, mm, W, N, mn, 0.0, F, N, mn, nb));
    ND4_TRY(nd4_gemm_member_order(h, false, true, M, N, N, 1.0, F, N, mn, QB, N, nn, 0.0, X + b0 * mn, N, mn, nb));
    hipLaunchKernelGGL(trsyl_poison, dim3((unsigned)((mn + TS_T - 1) / TS_T < 1024 ? (mn + TS_T - 1) / TS_T : 1024), (unsigned)nb), dim3(TS_T), 0,
                       h->stream, X + b0 * mn, (long)mn, flags);
    ND4_HIP(hipGetLastError());
    ND4_TRY(ts_verdict(h, nb, flags, info ? info + b0 : nullptr, member0 + b0, what, first_bad));
  }
  return 0;
}
