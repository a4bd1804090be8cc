// Complex128 bidiagonalisation and SVD on the device: zbidiag_factor / zbidiag_apply_p / zsvd_decomp / zsvd_vals, LAPACK's
// zgebrd (upper form) / zunmbr ('P') / zgesdd on row-major members, interleaved (re, im) doubles.
//   A = Q B P^H for N <= M <= 2048, B real upper bidiagonal (d [N], e [N-1]).
//   Q = H_0 ... H_{N-1}, H_k = I - tauq_k v_k v_k^H, v_k zero above row k, 1 in row k, its tail in F[k+1:, k]: zgeqrf.hip's layout, so
//   nd4_zunmqr applies Q. P = G_0 ... G_{N-2}, G_k = I - taup_k u_k u_k^H, u_k zero up to column k, 1 in column k + 1, its tail in
//   F[k, k+2:]; taup [N] ends in 0. d and e stand on F's diagonal and superdiagonal.
//   Step k, left: x = A[k:, k] is reflected (zlarfg.h) so that H_k^H x = d_k e_1, and A[k:, k+1:] <- H_k^H A[k:, k+1:] = A - v w,
//   w_c = conj(tauq) sum_i conj(v_i) a_ic. Right: y = conj(A[k, k+1:]) is reflected so that G_k^H y = e_k e_1, and
//   A[k+1:, k+1:] <- A G_k = A - (taup z) u^H, z = A u. A reflector with an empty tail and Im alpha != 0 is a pure phase: d and e are real.
// Every member is scaled on load by 2^-e1, e1 the exponent that puts max(|Re a_ij|, |Im a_ij|) in [0.5, 1); d and e get 2^e1 back on
// their store (unless the caller is the SVD, which solves the scaled problem and gives 2^e1 to the singular values): A -> 2^m A leaves
// tails, tauq and taup bit-identical. Columns and rows below 2^-450 of the maximum are lifted as in hetrd.hip. NaN or Inf shows in the
// bits of the maximum: one flag word per call.
// Every sum has an order fixed by (M, N, k): no atomics on doubles; the only synchronisation is __syncthreads(), wave shuffles and the
// kernel boundary; every loop bound comes from the shape (the lift: at most two rounds). The file is built without FMA contraction.
//   Tier A, zgebrd_small: the member in one workgroup's LDS at the odd pitch N | 1, one launch per call, when
//       16 (M (N | 1) + 2 M + 6 N + 256) + 96 <= 163840   (the member, v, z, w, u, the partial dot products of at most 4 N + 256, the
//                                                          reduction scratch)                      square members: up to 95 x 95
//     The dot products w are taken by 256 / CW groups of rows and added in group order, as in zgeqr2_small. The row reflector is
//     formed from row k of A - v w before the rest of the block is touched, so that one pass writes A - v w and takes z = (A - v w) u
//     by rows (CW lanes per row, xor tree); a second pass subtracts (taup z) u^H.
//   Tier B, everything else: two launches per column over a grid (blocks of 64 rows, members); the rank-2 update is applied lazily.
//     zgebrd_left  (L_k): every block forms column k from the pending (v, w, z, u) of step k-1 (O(M)) and reflects it; in one pass
//                  over its own rows it applies A -= v w + (taup z) u^H and accumulates its column partials of A^H v_k. The four
//                  waves' partial sums meet in two alternating 4 x 64 LDS buffers per chunk of 64 columns. 16 M bytes of dynamic LDS
//                  (the column) beside 11 KB of static LDS.
//     zgebrd_right (R_k): every block adds the column partials in block order to w, brings row k up to date and reflects it; in one
//                  read-only pass over its rows it forms z = (A - v w) u, row sums that are complete within the block. 32 N bytes of
//                  dynamic LDS (w and u) beside 1 KB of static LDS: 65536 at N = 2048.
//     A block never writes what another block of the same launch reads: the tail of v_k reaches column k of F in R_k, the tail of u_k
//     reaches row k in L_{k+1}.
//   nd4_zunmbr_p: zunmbr_repack writes Fp [N, N] with Fp[i][j] = F[j-1][i] (i > j >= 1) and tau' = (0, taup_0 .. taup_{N-2}); P is then
//     the Q of (Fp, tau') and nd4_zunmqr applies it. The leading reflector has tau' = 0 and a zero tail: the identity.
//   nd4_zgesdd: M < N through the conjugate transpose; 3 M >= 5 N and M > N through nd4_zgeqrf and the bidiagonalisation of R; the real
//     solvers nd4_bdsdc_rows (all triplets) or nd4_bdsvdx (values alone, or a subset) on (d, e); U = Q U2, V = (P V2^T)^H.
#include "nd4hip_internal.h"
#include "zlarfg.h"
#include <cfloat>

namespace {

constexpr int ZBRD_MAXN = 2048;
constexpr int ZBRD_T = 256;
constexpr int ZBRD_ROWS = 64;                    // tier B: rows per workgroup
constexpr size_t ZBRD_LDS = 163840;
constexpr int64_t ZBRD_CHUNK = 32768;            // members per pass
constexpr int64_t ZBRD_WS_ELEMS = 1ll << 26;     // a pass's workspace takes about 1 GiB

__host__ __device__ inline int zbrd_cw(int N) { return N > 32 ? 64 : N > 16 ? 32 : N > 8 ? 16 : 8; }

// the reflector of [alpha; tail] from the block sums (sigma, count of non-zero tail entries); `again(c)` returns this thread's share of
// |c tail|^2 for the lift
template <class Again>
__device__ __forceinline__ HetRefl zbrd_reflect(cd alpha, cd sn, double* red, Again again) {
  double sigma = sn.x, c = 1.0;
  for (int lvl = 0; lvl < 2 && het_tiny(alpha, c, sigma, sn.y); ++lvl) {
    c *= HET_LIFT;
    sigma = het_block_sum(cmk(again(c), 0.0), red).x;
  }
  return het_reflector(alpha, sigma, c);
}
__device__ __forceinline__ cd zbrd_sq(cd x) { return cmk(x.x * x.x + x.y * x.y, x.x != 0.0 || x.y != 0.0 ? 1.0 : 0.0); }

// ---- tier A ---------------------------------------------------------------------------------------------------------------------
// grid (members), 256 threads. A, F [members, M, N], tauq, taup, d [members, N], e [members, N - 1]; mx [members] receives the bits of
// the member's maximum; unscale = 0 leaves d and e (and F's two diagonals) scaled by 2^-e1
__global__ __launch_bounds__(ZBRD_T) void zgebrd_small(const cd* __restrict__ A, cd* __restrict__ F, cd* __restrict__ tauq, cd* __restrict__ taup,
                                                       double* __restrict__ d, double* __restrict__ e, u64* __restrict__ mx, int M, int N,
                                                       int unscale, int* __restrict__ flag) {
  extern __shared__ __attribute__((aligned(16))) char zbrd_smem[];
  const int P = N | 1, t = threadIdx.x;
  const long b = blockIdx.x;
  cd* S = reinterpret_cast<cd*>(zbrd_smem);                   // [M][P]
  cd* v = S + (size_t)M * P;                                  // [M]
  cd* z = v + M;                                              // [M] taup (A - v w) u
  cd* w = z + M;                                              // [N] conj(tauq) v^H a_c
  cd* u = w + N;                                              // [N]
  cd* part = u + N;                                           // [256 / CW][N]: at most 4 N + 256
  double* red = reinterpret_cast<double*>(part + 4 * N + 256);   // [8]
  u64* redu = reinterpret_cast<u64*>(red + 8);                // [4]
  const cd* a = A + b * M * N;
  const cd zero = cmk(0.0, 0.0), one = cmk(1.0, 0.0);
  u64 m = 0;
  for (int idx = t; idx < M * N; idx += ZBRD_T) {
    const int i = idx / N, j = idx - i * N;
    const cd x = a[idx];
    const u64 br = het_bits(x.x), bi = het_bits(x.y);
    m = br > m ? br : m; m = bi > m ? bi : m;
    S[i * P + j] = x;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) { const u64 o = __shfl_xor(m, off); m = o > m ? o : m; }
  if ((t & 63) == 0) redu[t >> 6] = m;
  __syncthreads();
  for (int q = 0; q < 4; ++q) m = redu[q] > m ? redu[q] : m;
  const int e1 = syev_exp(m), eo = unscale ? e1 : 0;
  if (t == 0) { mx[b] = m; if (m > SYEV_MAX_BITS) atomicMax(flag, 1); }
  for (int idx = t; idx < M * N; idx += ZBRD_T) {
    const int i = idx / N, j = idx - i * N;
    const cd x = S[i * P + j];
    S[i * P + j] = cmk(ldexp(x.x, -e1), ldexp(x.y, -e1));
  }
  __syncthreads();
  const int CW = zbrd_cw(N), RG = ZBRD_T / CW, cl = t % CW, q = t / CW;
  for (int k = 0; k < N; ++k) {
    // left: the reflector of A[k:, k]
    cd sn = zero;
    for (int i = k + 1 + t; i < M; i += ZBRD_T) sn = cadd(sn, zbrd_sq(S[i * P + k]));
    const cd alpha = S[k * P + k];
    sn = het_block_sum(sn, red);
    const HetRefl r = zbrd_reflect(alpha, sn, red, [&](double c) {
      double a2 = 0.0;
      for (int i = k + 1 + t; i < M; i += ZBRD_T) { const double xr = c * S[i * P + k].x, xi = c * S[i * P + k].y; a2 += xr * xr + xi * xi; }
      return a2;
    });
    for (int i = k + t; i < M; i += ZBRD_T) v[i] = i == k ? one : (r.on ? cdiv_re(S[i * P + k], r.div) : zero);
    __syncthreads();
    for (int col = k + 1 + cl; col < N; col += CW) {
      cd s = zero;
      for (int i = k + q; i < M; i += RG) s = cadd(s, cmulc(S[i * P + col], v[i]));   // conj(v_i) a_ic
      part[q * N + col] = s;
    }
    __syncthreads();
    const cd ctau = cconj(r.tau);
    // w, and row k of A - v w (v_k = 1) with the sums for its reflector
    cd rn = zero;
    for (int col = k + 1 + t; col < N; col += ZBRD_T) {
      cd s = part[col];
      for (int g = 1; g < RG; ++g) s = cadd(s, part[g * N + col]);
      const cd wc = cmul(ctau, s);
      w[col] = wc;
      const cd x = csub(S[k * P + col], wc);
      S[k * P + col] = x;
      if (col > k + 1) rn = cadd(rn, zbrd_sq(x));
    }
    rn = het_block_sum(rn, red);                              // (its barriers publish w and row k)
    HetRefl g; g.tau = zero; g.beta = 0.0; g.div = one; g.on = false;
    if (k + 1 < N) {                                          // right: the reflector of conj(A[k, k+1:])
      g = zbrd_reflect(cconj(S[k * P + k + 1]), rn, red, [&](double c) {
        double a2 = 0.0;
        for (int col = k + 2 + t; col < N; col += ZBRD_T) { const double xr = c * S[k * P + col].x, xi = c * S[k * P + col].y; a2 += xr * xr + xi * xi; }
        return a2;
      });
      for (int col = k + 1 + t; col < N; col += ZBRD_T) u[col] = col == k + 1 ? one : (g.on ? cdiv_re(cconj(S[k * P + col]), g.div) : zero);
      __syncthreads();
      // one pass over the rows below k: A - v w is written, z = taup (A - v w) u taken by rows
      for (int i0 = k + 1; i0 < M; i0 += RG) {                 // (uniform bounds: the shuffles below are reached by whole groups)
        const int i = i0 + q;
        cd acc = zero;
        if (i < M) {
          const cd vi = v[i];
          for (int col = k + 1 + cl; col < N; col += CW) {
            const cd x = csub(S[i * P + col], cmul(vi, w[col]));
            S[i * P + col] = x;
            acc = cadd(acc, cmul(x, u[col]));
          }
        }
        for (int off = CW >> 1; off > 0; off >>= 1) { acc.x += __shfl_xor(acc.x, off); acc.y += __shfl_xor(acc.y, off); }
        if (cl == 0 && i < M) z[i] = cmul(g.tau, acc);
      }
      __syncthreads();
      const int mm = M - k - 1, nn = N - k - 1;
      if (g.on)                                               // (uniform)
        for (int idx = t; idx < mm * nn; idx += ZBRD_T) {
          const int i = k + 1 + idx / nn, col = k + 1 + idx % nn;
          S[i * P + col] = csub(S[i * P + col], cmulc(z[i], u[col]));   // (taup z_i) conj(u_c)
        }
      for (int col = k + 1 + t; col < N; col += ZBRD_T)
        if (col == k + 1) S[k * P + col] = cmk(g.beta, 0.0); else if (g.on) S[k * P + col] = u[col];
    }
    for (int i = k + t; i < M; i += ZBRD_T)
      if (i == k) S[k * P + k] = cmk(r.beta, 0.0); else if (r.on) S[i * P + k] = v[i];
    if (t == 0) {
      tauq[b * N + k] = r.tau; taup[b * N + k] = g.tau;
      d[b * N + k] = ldexp(r.beta, eo);
      if (k + 1 < N) e[b * (N - 1) + k] = ldexp(g.beta, eo);
    }
    __syncthreads();
  }
  cd* f = F + b * M * N;
  for (int idx = t; idx < M * N; idx += ZBRD_T) {
    const int i = idx / N, j = idx - i * N;
    const cd x = S[i * P + j];
    f[idx] = (j == i || j == i + 1) ? cmk(ldexp(x.x, eo), 0.0) : x;
  }
}

// ---- tier B ---------------------------------------------------------------------------------------------------------------------
// mx[b] = the bits of max(|Re|, |Im|) over A[b] (mx zero on entry; the maximum of integers: any order gives the same word), the flag
// for NaN or Inf; grid (256, members)
__global__ __launch_bounds__(ZBRD_T) void zbrd_absmax(const cd* __restrict__ A, long count, u64* __restrict__ mx, int* __restrict__ flag) {
  const cd* s = A + (long)blockIdx.y * count;
  u64 m = 0;
  for (long i = (long)blockIdx.x * ZBRD_T + threadIdx.x; i < count; i += (long)gridDim.x * ZBRD_T) {
    const u64 br = het_bits(s[i].x), bi = het_bits(s[i].y);
    m = br > m ? br : m; m = bi > m ? bi : m;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) { const u64 o = __shfl_xor(m, off); m = o > m ? o : m; }
  if ((threadIdx.x & 63) == 0 && m) { atomicMax(mx + blockIdx.y, m); if (m > SYEV_MAX_BITS) atomicMax(flag, 1); }
}
// F[b] = 2^-e1 A[b]; grid (tiles of 256 elements, members)
__global__ __launch_bounds__(ZBRD_T) void zbrd_load(const cd* __restrict__ A, cd* __restrict__ F, long count, const u64* __restrict__ mx) {
  const long i = (long)blockIdx.x * ZBRD_T + threadIdx.x;
  if (i >= count) return;
  const int e1 = syev_exp(mx[blockIdx.y]);
  const cd x = A[(long)blockIdx.y * count + i];
  F[(long)blockIdx.y * count + i] = cmk(ldexp(x.x, -e1), ldexp(x.y, -e1));
}
// x[0 .. n) = 0 (the pending update of step -1)
__global__ __launch_bounds__(ZBRD_T) void zbrd_clear(cd* __restrict__ x, long n) {
  const long i = (long)blockIdx.x * ZBRD_T + threadIdx.x;
  if (i < n) x[i] = cmk(0.0, 0.0);
}

// the work of one member between launches: everything [members, ...]
struct ZbrdWs {
  cd *tauq, *taup;  // [N] (the caller's)
  double *dsc, *esc;   // [N] scaled d and e
  cd* vd;           // [2][M] v_k, dense, by the parity of k
  cd* z;            // [M] taup (A - v w) u of the last right half
  cd* w;            // [N]
  cd* u;            // [N]
  cd* colpart;      // [nblk][N] column partials of A^H v_k per row block
};

// L_k; grid (nblk, members), 256 threads, 16 M bytes of dynamic LDS
__global__ __launch_bounds__(ZBRD_T) void zgebrd_left(cd* __restrict__ F, int M, int N, int k, ZbrdWs ws) {
  extern __shared__ __attribute__((aligned(16))) char zbrd_smem[];
  __shared__ cd cw[2][4][64], vps[ZBRD_ROWS], zps[ZBRD_ROWS];
  __shared__ double red[8];
  cd* ck = reinterpret_cast<cd*>(zbrd_smem);                  // [M] column k, then v_k
  const int t = threadIdx.x, blk = blockIdx.x, nblk = gridDim.x;
  const long b = blockIdx.y;
  const int r0 = blk * ZBRD_ROWS, r1 = min(M, r0 + ZBRD_ROWS);
  const bool last = blk == nblk - 1;
  if (r1 < k && !last) return;                                // rows < k - 1 are finished (row k - 1 still receives the tail of u_{k-1})
  cd* A = F + b * M * N;
  const int par = k & 1;
  const cd* vp = ws.vd + (b * 2 + (par ^ 1)) * M;
  const cd* zp = ws.z + b * M;
  const cd* wp = ws.w + b * N;
  const cd* up = ws.u + b * N;
  const cd zero = cmk(0.0, 0.0), one = cmk(1.0, 0.0);
  // column k after step k-1, its reflector
  const cd wk = wp[k], cuk = cconj(up[k]);
  cd sn = zero;
  for (int i = k + t; i < M; i += ZBRD_T) {
    const cd c = csub(csub(A[(long)i * N + k], cmul(vp[i], wk)), cmul(zp[i], cuk));
    ck[i] = c;
    if (i > k) sn = cadd(sn, zbrd_sq(c));
  }
  if (t < ZBRD_ROWS && r0 + t < M) { vps[t] = vp[r0 + t]; zps[t] = zp[r0 + t]; }
  sn = het_block_sum(sn, red);                                // (its barriers publish ck)
  const HetRefl r = zbrd_reflect(ck[k], sn, red, [&](double c) {
    double a2 = 0.0;
    for (int i = k + 1 + t; i < M; i += ZBRD_T) { const double xr = c * ck[i].x, xi = c * ck[i].y; a2 += xr * xr + xi * xi; }
    return a2;
  });
  __syncthreads();
  cd* vout = ws.vd + (b * 2 + par) * M;
  for (int i = k + t; i < M; i += ZBRD_T) {
    const cd x = i == k ? one : (r.on ? cdiv_re(ck[i], r.div) : zero);
    ck[i] = x;
    if (last) vout[i] = x;
  }
  if (last && t == 0) { ws.dsc[b * N + k] = r.beta; ws.tauq[b * N + k] = r.tau; }
  __syncthreads();
  // rows max(r0, k) .. r1 - 1, columns k + 1 .. N - 1: the update of step k-1, and the column sums of conj(v_i) a_ic
  const int wv = t >> 6, lane = t & 63;
  cd* cp = ws.colpart + (b * nblk + blk) * N;
  int chunk = 0;
  for (int j0 = k + 1; j0 < N; j0 += 64, ++chunk) {           // (uniform bounds: the barrier below is reached by all)
    const int j = j0 + lane;
    const bool jin = j < N;
    const cd wj = jin ? wp[j] : zero, cuj = jin ? cconj(up[j]) : zero;
    cd colacc = zero;
#pragma unroll
    for (int rr = 0; rr < ZBRD_ROWS / 4; ++rr) {
      const int i = r0 + wv + 4 * rr;
      if (i >= k && i < r1 && jin) {
        const cd x = csub(csub(A[(long)i * N + j], cmul(vps[i - r0], wj)), cmul(zps[i - r0], cuj));
        A[(long)i * N + j] = x;
        colacc = cadd(colacc, cmulc(x, ck[i]));
      }
    }
    cd* buf = &cw[chunk & 1][0][0];
    buf[wv * 64 + lane] = colacc;
    __syncthreads();                                          // one per chunk: the buffers alternate
    if (t < 64 && jin) cp[j] = cadd(cadd(cadd(buf[lane], buf[64 + lane]), buf[128 + lane]), buf[192 + lane]);
  }
  // the tail of u_{k-1} takes its place in row k-1, which R_{k-1} was the last to read
  if (k > 0 && k - 1 >= r0 && k - 1 < r1)
    for (int j = k + 1 + t; j < N; j += ZBRD_T) A[(long)(k - 1) * N + j] = up[j];
}

// R_k; grid (nblk, members), 256 threads, 32 N bytes of dynamic LDS
__global__ __launch_bounds__(ZBRD_T) void zgebrd_right(cd* __restrict__ F, int M, int N, int k, ZbrdWs ws) {
  extern __shared__ __attribute__((aligned(16))) char zbrd_smem[];
  __shared__ cd vks[ZBRD_ROWS];
  __shared__ double red[8];
  cd* w = reinterpret_cast<cd*>(zbrd_smem);                   // [N]
  cd* u = w + N;                                              // [N]
  const int t = threadIdx.x, blk = blockIdx.x, nblk = gridDim.x;
  const long b = blockIdx.y;
  const int r0 = blk * ZBRD_ROWS, r1 = min(M, r0 + ZBRD_ROWS);
  const bool last = blk == nblk - 1;
  if (r1 <= k + 1 && !last) return;                           // rows <= k are finished
  cd* A = F + b * M * N;
  const cd* vk = ws.vd + (b * 2 + (k & 1)) * M;
  const cd zero = cmk(0.0, 0.0), one = cmk(1.0, 0.0);
  if (t < ZBRD_ROWS && r0 + t < M) vks[t] = vk[r0 + t];
  // the tail of v_k takes the place of column k, which L_k was the last to read (tauq = 0: the tail is zero already, or not finite)
  const cd tq = ws.tauq[b * N + k];
  if (tq.x != 0.0 || tq.y != 0.0)
    for (int i = max(r0, k + 1) + t; i < r1; i += ZBRD_T) A[(long)i * N + k] = vk[i];
  if (k + 1 >= N) {
    if (last && t == 0) ws.taup[b * N + k] = zero;
    return;
  }
  // w from the partials of the blocks that hold rows >= k, in block order; row k of A - v w and its reflector
  const cd ctau = cconj(tq);
  const cd* cp = ws.colpart + b * nblk * N;
  cd rn = zero;
  for (int j = k + 1 + t; j < N; j += ZBRD_T) {
    const int q0 = k / ZBRD_ROWS;
    cd s = cp[(long)q0 * N + j];
    for (int q = q0 + 1; q < nblk; ++q) s = cadd(s, cp[(long)q * N + j]);
    const cd wj = cmul(ctau, s);
    w[j] = wj;
    const cd x = csub(A[(long)k * N + j], wj);
    u[j] = x;
    if (j > k + 1) rn = cadd(rn, zbrd_sq(x));
  }
  rn = het_block_sum(rn, red);                                // (its barriers publish w and the row)
  const HetRefl g = zbrd_reflect(cconj(u[k + 1]), rn, red, [&](double c) {
    double a2 = 0.0;
    for (int j = k + 2 + t; j < N; j += ZBRD_T) { const double xr = c * u[j].x, xi = c * u[j].y; a2 += xr * xr + xi * xi; }
    return a2;
  });
  __syncthreads();
  for (int j = k + 1 + t; j < N; j += ZBRD_T) {               // (each thread rewrites the entries it read)
    const cd x = j == k + 1 ? one : (g.on ? cdiv_re(cconj(u[j]), g.div) : zero);
    u[j] = x;
    if (last) { ws.u[b * N + j] = x; ws.w[b * N + j] = w[j]; }
  }
  if (last && t == 0) { ws.esc[b * N + k] = g.beta; ws.taup[b * N + k] = g.tau; }
  __syncthreads();
  // rows max(r0, k + 1) .. r1 - 1: z = taup (A - v w) u by rows
  const int wv = t >> 6, lane = t & 63;
  cd rowacc[ZBRD_ROWS / 4];
#pragma unroll
  for (int rr = 0; rr < ZBRD_ROWS / 4; ++rr) rowacc[rr] = zero;
  for (int j0 = k + 1; j0 < N; j0 += 64) {
    const int j = j0 + lane;
    if (j < N) {
      const cd wj = w[j], uj = u[j];
#pragma unroll
      for (int rr = 0; rr < ZBRD_ROWS / 4; ++rr) {
        const int i = r0 + wv + 4 * rr;
        if (i > k && i < r1) rowacc[rr] = cadd(rowacc[rr], cmul(csub(A[(long)i * N + j], cmul(vks[i - r0], wj)), uj));
      }
    }
  }
  cd* zo = ws.z + b * M;
#pragma unroll
  for (int rr = 0; rr < ZBRD_ROWS / 4; ++rr) {
    cd x = rowacc[rr];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { x.x += __shfl_xor(x.x, off); x.y += __shfl_xor(x.y, off); }
    const int i = r0 + wv + 4 * rr;
    if (lane == 0 && i > k && i < r1) zo[i] = cmul(g.tau, x);
  }
}

// after the last launch: d and e onto F's diagonals and into their own arrays; grid (members)
__global__ __launch_bounds__(ZBRD_T) void zgebrd_finish(cd* __restrict__ F, int M, int N, ZbrdWs ws, const u64* __restrict__ mx, double* __restrict__ d,
                                                        double* __restrict__ e, int unscale) {
  const long b = blockIdx.x;
  const int e1 = unscale ? syev_exp(mx[b]) : 0;
  cd* f = F + b * M * N;
  for (int i = threadIdx.x; i < N; i += ZBRD_T) {
    const double di = ldexp(ws.dsc[b * N + i], e1);
    f[(long)i * N + i] = cmk(di, 0.0);
    d[b * N + i] = di;
    if (i + 1 < N) {
      const double ei = ldexp(ws.esc[b * N + i], e1);
      f[(long)i * N + i + 1] = cmk(ei, 0.0);
      e[b * (N - 1) + i] = ei;
    }
  }
}

// ---- the small kernels of the routes --------------------------------------------------------------------------------------------
// Fp [members, N, N]: Fp[i][j] = F[j-1][i] for i > j >= 1, zero elsewhere; tp [members, N] = (0, taup_0 .. taup_{N-2}). F [.., M, N] and taup
// members sF and sT apart. grid (tiles of 256 over N N, members)
__global__ __launch_bounds__(ZBRD_T) void zunmbr_repack(const cd* __restrict__ F, long sF, const cd* __restrict__ taup, long sT, int N,
                                                        cd* __restrict__ Fp, cd* __restrict__ tp) {
  const long idx = (long)blockIdx.x * ZBRD_T + threadIdx.x, b = blockIdx.y;
  if (idx >= (long)N * N) return;
  const int i = (int)(idx / N), j = (int)(idx - (long)i * N);
  Fp[b * N * N + idx] = (j >= 1 && i > j) ? F[b * sF + (long)(j - 1) * N + i] : cmk(0.0, 0.0);
  if (i == 0) tp[b * N + j] = j == 0 ? cmk(0.0, 0.0) : taup[b * sT + j - 1];
}

// D [members, cols, rows] = S^H for S [members, rows, cols]; 32 x 32 tiles through LDS, grid (tiles of cols, tiles of rows, members)
__global__ __launch_bounds__(ZBRD_T) void zbrd_conj_transpose(const cd* __restrict__ S, cd* __restrict__ D, int rows, int cols) {
  __shared__ cd tile[32][33];
  const int c0 = blockIdx.x * 32, q0 = blockIdx.y * 32, c = threadIdx.x & 31;
  const cd* s = S + (long)blockIdx.z * rows * cols;
  cd* dm = D + (long)blockIdx.z * rows * cols;
  for (int r = threadIdx.x >> 5; r < 32; r += 8)
    if (q0 + r < rows && c0 + c < cols) tile[r][c] = s[(long)(q0 + r) * cols + c0 + c];
  __syncthreads();
  for (int r = threadIdx.x >> 5; r < 32; r += 8)
    if (c0 + r < cols && q0 + c < rows) dm[(long)(c0 + r) * rows + q0 + c] = cconj(tile[c][r]);
}

// D [members, rows, cols] complex from the top `top` rows, zero below: mode 0: of the real S [members, top, cols]; 1: of the complex S
// [members, top, cols]; 2: the upper triangle of the complex S [members, >= top, cols] (members sS apart). grid (tiles of 256, members)
__global__ __launch_bounds__(ZBRD_T) void zbrd_widen(int mode, const double* __restrict__ S, long sS, cd* __restrict__ D, int rows, int cols, int top) {
  const long idx = (long)blockIdx.x * ZBRD_T + threadIdx.x, b = blockIdx.y;
  if (idx >= (long)rows * cols) return;
  const int i = (int)(idx / cols), j = (int)(idx - (long)i * cols);
  cd x = cmk(0.0, 0.0);
  if (i < top) {
    if (mode == 0) x = cmk(S[b * sS + idx], 0.0);
    else if (mode == 1 || j >= i) x = reinterpret_cast<const cd*>(S)[b * sS + idx];
  }
  D[b * rows * cols + idx] = x;
}

// sv [members, k] *= 2^e1
__global__ __launch_bounds__(ZBRD_T) void zbrd_unscale(double* __restrict__ sv, long k, long total, const u64* __restrict__ mx) {
  const long i = (long)blockIdx.x * ZBRD_T + threadIdx.x;
  if (i < total) sv[i] = ldexp(sv[i], syev_exp(mx[i / k]));
}

// ---- host side ------------------------------------------------------------------------------------------------------------------
inline const cd* ccd(const double* p) { return reinterpret_cast<const cd*>(p); }
inline cd* mcd(double* p) { return reinterpret_cast<cd*>(p); }
inline const double* cdb(const cd* p) { return reinterpret_cast<const double*>(p); }
inline double* mdb(cd* p) { return reinterpret_cast<double*>(p); }
inline bool zbrd_al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
inline unsigned zbrd_tiles(int64_t n, int per) { return (unsigned)((n + per - 1) / per); }

int zbrd_attr(const void* fn, size_t lds) {
  if (lds > 64 * 1024) ND4_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  return 0;
}
template <class T> int zbrd_alloc(nd4hip_handle* h, size_t n, T** out) {
  void* p = nullptr;
  ND4_TRY(nd4_ws_alloc(h, sizeof(T) * (n ? n : 1), &p));
  *out = static_cast<T*>(p);
  return 0;
}
int zbrd_read_flag(nd4hip_handle* h, const int* flag, int* value) {
  void* hp = nullptr;
  ND4_TRY(nd4_pinned(h, sizeof(int), &hp));
  ND4_HIP(hipMemcpyAsync(hp, flag, sizeof(int), hipMemcpyDeviceToHost, h->stream));
  ND4_HIP(hipStreamSynchronize(h->stream));
  *value = *static_cast<int*>(hp);
  return 0;
}

inline size_t zbrd_small_lds(int64_t M, int64_t N) { return 16 * (size_t)(M * (N | 1) + 2 * M + 6 * N + 256) + 96; }
inline int64_t zbrd_blocks(int64_t M) { return (M + ZBRD_ROWS - 1) / ZBRD_ROWS; }
// complex elements of tier B's workspace per member: vd, z, w, u, colpart, and dsc, esc as one complex row
inline int64_t zbrd_ws_elems(int64_t M, int64_t N) { return 3 * M + 2 * N + zbrd_blocks(M) * N + N; }

// F, tauq, taup, d, e of nbm <= 32768 members from A; mx [nbm] and *flag ZERO on entry. Allocates from the caller's scope; enqueues only
int zbrd_factor(nd4hip_handle* h, int64_t nbm, int M, int N, const cd* A, cd* F, cd* tauq, cd* taup, double* d, double* e, u64* mx, bool unscale,
                int* flag) {
  if (nd4_zgebrd_tier(M, N) == 0) {
    const size_t lds = zbrd_small_lds(M, N);
    ND4_TRY(zbrd_attr(reinterpret_cast<const void*>(&zgebrd_small), lds));
    hipLaunchKernelGGL(zgebrd_small, dim3((unsigned)nbm), dim3(ZBRD_T), lds, h->stream, A, F, tauq, taup, d, e, mx, M, N, unscale ? 1 : 0, flag);
    ND4_HIP(hipGetLastError());
    return 0;
  }
  const int nblk = (int)zbrd_blocks(M);
  const long mn = (long)M * N;
  ZbrdWs ws;
  ws.tauq = tauq; ws.taup = taup;
  ND4_TRY(zbrd_alloc(h, (size_t)nbm * N, &ws.dsc)); ND4_TRY(zbrd_alloc(h, (size_t)nbm * N, &ws.esc));
  cd* pend = nullptr;                                         // vd, z, w, u in one block: cleared together
  const size_t pn = (size_t)nbm * (3 * (size_t)M + 2 * (size_t)N);
  ND4_TRY(zbrd_alloc(h, pn, &pend));
  ws.vd = pend; ws.z = ws.vd + (size_t)nbm * 2 * M; ws.w = ws.z + (size_t)nbm * M; ws.u = ws.w + (size_t)nbm * N;
  ND4_TRY(zbrd_alloc(h, (size_t)nbm * nblk * N, &ws.colpart));
  hipLaunchKernelGGL(zbrd_absmax, dim3(256u, (unsigned)nbm), dim3(ZBRD_T), 0, h->stream, A, mn, mx, flag);
  hipLaunchKernelGGL(zbrd_load, dim3(zbrd_tiles(mn, ZBRD_T), (unsigned)nbm), dim3(ZBRD_T), 0, h->stream, A, F, mn, mx);
  hipLaunchKernelGGL(zbrd_clear, dim3(zbrd_tiles((int64_t)pn, ZBRD_T)), dim3(ZBRD_T), 0, h->stream, pend, (long)pn);
  ND4_HIP(hipGetLastError());
  const size_t ldsl = 16 * (size_t)M, ldsr = 32 * (size_t)N;
  ND4_TRY(zbrd_attr(reinterpret_cast<const void*>(&zgebrd_left), ldsl));
  ND4_TRY(zbrd_attr(reinterpret_cast<const void*>(&zgebrd_right), ldsr));
  const dim3 grid((unsigned)nblk, (unsigned)nbm);
  for (int k = 0; k < N; ++k) {
    hipLaunchKernelGGL(zgebrd_left, grid, dim3(ZBRD_T), ldsl, h->stream, F, M, N, k, ws);
    hipLaunchKernelGGL(zgebrd_right, grid, dim3(ZBRD_T), ldsr, h->stream, F, M, N, k, ws);
  }
  hipLaunchKernelGGL(zgebrd_finish, dim3((unsigned)nbm), dim3(ZBRD_T), 0, h->stream, F, M, N, ws, mx, d, e, unscale ? 1 : 0);
  ND4_HIP(hipGetLastError());
  return 0;
}

// Z [nbm, N, K] <- P Z or P^H Z in place; F [.., M, N] and taup members sF, sT apart (0: one for all)
int zbrd_apply_p(nd4hip_handle* h, int64_t nbm, int N, int K, bool adjoint, const cd* F, int64_t sF, const cd* taup, int64_t sT, cd* Z) {
  if (N < 2) return 0;                                        // P = I
  Nd4WsScope scope(h);
  const int64_t nf = sF ? nbm : 1;
  cd *Fp = nullptr, *tp = nullptr;
  ND4_TRY(zbrd_alloc(h, (size_t)(nf * N * N), &Fp));
  ND4_TRY(zbrd_alloc(h, (size_t)(nf * N), &tp));
  hipLaunchKernelGGL(zunmbr_repack, dim3(zbrd_tiles((int64_t)N * N, ZBRD_T), (unsigned)nf), dim3(ZBRD_T), 0, h->stream, F, (long)sF, taup, (long)sT, N, Fp,
                     tp);
  ND4_HIP(hipGetLastError());
  return nd4_zunmqr(h, nbm, N, N, K, adjoint, cdb(Fp), sF ? (int64_t)N * N : 0, cdb(tp), sF ? N : 0, mdb(Z));
}

int zbrd_transpose(nd4hip_handle* h, int64_t nbm, const cd* S, cd* D, int rows, int cols) {
  hipLaunchKernelGGL(zbrd_conj_transpose, dim3(zbrd_tiles(cols, 32), zbrd_tiles(rows, 32), (unsigned)nbm), dim3(ZBRD_T), 0, h->stream, S, D, rows, cols);
  ND4_HIP(hipGetLastError());
  return 0;
}
int zbrd_widen_launch(nd4hip_handle* h, int64_t nbm, int mode, const double* S, int64_t sS, cd* D, int rows, int cols, int top) {
  hipLaunchKernelGGL(zbrd_widen, dim3(zbrd_tiles((int64_t)rows * cols, ZBRD_T), (unsigned)nbm), dim3(ZBRD_T), 0, h->stream, mode, S, (long)sS, D, rows, cols,
                     top);
  ND4_HIP(hipGetLastError());
  return 0;
}

}  // namespace

// ---- the host-side arithmetic of the tiers (tools/zsvd_host_check.hip) ----
// 0: a member in LDS, 1: two launches per column
int nd4_zgebrd_tier(int64_t M, int64_t N) { return zbrd_small_lds(M, N) <= ZBRD_LDS ? 0 : 1; }
// the largest dynamic LDS request of the reduction at this shape
size_t nd4_zgebrd_lds(int64_t M, int64_t N) {
  if (nd4_zgebrd_tier(M, N) == 0) return zbrd_small_lds(M, N);
  return 16 * (size_t)M > 32 * (size_t)N ? 16 * (size_t)M : 32 * (size_t)N;
}
// members per pass: at most 32768, and `extra` + tier B's workspace complex elements per member within about 1 GiB
int64_t nd4_zgebrd_chunk(int64_t batch, int64_t M, int64_t N, int64_t extra) {
  const int64_t per = extra + (nd4_zgebrd_tier(M, N) == 1 ? zbrd_ws_elems(M, N) : 0);
  int64_t c = ZBRD_CHUNK;
  if (per > 0 && ZBRD_WS_ELEMS / per < c) c = ZBRD_WS_ELEMS / per;
  if (c < 1) c = 1;
  return batch < c ? batch : c;
}
// does the SVD of a tall m x n member go through QR first? 2 m n^2 + 2 n^3 flops beat 4 m n^2 - 4 n^3 / 3 from m = 5 n / 3
bool nd4_zgesdd_qr_first(int64_t m, int64_t n) { return m > n && 3 * m >= 5 * n; }

#define ZBRD_CHECK_SHAPE(op, M, N)                                                                                  \
  ND4_CHECK_ARG((N) >= 1 && (N) <= (M) && (M) <= ZBRD_MAXN, "nd4hip_" op "_batched: 1 <= N <= M <= 2048")

// zbidiag_factor: arguments already checked, batch >= 1. Synchronises once per pass (the flag word): NaN or Inf in A is ND4HIP_ERR_NOCONV
// with `what`'s text
int nd4_zgebrd(nd4hip_handle* h, int64_t batch, int64_t M64, int64_t N64, const double* A, double* F, double* tauq, double* taup, double* d,
               double* e, const char* what) {
  ZBRD_CHECK_SHAPE("zgebrd", M64, N64);
  ND4_CHECK_ARG(zbrd_al16(A) && zbrd_al16(F) && zbrd_al16(tauq) && zbrd_al16(taup), "nd4hip_zgebrd_batched: complex operands must be 16-byte aligned");
  const int M = (int)M64, N = (int)N64;
  const int64_t mn = M64 * N64, chunk = nd4_zgebrd_chunk(batch, M, N, 0);
  for (int64_t b0 = 0; b0 < batch; b0 += chunk) {
    const int64_t nbm = batch - b0 < chunk ? batch - b0 : chunk;
    Nd4WsScope scope(h);
    u64* mx = nullptr; int* flag = nullptr; int bad = 0;
    ND4_TRY(zbrd_alloc(h, (size_t)nbm, &mx)); ND4_TRY(zbrd_alloc(h, 1, &flag));
    ND4_HIP(hipMemsetAsync(mx, 0, sizeof(u64) * (size_t)nbm, h->stream));
    ND4_HIP(hipMemsetAsync(flag, 0, sizeof(int), h->stream));
    ND4_TRY(zbrd_factor(h, nbm, M, N, ccd(A) + b0 * mn, mcd(F) + b0 * mn, mcd(tauq) + b0 * N64, mcd(taup) + b0 * N64, d + b0 * N64,
                        e + b0 * (N64 - 1), mx, true, flag));
    ND4_TRY(zbrd_read_flag(h, flag, &bad));
    if (bad) {
      nd4_set_error("%s: A contains NaN or Infinity.", what);
      return ND4HIP_ERR_NOCONV;
    }
  }
  return 0;
}

// zbidiag_apply_p: Z [batch, N, K] <- P Z (adjoint: P^H Z) in place; F [.., M, N] and taup [.., N] members sF, sT apart (0: one for all).
// Enqueues only
int nd4_zunmbr_p(nd4hip_handle* h, int64_t batch, int64_t M64, int64_t N64, int64_t K64, bool adjoint, const double* F, int64_t sF, const double* taup,
                 int64_t sT, double* Z) {
  ZBRD_CHECK_SHAPE("zunmbr_p", M64, N64);
  ND4_CHECK_ARG(zbrd_al16(F) && zbrd_al16(taup) && zbrd_al16(Z), "nd4hip_zunmbr_p_batched: complex operands must be 16-byte aligned");
  const int N = (int)N64, K = (int)K64;
  const int64_t chunk = nd4_zgebrd_chunk(batch, 1, 1, N64 * N64 + N64);
  for (int64_t b0 = 0; b0 < batch; b0 += chunk) {
    const int64_t nbm = batch - b0 < chunk ? batch - b0 : chunk;
    ND4_TRY(zbrd_apply_p(h, nbm, N, K, adjoint, ccd(F) + b0 * sF, sF, ccd(taup) + b0 * sT, sT, mcd(Z) + b0 * N64 * K64));
  }
  return 0;
}

// zsvd_decomp / zsvd_vals: the triplets i0 <= i < i1 of the descending spectrum of A [batch, M, N], k = i1 - i0: sv [batch, k] and, unless
// both are NULL, U [batch, M, k] and V [batch, k, N] with A = U diag(sv) V. Arguments already checked, batch >= 1, 1 <= M, N <= 2048.
// Synchronises (the flag word and the real solvers)
int nd4_zgesdd(nd4hip_handle* h, int64_t batch, int64_t M64, int64_t N64, int64_t i0, int64_t i1, const double* A, double* U, double* sv,
               double* V) {
  ND4_CHECK_ARG(M64 >= 1 && N64 >= 1 && M64 <= ZBRD_MAXN && N64 <= ZBRD_MAXN, "nd4hip_zgesdd_batched: 1 <= M, N <= 2048");
  ND4_CHECK_ARG(zbrd_al16(A) && zbrd_al16(U) && zbrd_al16(V), "nd4hip_zgesdd_batched: complex operands must be 16-byte aligned");
  const bool wide = M64 < N64, vectors = U != nullptr;
  const int m = (int)(wide ? N64 : M64), n = (int)(wide ? M64 : N64), k = (int)(i1 - i0);   // the tall problem that is solved
  const bool qr = nd4_zgesdd_qr_first(m, n), all = vectors && k == n;
  const int mb = qr ? n : m;                                    // rows of what is bidiagonalised
  const int64_t mn = (int64_t)m * n, bn = (int64_t)mb * n;
  // complex elements per member: A^H, the QR factor and R, F, the three scalar rows and d, e; the vectors in their stages
  const int64_t per = (wide ? mn : 0) + (qr ? mn + n + bn : 0) + bn + 4 * (int64_t)n +
                      (vectors ? (int64_t)n * k * 2 + (int64_t)m * k + (int64_t)n * (all ? n : k) : 0);
  const int64_t chunk = nd4_zgebrd_chunk(batch, mb, n, per);
  for (int64_t b0 = 0; b0 < batch; b0 += chunk) {
    const int64_t nbm = batch - b0 < chunk ? batch - b0 : chunk;
    Nd4WsScope scope(h);
    const cd* a = ccd(A) + b0 * mn;
    cd *At = nullptr, *Fq = nullptr, *tqr = nullptr, *R = nullptr, *F = nullptr, *tauq = nullptr, *taup = nullptr;
    double *d = nullptr, *e = nullptr, *U2 = nullptr, *V2 = nullptr;
    u64* mx = nullptr; int* flag = nullptr; int bad = 0;
    ND4_TRY(zbrd_alloc(h, (size_t)nbm, &mx)); ND4_TRY(zbrd_alloc(h, 1, &flag));
    ND4_TRY(zbrd_alloc(h, (size_t)(nbm * bn), &F)); ND4_TRY(zbrd_alloc(h, (size_t)(nbm * n), &tauq)); ND4_TRY(zbrd_alloc(h, (size_t)(nbm * n), &taup));
    ND4_TRY(zbrd_alloc(h, (size_t)(nbm * n), &d)); ND4_TRY(zbrd_alloc(h, (size_t)(nbm * n), &e));
    ND4_HIP(hipMemsetAsync(mx, 0, sizeof(u64) * (size_t)nbm, h->stream));
    ND4_HIP(hipMemsetAsync(flag, 0, sizeof(int), h->stream));
    if (wide) {
      ND4_TRY(zbrd_alloc(h, (size_t)(nbm * mn), &At));
      ND4_TRY(zbrd_transpose(h, nbm, a, At, n, m));
      a = At;
    }
    if (qr) {
      ND4_TRY(zbrd_alloc(h, (size_t)(nbm * mn), &Fq)); ND4_TRY(zbrd_alloc(h, (size_t)(nbm * n), &tqr)); ND4_TRY(zbrd_alloc(h, (size_t)(nbm * bn), &R));
      // (NaN or Inf: the flag comes from A itself; this first maximum is then cleared for the one of R)
      hipLaunchKernelGGL(zbrd_absmax, dim3(256u, (unsigned)nbm), dim3(ZBRD_T), 0, h->stream, a, (long)mn, mx, flag);
      ND4_HIP(hipGetLastError());
      ND4_HIP(hipMemsetAsync(mx, 0, sizeof(u64) * (size_t)nbm, h->stream));
      ND4_TRY(nd4_zgeqrf(h, nbm, m, n, cdb(a), mdb(Fq), mdb(tqr)));
      ND4_TRY(zbrd_widen_launch(h, nbm, 2, cdb(Fq), mn, R, n, n, n));
      a = R;
    }
    ND4_TRY(zbrd_factor(h, nbm, mb, n, a, F, tauq, taup, d, e, mx, false, flag));
    ND4_TRY(zbrd_read_flag(h, flag, &bad));
    if (bad) {
      nd4_set_error("zsvd_decomp(A): A contains NaN or Infinity.");
      return ND4HIP_ERR_NOCONV;
    }
    double* svo = sv + b0 * k;
    if (all) {
      ND4_TRY(zbrd_alloc(h, (size_t)(nbm * n * n), &U2)); ND4_TRY(zbrd_alloc(h, (size_t)(nbm * n * n), &V2));
      ND4_TRY(nd4_bdsdc_rows(h, nbm, n, n, d, e, U2, svo, V2));
    } else {
      if (vectors) { ND4_TRY(zbrd_alloc(h, (size_t)(nbm * n * k), &U2)); ND4_TRY(zbrd_alloc(h, (size_t)(nbm * k * n), &V2)); }
      ND4_TRY(nd4_bdsvdx(h, nbm, n, n, i0, i1, d, e, U2, svo, V2, nullptr));
    }
    hipLaunchKernelGGL(zbrd_unscale, dim3(zbrd_tiles(nbm * k, ZBRD_T)), dim3(ZBRD_T), 0, h->stream, svo, (long)k, (long)(nbm * k), mx);
    ND4_HIP(hipGetLastError());
    if (!vectors) continue;
    // the left vectors of the tall problem: Q [U2; 0] as [m, k], into U, or into workspace for V = (...)^H of a wide member
    cd *Ut = mcd(U) + b0 * m * k, *Vc = nullptr, *Ub = nullptr;
    if (wide) ND4_TRY(zbrd_alloc(h, (size_t)(nbm * m * k), &Ut));
    if (qr) {
      ND4_TRY(zbrd_alloc(h, (size_t)(nbm * n * k), &Ub));
      ND4_TRY(zbrd_widen_launch(h, nbm, 0, U2, (int64_t)n * k, Ub, n, k, n));
      ND4_TRY(nd4_zunmqr(h, nbm, n, n, k, false, cdb(F), bn, cdb(tauq), n, mdb(Ub)));
      ND4_TRY(zbrd_widen_launch(h, nbm, 1, cdb(Ub), (int64_t)n * k, Ut, m, k, n));
      ND4_TRY(nd4_zunmqr(h, nbm, m, n, k, false, cdb(Fq), mn, cdb(tqr), n, mdb(Ut)));
    } else {
      ND4_TRY(zbrd_widen_launch(h, nbm, 0, U2, (int64_t)n * k, Ut, m, k, n));
      ND4_TRY(nd4_zunmqr(h, nbm, m, n, k, false, cdb(F), bn, cdb(tauq), n, mdb(Ut)));
    }
    // the right vectors as columns: P V2^T [n, k], into U of a wide member, else into workspace for V = (...)^H
    if (wide) Vc = mcd(U) + b0 * n * k; else ND4_TRY(zbrd_alloc(h, (size_t)(nbm * n * k), &Vc));
    ND4_TRY(nd4_hetrd_rows_to_columns(h, nbm, n, k, V2, mdb(Vc)));
    ND4_TRY(zbrd_apply_p(h, nbm, n, k, false, F, bn, taup, n, Vc));
    cd* Vo = mcd(V) + b0 * k * (wide ? m : n);
    if (wide) ND4_TRY(zbrd_transpose(h, nbm, Ut, Vo, m, k)); else ND4_TRY(zbrd_transpose(h, nbm, Vc, Vo, n, k));
  }
  return 0;
}
