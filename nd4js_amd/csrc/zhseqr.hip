// Complex128 Schur form and eigenpairs on the device: zschur_qr / zschur_decomp / zschur_eigen / zeigen / zeigenvals,
// LAPACK's zlahqr / zgees / ztrevc / zgeev (without balancing) on row-major members, interleaved (re, im) doubles, 1 <= N <= 1024.
//   zhseqr_k: the single-shift implicit QR iteration, one workgroup of 256 threads per member, nothing waits on another workgroup.
//     H is scaled on load by 2^-e1 (max(|Re|, |Im|) in [0.5, 1)) and T gets 2^e1 back on its store, exactly.
//     Scalar decisions are taken by every lane from the same values, so nothing is broadcast: the Wilkinson shift of the trailing 2 x 2
//     block of the active window [l, i], zlahqr's exceptional shifts (0.75 |h_{l+1,l}| + h_ll, 0.75 |h_{i,i-1}| + h_ii) at every 10th
//     iteration without a deflation, each Givens rotation (c real, s complex). The deflation scan is the one exception to "every lane
//     the same work": the lanes test the subdiagonal of the window 256 entries at a time (|h_{k,k-1}| <= eps (|h_{k-1,k-1}| + |h_kk|)
//     in the |Re| + |Im| modulus) and the largest such k is a maximum of integers over the workgroup. A deflated entry is set to 0.
//     Window now, rest once per sweep: rotation k of the chase is applied at once only inside the window (rows l..i, columns l..i): the
//     row pair k, k+1 right of the 2 x 2 block on the diagonal, the column pair above it, and the block itself with the bulge by one
//     lane, in ONE pass of the 256 lanes and ONE barrier per rotation (the pair (r, 0) that the rotation leaves in column k-1 is
//     written a step late, when no lane reads it any more). (c, s) goes into an LDS buffer. At the end of the sweep the recorded
//     sequence is applied to the parts the chase never reads: H[l..i, i+1..N-1] (one lane per column walking down the rows),
//     H[0..l-1, l..i] and Q[:, l..i] (one lane per row walking along the columns, no barrier between rotations). Rows of Q, and of H when
//     it is in global memory, are staged through LDS in tiles of TR rows x 33 columns, so that global memory is read and written
//     along rows: that holds for this per-sweep pass only; inside the window the column pair above the block is walked one lane per
//     row at every rotation, a stride-N walk when H is in global memory. want_t = 0 (zeigenvals) skips the three parts and never forms Q.
//     Measured, the deferral lost 1 - 3 % to applying every rotation to the full rows, columns and Q at once at 64 x 256^2
//     and 512^2, so the global-memory tier applies at once ("eager", the same bits) and only the LDS tier, where eager would walk Q in
//     global memory at every rotation, defers. ND4HIP_ZHSEQR_EAGER=0 / 1 forces either form for the measurement.
//     Tiers by what fits: H in LDS at the odd pitch N | 1 while 16 N (N | 1) + 24 N + 16 * 33 * 64 <= 163776: N <= 89 (162664 bytes;
//     tile rows TR = 16 / 32 / 64 for N <= 16 / 32 / 89). A workgroup then owns a CU: 256 members run at a time. Above, H is in
//     global memory with the same code and TR = 256 (135168 + 24 N bytes). A member stops after 30 max(10, N) sweeps
//     (ND4HIP_EV_FLAG_NOCONV); NaN or Inf is seen in the maximum before anything iterates: every loop is bounded for every input.
//   ztrevc_k (N <= 64): (T[0:k, 0:k] - t_kk I) x = -T[0:k, k], x_k = 1, by back-substitution on the scaled T: one lane per column k,
//     the four waves of the workgroup split the rows of each axpy; ztrevc's pivot floor smin = max(eps |t_kk|, smallnum) and an
//     overflow guard that rescales a column by a power of two. X's columns leave with their maximum in [0.5, 1); V = Q X on nd4_zgemm,
//     then every column is scaled to unit 2-norm (zeig_unit_k, sums in a fixed order).
//   Above N = 64 the blocked form, nb = 64 as in eigvec.hip: ztrevc_init_k writes the scaled Ts and X = I; for the block rows
//     from the last, ztrevc_diag_k solves the 64 rows of every column block right of the diagonal in LDS (the same lane-per-column
//     step, pivot floor and guard), then X[0:r0, r0:] -= Ts[0:r0, block] X[block, r0:] runs on the fp64 matrix cores (zlu_update of
//     zgetrf.hip); ztrevc_scale_k brings the columns' maxima into [0.5, 1). Both Q and T are screened for NaN or Inf.
// No atomics on doubles; every new kernel uses 0 scratch. The file is built without FMA contraction.
#include "nd4hip_internal.h"
#include "zlarfg.h"
#include <cfloat>
#include <climits>
#include <cstdlib>
#include <cstring>

// zgehrd.hip
int nd4_zgehrd(nd4hip_handle* h, int64_t nbm, int64_t N, const double* A, double* F, double* tau, int64_t member0, int* flag);
int nd4_zeig_absmax(nd4hip_handle* h, int64_t nbm, int64_t count, const double* A, unsigned long long* mx, int64_t member0, int* flag);
int nd4_zeig_clear(nd4hip_handle* h, void* p, size_t bytes);
int nd4_zeig_read_flags(nd4hip_handle* h, const int* flags, int n, int* out);
int nd4_zhess_clean(nd4hip_handle* h, int64_t nbm, int N, const double* F, double* H);
int nd4_zeig_identity(nd4hip_handle* h, int64_t nbm, int N, double* Q);

namespace {

constexpr int ZHS_MAXN = 1024;
constexpr int ZHS_T = 256;
constexpr int ZHS_TC = 32, ZHS_TP = 33;          // staged tiles: 32 rotations per pass over 33 columns
constexpr size_t ZHS_LDS = 163840;
constexpr double ZHS_EPS = 0x1p-52;
constexpr size_t ZHS_TREVC_LDS = 2 * 16 * 64 * 65;   // ztrevc_diag_k: two 64 x 65 tiles

__device__ __forceinline__ double cabs1(cd a) { return fabs(a.x) + fabs(a.y); }
__device__ __forceinline__ cd cldexp(cd a, int e) { return cmk(ldexp(a.x, e), ldexp(a.y, e)); }
// a / b, Smith's form
__device__ __forceinline__ cd cdiv(cd a, cd b) {
  if (fabs(b.x) >= fabs(b.y)) { const double r = b.y / b.x, den = b.x + b.y * r; return cmk((a.x + a.y * r) / den, (a.y - a.x * r) / den); }
  const double r = b.x / b.y, den = b.y + b.x * r;
  return cmk((a.x * r + a.y) / den, (a.y * r - a.x) / den);
}
__device__ __forceinline__ cd csqrt_(cd z) {
  if (z.x == 0.0 && z.y == 0.0) return z;
  const double t = sqrt(0.5 * (fabs(z.x) + hypot(z.x, z.y)));
  return z.x >= 0.0 ? cmk(t, z.y / (2.0 * t)) : cmk(fabs(z.y) / (2.0 * t), z.y >= 0.0 ? t : -t);
}
// [c s; -conj(s) c] [f; g] = [r; 0], c real
struct ZhsRot { double c; cd s, r; };
__device__ __forceinline__ ZhsRot zhs_rot(cd f, cd g) {
  ZhsRot o;
  if (g.x == 0.0 && g.y == 0.0) { o.c = 1.0; o.s = cmk(0.0, 0.0); o.r = f; return o; }
  const double g1 = hypot(g.x, g.y);
  if (f.x == 0.0 && f.y == 0.0) { o.c = 0.0; o.s = cmk(g.x / g1, -g.y / g1); o.r = cmk(g1, 0.0); return o; }
  const double f1 = hypot(f.x, f.y), d = hypot(f1, g1);
  const cd ph = cmk(f.x / f1, f.y / f1);
  o.c = f1 / d;
  o.s = cmulc(ph, cmk(g.x / d, g.y / d));
  o.r = cscale(ph, d);
  return o;
}

// M[r][l..i] <- M[r][l..i] G_l^H ... G_{i-1}^H for the rows 0 <= r < nrows of the global M (row pitch `pitch`), staged through `tile`
// [TR][33]; every thread calls it
__device__ void zhs_right_staged(cd* M, long pitch, int nrows, int l, int i, const double* rc, const cd* rs, cd* tile, int TR) {
  const int t = threadIdx.x;
  for (int rb = 0; rb < nrows; rb += TR) {
    const int nr = min(TR, nrows - rb);
    for (int c0 = l; c0 < i; c0 += ZHS_TC) {
      const int ce = min(c0 + ZHS_TC, i), w = ce - c0 + 1;
      for (int idx = t; idx < nr * w; idx += ZHS_T) { const int r = idx / w, c = idx - r * w; tile[r * ZHS_TP + c] = M[(long)(rb + r) * pitch + c0 + c]; }
      __syncthreads();
      if (t < nr) {
        cd a = tile[t * ZHS_TP];
        for (int k = c0; k < ce; ++k) {
          const double c = rc[k - l];
          const cd s = rs[k - l], bb = tile[t * ZHS_TP + k - c0 + 1];
          tile[t * ZHS_TP + k - c0] = cadd(cscale(a, c), cmulc(bb, s));     // a c + b conj(s)
          a = csub(cscale(bb, c), cmul(s, a));                              // -s a + c b
        }
        tile[t * ZHS_TP + ce - c0] = a;
      }
      __syncthreads();
      for (int idx = t; idx < nr * w; idx += ZHS_T) { const int r = idx / w, c = idx - r * w; M[(long)(rb + r) * pitch + c0 + c] = tile[r * ZHS_TP + c]; }
      __syncthreads();
    }
  }
}

// grid (members), 256 threads. T [members, N, N]: H on entry (Hessenberg: what lies below the subdiagonal is not read), T on return;
// Q [members, N, N] in place, or NULL with want_t = 0. flags[1]: no convergence, INT_MAX - (the lowest such member)
__global__ __launch_bounds__(ZHS_T) void zhseqr_k(cd* Tg, cd* Qg, const u64* __restrict__ mx, int N, int in_lds, int TR, int want_t,
                                                  int eager, long member0, int* __restrict__ flags) {
  extern __shared__ __attribute__((aligned(16))) char zhs_smem[];
  __shared__ int redi[4];
  const int t = threadIdx.x;
  const long b = blockIdx.x;
  cd* rs = reinterpret_cast<cd*>(zhs_smem);                   // [N] the sweep's s
  cd* tile = rs + N;                                          // [TR][33]
  cd* Sl = tile + (size_t)TR * ZHS_TP;                        // [N][N | 1] in the LDS tier
  double* rc = reinterpret_cast<double*>(Sl + (in_lds ? (size_t)N * (N | 1) : 0));   // [N] the sweep's c
  cd* Tm = Tg + b * N * N;
  cd* Q = Qg ? Qg + b * N * N : nullptr;
  const u64 m = mx[b];
  if (m > SYEV_MAX_BITS) return;                              // (uniform) NaN or Inf: the flag is raised already
  const int e1 = syev_exp(m);
  const int P = in_lds ? (N | 1) : N;
  eager = eager && want_t;
  cd* S = in_lds ? Sl : Tm;
  const cd zero = cmk(0.0, 0.0);
  for (int idx = t; idx < N * N; idx += ZHS_T) {
    const int r = idx / N, c = idx - r * N;
    S[r * P + c] = c + 1 >= r ? cldexp(Tm[idx], -e1) : zero;
  }
  __syncthreads();
  const int budget = 30 * (N > 10 ? N : 10);
  int i = N - 1, its = 0, total = 0;
  bool failed = false;
  while (i >= 1) {
    // the deflation scan up the subdiagonal of rows i, i-1, .., 1
    int cand = 0;
    for (int k = i - t; k >= 1; k -= ZHS_T)
      if (cabs1(S[k * P + k - 1]) <= ZHS_EPS * (cabs1(S[(k - 1) * P + k - 1]) + cabs1(S[k * P + k]))) { cand = k; break; }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { const int o = __shfl_xor(cand, off); cand = o > cand ? o : cand; }
    __syncthreads();
    if ((t & 63) == 0) redi[t >> 6] = cand;
    __syncthreads();
    const int l = max(max(redi[0], redi[1]), max(redi[2], redi[3]));
    if (l > 0 && t == 0) S[l * P + l - 1] = zero;
    if (l == i) { --i; its = 0; continue; }
    if (total >= budget) { failed = true; break; }
    ++its; ++total;
    // the shift
    cd shift;
    if (its % 20 == 10) shift = cadd(S[l * P + l], cmk(0.75 * cabs1(S[(l + 1) * P + l]), 0.0));
    else if (its % 20 == 0) shift = cadd(S[i * P + i], cmk(0.75 * cabs1(S[i * P + i - 1]), 0.0));
    else {
      shift = S[i * P + i];
      const cd u = cmul(csqrt_(S[(i - 1) * P + i]), csqrt_(S[i * P + i - 1]));
      double s1 = cabs1(u);
      if (s1 != 0.0) {
        const cd x = cscale(csub(S[(i - 1) * P + i - 1], shift), 0.5);
        const double sx = cabs1(x);
        s1 = fmax(s1, sx);
        const cd xs = cscale(x, 1.0 / s1), us = cscale(u, 1.0 / s1);
        cd y = cscale(csqrt_(cadd(cmul(xs, xs), cmul(us, us))), s1);
        if (sx > 0.0 && (x.x / sx) * y.x + (x.y / sx) * y.y < 0.0) y = cmk(-y.x, -y.y);
        shift = csub(shift, cmul(u, cdiv(u, cadd(x, y))));
      }
    }
    cd f = csub(S[l * P + l], shift), g = S[(l + 1) * P + l];
    cd pend_r = zero;
    __syncthreads();                                          // the reads above precede the first rotation's writes
    for (int k = l; k < i; ++k) {
      if (k > l) { f = S[k * P + k - 1]; g = S[(k + 1) * P + k - 1]; }
      const ZhsRot G = zhs_rot(f, g);
      const double c = G.c;
      const cd s = G.s, cs = cconj(G.s);
      const int top = eager ? 0 : l;                          // eager: full rows, full columns and Q at every rotation
      const int ncol = (eager ? N - 1 : i) - k - 1, nrow = k - top, nq = eager ? N : 0;
      if (t == 0) {
        rc[k - l] = c; rs[k - l] = s;
        if (k > l + 1) { S[(k - 1) * P + k - 2] = pend_r; S[k * P + k - 2] = zero; }   // what rotation k-1 left in column k-2
      }
      pend_r = G.r;
      for (int idx = t; idx <= ncol + nrow + nq; idx += ZHS_T) {
        if (idx < ncol) {                                     // rows k, k+1 right of the block
          const int j = k + 2 + idx;
          const cd a = S[k * P + j], bb = S[(k + 1) * P + j];
          S[k * P + j] = cadd(cscale(a, c), cmul(s, bb));
          S[(k + 1) * P + j] = csub(cscale(bb, c), cmul(cs, a));
        } else if (idx < ncol + nrow) {                       // columns k, k+1 above the block
          const int r = top + idx - ncol;
          const cd a = S[r * P + k], bb = S[r * P + k + 1];
          S[r * P + k] = cadd(cscale(a, c), cmul(cs, bb));
          S[r * P + k + 1] = csub(cscale(bb, c), cmul(s, a));
        } else if (idx > ncol + nrow) {                       // (eager) columns k, k+1 of Q
          const int r = idx - ncol - nrow - 1;
          const cd a = Q[(long)r * N + k], bb = Q[(long)r * N + k + 1];
          Q[(long)r * N + k] = cadd(cscale(a, c), cmul(cs, bb));
          Q[(long)r * N + k + 1] = csub(cscale(bb, c), cmul(s, a));
        } else {                                              // the 2 x 2 block on the diagonal from both sides, and the bulge
          const cd a00 = S[k * P + k], a01 = S[k * P + k + 1], a10 = S[(k + 1) * P + k], a11 = S[(k + 1) * P + k + 1];
          const cd t00 = cadd(cscale(a00, c), cmul(s, a10)), t10 = csub(cscale(a10, c), cmul(cs, a00));
          const cd t01 = cadd(cscale(a01, c), cmul(s, a11)), t11 = csub(cscale(a11, c), cmul(cs, a01));
          S[k * P + k] = cadd(cscale(t00, c), cmul(cs, t01));
          S[k * P + k + 1] = csub(cscale(t01, c), cmul(s, t00));
          S[(k + 1) * P + k] = cadd(cscale(t10, c), cmul(cs, t11));
          S[(k + 1) * P + k + 1] = csub(cscale(t11, c), cmul(s, t10));
          if (k + 2 <= i) {
            const cd b2 = S[(k + 2) * P + k + 1];
            S[(k + 2) * P + k] = cmul(cs, b2);
            S[(k + 2) * P + k + 1] = cscale(b2, c);
          }
        }
      }
      __syncthreads();
    }
    if (t == 0 && i - 1 > l) { S[(i - 1) * P + i - 2] = pend_r; S[i * P + i - 2] = zero; }
    if (want_t && !eager) {
      // the columns right of the window: G_{i-1} ... G_l from the left, one lane per column
      for (int j = i + 1 + t; j < N; j += ZHS_T) {
        cd a = S[l * P + j];
        for (int k = l; k < i; ++k) {
          const double c = rc[k - l];
          const cd s = rs[k - l], bb = S[(k + 1) * P + j];
          S[k * P + j] = cadd(cscale(a, c), cmul(s, bb));
          a = csub(cscale(bb, c), cmulc(a, s));               // -conj(s) a + c b
        }
        S[i * P + j] = a;
      }
      // the rows above the window and the columns l..i of Q: G_l^H ... G_{i-1}^H from the right, one lane per row
      if (in_lds) {
        for (int r = t; r < l; r += ZHS_T) {
          cd a = S[r * P + l];
          for (int k = l; k < i; ++k) {
            const double c = rc[k - l];
            const cd s = rs[k - l], bb = S[r * P + k + 1];
            S[r * P + k] = cadd(cscale(a, c), cmulc(bb, s));
            a = csub(cscale(bb, c), cmul(s, a));
          }
          S[r * P + i] = a;
        }
      } else {
        zhs_right_staged(S, P, l, l, i, rc, rs, tile, TR);
      }
      zhs_right_staged(Q, N, N, l, i, rc, rs, tile, TR);
    }
    __syncthreads();
  }
  if (failed && t == 0) atomicMax(flags + 1, INT_MAX - (int)(member0 + b < INT_MAX - 1 ? member0 + b : INT_MAX - 1));
  __syncthreads();
  for (int idx = t; idx < N * N; idx += ZHS_T) {
    const int r = idx / N, c = idx - r * N;
    Tm[idx] = c >= r ? cldexp(S[r * P + c], e1) : zero;
  }
}

// the eigenvectors of the upper triangular T [members, N, N] as the columns of X; grid (blocks of 64 columns, members)
__global__ __launch_bounds__(ZHS_T) void ztrevc_k(const cd* __restrict__ Tg, const u64* __restrict__ mx, cd* Xg, int N) {
  __shared__ u64 mxs[4][64];
  const int t = threadIdx.x, c = t & 63, w = t >> 6, k0 = blockIdx.x * 64, k = k0 + c;
  const long b = blockIdx.y;
  const u64 m = mx[b];
  if (m > SYEV_MAX_BITS) return;                              // (uniform)
  const int e1 = syev_exp(m);
  const cd* T = Tg + b * N * N;
  cd* X = Xg + b * N * N;
  const bool active = k < N;
  const cd zero = cmk(0.0, 0.0);
  const cd lam = active ? cldexp(T[(long)k * N + k], -e1) : zero;
  const double smin = fmax(ZHS_EPS * cabs1(lam), DBL_MIN * ((double)N / ZHS_EPS));
  if (active)
    for (int i = w; i < N; i += 4) X[(long)i * N + k] = i < k ? cldexp(cmk(-T[(long)i * N + k].x, -T[(long)i * N + k].y), -e1) : cmk(i == k ? 1.0 : 0.0, 0.0);
  const int jtop = min(k0 + 63, N - 1);
  for (int j = jtop - 1; j >= 0; --j) {
    __syncthreads();
    const bool on = active && j < k;
    cd xj = zero;
    int q = 0;
    if (on) {
      cd bj = X[(long)j * N + k], d = csub(cldexp(T[(long)j * N + j], -e1), lam);
      if (cabs1(d) < smin) d = cmk(smin, 0.0);
      const double ab = cabs1(bj), ad = cabs1(d);
      if (ab > 0x1p400 * ad) { q = ilogb(ab) - ilogb(ad) - 400; bj = cldexp(bj, -q); }   // the overflow guard
      xj = cdiv(bj, d);
    }
    __syncthreads();
    if (on) {
      if (q)
        for (int i = w; i <= k; i += 4)
          if (i != j) X[(long)i * N + k] = cldexp(X[(long)i * N + k], -q);
      if (w == 0) X[(long)j * N + k] = xj;
      for (int i = w; i < j; i += 4) X[(long)i * N + k] = csub(X[(long)i * N + k], cmul(xj, cldexp(T[(long)i * N + j], -e1)));
    }
  }
  __syncthreads();
  u64 cm = 0;
  if (active)
    for (int i = w; i <= k; i += 4) {
      const u64 br = het_bits(X[(long)i * N + k].x), bi = het_bits(X[(long)i * N + k].y);
      cm = br > cm ? br : cm; cm = bi > cm ? bi : cm;
    }
  mxs[w][c] = cm;
  __syncthreads();
  for (int g = 0; g < 4; ++g) cm = mxs[g][c] > cm ? mxs[g][c] : cm;
  const int e2 = syev_exp(cm);
  if (active && e2 != 0)
    for (int i = w; i <= k; i += 4) X[(long)i * N + k] = cldexp(X[(long)i * N + k], -e2);
}

// ---- the blocked back-substitution above N = 64 (nb = 64, as eigvec.hip) -----------------------------------------------------------------
// Ts = 2^-e1 triu(T), X = I (x_k = 1; the right-hand side -T[0:k, k] x_k comes from the same updates as every other x_j); grid (tiles of 256 over N N, members)
__global__ __launch_bounds__(ZHS_T) void ztrevc_init_k(const cd* __restrict__ Tg, const u64* __restrict__ mx, cd* __restrict__ Ts, cd* __restrict__ X, int N) {
  const long idx = (long)blockIdx.x * ZHS_T + threadIdx.x, b = blockIdx.y;
  if (idx >= (long)N * N) return;
  const int i = (int)(idx / N), j = (int)(idx - (long)i * N);
  const u64 m = mx[b];
  const int e1 = m > SYEV_MAX_BITS ? 0 : syev_exp(m);
  const cd x = j >= i ? cldexp(Tg[b * N * N + idx], -e1) : cmk(0.0, 0.0);
  Ts[b * N * N + idx] = x;
  X[b * N * N + idx] = cmk(i == j ? 1.0 : 0.0, 0.0);
}

// the rows r0 .. r0 + nr - 1 (block row I = r0 / 64) of the columns of block J = I + blockIdx.x: the diagonal block of Ts and the 64 x 64
// tile of X in LDS at pitch 65, one lane per column, the four waves split the rows of each axpy; the rows above r0 are left to the
// matrix-core update that follows. grid (column blocks from I, members), 133120 bytes of dynamic LDS
__global__ __launch_bounds__(ZHS_T) void ztrevc_diag_k(const cd* __restrict__ Tsg, const u64* __restrict__ mx, cd* Xg, int N, int r0) {
  extern __shared__ __attribute__((aligned(16))) char zhs_smem[];
  cd* Td = reinterpret_cast<cd*>(zhs_smem);                   // [64][65]
  cd* Xt = Td + 64 * 65;                                      // [64][65]
  const int t = threadIdx.x, c = t & 63, w = t >> 6, k0 = r0 + blockIdx.x * 64, k = k0 + c, nr = min(64, N - r0);
  const long b = blockIdx.y;
  if (mx[b] > SYEV_MAX_BITS) return;                          // (uniform)
  const cd* Ts = Tsg + b * N * N;
  cd* X = Xg + b * N * N;
  const bool active = k < N;
  const cd zero = cmk(0.0, 0.0);
  for (int e = t; e < nr * nr; e += ZHS_T) { const int i = e / nr, j = e - i * nr; Td[i * 65 + j] = Ts[(long)(r0 + i) * N + r0 + j]; }
  for (int i = w; i < nr; i += 4) Xt[i * 65 + c] = active ? X[(long)(r0 + i) * N + k] : zero;
  const cd lam = active ? Ts[(long)k * N + k] : zero;
  const double smin = fmax(ZHS_EPS * cabs1(lam), DBL_MIN * ((double)N / ZHS_EPS));
  for (int jj = nr - 1; jj >= 0; --jj) {
    __syncthreads();
    const bool on = active && r0 + jj < k, unit = active && r0 + jj == k;   // unit: x_k itself, no division
    cd xj = unit ? Xt[jj * 65 + c] : zero;
    int q = 0;
    if (on) {
      cd bj = Xt[jj * 65 + c], d = csub(Td[jj * 65 + jj], lam);
      if (cabs1(d) < smin) d = cmk(smin, 0.0);
      const double ab = cabs1(bj), ad = cabs1(d);
      if (ab > 0x1p400 * ad) { q = ilogb(ab) - ilogb(ad) - 400; bj = cldexp(bj, -q); }   // the overflow guard
      xj = cdiv(bj, d);
    }
    __syncthreads();
    if (on || unit) {
      if (q) {                                                // the whole column: the tile, the rows above it and the finished rows below
        for (int i = w; i < nr; i += 4)
          if (i != jj) Xt[i * 65 + c] = cldexp(Xt[i * 65 + c], -q);
        for (int i = w; i <= k; i += 4)
          if (i < r0 || i >= r0 + nr) X[(long)i * N + k] = cldexp(X[(long)i * N + k], -q);
      }
      if (on && w == 0) Xt[jj * 65 + c] = xj;
      for (int i = w; i < jj; i += 4) Xt[i * 65 + c] = csub(Xt[i * 65 + c], cmul(xj, Td[i * 65 + jj]));
    }
  }
  __syncthreads();
  if (active)
    for (int i = w; i < nr; i += 4) X[(long)(r0 + i) * N + k] = Xt[i * 65 + c];
}

// every column of X to a maximum in [0.5, 1) by a power of two; grid (blocks of 64 columns, members)
__global__ __launch_bounds__(ZHS_T) void ztrevc_scale_k(const u64* __restrict__ mx, cd* Xg, int N) {
  __shared__ u64 mxs[4][64];
  const int t = threadIdx.x, c = t & 63, w = t >> 6, k = blockIdx.x * 64 + c;
  const long b = blockIdx.y;
  if (mx[b] > SYEV_MAX_BITS) return;                          // (uniform)
  cd* X = Xg + b * N * N;
  u64 cm = 0;
  if (k < N)
    for (int i = w; i <= k; i += 4) {
      const u64 br = het_bits(X[(long)i * N + k].x), bi = het_bits(X[(long)i * N + k].y);
      cm = br > cm ? br : cm; cm = bi > cm ? bi : cm;
    }
  mxs[w][c] = cm;
  __syncthreads();
  for (int g = 0; g < 4; ++g) cm = mxs[g][c] > cm ? mxs[g][c] : cm;
  const int e2 = syev_exp(cm);
  if (k < N && e2 != 0)
    for (int i = w; i <= k; i += 4) X[(long)i * N + k] = cldexp(X[(long)i * N + k], -e2);
}


// every column of V [members, N, N] to unit 2-norm; grid (blocks of 64 columns, members)
__global__ __launch_bounds__(ZHS_T) void zeig_unit_k(cd* __restrict__ Vg, int N) {
  __shared__ double ss[4][64];
  const int t = threadIdx.x, c = t & 63, w = t >> 6, k = blockIdx.x * 64 + c;
  cd* V = Vg + (long)blockIdx.y * N * N;
  double a2 = 0.0;
  if (k < N)
    for (int i = w; i < N; i += 4) { const cd x = V[(long)i * N + k]; a2 += x.x * x.x + x.y * x.y; }
  ss[w][c] = a2;
  __syncthreads();
  const double nrm = sqrt(((ss[0][c] + ss[1][c]) + ss[2][c]) + ss[3][c]);
  if (k < N && nrm > 0.0)
    for (int i = w; i < N; i += 4) { const cd x = V[(long)i * N + k]; V[(long)i * N + k] = cmk(x.x / nrm, x.y / nrm); }
}

// lam [members, N] = diag(T); grid (tiles of 256 over N, members)
__global__ __launch_bounds__(ZHS_T) void zeig_diag_k(const cd* __restrict__ T, cd* __restrict__ lam, int N) {
  const int k = blockIdx.x * ZHS_T + threadIdx.x;
  if (k < N) lam[(long)blockIdx.y * N + k] = T[(long)blockIdx.y * N * N + (long)k * N + k];
}

inline bool zhs_al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
template <class T> int zhs_alloc(nd4hip_handle* h, size_t n, T** out) {
  void* p = nullptr;
  ND4_TRY(nd4_ws_alloc(h, sizeof(T) * (n ? n : 1), &p));
  *out = static_cast<T*>(p);
  return 0;
}
inline size_t zhs_lds_of(int64_t N, bool in_lds, int TR) { return 24 * (size_t)N + 16 * (size_t)ZHS_TP * TR + (in_lds ? 16 * (size_t)(N * (N | 1)) : 0); }

// one pass of at most 32768 members; flags [2] (NaN or Inf, no convergence). All enqueue only
int zhs_pass_hseqr(nd4hip_handle* h, int64_t nbm, int N, double* Q, double* T, bool want_t, int64_t member0, int* flags) {
  u64* mx = nullptr;
  ND4_TRY(zhs_alloc(h, (size_t)nbm, &mx));
  ND4_TRY(nd4_zeig_clear(h, mx, sizeof(u64) * (size_t)nbm));
  ND4_TRY(nd4_zeig_absmax(h, nbm, (int64_t)N * N, T, mx, member0, flags));
  const int tier = nd4_zhseqr_tier(N), TR = nd4_zhseqr_tile_rows(N);
  const size_t lds = nd4_zhseqr_lds(N);
  // with H in global memory every rotation goes to the full rows, columns and Q as it is produced ("eager"): there the per-sweep deferral
  // lost 1 - 3 % when measured; with H in LDS the deferral stays. ND4HIP_ZHSEQR_EAGER=0 / 1 forces either form for the
  // measurement (tools/time_zeig.py); both give the same bits
  const char* ev = std::getenv("ND4HIP_ZHSEQR_EAGER");
  const int eager = ev && (ev[0] == '0' || ev[0] == '1') ? ev[0] - '0' : tier;
  hipLaunchKernelGGL(zhseqr_k, dim3((unsigned)nbm), dim3(ZHS_T), lds, h->stream, reinterpret_cast<cd*>(T), reinterpret_cast<cd*>(want_t ? Q : nullptr), mx, N,
                     tier == 0 ? 1 : 0, TR, want_t ? 1 : 0, eager, (long)member0, flags);
  ND4_HIP(hipGetLastError());
  return 0;
}
int zhs_pass_gees(nd4hip_handle* h, int64_t nbm, int N, const double* A, double* Q, double* T, bool want_t, int64_t member0, int* flags) {
  double* tau = nullptr;
  ND4_TRY(zhs_alloc(h, 2 * (size_t)nbm * N, &tau));
  ND4_TRY(nd4_zgehrd(h, nbm, N, A, T, tau, member0, flags));
  if (want_t) {
    ND4_TRY(nd4_zeig_identity(h, nbm, N, Q));
    if (N > 1) ND4_TRY(nd4_zunmtr(h, nbm, N, N, false, T, tau, Q));
  }
  ND4_TRY(nd4_zhess_clean(h, nbm, N, T, T));                  // the tails leave: the maximum below is H's
  return zhs_pass_hseqr(h, nbm, N, Q, T, want_t, member0, flags);
}
int zhs_pass_trevc(nd4hip_handle* h, int64_t nbm, int N, const double* Q, const double* T, double* lam, double* V, int64_t member0, int* flags) {
  u64 *mx = nullptr, *mq = nullptr; double* X = nullptr;
  const int64_t nn = (int64_t)N * N;
  ND4_TRY(zhs_alloc(h, 2 * (size_t)nbm, &mx)); ND4_TRY(zhs_alloc(h, 2 * (size_t)(nbm * nn), &X));
  mq = mx + nbm;                                              // Q's maximum is taken only for its NaN or Inf flag
  ND4_TRY(nd4_zeig_clear(h, mx, sizeof(u64) * 2 * (size_t)nbm));
  ND4_TRY(nd4_zeig_absmax(h, nbm, nn, T, mx, member0, flags));
  ND4_TRY(nd4_zeig_absmax(h, nbm, nn, Q, mq, member0, flags));
  const unsigned cb = (unsigned)((N + 63) / 64);
  hipLaunchKernelGGL(zeig_diag_k, dim3((unsigned)((N + ZHS_T - 1) / ZHS_T), (unsigned)nbm), dim3(ZHS_T), 0, h->stream, reinterpret_cast<const cd*>(T),
                     reinterpret_cast<cd*>(lam), N);
  if (nd4_ztrevc_tier(N) == 0) {
    hipLaunchKernelGGL(ztrevc_k, dim3(cb, (unsigned)nbm), dim3(ZHS_T), 0, h->stream, reinterpret_cast<const cd*>(T), mx, reinterpret_cast<cd*>(X), N);
    ND4_HIP(hipGetLastError());
  } else {
    double* Ts = nullptr;
    ND4_TRY(zhs_alloc(h, 2 * (size_t)(nbm * nn), &Ts));
    hipLaunchKernelGGL(ztrevc_init_k, dim3((unsigned)((nn + ZHS_T - 1) / ZHS_T), (unsigned)nbm), dim3(ZHS_T), 0, h->stream, reinterpret_cast<const cd*>(T), mx,
                       reinterpret_cast<cd*>(Ts), reinterpret_cast<cd*>(X), N);
    ND4_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&ztrevc_diag_k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)ZHS_TREVC_LDS));
    for (int I = (int)cb - 1; I >= 0; --I) {
      const int r0 = I * 64, nr = N - r0 < 64 ? N - r0 : 64;
      hipLaunchKernelGGL(ztrevc_diag_k, dim3(cb - (unsigned)I, (unsigned)nbm), dim3(ZHS_T), ZHS_TREVC_LDS, h->stream, reinterpret_cast<const cd*>(Ts), mx,
                         reinterpret_cast<cd*>(X), N, r0);
      ND4_HIP(hipGetLastError());
      if (r0 == 0) break;
      // X[0:r0, r0:] -= Ts[0:r0, r0:r0+nr] X[r0:r0+nr, r0:] on the fp64 matrix cores
      const ZluUpd u{Ts + 2 * (int64_t)r0, N, nn, X + 2 * ((int64_t)r0 * N + r0), N, nn, X + 2 * (int64_t)r0, N, nn, r0, N - r0, nr};
      ND4_TRY(zlu_update_launch(h, nbm, u));
    }
    hipLaunchKernelGGL(ztrevc_scale_k, dim3(cb, (unsigned)nbm), dim3(ZHS_T), 0, h->stream, mx, reinterpret_cast<cd*>(X), N);
    ND4_HIP(hipGetLastError());
  }
  ND4_TRY(nd4_zgemm(h, true, nbm, N, N, N, Q, nn, X, nn, V));
  hipLaunchKernelGGL(zeig_unit_k, dim3(cb, (unsigned)nbm), dim3(ZHS_T), 0, h->stream, reinterpret_cast<cd*>(V), N);
  ND4_HIP(hipGetLastError());
  return 0;
}

// reads the pass's two flag words back (synchronises) and words the error: '<fn>(..): <operand> contains NaN or Infinity. (matrix b)' or
// '<fn>(..): no convergence (matrix b)'; what = "<fn>(..): <operand>"
int zhs_report(nd4hip_handle* h, const int* flags, const char* what, int64_t* first_bad) {
  int f[2] = {0, 0};
  ND4_TRY(nd4_zeig_read_flags(h, flags, 2, f));
  if (!f[0] && !f[1]) return 0;
  const long long mb = (long long)INT_MAX - (f[0] ? f[0] : f[1]);
  if (first_bad) *first_bad = mb;
  const char* colon = std::strchr(what, ':');
  if (f[0]) nd4_set_error("%s contains NaN or Infinity. (matrix %lld)", what, mb);
  else nd4_set_error("%.*s: no convergence (matrix %lld)", (int)(colon ? colon - what : (long)std::strlen(what)), what, mb);
  return ND4HIP_ERR_NOCONV;
}
int zhs_flags(nd4hip_handle* h, int** flags) {
  ND4_TRY(zhs_alloc(h, 2, flags));
  return nd4_zeig_clear(h, *flags, 8);
}
int zhs_copy(nd4hip_handle* h, const double* src, double* dst, size_t doubles) {
  if (src != dst) ND4_HIP(hipMemcpyAsync(dst, src, sizeof(double) * doubles, hipMemcpyDeviceToDevice, h->stream));
  return 0;
}

}  // namespace

// ---- the host-side arithmetic of the tiers (tools/zeig_host_check.hip) ----
// 0: H in one workgroup's LDS, 1: H in global memory
int nd4_zhseqr_tier(int64_t N) { return zhs_lds_of(N, true, 64) <= ZHS_LDS - 64 ? 0 : 1; }
int nd4_zhseqr_tile_rows(int64_t N) { return nd4_zhseqr_tier(N) == 1 ? 256 : N <= 16 ? 16 : N <= 32 ? 32 : 64; }
// the back-substitution: 0: a lane per column in one kernel (N <= 64), 1: blocks of 64 with the update on the matrix cores
int nd4_ztrevc_tier(int64_t N) { return N <= 64 ? 0 : 1; }
size_t nd4_zhseqr_lds(int64_t N) { return zhs_lds_of(N, nd4_zhseqr_tier(N) == 0, nd4_zhseqr_tile_rows(N)); }

#define ZHS_CHECK_N(op, N) ND4_CHECK_ARG((N) >= 1 && (N) <= ZHS_MAXN, "nd4hip_" op "_batched: 1 <= N <= 1024")

// zschur_qr: (Q, T) from the Hessenberg pair (Q0, H); want_t = false: T's diagonal alone is meaningful and Q0, Q are not touched. The
// four drivers take checked arguments, batch >= 1, synchronise once per pass (the flag words) and answer ND4HIP_ERR_NOCONV with the text
// of zhs_report and the lowest flagged member, counted from member0, in *first_bad (may be NULL)
int nd4_zhseqr_run(nd4hip_handle* h, int64_t batch, int64_t N64, const double* Q0, const double* H, double* Q, double* T, bool want_t,
                   const char* what, int64_t member0, int64_t* first_bad) {
  ZHS_CHECK_N("zhseqr", N64);
  ND4_CHECK_ARG(zhs_al16(Q0) && zhs_al16(H) && zhs_al16(Q) && zhs_al16(T), "nd4hip_zhseqr_batched: complex operands must be 16-byte aligned");
  const int N = (int)N64;
  const int64_t nn = N64 * N64, chunk = nd4_zeig_chunk(batch, 0);
  for (int64_t b0 = 0; b0 < batch; b0 += chunk) {
    const int64_t nbm = batch - b0 < chunk ? batch - b0 : chunk;
    Nd4WsScope scope(h);
    int* flags = nullptr;
    ND4_TRY(zhs_flags(h, &flags));
    ND4_TRY(zhs_copy(h, H + 2 * b0 * nn, T + 2 * b0 * nn, 2 * (size_t)(nbm * nn)));
    if (want_t) ND4_TRY(zhs_copy(h, Q0 + 2 * b0 * nn, Q + 2 * b0 * nn, 2 * (size_t)(nbm * nn)));
    ND4_TRY(zhs_pass_hseqr(h, nbm, N, want_t ? Q + 2 * b0 * nn : nullptr, T + 2 * b0 * nn, want_t, member0 + b0, flags));
    ND4_TRY(zhs_report(h, flags, what, first_bad));
  }
  return 0;
}

// zschur_decomp: A = Q T Q^H
int nd4_zgees_run(nd4hip_handle* h, int64_t batch, int64_t N64, const double* A, double* Q, double* T, const char* what, int64_t member0,
                  int64_t* first_bad) {
  ZHS_CHECK_N("zgees", N64);
  ND4_CHECK_ARG(zhs_al16(A) && zhs_al16(Q) && zhs_al16(T), "nd4hip_zgees_batched: complex operands must be 16-byte aligned");
  const int N = (int)N64;
  const int64_t nn = N64 * N64, chunk = nd4_zgehrd_chunk(batch, N, N + nd4_zunmtr_ws_elems(N, N));
  for (int64_t b0 = 0; b0 < batch; b0 += chunk) {
    const int64_t nbm = batch - b0 < chunk ? batch - b0 : chunk;
    Nd4WsScope scope(h);
    int* flags = nullptr;
    ND4_TRY(zhs_flags(h, &flags));
    ND4_TRY(zhs_pass_gees(h, nbm, N, A + 2 * b0 * nn, Q + 2 * b0 * nn, T + 2 * b0 * nn, true, member0 + b0, flags));
    ND4_TRY(zhs_report(h, flags, what, first_bad));
  }
  return 0;
}

// zschur_eigen: lam [batch, N] = diag(T) and the unit eigenvectors V [batch, N, N] of Q T Q^H
int nd4_ztrevc_run(nd4hip_handle* h, int64_t batch, int64_t N64, const double* Q, const double* T, double* lam, double* V, const char* what,
                   int64_t member0, int64_t* first_bad) {
  ZHS_CHECK_N("ztrevc", N64);
  ND4_CHECK_ARG(zhs_al16(Q) && zhs_al16(T) && zhs_al16(lam) && zhs_al16(V), "nd4hip_ztrevc_batched: complex operands must be 16-byte aligned");
  const int N = (int)N64;
  const int64_t nn = N64 * N64, chunk = nd4_zeig_chunk(batch, 2 * nn);
  for (int64_t b0 = 0; b0 < batch; b0 += chunk) {
    const int64_t nbm = batch - b0 < chunk ? batch - b0 : chunk;
    Nd4WsScope scope(h);
    int* flags = nullptr;
    ND4_TRY(zhs_flags(h, &flags));
    ND4_TRY(zhs_pass_trevc(h, nbm, N, Q + 2 * b0 * nn, T + 2 * b0 * nn, lam + 2 * b0 * N, V + 2 * b0 * nn, member0 + b0, flags));
    ND4_TRY(zhs_report(h, flags, what, first_bad));
  }
  return 0;
}

// zeigen (V != NULL) / zeigenvals (V = NULL)
int nd4_zgeev_run(nd4hip_handle* h, int64_t batch, int64_t N64, const double* A, double* lam, double* V, const char* what, int64_t member0,
                  int64_t* first_bad) {
  ZHS_CHECK_N("zgeev", N64);
  ND4_CHECK_ARG(zhs_al16(A) && zhs_al16(lam) && zhs_al16(V), "nd4hip_zgeev_batched: complex operands must be 16-byte aligned");
  const int N = (int)N64;
  const int64_t nn = N64 * N64;
  const int64_t chunk = nd4_zgehrd_chunk(batch, N, (V ? 4 : 1) * nn + N + nd4_zunmtr_ws_elems(N, N));
  for (int64_t b0 = 0; b0 < batch; b0 += chunk) {
    const int64_t nbm = batch - b0 < chunk ? batch - b0 : chunk;
    Nd4WsScope scope(h);
    int* flags = nullptr;
    double *Q = nullptr, *T = nullptr;
    ND4_TRY(zhs_flags(h, &flags));
    ND4_TRY(zhs_alloc(h, 2 * (size_t)(nbm * nn), &T));
    if (V) ND4_TRY(zhs_alloc(h, 2 * (size_t)(nbm * nn), &Q));
    ND4_TRY(zhs_pass_gees(h, nbm, N, A + 2 * b0 * nn, Q, T, V != nullptr, member0 + b0, flags));
    if (V) {
      ND4_TRY(zhs_pass_trevc(h, nbm, N, Q, T, lam + 2 * b0 * N, V + 2 * b0 * nn, member0 + b0, flags));
    } else {
      hipLaunchKernelGGL(zeig_diag_k, dim3((unsigned)((N + ZHS_T - 1) / ZHS_T), (unsigned)nbm), dim3(ZHS_T), 0, h->stream, reinterpret_cast<const cd*>(T),
                         reinterpret_cast<cd*>(lam) + b0 * N, N);
      ND4_HIP(hipGetLastError());
    }
    ND4_TRY(zhs_report(h, flags, what, first_bad));
  }
  return 0;
}
