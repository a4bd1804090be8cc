// herm_tridiag_factor / herm_tridiag_apply_q / herm_tridiag_decomp and eigen_herm(H, subset): the reduction of a Hermitian matrix to a
// real symmetric tridiagonal one, H = Q tridiag(d, e) Q^H, and the application of its unitary Q (LAPACK's zhetrd / zunmtr, lower, on
// row-major complex128 members: interleaved (re, im) doubles), DESIGN.md 4.24. The reference has neither. Built the way sytrd.hip
// builds the real ones, whose header states the discipline that holds here too.
//   Q = H_0 H_1 ... H_{N-2}, H_k = I - tau_k v_k v_k^H, v_k zero in rows 0..k, 1 in row k+1, its tail in F[k+2:, k], tau_k complex.
//   N - 1 reflectors, one more than in the real case: the last one has an empty tail and exists only to make e_{N-2} real.
//   Step k takes the column x = A[k+1:, k] = [alpha; tail] of the matrix as the steps before left it, sigma = |tail|^2:
//     sigma = 0 and Im alpha = 0: tau_k = 0, e_k = Re alpha (the step changes nothing);
//     else beta = -sign(Re alpha) sqrt(Re alpha^2 + Im alpha^2 + sigma) (sign(0) = +1), tau_k = ((beta - Re alpha) / beta, -Im alpha / beta),
//          tail / (alpha - beta) (a complex division), e_k = beta. sigma = 0 with Im alpha != 0 is a pure phase reflector;
//     p = tau A v,  w = p - (tau / 2)(p^H v) v,  A -= v w^H + w v^H  on the trailing block (rows and columns > k).
// Every member is scaled on load by 2^-e1, e1 the exponent that puts max(|Re h_ij|, |Im h_ij|) over its lower triangle in [0.5, 1)
// (the imaginary part of the diagonal is not read); d and e get 2^e1 back on their store, exactly. So H -> 2^m H leaves tails, tau
// and Q bit-identical. NaN or Inf in what is read shows in the bit pattern of that maximum: one flag word per call.
// Every sum has a fixed order that depends on N and k alone: no atomics on doubles. The only synchronisation is __syncthreads() and
// the kernel boundary; the host decides nothing from data. Mirrored entries are exact conjugates and the diagonal is exactly real:
// the rank-2 update computes one triangle and mirrors it (tier A) or only stores one (tier B), and sets Im a_ii = 0.
//   Tier A (N <= 96): hetrd_small, one workgroup per member and one launch per call; the member stays in LDS as a full Hermitian
//     square at an odd pitch (16-byte elements: a column walk touches 16 different slots per lane group) for all N - 1 steps.
//     16 (N (N | 1) + 2 N + 264) bytes: 156288 at N = 96 (N = 98 would still fit 163840, 99 does not).
//   Tier B (N <= 2048): hetrd_step, one launch per column k = 0 .. N-1 over a grid (blocks of 64 rows, batch) on the scaled lower
//     triangle in F, the structure of sytrd_step: launch k finishes step k-1 (p from the row sums and the per-block column partials,
//     added in block order, then w), reflects column k, and in one pass over its rows of the trailing triangle applies the rank-2
//     update of step k-1 and accumulates its share of A v_k. The product with the part above the diagonal uses the conjugates of
//     the stored lower entries. 16 (3 N + 512) + 64 bytes of LDS: the column sums of the four waves meet in two 4 x 64 buffers per
//     chunk of 64 columns, not in four rows of N (which would not fit for complex N = 2048).
//   zunmtr: N <= 96: unmtr_small, one workgroup per 64 columns of a member's Z, in LDS (16 * 67 N bytes), reflector by reflector.
//     Above: blocks of 64 reflectors in compact WY form, I - V T V^H (Q^H: T^H), zlarft forward / columnwise. The three large products
//     run on nd4_zgemm, which has no transposition or accumulation: V^H is a stored array, and Z -= V W is a kernel of this file.
#include "syev_internal.h"
#include <algorithm>

namespace {

constexpr int HET_MAXN = 2048;
constexpr int HET_SMALL = 96;              // tier A
constexpr int HET_ROWS = 64;               // tier B: rows of the triangle per workgroup
constexpr int HET_WY = 64;                 // zunmtr above tier A: reflectors per compact WY block
constexpr int HET_ZT = 64;                 // unmtr_small: columns of Z per workgroup

typedef double2 cd;                        // (re, im)

__device__ __forceinline__ cd cmk(double re, double im) { cd r; r.x = re; r.y = im; return r; }
__device__ __forceinline__ cd cadd(cd a, cd b) { return cmk(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ cd csub(cd a, cd b) { return cmk(a.x - b.x, a.y - b.y); }
__device__ __forceinline__ cd cconj(cd a) { return cmk(a.x, -a.y); }
__device__ __forceinline__ cd cmul(cd a, cd b) { return cmk(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }
__device__ __forceinline__ cd cmulc(cd a, cd b) { return cmk(a.x * b.x + a.y * b.y, a.y * b.x - a.x * b.y); }   // a conj(b)
__device__ __forceinline__ cd cscale(cd a, double s) { return cmk(a.x * s, a.y * s); }
// a / b for |Re b| >= |Im b| (the divisor alpha - beta: |Re| = |Re alpha| + |beta| >= |Im alpha|), Smith's form: no |b|^2
__device__ __forceinline__ cd cdiv_re(cd a, cd b) {
  const double r = b.y / b.x, den = b.x + b.y * r;
  return cmk((a.x + a.y * r) / den, (a.y - a.x * r) / den);
}
__device__ __forceinline__ u64 het_bits(double x) { return (u64)__double_as_longlong(fabs(x)); }

// the sum of x over the 256 threads in a fixed order: the xor tree of each wave, then the four waves in order. red: 8 doubles
__device__ __forceinline__ cd het_block_sum(cd x, double* red) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) { x.x += __shfl_xor(x.x, off); x.y += __shfl_xor(x.y, off); }
  __syncthreads();
  if ((threadIdx.x & 63) == 0) { red[2 * (threadIdx.x >> 6)] = x.x; red[2 * (threadIdx.x >> 6) + 1] = x.y; }
  __syncthreads();
  return cmk(((red[0] + red[2]) + red[4]) + red[6], ((red[1] + red[3]) + red[5]) + red[7]);
}

// Members are scaled to a maximum in [0.5, 1): the squares of a column cannot overflow, but those of a column below 2^-450 of the
// maximum lose bits or vanish (a block coupled to the rest by a tiny complex entry), and the reflector would not be unitary. Such a
// column, x = [alpha; tail] with nz non-zero tail entries, takes its sum of squares again on c x, c = 2^450, then 2^900 (which lifts
// the smallest subnormal number to 2^-174), as zlarfg rescales. The test is uniform over the workgroup; a NaN fails it.
constexpr double HET_TINY = 0x1p-900, HET_LIFT = 0x1p450;
__device__ __forceinline__ bool het_tiny(cd alpha, double c, double sigma_c, double nz) {
  const double ar = c * alpha.x, ai = c * alpha.y;
  return (ar * ar + ai * ai) + sigma_c < HET_TINY && (nz > 0.0 || alpha.x != 0.0 || alpha.y != 0.0);
}

// tau, beta = e_k and the divisor of the tail for x = [alpha; tail], sigma_c = |c tail|^2 with c as above (a NaN sigma counts as zero)
struct HetRefl { cd tau, div; double beta; bool on; };
__device__ __forceinline__ HetRefl het_reflector(cd alpha, double sigma_c, double c) {
  HetRefl r;
  if (!(sigma_c > 0.0) && alpha.y == 0.0) { r.tau = cmk(0.0, 0.0); r.beta = alpha.x; r.div = cmk(1.0, 0.0); r.on = false; return r; }
  const double s = sigma_c > 0.0 ? sigma_c : 0.0, ar = c * alpha.x, ai = c * alpha.y;
  const double nrm = sqrt((ar * ar + ai * ai) + s) / c;
  r.beta = alpha.x >= 0.0 ? -nrm : nrm;
  r.tau = cmk((r.beta - alpha.x) / r.beta, -alpha.y / r.beta);
  r.div = cmk(alpha.x - r.beta, alpha.y);
  r.on = true;
  return r;
}

// ---- tier A ---------------------------------------------------------------------------------------------------------------------
// grid (batch), 256 threads, dynamic LDS. H, F [batch, N, N] and tau [batch, N-1] complex; d [batch, N] and e [batch, N-1] real (both
// may be NULL), mx [batch] (may be NULL) receives the bits of the member's maximum. unscale = 0 leaves d and e scaled by 2^-e1.
__global__ __launch_bounds__(256) void hetrd_small(const cd* __restrict__ H, int N, cd* __restrict__ F, cd* __restrict__ tau, double* __restrict__ d,
                                                   double* __restrict__ e, u64* __restrict__ mx, int unscale, int* __restrict__ flag) {
  extern __shared__ __attribute__((aligned(16))) char het_smem[];
  const int P = N | 1, t = threadIdx.x, b = blockIdx.x;
  cd* A = reinterpret_cast<cd*>(het_smem);                    // [N][P], the full Hermitian square
  cd* v = A + (size_t)N * P;                                  // [N]
  cd* w = v + N;                                              // [N]: p, then w
  cd* part = w + N;                                           // [2][128]
  double* red = reinterpret_cast<double*>(part + 256);        // [8]
  u64* redu = reinterpret_cast<u64*>(red + 8);                // [4]
  const cd* s = H + (size_t)b * N * N;
  cd* f = F + (size_t)b * N * N;
  u64 m = 0;
  for (int idx = t; idx < N * N; idx += 256) {
    const int i = idx / N, j = idx - i * N;
    if (j <= i) {
      cd x = s[idx];
      if (i == j) x.y = 0.0;                                  // the imaginary part of the diagonal is ignored
      const u64 br = het_bits(x.x), bi = het_bits(x.y);
      m = br > m ? br : m; m = bi > m ? bi : m;
      A[i * P + j] = x;
      if (i != j) A[j * P + i] = cconj(x);
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) { const u64 o = __shfl_xor(m, off); m = o > m ? o : m; }
  if ((t & 63) == 0) redu[t >> 6] = m;
  __syncthreads();
  for (int q = 0; q < 4; ++q) m = redu[q] > m ? redu[q] : m;
  const int e1 = syev_exp(m);
  if (t == 0) { if (mx) mx[b] = m; if (m > SYEV_MAX_BITS) atomicMax(flag, 1); }
  for (int idx = t; idx < N * N; idx += 256) {
    const int i = idx / N, j = idx - i * N;
    const cd x = A[i * P + j];
    A[i * P + j] = cmk(ldexp(x.x, -e1), ldexp(x.y, -e1));
  }
  __syncthreads();
  cd* tb = tau + (size_t)b * (N > 1 ? N - 1 : 0);
  for (int k = 0; k + 1 < N; ++k) {
    // x = A[k+1:, k]
    const int it = k + 2 + t;
    const cd xt = it < N ? A[it * P + k] : cmk(0.0, 0.0);
    const cd alpha = A[(k + 1) * P + k];
    const cd sn = het_block_sum(cmk(xt.x * xt.x + xt.y * xt.y, xt.x != 0.0 || xt.y != 0.0 ? 1.0 : 0.0), red);
    double sigma = sn.x, c = 1.0;
    for (int lvl = 0; lvl < 2 && het_tiny(alpha, c, sigma, sn.y); ++lvl) {
      c *= HET_LIFT;
      const double xr = c * xt.x, xi = c * xt.y;
      sigma = het_block_sum(cmk(xr * xr + xi * xi, 0.0), red).x;
    }
    const HetRefl r = het_reflector(alpha, sigma, c);
    if (r.on) {                                               // (uniform) else: the step changes nothing
      if (t < N) v[t] = t <= k ? cmk(0.0, 0.0) : (t == k + 1 ? cmk(1.0, 0.0) : cdiv_re(A[t * P + k], r.div));
      __syncthreads();
      // p = tau A v over the trailing block: two threads per row, the even and the odd columns
      const int row = k + 1 + (t & 127), half = t >> 7;
      if (row < N) {
        cd acc = cmk(0.0, 0.0);
        for (int j = k + 1 + half; j < N; j += 2) acc = cadd(acc, cmul(A[row * P + j], v[j]));
        part[half * 128 + (t & 127)] = acc;
      }
      __syncthreads();
      cd pi = cmk(0.0, 0.0), pv = cmk(0.0, 0.0);
      if (t < 128 && row < N) { pi = cmul(r.tau, cadd(part[t], part[128 + t])); pv = cmulc(v[row], pi); }   // conj(p_i) v_i
      const cd dot = het_block_sum(pv, red);
      const cd half_tau_dot = cmul(cscale(r.tau, 0.5), dot);
      if (t < 128 && row < N) w[row] = csub(pi, cmul(half_tau_dot, v[row]));
      __syncthreads();
      // A -= v w^H + w v^H: the lower triangle is computed, the upper one is its mirror; the diagonal stays real
      const int mm = N - k - 1;
      for (int idx = t; idx < mm * mm; idx += 256) {
        const int i = k + 1 + idx / mm, j = k + 1 + idx % mm;
        if (j <= i) {
          cd a = csub(A[i * P + j], cadd(cmulc(v[i], w[j]), cmulc(w[i], v[j])));
          if (i == j) a.y = 0.0;
          A[i * P + j] = a;
          if (i != j) A[j * P + i] = cconj(a);
        }
      }
      // column k of the lower triangle is finished: e_k and the tail of v_k (row k of the square is not read again)
      if (t < N && t > k) A[t * P + k] = t == k + 1 ? cmk(r.beta, 0.0) : v[t];
    } else if (t == 0) A[(k + 1) * P + k] = cmk(r.beta, 0.0);  // tails are zero already
    if (t == 0) tb[k] = r.tau;
    __syncthreads();
  }
  for (int idx = t; idx < N * N; idx += 256) {
    const int i = idx / N, j = idx - i * N;
    cd x = j <= i ? A[i * P + j] : cmk(0.0, 0.0);
    if (j + 1 >= i && j <= i) {                               // d_i and e_j
      x.y = 0.0;
      if (unscale) x.x = ldexp(x.x, e1);
      if (d && j == i) d[(size_t)b * N + i] = x.x;
      if (e && j + 1 == i) e[(size_t)b * (N - 1) + j] = x.x;
    }
    f[idx] = x;
  }
}

// ---- tier B ---------------------------------------------------------------------------------------------------------------------
// mx[b] = bits of max(|Re|, |Im|) of H[b, i, j] over j <= i (Im of the diagonal excluded); grid (rows, batch). The maximum of
// integers: any order gives the same word.
__global__ __launch_bounds__(256) void hetrd_absmax(const cd* __restrict__ H, int N, u64* __restrict__ mx) {
  const cd* s = H + (size_t)blockIdx.y * N * N;
  u64 m = 0;
  for (int r = blockIdx.x; r < N; r += gridDim.x)
    for (int c = threadIdx.x; c <= r; c += 256) {
      const cd x = s[(size_t)r * N + c];
      const u64 br = het_bits(x.x), bi = c == r ? 0 : het_bits(x.y);
      m = br > m ? br : m; m = bi > m ? bi : m;
    }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) { const u64 o = __shfl_xor(m, off); m = o > m ? o : m; }
  if ((threadIdx.x & 63) == 0 && m) atomicMax(mx + blockIdx.y, m);
}

// F[b] = 2^-e1 lower(H[b]) with a real diagonal, zero above the diagonal; grid (N, batch)
__global__ __launch_bounds__(256) void hetrd_load(const cd* __restrict__ H, cd* __restrict__ F, int N, const u64* __restrict__ mx) {
  const int i = blockIdx.x, e1 = syev_exp(mx[blockIdx.y]);
  const cd* s = H + ((size_t)blockIdx.y * N + i) * N;
  cd* f = F + ((size_t)blockIdx.y * N + i) * N;
  for (int j = threadIdx.x; j < N; j += 256) {
    cd x = cmk(0.0, 0.0);
    if (j <= i) { x = s[j]; x = cmk(ldexp(x.x, -e1), j == i ? 0.0 : ldexp(x.y, -e1)); }
    f[j] = x;
  }
}

// the work of one member between launches: everything [batch, ...]
struct HetWs {
  cd* tau;          // [N-1] (the caller's)
  double* dsc;      // [N] scaled d
  double* esc;      // [N] scaled e
  cd* vd;           // [2][N] v_k, dense, by the parity of k
  cd* rowsum;       // [2][N] row sums of A v_k, by the parity of k
  cd* colpart;      // [2][nblk][N] column partials of A v_k per row block, by the parity of k
};

// launch k of tier B; grid (nblk, batch), 256 threads, dynamic LDS of 3 N + 512 complex and 8 doubles
__global__ __launch_bounds__(256) void hetrd_step(cd* __restrict__ F, int N, int k, HetWs ws) {
  extern __shared__ __attribute__((aligned(16))) char het_smem[];
  cd* vp = reinterpret_cast<cd*>(het_smem);                   // [N] v_{k-1}
  cd* wp = vp + N;                                            // [N] w_{k-1}
  cd* vk = wp + N;                                            // [N] v_k
  cd* cw = vk + N;                                            // [2][4][64] column sums per wave of one chunk, by the parity of the chunk
  double* red = reinterpret_cast<double*>(cw + 512);          // [8]
  const int t = threadIdx.x, b = blockIdx.y, blk = blockIdx.x, nblk = gridDim.x;
  const int r0 = blk * HET_ROWS, r1 = min(N, r0 + HET_ROWS);
  const bool last = blk == nblk - 1;
  if (r1 <= k + 1 && !last) return;                           // rows <= k are finished (the last block stores the scalars)
  cd* A = F + (size_t)b * N * N;
  cd* tb = ws.tau + (size_t)b * (N - 1);
  const int par = k & 1, ppar = par ^ 1;
  const cd zero = cmk(0.0, 0.0);
  // (i) w_{k-1} over the trailing indices of step k-1, j >= k
  if (k == 0) {
    for (int j = t; j < N; j += 256) { vp[j] = zero; wp[j] = zero; }
  } else {
    const cd taup = tb[k - 1];
    const cd* vprev = ws.vd + ((size_t)b * 2 + ppar) * N;
    const cd* rs = ws.rowsum + ((size_t)b * 2 + ppar) * N;
    const cd* cp = ws.colpart + ((size_t)b * 2 + ppar) * nblk * N;
    cd acc = zero;
    for (int j = k + t; j < N; j += 256) {
      cd s = rs[j];
      for (int q = j / HET_ROWS; q < nblk; ++q) s = cadd(s, cp[(size_t)q * N + j]);
      const cd pj = cmul(taup, s), vj = vprev[j];
      vp[j] = vj; wp[j] = pj; acc = cadd(acc, cmulc(vj, pj));  // conj(p_j) v_j
    }
    const cd dot = het_block_sum(acc, red);
    const cd htd = cmul(cscale(taup, 0.5), dot);
    for (int j = k + t; j < N; j += 256) wp[j] = csub(wp[j], cmul(htd, vp[j]));
  }
  __syncthreads();
  // (ii) column k after step k-1: d_k, then the reflector of [alpha; tail]
  {
    const cd wk = wp[k], vpk = vp[k];
    double acc = 0.0, cnt = 0.0;
    for (int i = k + t; i < N; i += 256) {
      const cd c = csub(A[(size_t)i * N + k], cadd(cmulc(vp[i], wk), cmulc(wp[i], vpk)));
      vk[i] = c;
      if (i >= k + 2) { acc += c.x * c.x + c.y * c.y; cnt += c.x != 0.0 || c.y != 0.0 ? 1.0 : 0.0; }
    }
    const cd sn = het_block_sum(cmk(acc, cnt), red);          // (its barriers make vk visible)
    const double dk = vk[k].x;
    HetRefl r; r.tau = zero; r.beta = 0.0; r.div = cmk(1.0, 0.0); r.on = false;
    if (k + 1 < N) {
      const cd alpha = vk[k + 1];
      double sigma = sn.x, lift = 1.0;
      for (int lvl = 0; lvl < 2 && het_tiny(alpha, lift, sigma, sn.y); ++lvl) {
        lift *= HET_LIFT;
        double a2 = 0.0;
        for (int i = k + 2 + t; i < N; i += 256) { const double xr = lift * vk[i].x, xi = lift * vk[i].y; a2 += xr * xr + xi * xi; }
        sigma = het_block_sum(cmk(a2, 0.0), red).x;
      }
      r = het_reflector(alpha, sigma, lift);
    }
    __syncthreads();
    cd* vout = ws.vd + ((size_t)b * 2 + par) * N;
    for (int i = k + t; i < N; i += 256) {
      const cd x = i == k ? zero : (i == k + 1 ? cmk(1.0, 0.0) : (r.on ? cdiv_re(vk[i], r.div) : zero));
      vk[i] = x;
      if (last) vout[i] = x;
    }
    if (last && t == 0) {
      ws.dsc[(size_t)b * N + k] = dk;
      if (k + 1 < N) { ws.esc[(size_t)b * N + k] = r.beta; tb[k] = r.tau; }
    }
  }
  __syncthreads();
  // (iii) rows max(r0, k+1) .. r1-1, columns k+1 .. row: the update of step k-1, and the sums of A v_k. A stored a_ij (j < i) also
  // stands for a_ji = conj(a_ij): its share of (A v)_j is conj(a_ij) v_i.
  const int wv = t >> 6, lane = t & 63;
  cd rowacc[HET_ROWS / 4];
#pragma unroll
  for (int r = 0; r < HET_ROWS / 4; ++r) rowacc[r] = zero;
  cd* cp = ws.colpart + (((size_t)b * 2 + par) * nblk + blk) * N;
  int chunk = 0;
  for (int j0 = k + 1; j0 < r1; j0 += 64, ++chunk) {          // (uniform bounds: the barrier below is reached by all)
    const int j = j0 + lane;
    const bool jin = j < N;
    const cd vkj = jin ? vk[j] : zero, vpj = jin ? vp[j] : zero, wpj = jin ? wp[j] : zero;
    cd colacc = zero;
#pragma unroll
    for (int r = 0; r < HET_ROWS / 4; ++r) {
      const int i = r0 + wv + 4 * r;
      if (i > k && i < r1 && j <= i) {                        // j <= i < r1 <= N
        cd a = csub(A[(size_t)i * N + j], cadd(cmulc(vp[i], wpj), cmulc(wp[i], vpj)));
        if (j == i) a.y = 0.0;
        A[(size_t)i * N + j] = a;
        rowacc[r] = cadd(rowacc[r], cmul(a, vkj));
        if (j < i) colacc = cadd(colacc, cmul(cconj(a), vk[i]));
      }
    }
    cd* buf = cw + (chunk & 1) * 256;
    buf[wv * 64 + lane] = colacc;
    __syncthreads();                                          // one per chunk: the buffers alternate
    if (t < 64 && j < r1) cp[j] = cadd(cadd(cadd(buf[lane], buf[64 + lane]), buf[128 + lane]), buf[192 + lane]);
  }
  cd* rs = ws.rowsum + ((size_t)b * 2 + par) * N;
#pragma unroll
  for (int r = 0; r < HET_ROWS / 4; ++r) {
    cd x = rowacc[r];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { x.x += __shfl_xor(x.x, off); x.y += __shfl_xor(x.y, off); }
    const int i = r0 + wv + 4 * r;
    if (lane == 0 && i > k && i < r1) rs[i] = x;
  }
  // the tail of v_{k-1} takes the place of column k-1, which launch k-1 was the last to read
  if (k > 0)
    for (int i = max(r0, k + 1) + t; i < r1; i += 256) A[(size_t)i * N + k - 1] = vp[i];
}

// after the last launch: d and e onto F's diagonals and into their own arrays, the flag; grid (batch)
__global__ __launch_bounds__(256) void hetrd_finish(cd* __restrict__ F, int N, HetWs ws, const u64* __restrict__ mx, double* __restrict__ d,
                                                    double* __restrict__ e, int unscale, int* __restrict__ flag) {
  const int b = blockIdx.x, e1 = unscale ? syev_exp(mx[b]) : 0;
  cd* f = F + (size_t)b * N * N;
  for (int i = threadIdx.x; i < N; i += 256) {
    const double di = ldexp(ws.dsc[(size_t)b * N + i], e1);
    f[(size_t)i * N + i] = cmk(di, 0.0);
    if (d) d[(size_t)b * N + i] = di;
    if (i + 1 < N) {
      const double ei = ldexp(ws.esc[(size_t)b * N + i], e1);
      f[(size_t)(i + 1) * N + i] = cmk(ei, 0.0);
      if (e) e[(size_t)b * (N - 1) + i] = ei;
    }
  }
  if (threadIdx.x == 0 && mx[b] > SYEV_MAX_BITS) atomicMax(flag, 1);
}

// ---- zunmtr ---------------------------------------------------------------------------------------------------------------------
// N <= 96: grid (ceil(K / 64), batch), 64 threads, one column of Z [batch, N, K] per thread, in LDS (N x 64 + 3 N complex).
// Reflector k: z -= v (tau (v^H z)); Q Z applies k = N-2 .. 0 with tau, Q^H Z applies k = 0 .. N-2 with conj(tau).
__global__ __launch_bounds__(64) void unmtr_small(const cd* __restrict__ F, const cd* __restrict__ tau, cd* __restrict__ Z, int N, int K, int adjoint) {
  extern __shared__ __attribute__((aligned(16))) char het_smem[];
  cd* z = reinterpret_cast<cd*>(het_smem);                    // [N][64]
  cd* vb = z + (size_t)N * HET_ZT;                            // [2][N]
  cd* tl = vb + 2 * (size_t)N;                                // [N] tau
  const int t = threadIdx.x, b = blockIdx.y, c = blockIdx.x * HET_ZT + t;
  const bool active = c < K;
  const cd* f = F + (size_t)b * N * N;
  const cd* tb = tau + (size_t)b * (N - 1);
  cd* zb = Z + (size_t)b * N * K;
  for (int i = 0; i < N; ++i) z[i * HET_ZT + t] = active ? zb[(size_t)i * K + c] : cmk(0.0, 0.0);
  for (int i = t; i < N - 1; i += 64) tl[i] = adjoint ? cconj(tb[i]) : tb[i];   // (made visible by the first step's barrier)
  const int nref = N - 1;                                     // N >= 2 here
  for (int s = 0; s < nref; ++s) {
    const int k = adjoint ? s : nref - 1 - s;
    cd* v = vb + (s & 1) * N;
    for (int i = k + 1 + t; i < N; i += 64) v[i] = i == k + 1 ? cmk(1.0, 0.0) : f[(size_t)i * N + k];
    __syncthreads();                                          // one per step: v alternates between two buffers
    cd dot = cmk(0.0, 0.0);
    for (int i = k + 1; i < N; ++i) dot = cadd(dot, cmulc(z[i * HET_ZT + t], v[i]));   // conj(v_i) z_i
    dot = cmul(tl[k], dot);
    for (int i = k + 1; i < N; ++i) z[i * HET_ZT + t] = csub(z[i * HET_ZT + t], cmul(v[i], dot));
  }
  if (active)
    for (int i = 0; i < N; ++i) zb[(size_t)i * K + c] = z[i * HET_ZT + t];
}

// compact WY, the reflectors k0 .. k0 + nb - 1 of every member as the dense V [batch, rows, 64], rows = N - k0 - 1 (row r is row
// k0 + 1 + r of the member): unit diagonal, zero above, columns >= nb zero; and Vh [batch, 64, rows] = V^H. grid (rows, batch), 64 threads
__global__ __launch_bounds__(64) void unmtr_wy_v(const cd* __restrict__ F, int N, int k0, int nb, cd* __restrict__ V, cd* __restrict__ Vh) {
  const int r = blockIdx.x, c = threadIdx.x, rows = N - k0 - 1;
  const cd* f = F + (size_t)blockIdx.y * N * N;
  cd x = cmk(0.0, 0.0);
  if (c < nb) x = r < c ? cmk(0.0, 0.0) : (r == c ? cmk(1.0, 0.0) : f[(size_t)(k0 + 1 + r) * N + k0 + c]);
  V[((size_t)blockIdx.y * rows + r) * HET_WY + c] = x;
  Vh[((size_t)blockIdx.y * HET_WY + c) * rows + r] = cconj(x);
}

// T [batch, 64, 64] upper triangular with I - V T V^H = H_k0 ... H_{k0+nb-1}, from G = V^H V [batch, 64, 64] (zlarft, forward,
// columnwise): T_jj = tau_j, T[0:j, j] = -tau_j T[0:j, 0:j] G[0:j, j]. adjoint: T^H is stored. One workgroup of 64 per member;
// thread i owns row i of T, column after column (G[l, j] is one address for the whole wave).
__global__ __launch_bounds__(64) void unmtr_wy_t(const cd* __restrict__ G, const cd* __restrict__ tau, int N, int k0, int nb, int adjoint,
                                                 cd* __restrict__ T) {
  extern __shared__ __attribute__((aligned(16))) char het_smem[];
  cd* tl = reinterpret_cast<cd*>(het_smem);                   // [64][65]
  const int i = threadIdx.x, b = blockIdx.x, P = HET_WY + 1;
  const cd* g = G + (size_t)b * HET_WY * HET_WY;
  for (int r = 0; r < HET_WY; ++r) tl[r * P + i] = cmk(0.0, 0.0);
  __syncthreads();
  const cd* tb = tau + (size_t)b * (N - 1) + k0;
  for (int j = 0; j < nb; ++j) {
    const cd tj = tb[j];
    if (i < j) {
      cd s = cmk(0.0, 0.0);
      for (int l = i; l < j; ++l) s = cadd(s, cmul(tl[i * P + l], g[l * HET_WY + j]));
      const cd x = cmul(tj, s);
      tl[i * P + j] = cmk(-x.x, -x.y);
    } else if (i == j) tl[i * P + j] = tj;
    __syncthreads();
  }
  cd* tt = T + (size_t)b * HET_WY * HET_WY;
  for (int r = 0; r < HET_WY; ++r) tt[r * HET_WY + i] = adjoint ? cconj(tl[i * P + r]) : tl[r * P + i];
}

// Zs [batch, rows, K] (members N K apart) -= V [batch, rows, 64] W [batch, 64, K]; grid (ceil(K / 256), rows, batch). The 64 terms of
// an element are added in order.
__global__ __launch_bounds__(256) void unmtr_wy_sub(const cd* __restrict__ V, const cd* __restrict__ W, cd* __restrict__ Zs, int rows, int K,
                                                    long sZ) {
  const int c = blockIdx.x * 256 + threadIdx.x, r = blockIdx.y, b = blockIdx.z;
  if (c >= K) return;
  const cd* v = V + ((size_t)b * rows + r) * HET_WY;
  const cd* w = W + (size_t)b * HET_WY * K + c;
  cd acc = cmk(0.0, 0.0);
#pragma unroll 8
  for (int l = 0; l < HET_WY; ++l) acc = cadd(acc, cmul(v[l], w[(size_t)l * K]));
  cd* z = Zs + (size_t)b * sZ + (size_t)r * K + c;
  *z = csub(*z, acc);
}

// ---- the routes' small kernels --------------------------------------------------------------------------------------------------
// d and e of F's diagonals onto the diagonals of the real Tr [batch, N, N] (nothing else of Tr is written), where the real
// kernels of syev.hip read them; grid (batch)
__global__ __launch_bounds__(256) void hetrd_diagonals(const cd* __restrict__ F, int N, double* __restrict__ Tr) {
  const cd* f = F + (size_t)blockIdx.x * N * N;
  double* tr = Tr + (size_t)blockIdx.x * N * N;
  for (int i = threadIdx.x; i < N; i += 256) {
    tr[(size_t)i * N + i] = f[(size_t)i * N + i].x;
    if (i + 1 < N) tr[(size_t)(i + 1) * N + i] = f[(size_t)(i + 1) * N + i].x;
  }
}

// V [batch, N, k] complex = the transposed rows of the real R [batch, k, N], Im = 0; 64 x 64 tiles through LDS, grid (tiles of N,
// tiles of k, batch)
__global__ __launch_bounds__(256) void hetrd_rows_to_columns(const double* __restrict__ R, cd* __restrict__ V, int N, int k) {
  __shared__ double tile[64][65];
  const int n0 = blockIdx.x * 64, k0 = blockIdx.y * 64, c = threadIdx.x & 63;
  const double* rb = R + (size_t)blockIdx.z * k * N;
  cd* vb = V + (size_t)blockIdx.z * N * k;
  for (int r = threadIdx.x >> 6; r < 64; r += 4)
    if (k0 + r < k && n0 + c < N) tile[r][c] = rb[(size_t)(k0 + r) * N + n0 + c];
  __syncthreads();
  for (int r = threadIdx.x >> 6; r < 64; r += 4)
    if (n0 + r < N && k0 + c < k) vb[(size_t)(n0 + r) * k + k0 + c] = cmk(tile[c][r], 0.0);
}

// N = 1: lambda = Re h_00, V = 1; one thread per member; *flag is raised for NaN or Inf
__global__ __launch_bounds__(256) void hetrd_order_one(const cd* __restrict__ H, long total, double* __restrict__ lam, cd* __restrict__ V,
                                                       int* __restrict__ flag) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  lam[i] = H[i].x;
  if (het_bits(H[i].x) > SYEV_MAX_BITS) atomicMax(flag, 1);
  if (V) V[i] = cmk(1.0, 0.0);
}

template <class T> int het_alloc(nd4hip_handle* h, size_t count, T** out) {
  void* p = nullptr;
  ND4_TRY(nd4_ws_alloc(h, sizeof(T) * (count ? count : 1), &p));
  *out = static_cast<T*>(p);
  return 0;
}

// above 64 KB of dynamic LDS the launch needs the function attribute (set every time: it is per device)
int het_lds_attr(const void* fn, size_t lds) {
  if (lds > 64 * 1024) ND4_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  return 0;
}

int het_read_flag(nd4hip_handle* h, const int* flag, int* value) {
  void* hp = nullptr;
  ND4_TRY(nd4_pinned(h, sizeof(int), &hp));
  ND4_HIP(hipMemcpyAsync(hp, flag, sizeof(int), hipMemcpyDeviceToHost, h->stream));
  ND4_HIP(hipStreamSynchronize(h->stream));
  *value = *static_cast<int*>(hp);
  return 0;
}

}  // namespace

// the host-side arithmetic of the tiers (also what the stand-alone host check exercises). Bytes of dynamic LDS of the reduction and of
// zunmtr's small tier (0 above it), row blocks, and bytes of workspace per member of tier B: dsc, esc, vd, rowsum, colpart
int nd4_hetrd_tier(int64_t N) { return N <= HET_SMALL ? 0 : 1; }
size_t nd4_hetrd_lds(int64_t N) {
  return nd4_hetrd_tier(N) == 0 ? 16 * ((size_t)N * (size_t)(N | 1) + 2 * (size_t)N + 264) : 16 * (3 * (size_t)N + 512) + 64;
}
size_t nd4_zunmtr_lds(int64_t N) { return nd4_hetrd_tier(N) == 0 ? 16 * ((size_t)N * HET_ZT + 3 * (size_t)N) : 0; }
int64_t nd4_hetrd_blocks(int64_t N) { return (N + HET_ROWS - 1) / HET_ROWS; }
size_t nd4_hetrd_ws_bytes(int64_t N) { return (size_t)N * (8 * 2 + 16 * (2 + 2 + 2 * (size_t)nd4_hetrd_blocks(N))); }

// H [batch, N, N] -> F, tau [batch, N-1] (complex, as interleaved doubles); d [batch, N] and e [batch, N-1] may be NULL. mx [batch] must
// be ZERO on entry and receives the bits of the member's maximum; *flag (zero on entry) is raised for NaN or Inf. unscale = false
// leaves d and e (on F's diagonals and in d, e) scaled by 2^-e1. batch <= 32768, 1 <= N <= 2048. Enqueues only.
int nd4_hetrd(nd4hip_handle* h, int64_t batch, int64_t N64, const double* Hm, double* Fm, double* taum, double* d, double* e, u64* mx,
              bool unscale, int* flag) {
  ND4_CHECK_ARG(N64 >= 1 && N64 <= HET_MAXN && batch >= 1 && batch <= 32768, "nd4hip_zhetrd_batched: extent out of range");
  const int N = (int)N64;
  const cd* H = reinterpret_cast<const cd*>(Hm);
  cd* F = reinterpret_cast<cd*>(Fm);
  cd* tau = reinterpret_cast<cd*>(taum);
  const size_t lds = nd4_hetrd_lds(N);
  if (nd4_hetrd_tier(N) == 0) {
    ND4_TRY(het_lds_attr(reinterpret_cast<const void*>(&hetrd_small), lds));
    hipLaunchKernelGGL(hetrd_small, dim3((unsigned)batch), dim3(256), lds, h->stream, H, N, F, tau, d, e, mx, unscale ? 1 : 0, flag);
    ND4_HIP(hipGetLastError());
    return 0;
  }
  const int nblk = (int)nd4_hetrd_blocks(N);
  HetWs ws;
  ws.tau = tau;
  ND4_TRY(het_alloc(h, (size_t)batch * N, &ws.dsc)); ND4_TRY(het_alloc(h, (size_t)batch * N, &ws.esc));
  ND4_TRY(het_alloc(h, (size_t)batch * 2 * N, &ws.vd)); ND4_TRY(het_alloc(h, (size_t)batch * 2 * N, &ws.rowsum));
  ND4_TRY(het_alloc(h, (size_t)batch * 2 * nblk * N, &ws.colpart));
  hipLaunchKernelGGL(hetrd_absmax, dim3(256u, (unsigned)batch), dim3(256), 0, h->stream, H, N, mx);
  hipLaunchKernelGGL(hetrd_load, dim3((unsigned)N, (unsigned)batch), dim3(256), 0, h->stream, H, F, N, mx);
  ND4_TRY(het_lds_attr(reinterpret_cast<const void*>(&hetrd_step), lds));
  for (int k = 0; k < N; ++k) hipLaunchKernelGGL(hetrd_step, dim3((unsigned)nblk, (unsigned)batch), dim3(256), lds, h->stream, F, N, k, ws);
  hipLaunchKernelGGL(hetrd_finish, dim3((unsigned)batch), dim3(256), 0, h->stream, F, N, ws, mx, d, e, unscale ? 1 : 0, flag);
  ND4_HIP(hipGetLastError());
  return 0;
}

// Z [batch, N, K] complex <- Q Z (adjoint: Q^H Z) in place, Q from F, tau of nd4_hetrd. batch <= 32768, 1 <= N <= 2048, K >= 1.
// Enqueues only.
int nd4_zunmtr(nd4hip_handle* h, int64_t batch, int64_t N64, int64_t K64, bool adjoint, const double* Fm, const double* taum, double* Zm) {
  ND4_CHECK_ARG(N64 >= 1 && N64 <= HET_MAXN && batch >= 1 && batch <= 32768 && K64 >= 1 && K64 < (1 << 30),
                "nd4hip_zunmtr_batched: extent out of range");
  const int N = (int)N64, K = (int)K64, nref = N - 1;
  if (nref <= 0) return 0;                                    // Q = I
  const cd* F = reinterpret_cast<const cd*>(Fm);
  const cd* tau = reinterpret_cast<const cd*>(taum);
  cd* Z = reinterpret_cast<cd*>(Zm);
  if (nd4_hetrd_tier(N) == 0) {
    const size_t lds = nd4_zunmtr_lds(N);
    const int64_t tiles = (K64 + HET_ZT - 1) / HET_ZT;
    ND4_CHECK_ARG(tiles <= 0x7fffffffll, "nd4hip_zunmtr_batched: extent out of range");
    ND4_TRY(het_lds_attr(reinterpret_cast<const void*>(&unmtr_small), lds));
    hipLaunchKernelGGL(unmtr_small, dim3((unsigned)tiles, (unsigned)batch), dim3(64), lds, h->stream, F, tau, Z, N, K, adjoint ? 1 : 0);
    ND4_HIP(hipGetLastError());
    return 0;
  }
  Nd4WsScope scope(h);
  cd *V, *Vh, *G, *T, *Y, *W;
  ND4_TRY(het_alloc(h, (size_t)batch * N * HET_WY, &V)); ND4_TRY(het_alloc(h, (size_t)batch * N * HET_WY, &Vh));
  ND4_TRY(het_alloc(h, (size_t)batch * HET_WY * HET_WY, &G)); ND4_TRY(het_alloc(h, (size_t)batch * HET_WY * HET_WY, &T));
  ND4_TRY(het_alloc(h, (size_t)batch * HET_WY * K, &Y)); ND4_TRY(het_alloc(h, (size_t)batch * HET_WY * K, &W));
  const int nblocks = (nref + HET_WY - 1) / HET_WY;
  const int64_t w2 = (int64_t)HET_WY * HET_WY, wk = (int64_t)HET_WY * K;
  const size_t tlds = 16 * (size_t)HET_WY * (HET_WY + 1);
  ND4_TRY(het_lds_attr(reinterpret_cast<const void*>(&unmtr_wy_t), tlds));
  const unsigned ktiles = (unsigned)((K + 255) / 256);
  for (int s = 0; s < nblocks; ++s) {
    const int k0 = (adjoint ? s : nblocks - 1 - s) * HET_WY, nb = std::min(HET_WY, nref - k0), rows = N - k0 - 1;
    const int64_t sv = (int64_t)rows * HET_WY;
    cd* Zs = Z + (size_t)(k0 + 1) * K;                        // rows k0 + 1 .. N - 1 of every member
    hipLaunchKernelGGL(unmtr_wy_v, dim3((unsigned)rows, (unsigned)batch), dim3(64), 0, h->stream, F, N, k0, nb, V, Vh);
    ND4_HIP(hipGetLastError());
    ND4_TRY(nd4_zgemm(h, true, batch, HET_WY, rows, HET_WY, reinterpret_cast<const double*>(Vh), sv, reinterpret_cast<const double*>(V), sv,
                      reinterpret_cast<double*>(G)));
    hipLaunchKernelGGL(unmtr_wy_t, dim3((unsigned)batch), dim3(64), tlds, h->stream, G, tau, N, k0, nb, adjoint ? 1 : 0, T);
    ND4_HIP(hipGetLastError());
    ND4_TRY(nd4_zgemm(h, true, batch, HET_WY, rows, K, reinterpret_cast<const double*>(Vh), sv, reinterpret_cast<const double*>(Zs),
                      (int64_t)N * K, reinterpret_cast<double*>(Y)));
    ND4_TRY(nd4_zgemm(h, true, batch, HET_WY, HET_WY, K, reinterpret_cast<const double*>(T), w2, reinterpret_cast<const double*>(Y), wk,
                      reinterpret_cast<double*>(W)));
    hipLaunchKernelGGL(unmtr_wy_sub, dim3(ktiles, (unsigned)rows, (unsigned)batch), dim3(256), 0, h->stream, V, W, Zs, rows, K, (long)N * K);
    ND4_HIP(hipGetLastError());
  }
  return 0;
}

// herm_tridiag_factor on device pointers: arguments already checked, batch in 1 .. 32768, 1 <= N <= 2048. Synchronises (the flag word).
int nd4_hetrd_run(nd4hip_handle* h, int64_t batch, int64_t N, const double* H, double* F, double* tau, double* d, double* e) {
  Nd4WsScope scope(h);
  u64* mx = nullptr; int* flag = nullptr; int bad = 0;
  ND4_TRY(het_alloc(h, (size_t)batch, &mx)); ND4_TRY(het_alloc(h, 1, &flag));
  ND4_HIP(hipMemsetAsync(mx, 0, sizeof(u64) * (size_t)batch, h->stream));
  ND4_HIP(hipMemsetAsync(flag, 0, sizeof(int), h->stream));
  ND4_TRY(nd4_hetrd(h, batch, N, H, F, tau, d, e, mx, true, flag));
  ND4_TRY(het_read_flag(h, flag, &bad));
  if (bad) {
    nd4_set_error("herm_tridiag_decomp(H): H contains NaN or Infinity in its lower triangle.");
    return ND4HIP_ERR_NOCONV;
  }
  return 0;
}

// the pieces the eigen routes take from this file (syev.hip: nd4_zheevd): the first two enqueue only, the N = 1 route synchronises
int nd4_hetrd_diagonals(nd4hip_handle* h, int64_t batch, int N, const double* F, double* Tr) {
  hipLaunchKernelGGL(hetrd_diagonals, dim3((unsigned)batch), dim3(256), 0, h->stream, reinterpret_cast<const cd*>(F), N, Tr);
  ND4_HIP(hipGetLastError());
  return 0;
}
int nd4_hetrd_rows_to_columns(nd4hip_handle* h, int64_t batch, int N, int k, const double* R, double* V) {
  hipLaunchKernelGGL(hetrd_rows_to_columns, dim3((unsigned)((N + 63) / 64), (unsigned)((k + 63) / 64), (unsigned)batch), dim3(256), 0, h->stream, R,
                     reinterpret_cast<cd*>(V), N, k);
  ND4_HIP(hipGetLastError());
  return 0;
}
int nd4_hetrd_order_one(nd4hip_handle* h, int64_t batch, const double* H, double* lambda, double* V) {
  Nd4WsScope scope(h);
  int* flag = nullptr; int bad = 0;
  ND4_TRY(het_alloc(h, 1, &flag));
  ND4_HIP(hipMemsetAsync(flag, 0, sizeof(int), h->stream));
  hipLaunchKernelGGL(hetrd_order_one, dim3((unsigned)((batch + 255) / 256)), dim3(256), 0, h->stream, reinterpret_cast<const cd*>(H), (long)batch,
                     lambda, reinterpret_cast<cd*>(V), flag);
  ND4_HIP(hipGetLastError());
  ND4_TRY(het_read_flag(h, flag, &bad));
  if (bad) {
    nd4_set_error("eigen_herm(H): H contains NaN or Infinity in its lower triangle.");
    return ND4HIP_ERR_NOCONV;
  }
  return 0;
}

// eigen_herm(H, subset): nd4_hetrd, nd4_stevx (syevx.hip) on (d, e) for the slice i0 .. i1 - 1 of the descending spectrum, and nd4_zunmtr
// on the k = i1 - i0 selected vectors: lambda [batch, k], V [batch, N, k] complex (columns) or NULL. Synchronises twice: the
// reduction's flag is read before the solver starts, so that its text is this route's.
int nd4_zheevx(nd4hip_handle* h, int64_t batch, int64_t N64, int64_t i0, int64_t i1, const double* H, double* lambda, double* V) {
  ND4_CHECK_ARG(N64 >= 1 && N64 <= HET_MAXN && batch >= 1 && batch <= 32768, "nd4hip_zheevx_batched: extent out of range");
  const int N = (int)N64, k = (int)(i1 - i0);
  if (N == 1) return nd4_hetrd_order_one(h, batch, H, lambda, V);
  Nd4WsScope scope(h);
  const size_t nn = (size_t)N * N;
  u64* mx = nullptr; int* flag = nullptr; int bad = 0;
  double *F, *tau, *d, *e, *Z = nullptr;
  ND4_TRY(het_alloc(h, (size_t)batch, &mx)); ND4_TRY(het_alloc(h, 1, &flag));
  ND4_TRY(het_alloc(h, 2 * (size_t)batch * nn, &F)); ND4_TRY(het_alloc(h, 2 * (size_t)batch * N, &tau));
  ND4_TRY(het_alloc(h, (size_t)batch * N, &d)); ND4_TRY(het_alloc(h, (size_t)batch * N, &e));
  if (V) ND4_TRY(het_alloc(h, (size_t)batch * k * N, &Z));
  ND4_HIP(hipMemsetAsync(mx, 0, sizeof(u64) * (size_t)batch, h->stream));
  ND4_HIP(hipMemsetAsync(flag, 0, sizeof(int), h->stream));
  double reduce_ms = 0.0;
  Nd4StageStamps<1> st(h, &reduce_ms);
  st.mark();
  ND4_TRY(nd4_hetrd(h, batch, N, H, F, tau, d, e, mx, true, flag));
  st.mark();
  ND4_TRY(het_read_flag(h, flag, &bad));
  st.collect();
  if (bad) {
    nd4_set_error("eigen_herm(H): H contains NaN or Infinity in its lower triangle.");
    return ND4HIP_ERR_NOCONV;
  }
  ND4_TRY(nd4_stevx(h, batch, N, i0, i1, d, e, lambda, Z));    // synchronises; sets the solver's stage times
  h->syevx_stage_ms[1] = reduce_ms;
  if (V) {
    ND4_TRY(nd4_hetrd_rows_to_columns(h, batch, N, k, Z, V));
    ND4_TRY(nd4_zunmtr(h, batch, N, k, false, F, tau, V));
  }
  return 0;
}
