// svd_dc.hip: divide & conquer SVD of an upper bidiagonal matrix on the device, and svd_decomp through it (algo = 'dc').
//
// The reference's svd_decomp IS this algorithm (src/la/svd_dc.js:37-932): bidiagonalise, then solve the K x (K+1) bidiagonal
// problem by divide & conquer. The kernels below restate its stages in its own order, with oracle/nd4_oracle_svd_dc.c (the
// line-cited C restatement that is pinned to the goldens) as the specification. Line numbers in the comments are svd_dc.js's.
//
// Tree (_svd_dc_bidiag, :666-824). A node is a block of n columns, n - 1 rows, at offset `off` of the (K+1)-column problem; it
// splits at n0 = n >> 1 into (off, n0) and (off + n0, n - n0), row n0 - 1 is the middle row that joins the two. Nodes of
// n = 2 and n = 3 are leaves with closed forms (:37-143). The recursion is replaced by a host-computed list of levels
// (dc_plan): level 0 holds every leaf, level l >= 1 the merges of one depth, the deepest depth first, so both children of a merge
// always sit in an earlier level. The nodes of one depth differ in size by at most one. All merges of a level, over all batch
// members, are independent: each stage is ONE launch per level with the merge in one grid dimension and the member in
// another. Nothing waits on another workgroup inside a kernel; the launch boundary is the only synchronisation.
//
// Per level (_svd_dc_neves, :169-657), m = n - 1 values per merge:
//   dc_prep    one workgroup per merge: the z row b1 V[m0, :], b2 V[n0, :], the Givens rotation that zeroes the last column
//              (:737-794), the merge of the two sorted diagonals into the outer order (:803-822), normalisation by `scale`
//              (:211-229) and the two deflations with their rotation bookkeeping (:261-378). The sequential parts are short,
//              data dependent compactions: thread 0 runs them on LDS copies, in the reference's order. O(m) steps.
//   dc_roots   one wave per secular root (:389-437): the reference's shift choice, then bisection in the shifted variable until
//              the midpoint equals an end point; the m terms of the secular sum are spread over the 64 lanes and added by a
//              butterfly, so every lane holds the same bits. At most DC_BISECT_CAP steps (derivation at the constant).
//   dc_zhat    one wave per entry: the Gu-Eisenstat recomputation of z (:443-469) as a product of O(1) ratios, lanes over the
//              factors; one more workgroup per merge runs the triple merge that gives the inner order (:473-488).
//   dc_wbuild  one wave per row of the two W matrices (:493-519, :569-601): build, normalise (scaled 2-norm), store transposed.
//   dc_wrot    one thread per column of W: the identity block of the deflated part and the stored deflation rotations in the
//              reference's order (:521-541, :603-621). The rotations act on rows, so the columns are independent and each
//              thread applies the whole sequence to its own column: the order is kept without a barrier. Also writes the
//              level's singular values back (:651-658).
//   updates    U <- U[:, outer] W^T scattered by the inner order, the same for V (:544-564, :624-644): dc_gather packs the
//              permuted blocks of all merges into one uniformly strided batch (padded with zeros to the level's largest m),
//              ONE call of the fp64 MFMA GEMM (nd4_gemm, batched) multiplies them, dc_scatter writes them back. A level whose
//              largest m is <= DC_SMALL_M runs dc_apply_small instead: gather, product and scatter of one merge in one
//              workgroup through LDS (three launches and two round trips through memory cost more than the product there).
//
// Errors. Where the reference throws 'Assertion failed.' the kernel stores that line number into the call's flag word (the
// first one wins) and leaves; every later kernel of the call returns at once when the word is set, so nothing is indexed by
// data that failed a check. All loops have fixed bounds (m, or DC_BISECT_CAP), so no input can hold the device. The entry
// point reads the word back once, at the end.
//
// Every index that is read from memory (outer / inner order, rotation partner) is produced by counting loops whose bounds do
// not depend on the floating-point data, so it is in range for any input, NaN included.
#include "nd4hip_internal.h"
#include <cmath>
#include <cfloat>
#include <cstring>
#include <vector>

namespace {

constexpr int DC_MAXM = 2048;              // largest K: the LDS copies of one merge (dc_prep: 56 KB) are sized for it
// Up to this m the update of a merge is one workgroup (dc_apply_small); above, gather + batched GEMM + scatter. Measured with
// 8, 16, 32 and 64 (bidiag_svd, median of 10): 64 x 512 values 8.64 / 8.51 / 8.47 / 8.46 ms, 1024 x 64 values 7.24 / 7.09 /
// 6.98 / 7.04 ms, one problem of 2048 values 6.08 / 6.01 / 6.04 / 6.04 ms. The levels below m = 64 are a few per cent of the
// solver; 32 is the best or within 0.2 % of it everywhere and keeps the kernel's LDS at 16.5 KB.
constexpr int DC_SMALL_M = 32;
// Bisection length. The data of a merge are normalised by `scale`, so d_i <= 1 and zNorm <= 1: the shifted interval starts
// inside [2^-1074, 2] (or its mirror image) and every iterate is a double in it. A step that does not terminate puts the
// midpoint strictly between the ends. While the ends lie in different binades the midpoint is at least half the larger end
// (in magnitude), so a step either lowers the larger end by a binade or brings the smaller end within a factor two of it: at
// most 1076 such steps. Two ends within a factor two have at most 2^53 doubles between them and the midpoint halves that
// count: at most 53 more steps. 1076 + 53 = 1129 < 1200.
constexpr int DC_BISECT_CAP = 1200;
constexpr double DC_EPS = 2.220446049250313e-16;            // Number.EPSILON
constexpr double DC_MINV = 4.9406564584124654e-324;         // Number.MIN_VALUE

struct DcNode { int off, n; };

// Device state of one chunk of the batch. N = K + 1 columns; per member: U [N-1, N-1], V [N, N], vectors of N (or 2 N).
struct DcBufs {
  double* U; long sU;        // left vectors, leading dimension N - 1
  double* V; long sV;        // right vectors as COLUMNS (the reference's V1), leading dimension N
  double* dd;                // [N] the diagonal; holds each finished node's singular values
  double* ee;                // [N] the super-diagonal (e[N-2] = 0 when the input has J = K columns)
  double* dw; double* zw;    // [N] one level's normalised, ordered, compacted (d, z)
  double* sg;                // [N] sigma: deflated values, shifted secular roots
  double* rc;                // [2 N] (c, s) of the deflation rotations
  double* metaD;             // [2 N] (scale, zNorm) at 2 off
  int* outI; int* innI; int* rotI;   // [N] outer order, inner order, rotation partner (block relative)
  int* metaI;                // [2 N] (n0, n1) at 2 off
  int N;
};

__device__ __forceinline__ void dc_fail(int* flag, int line) { atomicCAS(flag, 0, line); }

// _giv_rot.js:22-37
__device__ __forceinline__ void dc_givens(double a, double b, double& c, double& s, double& nrm) {
  const double fa = fabs(a), fb = fabs(b), mx = fa > fb ? fa : fb;
  if (0.0 == mx) { c = 1; s = 0; nrm = 0; return; }
  a /= mx; b /= mx;
  double n = sqrt(a * a + b * b);
  c = a / n; s = b / n; nrm = n * mx;
}

// _svd_jac_utils.js:72-114
__device__ void dc_jac_angles(double S_pp, double S_pq, double S_qp, double S_qq, double& ca, double& sa, double& cb, double& sb) {
  double x = atan2(S_qp - S_pq, S_qq + S_pp), y = atan2(S_qp + S_pq, S_qq - S_pp);
  const double a = (x - y) / 2, b = (x + y) / 2;
  ca = cos(a); sa = sin(a); cb = cos(b); sb = sin(b);
  x = cb * (sa * S_qp + ca * S_pp) - sb * (sa * S_qq + ca * S_pq);
  y = sb * (ca * S_qp - sa * S_pp) + cb * (ca * S_qq - sa * S_pq);
  if (fabs(x) < fabs(y)) {
    double t = sa; sa = ca; ca = -t;
    t = cb; cb = sb; sb = -t;
    x = y;
  }
  if (x < 0) { cb = -cb; sb = -sb; }
}

// norm.js:22-67: scaled sum of squares
struct DcFro { double sum, mx; };
__device__ __forceinline__ void dc_fro_inc(DcFro& f, double x) {
  x = fabs(x);
  if (x != 0) {
    if (f.mx < x) { const double s = f.mx / x; f.sum *= s * s; f.mx = x; }
    x /= f.mx;
    f.sum += x * x;
  }
}
__device__ __forceinline__ double dc_fro_res(const DcFro& f) { return isfinite(f.mx) ? sqrt(f.sum) * f.mx : f.mx; }

// butterflies: every lane ends with the same bits (a + b and b + a round alike)
__device__ __forceinline__ double dc_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ __forceinline__ double dc_wave_prod(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v *= __shfl_xor(v, o);
  return v;
}
__device__ __forceinline__ double dc_wave_max(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
  return v;
}

// dd / ee from a strided diagonal and super-diagonal: d[i dinc], e[i einc]; e beyond ne is 0
__global__ __launch_bounds__(256) void dc_init(DcBufs B, const double* __restrict__ d, long dinc, long sd,
                                               const double* __restrict__ e, long einc, long se, int ne) {
  const int i = blockIdx.x * 256 + threadIdx.x, N = B.N;
  const long b = blockIdx.y;
  if (i >= N) return;
  B.dd[b * N + i] = i < N - 1 ? d[b * sd + i * dinc] : 0.0;
  B.ee[b * N + i] = i < ne ? e[b * se + i * einc] : 0.0;
}

// the leaves: _svd_dc_1x2 (:37-61) and _svd_dc_2x3 (:72-143); U and V are zero on entry
__global__ __launch_bounds__(64) void dc_leaves(DcBufs B, const DcNode* __restrict__ nodes, int count) {
  const int q = blockIdx.x * 64 + threadIdx.x;
  if (q >= count) return;
  const long b = blockIdx.y;
  const DcNode nd = nodes[q];
  const long N = B.N, M = N - 1;
  double* U = B.U + b * B.sU + nd.off * M + nd.off;
  double* V = B.V + b * B.sV + nd.off * N + nd.off;
  double* d = B.dd + b * N + nd.off;
  const double* e = B.ee + b * N + nd.off;
  if (nd.n == 2) {
    double c, s, nrm;
    dc_givens(d[0], e[0], c, s, nrm);
    if (0 != nrm) { d[0] = nrm; V[0] = c; V[1] = -s; V[N] = s; V[N + 1] = c; }
    else { V[0] = 1; V[N + 1] = 1; }
    U[0] = 1;
    return;
  }
  double b1 = d[0], b2 = e[0], b3 = d[1], b4 = e[1];
  if (0 != b4) {
    double ca, sa, nrm;
    dc_givens(b3, b4, ca, sa, nrm);
    V[N + 1] = ca;
    V[2 * N + 1] = sa;
    b3 = nrm;
    b4 = -sa * b2;
    b2 = ca * b2;
    if (0 != b4) {
      double cb, sb, nrm2;
      dc_givens(b1, b4, cb, sb, nrm2);
      b1 = nrm2;
      V[0] = cb; V[N] = sb * -sa; V[2 * N] = sb * ca;
      V[2] = -sb; V[N + 2] = cb * -sa; V[2 * N + 2] = cb * ca;
    } else {
      V[0] = 1; V[N + 2] = -sa; V[2 * N + 2] = ca;
    }
  } else {
    V[0] = 1; V[N + 1] = 1; V[2 * N + 2] = 1;
  }
  double ca, sa, cb, sb;
  dc_jac_angles(b1, b2, 0, b3, ca, sa, cb, sb);
  d[0] = ca * b1 * cb - (ca * b2 + sa * b3) * sb;
  b3 = (-sa * b2 + ca * b3) * cb - sa * b1 * sb;
  const double sgn = b3 < 0 ? -1 : +1;
  d[1] = sgn * b3;
  U[0] = ca; U[1] = -sa * sgn; U[M] = sa; U[M + 1] = ca * sgn;
  V[1] = sb * V[0];
  V[0] *= cb;
  const double V1 = V[N] * cb - V[N + 1] * sb;
  V[N + 1] = V[N] * sb + V[N + 1] * cb;
  V[N] = V1;
  const double V2 = V[2 * N] * cb - V[2 * N + 1] * sb;
  V[2 * N + 1] = V[2 * N] * sb + V[2 * N + 1] * cb;
  V[2 * N] = V2;
}

// preparation and deflation of one merge (:737-822, :195-378)
__global__ __launch_bounds__(256) void dc_prep(DcBufs B, const DcNode* __restrict__ nodes, int* __restrict__ flag) {
  __shared__ double sD[DC_MAXM], sZ[DC_MAXM];
  __shared__ int sOut[DC_MAXM], sInn[DC_MAXM], sRot[DC_MAXM];
  __shared__ double sScale;
  __shared__ int sFail;
  const int t = threadIdx.x;
  if (t == 0) sFail = *flag;               // another merge of this launch may raise it meanwhile: one read decides for all waves
  __syncthreads();
  if (sFail) return;
  const long b = blockIdx.y;
  const DcNode nd = nodes[blockIdx.x];
  const long N = B.N, M = N - 1;
  const int n = nd.n, m = n - 1, h0 = n >> 1, m0 = h0 - 1, off = nd.off;
  double* U = B.U + b * B.sU + off * M + off;
  double* V = B.V + b * B.sV + off * N + off;
  double* dd = B.dd + b * N + off;
  const double b1 = dd[m0], b2 = B.ee[b * N + off + m0];
  double c, s, hh;
  dc_givens(b1 * V[m0 * N + m0], b2 * V[h0 * N + m], c, s, hh);                   // :779-782
  for (int i = t; i < m; i += 256) sZ[i] = i == m0 ? 0.0 : dd[i];                 // the children's values, unsorted
  __syncthreads();                                                                // ... and everyone holds (c, s, hh)
  if (t == 0) {
    U[m0 * M + m0] = 1;
    sOut[m - 1] = m0;                                                             // :803-809
    for (int i = 0, j = h0, k = 0; k < m - 1; k++) sOut[k] = (j >= m || (i < m0 && sZ[i] >= sZ[j])) ? i++ : j++;
  }
  if (0 != hh)                                                                    // :789-794
    for (int i = t; i < n; i += 256) {
      if (i < h0) { const double v = V[i * N + m0]; V[i * N + m] = v * -s; V[i * N + m0] = v * c; }
      else        { const double v = V[i * N + m];  V[i * N + m0] = v * s; V[i * N + m] = v * c; }
    }
  __syncthreads();
  for (int i = t; i < m; i += 256) sD[i] = sZ[sOut[i]];
  __syncthreads();
  for (int i = t; i < m; i += 256) {                                              // :741-742 in the outer order; columns m0 and m are not read
    const int p = sOut[i];
    sZ[i] = p < m0 ? b1 * V[m0 * N + p] : (p == m0 ? hh : b2 * V[h0 * N + p]);
  }
  __syncthreads();
  double zNorm = 0;
  if (t == 0) {
    int bad = 0;
    if (sD[m - 1] != 0) bad = 202;
    for (int i = 1; i < m && !bad; i++) if (sD[i - 1] < sD[i]) bad = 206;
    DcFro f = {0.0, 0.0};                                                         // :211-225
    for (int i = 0; i < m; i++) dc_fro_inc(f, sZ[i]);
    zNorm = dc_fro_res(f);
    for (int i = 0; i < m; i++) dc_fro_inc(f, sD[i]);
    double scale = dc_fro_res(f);
    if (scale == 0) scale = 1;
    zNorm = zNorm / scale;
    sScale = scale;
    if (bad) { dc_fail(flag, bad); sFail = 1; }
  }
  __syncthreads();
  if (sFail) return;
  const double scale = sScale;
  for (int i = t; i < m; i += 256) { sD[i] /= scale; sZ[i] /= scale; }           // :228-229
  __syncthreads();
  if (t == 0) {
    double* sg = B.sg + b * N + off;
    double* rc = B.rc + (b * N + off) * 2;
    int n0 = 0;
    for (int j = m - 1, i = m - 1; i-- > 0;) {                                    // deflation of z = 0 (:261-281)
      const double di = sD[i], zi = sZ[i];
      const int oi = sOut[i];
      if (fabs(zi) / DC_EPS <= di) { sg[n0] = di; sInn[n0] = oi; ++n0; }
      else { --j; sD[j] = di; sZ[j] = zi; sInn[j] = oi; }
    }
    for (int i = 0; i < n0; i++) sOut[i] = sInn[i];                               // :284-285
    int n1 = n0;
    const double sqm = sqrt((double)m);
    for (int j = m - 1, i = m - 1; i-- > n0;) {                                   // equal diagonal entries (:346-378)
      const double di = sD[i], dj = sD[j];
      const int oi = sInn[i];
      const double zi = sZ[i], zj = sZ[j];
      double cc, ss, z;
      dc_givens(zj, zi, cc, ss, z);
      if ((di - dj) / DC_EPS <= di || !isfinite(sqm / (di - dj))) {
        rc[2 * n1] = cc; rc[2 * n1 + 1] = ss;
        sZ[j] = z;
        sD[j] = di; sg[n1] = di;
        sOut[n1] = oi;
        sRot[n1] = j;
        ++n1;
      } else { --j; sD[j] = di; sZ[j] = zi; sOut[j] = oi; }
    }
    B.metaI[(b * N + off) * 2] = n0; B.metaI[(b * N + off) * 2 + 1] = n1;
    B.metaD[(b * N + off) * 2] = scale; B.metaD[(b * N + off) * 2 + 1] = zNorm;
  }
  __syncthreads();
  for (int i = t; i < m; i += 256) {
    B.dw[b * N + off + i] = sD[i]; B.zw[b * N + off + i] = sZ[i];
    B.outI[b * N + off + i] = sOut[i]; B.rotI[b * N + off + i] = sRot[i];
  }
}

// the secular equations, one wave per root (:389-437)
__global__ __launch_bounds__(256) void dc_roots(DcBufs B, const DcNode* __restrict__ nodes, int* __restrict__ flag) {
  __shared__ double sD[DC_MAXM], sZ[DC_MAXM];
  if (*flag) return;
  const int t = threadIdx.x, lane = t & 63;
  const long b = blockIdx.z;
  const DcNode nd = nodes[blockIdx.y];
  const long N = B.N, base = b * N + nd.off;
  const int m = nd.n - 1, n1 = B.metaI[base * 2 + 1];
  if (n1 + (int)blockIdx.x * 4 >= m) return;
  for (int k = n1 + t; k < m; k += 256) { sD[k] = B.dw[base + k]; sZ[k] = B.zw[base + k]; }
  __syncthreads();
  const int i = n1 + blockIdx.x * 4 + (t >> 6);
  if (i >= m) return;
  const double zNorm = B.metaD[base * 2 + 1];
  double sLo = sD[i], sHi = n1 < i ? sD[i - 1] : (sLo + zNorm);
  if (sLo > sHi) { dc_fail(flag, 393); return; }
  double shift = 0;
  bool taken = false;
  if (i > n1) {                                                                   // the shift: the nearer pole (:396-412)
    const double mid = (sLo + sHi) / 2;
    double part = 0;
    for (int k = n1 + lane; k < m; k += 64) { const double dk = sD[k], zk = sZ[k]; part += zk / (dk - mid) * (zk / (dk + mid)); }
    const double sum = 1 + dc_wave_sum(part);
    if (!isfinite(sum)) { dc_fail(flag, 405); return; }
    if (sum < 0) { shift = sHi; sLo = sLo - sHi; sHi = -DC_MINV; taken = true; }
  }
  if (!taken) { shift = sLo; sHi = sHi - sLo; sLo = +DC_MINV; }
  double res = 0;
  int it = 0;
  for (; it < DC_BISECT_CAP; ++it) {
    const double x = (sLo + sHi) / 2;
    if (x == sLo || x == sHi) { res = x; break; }
    double part = 0;
    for (int k = n1 + lane; k < m; k += 64) { const double dk = sD[k], zk = sZ[k]; part += zk / (dk - shift - x) * (zk / (dk + shift + x)); }
    const double sum = 1 + dc_wave_sum(part);
    if (!isfinite(sum)) { dc_fail(flag, 429); return; }
    if (sum <= 0) sLo = x;
    if (sum >= 0) sHi = x;
  }
  if (it == DC_BISECT_CAP) { dc_fail(flag, 429); return; }                        // cannot happen on finite data (see the constant)
  if (i == m - 1 && fabs(sZ[m - 1]) == 0) res = 0;                                // :437-440 (d[m-1] is 0 already)
  if (lane == 0) B.sg[base + i] = res;
}

// z recomputed from the roots, one wave per entry (:443-469); the last workgroup of a merge runs the triple merge (:473-488)
__global__ __launch_bounds__(256) void dc_zhat(DcBufs B, const DcNode* __restrict__ nodes, int* __restrict__ flag) {
  __shared__ double sD[DC_MAXM], sS[DC_MAXM];
  if (*flag) return;
  const int t = threadIdx.x, lane = t & 63;
  const long b = blockIdx.z;
  const DcNode nd = nodes[blockIdx.y];
  const long N = B.N, base = b * N + nd.off;
  const int m = nd.n - 1, n0 = B.metaI[base * 2], n1 = B.metaI[base * 2 + 1];
  const bool order = blockIdx.x == gridDim.x - 1;
  if (!order && n1 + (int)blockIdx.x * 4 >= m) return;
  for (int k = t; k < m; k += 256) { sD[k] = B.dw[base + k]; sS[k] = B.sg[base + k]; }
  __syncthreads();
  if (order) {
    if (t != 0) return;
    int* inn = B.innI + base;
    for (int h = n0 - 1, i = n1 - 1, j = n1, k = 0; k < m; k++) {
      double val = -INFINITY;
      int best = 3;
      if (j < m) { const double sj_ = sS[j]; best = 2; val = sj_ + sD[j - (sj_ < 0 && j > n1)]; }
      if (i >= n0) { const double si_ = sS[i]; if (!(si_ < val)) { best = 1; val = si_; } }
      if (h >= 0) { const double sh_ = sS[h]; if (!(sh_ < val)) { best = 0; val = sh_; } }
      if (best == 0) inn[h--] = k;
      else if (best == 1) inn[i--] = k;
      else if (best == 2) inn[j++] = k;
      else { dc_fail(flag, 486); return; }
    }
    return;
  }
  const int i = n1 + blockIdx.x * 4 + (t >> 6);
  if (i >= m) return;
  const double sn_ = sS[m - 1], sn = sD[m - 1 - (sn_ < 0 && m - 1 > n1)], di = sD[i];
  const double lead = (sn - di + sn_) * (sn + di + sn_);
  double p = 1;
  for (int j = n1 + lane; j < m - 1; j += 64) {                                   // each factor is a ratio of O(1)
    const double sj_ = sS[j], sj = sD[j - (sj_ < 0 && j > n1)], dj = sD[j + (j >= i)];
    p *= ((sj - di + sj_) / (dj - di)) * ((sj + di + sj_) / (dj + di));
  }
  const double zi = lead * dc_wave_prod(p);
  if (lane == 0) {
    const double z = B.zw[base + i];
    B.zw[base + i] = (z > 0 ? 1.0 : (z < 0 ? -1.0 : z)) * sqrt(zi);
  }
}

// the two W matrices, one wave per row, stored transposed into the level's packed [merge][mmax][mmax] buffers, which are zero
__global__ __launch_bounds__(256) void dc_wbuild(DcBufs B, const DcNode* __restrict__ nodes, int* __restrict__ flag,
                                                 double* __restrict__ WU, double* __restrict__ WV, int mmax, long sW) {
  __shared__ double sD[DC_MAXM], sZ[DC_MAXM];
  if (*flag) return;
  const int t = threadIdx.x, lane = t & 63;
  const long b = blockIdx.z;
  const DcNode nd = nodes[blockIdx.y];
  const long N = B.N, base = b * N + nd.off;
  const int m = nd.n - 1, n1 = B.metaI[base * 2 + 1];
  if (n1 + (int)blockIdx.x * 4 >= m) return;
  for (int k = n1 + t; k < m; k += 256) { sD[k] = B.dw[base + k]; sZ[k] = B.zw[base + k]; }
  __syncthreads();
  const int i = n1 + blockIdx.x * 4 + (t >> 6);
  if (i >= m) return;
  const double si_ = B.sg[base + i], si = sD[i - (si_ < 0 && i > n1)];
  double* wu = WU + b * sW + (long)blockIdx.y * mmax * mmax;
  double* wv = WV + b * sW + (long)blockIdx.y * mmax * mmax;
  {                                                                               // U (:493-519); the last entry of a row is -1
    double mx = 1;
    for (int j = n1 + lane; j < m - 1; j += 64) { const double dj = sD[j], zj = sZ[j]; mx = fmax(mx, fabs((zj / (dj - si - si_)) * (dj / (dj + si + si_)))); }
    mx = dc_wave_max(mx);
    double part = lane == 0 ? (1 / mx) * (1 / mx) : 0.0;
    for (int j = n1 + lane; j < m - 1; j += 64) { const double dj = sD[j], zj = sZ[j], w = (zj / (dj - si - si_)) * (dj / (dj + si + si_)) / mx; part += w * w; }
    const double sum = dc_wave_sum(part), nrm = isfinite(mx) ? sqrt(sum) * mx : mx;
    if (!(0 < nrm)) { dc_fail(flag, 507); return; }
    for (int j = n1 + lane; j < m - 1; j += 64) { const double dj = sD[j], zj = sZ[j]; wu[(long)j * mmax + i] = (zj / (dj - si - si_)) * (dj / (dj + si + si_)) / nrm; }
    if (lane == 0) wu[(long)(m - 1) * mmax + i] = -1 / nrm;
  }
  {                                                                               // V (:569-601)
    double mx = 0;
    for (int j = n1 + lane; j < m; j += 64) { const double dj = sD[j], zj = sZ[j]; mx = fmax(mx, fabs(zj / (dj - si - si_) / (dj + si + si_))); }
    mx = dc_wave_max(mx);
    double part = 0;
    if (mx != 0) for (int j = n1 + lane; j < m; j += 64) { const double dj = sD[j], zj = sZ[j], w = zj / (dj - si - si_) / (dj + si + si_) / mx; part += w * w; }
    const double sum = dc_wave_sum(part), nrm = isfinite(mx) ? sqrt(sum) * mx : mx;
    if (!(0 < nrm || i == m - 1)) { dc_fail(flag, 583); return; }
    const bool unit = i == m - 1 && 0 == sZ[m - 1];                               // :589-593
    for (int j = n1 + lane; j < m; j += 64) {
      const double dj = sD[j], zj = sZ[j];
      wv[(long)j * mmax + i] = unit ? (j == m - 1 ? 1.0 : 0.0) : zj / (dj - si - si_) / (dj + si + si_) / nrm;
    }
  }
}

// one thread per column c of a merge's two W matrices: the identity of the deflated part, then the deflation rotations in the
// reference's order (:521-541, :603-621); blockIdx.z & 1 selects V. The U pass also writes the level's values back (:651-658).
__global__ __launch_bounds__(256) void dc_wrot(DcBufs B, const DcNode* __restrict__ nodes, int* __restrict__ flag,
                                               double* __restrict__ WU, double* __restrict__ WV, int mmax, long sW) {
  if (*flag) return;
  const long b = blockIdx.z >> 1;
  const bool isV = blockIdx.z & 1;
  const DcNode nd = nodes[blockIdx.y];
  const long N = B.N, base = b * N + nd.off;
  const int m = nd.n - 1, n0 = B.metaI[base * 2], n1 = B.metaI[base * 2 + 1];
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= m) return;
  if (!isV) {
    const double s_ = B.sg[base + c];
    const double val = c >= n1 ? s_ + B.dw[base + c - (s_ < 0 && c > n1)] : s_;
    B.dd[base + B.innI[base + c]] = val * B.metaD[base * 2];
  }
  double* W = (isV ? WV : WU) + b * sW + (long)blockIdx.y * mmax * mmax;
  if (c < n1) W[(long)c * mmax + c] = 1;
  for (int i = (c < n1 - 1 ? c : n1 - 1); i >= n0; --i) {
    const int j = B.rotI[base + i];
    if ((unsigned)j >= (unsigned)m || (!isV && j >= m - 1)) continue;
    const double cc = B.rc[(base + i) * 2], ss = B.rc[(base + i) * 2 + 1];
    const double wi = W[(long)i * mmax + c], wj = W[(long)j * mmax + c];
    W[(long)i * mmax + c] = cc * wi + ss * wj;
    W[(long)j * mmax + c] = cc * wj - ss * wi;
  }
}

// G[merge][r][i] = Blk[r][outer[i]], zero padded to [rmax][mmax]; grid (ceil(mmax / 64), rmax, merges * members)
__global__ __launch_bounds__(64) void dc_gather(DcBufs B, const DcNode* __restrict__ nodes, int nm, const int* __restrict__ flag, int isV,
                                                double* __restrict__ G, int rmax, int mmax) {
  if (*flag) return;
  const int q = blockIdx.z % nm;
  const long b = blockIdx.z / nm;
  const DcNode nd = nodes[q];
  const long N = B.N, ld = isV ? N : N - 1;
  const int m = nd.n - 1, rows = isV ? nd.n : m;
  const int i = blockIdx.x * 64 + threadIdx.x, r = blockIdx.y;
  if (i >= mmax) return;
  const double* blk = (isV ? B.V + b * B.sV : B.U + b * B.sU) + nd.off * ld + nd.off;
  G[((long)blockIdx.z * rmax + r) * mmax + i] = (r < rows && i < m) ? blk[r * ld + B.outI[b * N + nd.off + i]] : 0.0;
}

// Blk[r][inner[i]] = R[merge][r][i]
__global__ __launch_bounds__(64) void dc_scatter(DcBufs B, const DcNode* __restrict__ nodes, int nm, const int* __restrict__ flag, int isV,
                                                 const double* __restrict__ R, int rmax, int mmax) {
  if (*flag) return;
  const int q = blockIdx.z % nm;
  const long b = blockIdx.z / nm;
  const DcNode nd = nodes[q];
  const long N = B.N, ld = isV ? N : N - 1;
  const int m = nd.n - 1, rows = isV ? nd.n : m;
  const int i = blockIdx.x * 64 + threadIdx.x, r = blockIdx.y;
  if (i >= m || r >= rows) return;
  double* blk = (isV ? B.V + b * B.sV : B.U + b * B.sU) + nd.off * ld + nd.off;
  blk[r * ld + B.innI[b * N + nd.off + i]] = R[((long)blockIdx.z * rmax + r) * mmax + i];
}

// m <= DC_SMALL_M: both updates of one merge in one workgroup
__global__ __launch_bounds__(256) void dc_apply_small(DcBufs B, const DcNode* __restrict__ nodes, const int* __restrict__ flag,
                                                      const double* __restrict__ WU, const double* __restrict__ WV, int mmax, long sW) {
  __shared__ double sB[(DC_SMALL_M + 1) * DC_SMALL_M], sW_[DC_SMALL_M * DC_SMALL_M];
  __shared__ int sO[DC_SMALL_M], sI[DC_SMALL_M];
  if (*flag) return;
  const int t = threadIdx.x;
  const long b = blockIdx.y;
  const DcNode nd = nodes[blockIdx.x];
  const long N = B.N;
  const int m = nd.n - 1;
  if (t < m) { sO[t] = B.outI[b * N + nd.off + t]; sI[t] = B.innI[b * N + nd.off + t]; }
  for (int isV = 0; isV < 2; ++isV) {
    const long ld = isV ? N : N - 1;
    const int rows = isV ? nd.n : m;
    double* blk = (isV ? B.V + b * B.sV : B.U + b * B.sU) + nd.off * ld + nd.off;
    const double* W = (isV ? WV : WU) + b * sW + (long)blockIdx.x * mmax * mmax;
    __syncthreads();
    for (int e = t; e < m * m; e += 256) sW_[e] = W[(long)(e / m) * mmax + e % m];
    for (int e = t; e < rows * m; e += 256) sB[e] = blk[(e / m) * ld + sO[e % m]];
    __syncthreads();
    for (int e = t; e < rows * m; e += 256) {
      const int r = e / m, j = e % m;
      double acc = 0;
      for (int i = 0; i < m; ++i) acc += sB[r * m + i] * sW_[i * m + j];
      blk[r * ld + sI[j]] = acc;
    }
  }
}

// the level list of a problem of n columns: leaves first, then the merges of each depth, the deepest first
struct DcPlan {
  std::vector<DcNode> nodes;
  struct Level { int first, count, mmax; };
  std::vector<Level> levels;          // levels[0]: the leaves
};

void dc_plan_rec(int off, int n, int depth, std::vector<DcNode>& leaves, std::vector<std::vector<DcNode>>& merges) {
  if (n <= 3) { leaves.push_back({off, n}); return; }
  if ((int)merges.size() <= depth) merges.resize(depth + 1);
  merges[depth].push_back({off, n});
  dc_plan_rec(off, n >> 1, depth + 1, leaves, merges);
  dc_plan_rec(off + (n >> 1), n - (n >> 1), depth + 1, leaves, merges);
}

DcPlan dc_plan(int n) {
  DcPlan p;
  std::vector<DcNode> leaves;
  std::vector<std::vector<DcNode>> merges;
  dc_plan_rec(0, n, 0, leaves, merges);
  p.levels.push_back({0, (int)leaves.size(), 2});
  p.nodes = leaves;
  for (size_t d = merges.size(); d-- > 0;) {
    int mmax = 0;
    for (const DcNode& nd : merges[d]) mmax = nd.n - 1 > mmax ? nd.n - 1 : mmax;
    p.levels.push_back({(int)p.nodes.size(), (int)merges[d].size(), mmax});
    p.nodes.insert(p.nodes.end(), merges[d].begin(), merges[d].end());
  }
  return p;
}

// Per-stage HIP-event times of one call, kept while the handle's profile is enabled (tools/time_svd_dc.py): mark(s) opens stage
// s at this point of the stream and closes the one before it; collect() runs after the call's synchronisation.
struct DcStamps {
  nd4hip_handle* h; bool on;
  std::vector<hipEvent_t> ev; std::vector<int> stage;
  explicit DcStamps(nd4hip_handle* hh) : h(hh), on(hh->prof_on) {}
  void mark(int s) {
    if (!on) return;
    hipEvent_t e = nullptr;
    if (hipEventCreate(&e) != hipSuccess) { on = false; return; }
    (void)hipEventRecord(e, h->stream);
    ev.push_back(e); stage.push_back(s);
  }
  void collect() {
    for (int i = 0; i < ND4HIP_DC_STAGES; ++i) h->dc_stage_ms[i] = 0.0;
    for (size_t i = 0; i + 1 < ev.size(); ++i) {
      float ms = 0.f;
      if (on && stage[i] >= 0 && hipEventElapsedTime(&ms, ev[i], ev[i + 1]) == hipSuccess) h->dc_stage_ms[stage[i]] += ms;
    }
    for (hipEvent_t e : ev) (void)hipEventDestroy(e);
    ev.clear(); stage.clear();
  }
  ~DcStamps() { for (hipEvent_t e : ev) (void)hipEventDestroy(e); }
};
enum { DC_ST_BIDIAG = 0, DC_ST_LEAVES, DC_ST_PREP, DC_ST_ROOTS, DC_ST_ZHAT, DC_ST_W, DC_ST_MERGE, DC_ST_FINAL };

template <class T> int dc_alloc(nd4hip_handle* h, size_t count, T** out) {
  void* p = nullptr;
  ND4_TRY(nd4_ws_alloc(h, sizeof(T) * count, &p));
  *out = static_cast<T*>(p);
  return 0;
}

}  // namespace

// host-side copy of the level list for the tests: (level, off, n) per node in launch order; returns the number of nodes
int nd4_bdsdc_plan(int64_t n, int32_t* out, int64_t capacity) {
  const DcPlan p = dc_plan((int)n);
  int64_t k = 0;
  for (size_t l = 0; l < p.levels.size(); ++l)
    for (int i = 0; i < p.levels[l].count; ++i, ++k)
      if (out && k < capacity) { out[3 * k] = (int32_t)l; out[3 * k + 1] = p.nodes[p.levels[l].first + i].off; out[3 * k + 2] = p.nodes[p.levels[l].first + i].n; }
  return (int)k;
}

// The solver on K rows: d [K] at d[i dinc], e [ne] at e[i einc] (ne = K or K - 1), member strides sd / se.
// U [batch, K, K] receives the left vectors, Vc [batch, K+1, K+1] the right vectors as columns, sv [batch, K] the values.
// Enqueues only; *flag (device, zeroed by the caller) receives the line of a failed assertion.
static int nd4_bdsdc(nd4hip_handle* h, int64_t batch, int64_t K, const double* d, int64_t dinc, int64_t sd, const double* e, int64_t einc,
              int64_t se, int64_t ne, double* U, double* sv, double* Vc, int* flag, DcStamps& st) {
  ND4_CHECK_ARG(K >= 1 && K <= DC_MAXM, "svd_dc: the divide & conquer solver takes 1 <= min(M, N) <= %d", DC_MAXM);
  const int N = (int)K + 1;
  const DcPlan plan = dc_plan(N);
  Nd4WsScope scope(h);
  DcNode* nodes = nullptr;
  ND4_TRY(dc_alloc(h, plan.nodes.size(), &nodes));
  void* hp = nullptr;
  ND4_TRY(nd4_pinned(h, sizeof(DcNode) * plan.nodes.size(), &hp));
  memcpy(hp, plan.nodes.data(), sizeof(DcNode) * plan.nodes.size());
  ND4_HIP(hipMemcpyAsync(nodes, hp, sizeof(DcNode) * plan.nodes.size(), hipMemcpyHostToDevice, h->stream));
  // the merges of one level times the members of a chunk go into one grid dimension and one GEMM batch (<= 65535)
  int64_t chunk = 32767 / (N / 4 + 1);
  if (chunk > batch) chunk = batch;
  const size_t sq = (size_t)(N + 2) * (N + 2);               // >= merges * rmax * mmax of any level
  DcBufs B;
  double *WU, *WV, *G, *R;
  B.N = N; B.sU = (long)K * K; B.sV = (long)N * N;
  ND4_TRY(dc_alloc(h, (size_t)chunk * N, &B.dd)); ND4_TRY(dc_alloc(h, (size_t)chunk * N, &B.ee));
  ND4_TRY(dc_alloc(h, (size_t)chunk * N, &B.dw)); ND4_TRY(dc_alloc(h, (size_t)chunk * N, &B.zw));
  ND4_TRY(dc_alloc(h, (size_t)chunk * N, &B.sg)); ND4_TRY(dc_alloc(h, (size_t)chunk * N * 2, &B.rc));
  ND4_TRY(dc_alloc(h, (size_t)chunk * N * 2, &B.metaD));
  ND4_TRY(dc_alloc(h, (size_t)chunk * N, &B.outI)); ND4_TRY(dc_alloc(h, (size_t)chunk * N, &B.innI));
  ND4_TRY(dc_alloc(h, (size_t)chunk * N, &B.rotI)); ND4_TRY(dc_alloc(h, (size_t)chunk * N * 2, &B.metaI));
  ND4_TRY(dc_alloc(h, (size_t)chunk * sq, &WU)); ND4_TRY(dc_alloc(h, (size_t)chunk * sq, &WV));
  ND4_TRY(dc_alloc(h, (size_t)chunk * sq, &G)); ND4_TRY(dc_alloc(h, (size_t)chunk * sq, &R));
  // the vectors are read at positions a level has not written (never used, but loaded): define them
  ND4_HIP(hipMemsetAsync(B.dw, 0, sizeof(double) * (size_t)chunk * N, h->stream));
  ND4_HIP(hipMemsetAsync(B.sg, 0, sizeof(double) * (size_t)chunk * N, h->stream));
  ND4_HIP(hipMemsetAsync(B.rotI, 0, sizeof(int) * (size_t)chunk * N, h->stream));
  ND4_HIP(hipMemsetAsync(B.outI, 0, sizeof(int) * (size_t)chunk * N, h->stream));
  ND4_HIP(hipMemsetAsync(B.innI, 0, sizeof(int) * (size_t)chunk * N, h->stream));
  ND4_HIP(hipMemsetAsync(B.metaI, 0, sizeof(int) * (size_t)chunk * N * 2, h->stream));
  for (int64_t b0 = 0; b0 < batch; b0 += chunk) {
    const int nb = (int)(batch - b0 < chunk ? batch - b0 : chunk);
    B.U = U + b0 * K * K; B.V = Vc + b0 * (int64_t)N * N;
    ND4_HIP(hipMemsetAsync(B.U, 0, sizeof(double) * (size_t)nb * K * K, h->stream));
    ND4_HIP(hipMemsetAsync(B.V, 0, sizeof(double) * (size_t)nb * N * N, h->stream));
    st.mark(DC_ST_LEAVES);
    hipLaunchKernelGGL(dc_init, dim3((N + 255) / 256, nb), dim3(256), 0, h->stream, B, d + b0 * sd, (long)dinc, (long)sd,
                       e + b0 * se, (long)einc, (long)se, (int)ne);
    const DcPlan::Level& lv0 = plan.levels[0];
    hipLaunchKernelGGL(dc_leaves, dim3((lv0.count + 63) / 64, nb), dim3(64), 0, h->stream, B, nodes, lv0.count);
    ND4_HIP(hipGetLastError());
    for (size_t l = 1; l < plan.levels.size(); ++l) {
      const DcPlan::Level& lv = plan.levels[l];
      const DcNode* nl = nodes + lv.first;
      const int nm = lv.count, mmax = lv.mmax, rmax = mmax + 1, xw = (mmax + 3) / 4;
      const long sW = (long)nm * mmax * mmax;
      st.mark(DC_ST_PREP);
      hipLaunchKernelGGL(dc_prep, dim3(nm, nb), dim3(256), 0, h->stream, B, nl, flag);
      st.mark(DC_ST_ROOTS);
      hipLaunchKernelGGL(dc_roots, dim3(xw, nm, nb), dim3(256), 0, h->stream, B, nl, flag);
      st.mark(DC_ST_ZHAT);
      hipLaunchKernelGGL(dc_zhat, dim3(xw + 1, nm, nb), dim3(256), 0, h->stream, B, nl, flag);
      st.mark(DC_ST_W);
      ND4_HIP(hipMemsetAsync(WU, 0, sizeof(double) * (size_t)nb * sW, h->stream));
      ND4_HIP(hipMemsetAsync(WV, 0, sizeof(double) * (size_t)nb * sW, h->stream));
      hipLaunchKernelGGL(dc_wbuild, dim3(xw, nm, nb), dim3(256), 0, h->stream, B, nl, flag, WU, WV, mmax, sW);
      hipLaunchKernelGGL(dc_wrot, dim3((mmax + 255) / 256, nm, nb * 2), dim3(256), 0, h->stream, B, nl, flag, WU, WV, mmax, sW);
      ND4_HIP(hipGetLastError());
      st.mark(DC_ST_MERGE);
      if (mmax <= DC_SMALL_M) {
        hipLaunchKernelGGL(dc_apply_small, dim3(nm, nb), dim3(256), 0, h->stream, B, nl, flag, WU, WV, mmax, sW);
        ND4_HIP(hipGetLastError());
        continue;
      }
      for (int isV = 0; isV < 2; ++isV) {
        const dim3 grid((mmax + 63) / 64, rmax, nm * nb);
        hipLaunchKernelGGL(dc_gather, grid, dim3(64), 0, h->stream, B, nl, nm, flag, isV, G, rmax, mmax);
        ND4_HIP(hipGetLastError());
        ND4_TRY(nd4_gemm(h, false, false, rmax, mmax, mmax, 1.0, G, mmax, (int64_t)rmax * mmax, isV ? WV : WU, mmax, (int64_t)mmax * mmax,
                         0.0, R, mmax, (int64_t)rmax * mmax, (int64_t)nm * nb));
        hipLaunchKernelGGL(dc_scatter, grid, dim3(64), 0, h->stream, B, nl, nm, flag, isV, R, rmax, mmax);
        ND4_HIP(hipGetLastError());
      }
    }
    ND4_TRY(nd4_copy_matrix(h, 1, K, B.dd, N, sv + b0 * K, K, nb, N, K));
  }
  st.mark(DC_ST_FINAL);
  return 0;
}

// reads the flag word back (synchronises) and turns it into the reference's error
static int nd4_bdsdc_finish(nd4hip_handle* h, const int* flag, DcStamps& st) {
  st.mark(-1);
  void* hp = nullptr;
  ND4_TRY(nd4_pinned(h, sizeof(int), &hp));
  int* host = static_cast<int*>(hp);
  ND4_HIP(hipMemcpyAsync(host, flag, sizeof(int), hipMemcpyDeviceToHost, h->stream));
  ND4_HIP(hipStreamSynchronize(h->stream));
  st.collect();
  ND4_TRY(nd4_xchg_check(h, "svd_dc"));
  if (host[0] != 0) {
    nd4_set_error("svd_dc: Assertion failed. (svd_dc.js:%d)", host[0]);
    return ND4HIP_ERR_NOCONV;
  }
  return 0;
}

// bidiag_svd: d [batch,K], e [batch,J-1] -> U2 [batch,K,K], sv [batch,K], V2 [batch,J,J] (rows = right vectors)
int nd4_bdsdc_rows(nd4hip_handle* h, int64_t batch, int64_t K, int64_t J, const double* d, const double* e, double* U2, double* sv, double* V2) {
  Nd4WsScope scope(h);
  const int64_t N = K + 1;
  double* Vc = nullptr; int* flag = nullptr;
  ND4_TRY(dc_alloc(h, (size_t)batch * N * N, &Vc));
  ND4_TRY(dc_alloc(h, 1, &flag));
  ND4_HIP(hipMemsetAsync(flag, 0, sizeof(int), h->stream));
  DcStamps st(h);
  ND4_TRY(nd4_bdsdc(h, batch, K, d, 1, K, e, 1, J - 1, J - 1, U2, sv, Vc, flag, st));
  // J = K: e[K-1] = 0, the last row and column of Vc are a unit vector and drop out
  ND4_TRY(nd4_transpose(h, J, J, Vc, N, V2, J, batch, N * N, J * J));
  return nd4_bdsdc_finish(h, flag, st);
}

// svd_decomp by divide & conquer, M <= N or through the transpose (:883-932)
int nd4_gesdd(nd4hip_handle* h, int64_t batch, int64_t M, int64_t N, const double* A, double* U, double* sv, double* V) {
  ND4_CHECK_ARG(batch <= 65535, "svd_dc: batch %lld exceeds 65535 per call", (long long)batch);
  ND4_CHECK_ARG((M < N ? M : N) <= DC_MAXM, "svd_dc: the divide & conquer solver takes min(M, N) <= %d", DC_MAXM);
  Nd4WsScope scope(h);
  const bool tall = M > N;
  const int64_t m = tall ? N : M, n = tall ? M : N;          // the wide problem that is solved: m x n, m <= n
  const int64_t Jb = m < n ? m + 1 : m, Nc = m + 1, sA = m * n;
  unsigned long long* mx = nullptr;
  double *As, *Ub, *Bb, *Vb, *U2, *Vc, *Ut = nullptr, *Vt = nullptr;
  int* flag = nullptr;
  ND4_TRY(dc_alloc(h, (size_t)batch, &mx)); ND4_TRY(dc_alloc(h, 1, &flag));
  ND4_TRY(dc_alloc(h, (size_t)batch * sA, &As)); ND4_TRY(dc_alloc(h, (size_t)batch * m * m, &Ub));
  ND4_TRY(dc_alloc(h, (size_t)batch * m * Jb, &Bb)); ND4_TRY(dc_alloc(h, (size_t)batch * Jb * n, &Vb));
  ND4_TRY(dc_alloc(h, (size_t)batch * m * m, &U2)); ND4_TRY(dc_alloc(h, (size_t)batch * Nc * Nc, &Vc));
  if (tall) { ND4_TRY(dc_alloc(h, (size_t)batch * m * m, &Ut)); ND4_TRY(dc_alloc(h, (size_t)batch * sA, &Vt)); }
  ND4_HIP(hipMemsetAsync(flag, 0, sizeof(int), h->stream));
  DcStamps st(h);
  st.mark(DC_ST_BIDIAG);
  // the same exact power-of-two scaling as the Jacobi entry (svd.hip): the reflector norms of the bidiagonalisation are plain
  // sums of squares
  ND4_TRY(nd4_svd_scale_begin(h, batch, M * N, A, mx));
  if (tall) { ND4_TRY(nd4_transpose(h, M, N, A, N, As, M, batch, sA, sA)); ND4_TRY(nd4_svd_scale_apply(h, batch, sA, As, As, mx)); }
  else ND4_TRY(nd4_svd_scale_apply(h, batch, sA, A, As, mx));
  ND4_TRY(nd4_gebrd(h, batch, m, n, As, Ub, Bb, Vb));
  ND4_TRY(nd4_bdsdc(h, batch, m, Bb, Jb + 1, m * Jb, Bb + 1, Jb + 1, m * Jb, Jb - 1, U2, sv, Vc, flag, st));
  double* Uo = tall ? Ut : U;                               // [m, m]
  double* Vo = tall ? Vt : V;                               // [m, n]
  ND4_TRY(nd4_gemm(h, false, false, m, m, m, 1.0, Ub, m, m * m, U2, m, m * m, 0.0, Uo, m, m * m, batch));
  ND4_TRY(nd4_gemm(h, true, false, m, n, Jb, 1.0, Vc, Nc, Nc * Nc, Vb, n, Jb * n, 0.0, Vo, n, sA, batch));
  if (tall) {                                               // U = V'^T [M, N], V = U'^T [N, N]
    ND4_TRY(nd4_transpose(h, m, n, Vt, n, U, m, batch, sA, sA));
    ND4_TRY(nd4_transpose(h, m, m, Ut, m, V, m, batch, m * m, m * m));
  }
  ND4_TRY(nd4_svd_scale_undo(h, batch, m, sv, mx));
  return nd4_bdsdc_finish(h, flag, st);
}
