// The complex Householder reflector (LAPACK's zlarfg) of the Hermitian tridiagonal reduction (hetrd.hip) and of the complex QR
// (zgeqrf.hip): the complex arithmetic in one written order, the fixed-order sum over a workgroup of 256 threads, the lift of tiny
// columns and the reflector itself. Moved here unchanged from hetrd.hip, where the conventions are described.
#pragma once
#include "syev_internal.h"

namespace {

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

}  // namespace
