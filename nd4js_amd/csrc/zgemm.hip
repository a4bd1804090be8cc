// complex128 GEMM for gfx950 (MI355X): C[b] = A[b] * B[b], row-major, batched, on interleaved (re, im) doubles.
//
// Replaces the reference's matmul2_CC and matmul2_CR loops (src/la/matmul.js:79-87). A is complex (I x K), B is complex
// (K x J) or, for CR, real; C is complex (I x J). The RC pairing needs no kernel of its own: a real A times an interleaved
// B is the real product A * B' with B' the K x 2J real view of B (nd4hip_zgemm_batched_dev sends it to nd4_gemm).
//
// Arithmetic: the reference's products, no 3M/Gauss trick.
//   CC: Re += Ar*Br + Ai*(-Bi),  Im += Ar*Bi + Ai*Br      (four fp64 MFMA chains)
//   CR: Re += Ar*B,              Im += Ai*B               (two; never CC with Bi = 0, which would turn (inf+0i)*1 into inf+NaNi)
// Every accumulator sees exactly the reference's set of products, so the NaN / Inf positions of C are the reference's.
//
// Design (derived from dgemm_kernel in gemm.hip):
//  * 256-thread workgroup = 4 wave64 in a 2x2 grid; macro tile 128 x 64 complex, K-step 8 complex; each wave owns
//    64 x 32 complex = 4 x 2 tiles of v_mfma_f64_16x16x4_f64 for Re and 4 x 2 for Im: the same 16 accumulators
//    (128 doubles per lane) and the same 64 MFMAs per K-step and wave as the real kernel (32 for CR).
//  * one 16-byte global load is one complex element; operands are staged global -> registers -> LDS, where they are
//    split into separate re / im images, double-buffered, ONE barrier per K-step (as dgemm_kernel):
//      A image [128][17]: row x = [Ar k0..7 | Ai k0..7 | pad]: lane (x=l&15, k=l>>4) of a fragment read -> dword bank
//                         (34*x + 2*k) mod 64, every bank once over 32 lanes (the real kernel's "row" image);
//      B image [8][144]:  row k = [Br x0..63 | Bi x0..63 | pad]: stride 288 dwords = 32 mod 64, so lanes 16-31 (next k)
//                         take the other half of the banks (the real kernel's "kmaj" image). CR: [Br x0..63 | pad].
//  * the negation of Bi costs one VALU op per B fragment (2 per 32 MFMAs).
//  * XCD-aware tile map as dgemm_kernel.
//  * edges: rows / cols / k beyond the matrix load as zeros (predicated loads) and are never stored; a base pointer that
//    is not 16-byte aligned takes the scalar path (8-byte loads and stores).
#include "nd4hip_internal.h"

typedef double d4 __attribute__((ext_vector_type(4)));
typedef double d2 __attribute__((ext_vector_type(2)));

namespace {

constexpr int ZBM = 128, ZBN = 64, ZBK = 8;     // complex elements
constexpr int ZLDA = 2 * ZBK + 1;               // A image leading dim (doubles): Ar | Ai | pad
constexpr int ZLDB = 2 * ZBN + 16;              // B image leading dim (doubles): Br | Bi | pad
constexpr int ZTA = ZBM * ZLDA;                 // 2176 doubles
constexpr int ZTB = ZBK * ZLDB;                 // 1152 doubles
constexpr int ZBUF = ZTA + ZTB;                 // one stage: 26 KiB; two stages 52 KiB (two workgroups per CU)
constexpr int ZNXCD = 8, ZGROUP_M = 8;

struct ZgemmArgs {
  const double* A; const double* B; double* C;  // interleaved complex (B real for CR)
  int M, N, K;                                  // I, J, K
  long sA, sB, sC;                              // batch strides in elements of each operand
  int tiles_m, tiles_n;
};

// A (complex, I x K): thread t covers x = q*32 + t/8, k = t%8, q = 0..3: 8 lanes read one row's 128 contiguous bytes
template <bool VEC, bool FULL>
__device__ __forceinline__ void zload_a(d2 (&r)[4], const double* __restrict__ P, long ld, int x0, int X, int k0, int K, int t) {
  const int k = k0 + (t & 7);
#pragma unroll
  for (int q = 0; q < 4; q++) {
    const int x = x0 + q * 32 + (t >> 3);
    const double* p = P + 2 * ((long)x * ld + k);
    d2 v = {0.0, 0.0};
    if (FULL) {
      v = *reinterpret_cast<const d2*>(p);
    } else if (x < X && k < K) {
      if (VEC) v = *reinterpret_cast<const d2*>(p);
      else { v.x = p[0]; v.y = p[1]; }
    }
    r[q] = v;
  }
}
__device__ __forceinline__ void zstore_a(double* S, const d2 (&r)[4], int t) {
  const int k = t & 7;
#pragma unroll
  for (int q = 0; q < 4; q++) {
    double* s = S + (q * 32 + (t >> 3)) * ZLDA + k;
    s[0] = r[q].x; s[ZBK] = r[q].y;
  }
}
// B complex (K x J): thread t covers k = t/32, x = q*32 + t%32, q = 0..1 (one complex each)
// B real (K x J):    thread t covers k = t/32, x = 2*(t%32) + {0,1} (two reals)
template <bool BC, bool VEC, bool FULL>
__device__ __forceinline__ void zload_b(d2 (&r)[2], const double* __restrict__ P, long ld, int x0, int X, int k0, int K, int t) {
  const int k = k0 + (t >> 5);
  if (BC) {
#pragma unroll
    for (int q = 0; q < 2; q++) {
      const int x = x0 + q * 32 + (t & 31);
      const double* p = P + 2 * ((long)k * ld + x);
      d2 v = {0.0, 0.0};
      if (FULL) {
        v = *reinterpret_cast<const d2*>(p);
      } else if (k < K && x < X) {
        if (VEC) v = *reinterpret_cast<const d2*>(p);
        else { v.x = p[0]; v.y = p[1]; }
      }
      r[q] = v;
    }
  } else {
    const int x = x0 + 2 * (t & 31);
    const double* p = P + (long)k * ld + x;
    d2 v = {0.0, 0.0};
    if (FULL) {
      v = *reinterpret_cast<const d2*>(p);
    } else {   // a real B row need not start on 16 bytes (odd J): 8-byte loads
      if (k < K && x < X) v.x = p[0];
      if (k < K && x + 1 < X) v.y = p[1];
    }
    r[0] = v;
  }
}
template <bool BC>
__device__ __forceinline__ void zstore_b(double* S, const d2 (&r)[2], int t) {
  double* s = S + (t >> 5) * ZLDB;
  if (BC) {
#pragma unroll
    for (int q = 0; q < 2; q++) {
      const int x = q * 32 + (t & 31);
      s[x] = r[q].x; s[ZBN + x] = r[q].y;
    }
  } else {
    *reinterpret_cast<d2*>(s + 2 * (t & 31)) = r[0];
  }
}

// BC: B is complex (CC), else real (CR). VEC: 16-byte global loads / stores (16-byte aligned bases).
// FULL: I a multiple of 128, J of 64, K of 8 (and VEC): no bounds predicate anywhere.
template <bool BC, bool VEC, bool FULL>
__global__ __launch_bounds__(256, 2) void zgemm_kernel(ZgemmArgs g) {
  __shared__ __attribute__((aligned(16))) double lds[2 * ZBUF];   // [buf][A | B]

  // ---- XCD-aware tile assignment (bijective for any tile count), as dgemm_kernel ----
  const int nwg = g.tiles_m * g.tiles_n;
  int wg;
  {
    const int bid = blockIdx.x, xcd = bid % ZNXCD, within = bid / ZNXCD;
    const int q = nwg / ZNXCD, r = nwg % ZNXCD;
    wg = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + within;
  }
  const int per_group = ZGROUP_M * g.tiles_n;
  const int first_m = (wg / per_group) * ZGROUP_M;
  const int gsz = min(g.tiles_m - first_m, ZGROUP_M);
  const int tm = first_m + (wg % per_group) % gsz;
  const int tn = (wg % per_group) / gsz;
  const int m0 = tm * ZBM, n0 = tn * ZBN;

  const long bz = blockIdx.y;
  const double* __restrict__ A = g.A + 2 * bz * g.sA;
  const double* __restrict__ B = g.B + (BC ? 2 : 1) * bz * g.sB;
  double* __restrict__ C = g.C + 2 * bz * g.sC;
  const int K = g.K;

  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int wm = (wave >> 1) * 64, wn = (wave & 1) * 32;
  const int fx = lane & 15, fk = lane >> 4;

  d4 re[4][2], im[4][2];
#pragma unroll
  for (int i = 0; i < 4; i++)
#pragma unroll
    for (int j = 0; j < 2; j++) { re[i][j] = d4{0.0, 0.0, 0.0, 0.0}; im[i][j] = d4{0.0, 0.0, 0.0, 0.0}; }

  d2 ra[4], rb[2];
  auto gload = [&](int k0) {
    zload_a<VEC, FULL>(ra, A, K, m0, g.M, k0, K, t);
    zload_b<BC, VEC, FULL>(rb, B, g.N, n0, g.N, k0, K, t);
  };
  auto sstore = [&](int buf) {
    double* sa = lds + buf * ZBUF;
    zstore_a(sa, ra, t);
    zstore_b<BC>(sa + ZTA, rb, t);
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
      double ar[4], ai[4], br[2], bi[2];
#pragma unroll
      for (int i = 0; i < 4; i++) {
        const double* p = sa + (wm + i * 16 + fx) * ZLDA + kk * 4 + fk;
        ar[i] = p[0]; ai[i] = p[ZBK];
      }
#pragma unroll
      for (int j = 0; j < 2; j++) {
        const double* p = sb + (kk * 4 + fk) * ZLDB + wn + j * 16 + fx;
        br[j] = p[0];
        if (BC) bi[j] = p[ZBN];
      }
      if (kk == ZBK / 4 - 1 && kt + 1 < nk) {
        // stage tile kt+1 into the other buffer before the last MFMAs of this step (as dgemm_kernel)
        sstore(cur ^ 1);
        __builtin_amdgcn_sched_barrier(0);
      }
      __builtin_amdgcn_s_setprio(1);
      // pass 1: the products with Ar; pass 2: the products with Ai. Between two MFMAs on one accumulator lie 15 others.
#pragma unroll
      for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 2; j++) {
          re[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(ar[i], br[j], re[i][j], 0, 0, 0);
          if (BC) im[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(ar[i], bi[j], im[i][j], 0, 0, 0);
        }
      double nbi[2];
#pragma unroll
      for (int j = 0; j < 2; j++) nbi[j] = BC ? -bi[j] : 0.0;
#pragma unroll
      for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 2; j++) {
          if (BC) re[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(ai[i], nbi[j], re[i][j], 0, 0, 0);
          im[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(ai[i], br[j], im[i][j], 0, 0, 0);
        }
      __builtin_amdgcn_s_setprio(0);
    }
    __syncthreads();
  }

  // ---- epilogue: lane holds C[row = (lane>>4) + 4r][col = lane&15] of each 16x16 tile, re and im: one 16-byte store ----
#pragma unroll
  for (int i = 0; i < 4; i++)
#pragma unroll
    for (int j = 0; j < 2; j++) {
      const int col = n0 + wn + j * 16 + fx;
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const int row = m0 + wm + i * 16 + fk + 4 * r;
        if (FULL || (row < g.M && col < g.N)) {
          double* c = C + 2 * ((long)row * g.N + col);
          if (VEC) *reinterpret_cast<d2*>(c) = d2{re[i][j][r], im[i][j][r]};
          else { c[0] = re[i][j][r]; c[1] = im[i][j][r]; }
        }
      }
    }
}

template <bool BC>
int zlaunch(nd4hip_handle* h, const ZgemmArgs& g, bool vec, bool full, int64_t batch) {
  dim3 grid((unsigned)(g.tiles_m * g.tiles_n), (unsigned)batch, 1), block(256, 1, 1);
  if (full)     hipLaunchKernelGGL((zgemm_kernel<BC, true, true>), grid, block, 0, h->stream, g);
  else if (vec) hipLaunchKernelGGL((zgemm_kernel<BC, true, false>), grid, block, 0, h->stream, g);
  else          hipLaunchKernelGGL((zgemm_kernel<BC, false, false>), grid, block, 0, h->stream, g);
  ND4_HIP(hipGetLastError());
  return 0;
}

}  // namespace

// C[b] (I x J complex) = A[b] (I x K complex) * B[b] (K x J, complex if b_complex else real); strides in elements of each
// operand (0 = broadcast), C dense [batch, I, J]. batch <= 65535 per call (gridDim.y).
int nd4_zgemm(nd4hip_handle* h, bool b_complex, int64_t batch, int64_t I, int64_t K, int64_t J,
              const double* A, int64_t sA, const double* B, int64_t sB, double* C) {
  if (I <= 0 || J <= 0 || batch <= 0) return 0;
  ND4_CHECK_ARG(K >= 0 && I < (1 << 30) && J < (1 << 30) && K < (1 << 30), "nd4_zgemm: extent out of range");
  ND4_CHECK_ARG(batch <= 65535, "nd4_zgemm: batch %lld exceeds 65535 per launch", (long long)batch);
  ZgemmArgs g;
  g.A = A; g.B = B; g.C = C; g.M = (int)I; g.N = (int)J; g.K = (int)K;
  g.sA = sA; g.sB = sB; g.sC = I * J;
  g.tiles_m = (int)((I + ZBM - 1) / ZBM); g.tiles_n = (int)((J + ZBN - 1) / ZBN);
  ND4_CHECK_ARG((int64_t)g.tiles_m * g.tiles_n < (1ll << 31), "nd4_zgemm: too many tiles");
  auto al16 = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
  // complex rows are whole 16-byte elements: only the bases decide; a real B (CR) additionally needs even J and stride
  const bool vec = al16(A) && al16(C) && (b_complex ? al16(B) : true);
  const bool full = vec && I % ZBM == 0 && J % ZBN == 0 && K % ZBK == 0 && K > 0 &&
                    (b_complex || (al16(B) && (sB & 1) == 0));
  return b_complex ? zlaunch<true>(h, g, vec, full, batch) : zlaunch<false>(h, g, vec, full, batch);
}
