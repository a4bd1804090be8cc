// The operand staging of the complex fp64 MFMA kernels, shared by zgemm.hip (C = A B) and zgetrf.hip (C -= A B on sub-matrices): the
// macro tile, the split re / im LDS images and the global -> register -> LDS moves. The layout is described at the top of zgemm.hip.
#pragma once
typedef double d4 __attribute__((ext_vector_type(4)));
typedef double d2 __attribute__((ext_vector_type(2)));

namespace {

constexpr int ZBM = 128, ZBN = 64, ZBK = 8;     // complex elements
constexpr int ZLDA = 2 * ZBK + 1;               // A image leading dim (doubles): Ar | Ai | pad
constexpr int ZLDB = 2 * ZBN + 16;              // B image leading dim (doubles): Br | Bi | pad
constexpr int ZTA = ZBM * ZLDA;                 // 2176 doubles
constexpr int ZTB = ZBK * ZLDB;                 // 1152 doubles
constexpr int ZBUF = ZTA + ZTB;                 // one stage: 26 KiB; two stages 52 KiB (two workgroups per CU)

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

}  // namespace
