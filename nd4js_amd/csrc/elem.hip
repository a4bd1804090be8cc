// Elementwise arithmetic and ordered axis reductions on float64 device arrays: what nd.zip_elems, NDArray.mapElems and
// NDArray.reduceElems (zip_elems.js, nd_array.js:353-360, 464-529) come down to when the closure is one of nd.math's
// add, sub, mul, div, min, max, neg, abs. Each of them is one IEEE operation on float64, so every non-NaN result has the
// reference's 64 bits (a NaN result is a NaN; whose payload survives is the host CPU's rule and is not reproduced).
//
//   zip:    C[i] = op(A[a_off + sum_d i_d a_strides[d]], B[b_off + sum_d i_d b_strides[d]])   C dense row-major, strides >= 0,
//           0 = broadcast. Three kernels, chosen from the box as given:
//             dense  every operand is congruent with C or a single element: 16-byte accesses where the three addresses allow,
//                    four loads in flight per lane, one 8-byte tail; 8-byte accesses when an address is odd
//             rows   the innermost stride of each operand is 1 or 0: the item decomposition of gather_rows_kernel (outer axes
//                    staged in LDS, decomposed once per item from lane-uniform values)
//             elems  anything else and small boxes: one thread per element
//   reduce: per output the FIRST element met is copied and the others are folded in, acc = op(x, acc), in row-major order of the
//           reduced axes: the reference's order, so sums and products have its bits. Parallelism is across outputs only. The entry
//           point merges neighbouring axes of one kind, so the box alternates:
//             tile   [K, R] (innermost reduced) and [K1, R, K0] with few outputs: a workgroup stages RB outputs x 4096/RB reduced
//                    elements in LDS with coalesced loads (the next chunk's loads are in flight in registers meanwhile), lane r
//                    folds row r (column r) in order and carries its accumulator from chunk to chunk. RB = 64, fewer (16, 8 along
//                    rows, 16 down columns) when the workgroups would not fill the chip otherwise, 1 for the single chain
//                    of a full sum
//             cols   [K1, R, K0] with many outputs: one lane per output along K0, eight loads in flight per lane
//             tree   min / max only (the order is immaterial: a NaN anywhere gives NaN, -0 < +0), [K, R] with R >= 1024: a workgroup
//                    folds one row with all its lanes; when the outputs would not fill the chip each fold is split over
//                    workgroups into partials and a second pass of the same kernel finishes. No atomics; the result does not
//                    depend on the split
//             elems  any other alternation, up to 4 kept and 4 reduced axes: one lane per output walks its reduced multi-index
// All indexing is flat and 64-bit, no batch sits in a grid dimension, at most 8 workgroups per CU. No kernel checks an address:
// the entry points prove on the host that every operand stays inside its allocation and that C is disjoint from A and B.
#include "nd4hip_internal.h"
#include <algorithm>

namespace {

typedef uint32_t u32;
typedef unsigned long long u64;

constexpr int EW_MAX_ND = 8;
constexpr int EW_OUTER = EW_MAX_ND - 2;
constexpr int EW_COPY = 18;                       // internal: the copy of reduceElems with no axes
constexpr int64_t EW_ITEM = 2048;                 // elements per work item of the rows kernel
constexpr int64_t EW_SMALL = 1024;                // boxes of at most this many elements take the elems kernel
constexpr int RED_TILE = 4096;                    // doubles of LDS staging per workgroup of the tile kernel
constexpr int64_t TREE_MIN = 1024;                // min / max folds at least this long take the tree kernel
constexpr int64_t TREE_SEG = 2048;                // a split fold's pieces are at least this long

inline unsigned grid_for(const nd4hip_handle* h, int64_t items) {
  const int64_t cap = (int64_t)h->num_cu * 8;
  return (unsigned)(items < cap ? (items < 1 ? 1 : items) : cap);
}

// ---------------------------------------------------------------------------------------------- the operators
__device__ inline bool sign_of(double x) { return (__double_as_longlong(x) >> 63) != 0; }

// Math.min / Math.max: a NaN operand gives NaN, -0 is below +0. (v_min_f64 / v_max_f64 return the non-NaN operand.)
__device__ inline double js_min(double a, double b) {
  if (a != a) return a;
  if (b != b) return b;
  if (a < b) return a;
  if (b < a) return b;
  return sign_of(a) ? a : b;
}
__device__ inline double js_max(double a, double b) {
  if (a != a) return a;
  if (b != b) return b;
  if (a > b) return a;
  if (b > a) return b;
  return sign_of(a) ? b : a;
}
template <int OP>
__device__ inline double ew(double a, double b) {
  if constexpr (OP == ND4HIP_EW_ADD) return a + b;
  else if constexpr (OP == ND4HIP_EW_SUB) return a - b;
  else if constexpr (OP == ND4HIP_EW_MUL) return a * b;
  else if constexpr (OP == ND4HIP_EW_DIV) return a / b;
  else if constexpr (OP == ND4HIP_EW_MIN) return js_min(a, b);
  else if constexpr (OP == ND4HIP_EW_MAX) return js_max(a, b);
  else if constexpr (OP == ND4HIP_EW_NEG) return __longlong_as_double(__double_as_longlong(a) ^ (long long)0x8000000000000000ull);
  else if constexpr (OP == ND4HIP_EW_ABS) return __longlong_as_double(__double_as_longlong(a) & 0x7fffffffffffffffll);
  else return a;                                  // EW_COPY
}
template <int OP> constexpr bool is_unary() { return OP >= ND4HIP_EW_NEG; }

// ---------------------------------------------------------------------------------------------- zip: dense
// n elements; a_step / b_step: true = congruent with C, false = one element (compile-time, so that no load sits behind a
// branch). VEC: all congruent addresses are 16-byte aligned.
template <int OP, bool VEC, bool a_step, bool b_step>
__global__ __launch_bounds__(256) void zip_dense_kernel(const double* __restrict__ A, const double* __restrict__ B, double* __restrict__ C,
                                                        int64_t n) {
  const int64_t T = (int64_t)gridDim.x * 256;
  int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const double a1 = A[0];
  double b1 = 0.0;
  if constexpr (!is_unary<OP>()) b1 = B[0];
  if constexpr (VEC) {
    const int64_t nv = n >> 1;
    const double2* __restrict__ A2 = reinterpret_cast<const double2*>(A);
    const double2* __restrict__ B2 = reinterpret_cast<const double2*>(B);
    double2* __restrict__ C2 = reinterpret_cast<double2*>(C);
    const double2 as = make_double2(a1, a1), bs = make_double2(b1, b1);
    auto la = [&](int64_t k) { return a_step ? A2[k] : as; };
    auto lb = [&](int64_t k) { if constexpr (is_unary<OP>()) return bs; else return b_step ? B2[k] : bs; };
    auto op2 = [&](double2 x, double2 y) { return make_double2(ew<OP>(x.x, y.x), ew<OP>(x.y, y.y)); };
    for (; i + 3 * T < nv; i += 4 * T) {
      const double2 x0 = la(i), x1 = la(i + T), x2 = la(i + 2 * T), x3 = la(i + 3 * T);
      const double2 y0 = lb(i), y1 = lb(i + T), y2 = lb(i + 2 * T), y3 = lb(i + 3 * T);
      C2[i] = op2(x0, y0); C2[i + T] = op2(x1, y1); C2[i + 2 * T] = op2(x2, y2); C2[i + 3 * T] = op2(x3, y3);
    }
    for (; i < nv; i += T) C2[i] = op2(la(i), lb(i));
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {          // the 8-byte tail
      const int64_t e = n - 1;
      double y = b1;
      if constexpr (!is_unary<OP>()) y = b_step ? B[e] : b1;
      C[e] = ew<OP>(a_step ? A[e] : a1, y);
    }
  } else {
    auto la = [&](int64_t k) { return a_step ? A[k] : a1; };
    auto lb = [&](int64_t k) { if constexpr (is_unary<OP>()) return b1; else return b_step ? B[k] : b1; };
    for (; i + 3 * T < n; i += 4 * T) {
      const double x0 = la(i), x1 = la(i + T), x2 = la(i + 2 * T), x3 = la(i + 3 * T);
      const double y0 = lb(i), y1 = lb(i + T), y2 = lb(i + 2 * T), y3 = lb(i + 3 * T);
      C[i] = ew<OP>(x0, y0); C[i + T] = ew<OP>(x1, y1); C[i + 2 * T] = ew<OP>(x2, y2); C[i + 3 * T] = ew<OP>(x3, y3);
    }
    for (; i < n; i += T) C[i] = ew<OP>(la(i), lb(i));
  }
}

// ---------------------------------------------------------------------------------------------- zip: rows
// outer axes innermost first; axis 1 and axis 0 are the pair a work item spans (n1 x n0); C is dense: its pair strides are n0 and 1
struct ZipPairArgs {
  const double* A; const double* B; double* C;
  int64_t oas[EW_OUTER], obs[EW_OUTER], ocs[EW_OUTER];
  int64_t n1, n0, a1, a0, b1, b0;                 // a0, b0 in {0, 1}
  int64_t R, Cc;                                  // rows x columns per item
  u32 oshape[EW_OUTER];
  u32 nrb, ncb, items;
  int nout;
};
struct ZipOuter { int64_t as[EW_OUTER], bs[EW_OUTER], cs[EW_OUTER]; u32 n[EW_OUTER]; };

template <int OP>
__global__ __launch_bounds__(256) void zip_rows_kernel(ZipPairArgs a) {
  __shared__ ZipOuter outer;
  const int tid = threadIdx.x;
  if (tid < EW_OUTER) { outer.as[tid] = a.oas[tid]; outer.bs[tid] = a.obs[tid]; outer.cs[tid] = a.ocs[tid]; outer.n[tid] = a.oshape[tid]; }
  __syncthreads();
  const double* __restrict__ A = a.A;
  const double* __restrict__ B = a.B;
  double* __restrict__ C = a.C;
  for (u32 w = blockIdx.x; w < a.items; w += gridDim.x) {
    const u32 t = w / a.ncb, cb = w - t * a.ncb, o = t / a.nrb, rb = t - o * a.nrb;
    int64_t ao = 0, bo = 0, co = 0;
    { u32 q = o;
      for (int d = 0; d < a.nout; d++) {
        const u32 n = outer.n[d], q1 = q / n, i = q - q1 * n;
        ao += (int64_t)i * outer.as[d]; bo += (int64_t)i * outer.bs[d]; co += (int64_t)i * outer.cs[d];
        q = q1;
      } }
    const int64_t r0 = (int64_t)rb * a.R, c0 = (int64_t)cb * a.Cc;
    const u32 rc = (u32)(a.n1 - r0 < a.R ? a.n1 - r0 : a.R), cc = (u32)(a.n0 - c0 < a.Cc ? a.n0 - c0 : a.Cc);
    const double* pa = A + ao + r0 * a.a1 + c0 * a.a0;
    const double* pb = B;
    if constexpr (!is_unary<OP>()) pb = B + bo + r0 * a.b1 + c0 * a.b0;
    double* pc = C + co + r0 * a.n0 + c0;
    auto lb = [&](const double* row, int64_t j) { if constexpr (is_unary<OP>()) return 0.0; else return row[j * a.b0]; };
    if (rc == 1 || cc >= 256) {                   // row by row, no division, four loads per operand in flight
      for (u32 r = 0; r < rc; r++) {
        const double* ra = pa + (int64_t)r * a.a1;
        const double* rb_ = pb + (int64_t)r * a.b1;
        double* rcp = pc + (int64_t)r * a.n0;
        u32 j = tid;
        for (; j + 768 < cc; j += 1024) {
          const double x0 = ra[(int64_t)j * a.a0], x1 = ra[(int64_t)(j + 256) * a.a0], x2 = ra[(int64_t)(j + 512) * a.a0],
                       x3 = ra[(int64_t)(j + 768) * a.a0];
          const double y0 = lb(rb_, j), y1 = lb(rb_, j + 256), y2 = lb(rb_, j + 512), y3 = lb(rb_, j + 768);
          rcp[j] = ew<OP>(x0, y0); rcp[j + 256] = ew<OP>(x1, y1); rcp[j + 512] = ew<OP>(x2, y2); rcp[j + 768] = ew<OP>(x3, y3);
        }
        for (; j < cc; j += 256) rcp[j] = ew<OP>(ra[(int64_t)j * a.a0], lb(rb_, j));
      }
    } else {                                      // rc whole rows shorter than the workgroup: one 32-bit division per element
      const u32 n = rc * cc;
      for (u32 x = tid; x < n; x += 256) {
        const u32 r = x / cc, j = x - r * cc;
        pc[(int64_t)r * a.n0 + j] = ew<OP>(pa[(int64_t)r * a.a1 + (int64_t)j * a.a0], lb(pb + (int64_t)r * a.b1, j));
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------- zip: elems
// axes innermost first; unused axes have extent 1
struct ZipElemArgs {
  const double* A; const double* B; double* C;
  int64_t shape[EW_MAX_ND], as[EW_MAX_ND], bs[EW_MAX_ND];
  int64_t total;
  int nd;
};
template <int OP, typename I>
__global__ __launch_bounds__(256) void zip_elems_kernel(ZipElemArgs a) {
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < a.total; e += (int64_t)gridDim.x * blockDim.x) {
    I w = (I)e;
    int64_t ao = 0, bo = 0;
#pragma unroll
    for (int d = 0; d < EW_MAX_ND; d++) {
      if (d >= a.nd) break;
      const I n = (I)a.shape[d], q = w / n, i = w - q * n;
      ao += (int64_t)i * a.as[d]; bo += (int64_t)i * a.bs[d];
      w = q;
    }
    double y = 0.0;
    if constexpr (!is_unary<OP>()) y = a.B[bo];
    a.C[e] = ew<OP>(a.A[ao], y);
  }
}

// ---------------------------------------------------------------------------------------------- reduce: tile
// COLS = false: A is [K, R], outputs k (a block of RB rows per item), reduced index along the rows.      K1 = 1, K0 = K
// COLS = true:  A is [K1, R, K0], outputs (k1, k0) (a block of RB columns per item), reduced index down the columns.
// CH = RED_TILE / RB reduced elements per chunk. The tile is [RB][CH + 1] (rows) or [CH][RB] (cols): lane r reads 8-byte words
// an odd number of words apart, or consecutive ones.
struct TileArgs { const double* A; double* C; int64_t K1, R, K0; u32 items, nkb; };

template <int OP, int RB, bool COLS>
__global__ __launch_bounds__(256) void reduce_tile_kernel(TileArgs a) {
  constexpr int CH = RED_TILE / RB;
  constexpr int PER = RED_TILE / 256;             // 16 elements of a chunk per thread
  __shared__ double tile[RED_TILE + (COLS ? 0 : RB)];
  const double* __restrict__ A = a.A;
  const int tid = threadIdx.x;
  const int64_t nchunks = (a.R + CH - 1) / CH;
  for (u32 w = blockIdx.x; w < a.items; w += gridDim.x) {
    const u32 k1 = w / a.nkb, kb = w - k1 * a.nkb;
    const int64_t kk = (int64_t)kb * RB;                                    // first output of the block along K0
    const int64_t nk = a.K0 - kk < RB ? a.K0 - kk : RB;                     // outputs of this item
    const double* base = COLS ? A + (int64_t)k1 * a.R * a.K0 + kk : A + kk * a.R;
    double v[PER];
    // chunk c of the item into registers; an element outside the item reads the item's first element instead (never used)
    auto fetch = [&](int64_t c) {
      const int64_t c0 = c * CH;
#pragma unroll
      for (int i = 0; i < PER; i++) {
        const int q = i * 256 + tid;
        const int r = COLS ? q % RB : q / CH, j = COLS ? q / RB : q % CH;    // r: output within the block, j: reduced index within the chunk
        const bool ok = r < nk && c0 + j < a.R;
        const int64_t off = COLS ? (c0 + j) * a.K0 + r : (int64_t)r * a.R + c0 + j;
        v[i] = base[ok ? off : 0];
      }
    };
    double acc = 0.0;
    fetch(0);
    for (int64_t c = 0; c < nchunks; c++) {
      __syncthreads();                                                      // the previous chunk's fold has read the tile
#pragma unroll
      for (int i = 0; i < PER; i++) {
        const int q = i * 256 + tid;
        if constexpr (COLS) tile[q] = v[i];
        else tile[(q / CH) * (CH + 1) + q % CH] = v[i];
      }
      __syncthreads();
      if (c + 1 < nchunks) fetch(c + 1);                                    // in flight under the fold
      if (tid < nk) {
        const int64_t left = a.R - c * CH;
        const int nj = (int)(left < CH ? left : CH);
        const double* row = COLS ? tile + tid : tile + tid * (CH + 1);
        constexpr int step = COLS ? RB : 1;
        int j = 0;
        if (c == 0) { acc = row[0]; j = 1; }                                // the first element is copied
        // the chain is one dependent operation per element: the next 16 elements are read from LDS under the fold of these 16
        // (two register blocks that swap roles, so that nothing waits for a copy)
        const int nb = (nj - j) / 16;
        if (nb > 0) {
          double x[16], y[16];
          auto read = [&](double* z, int b) {
#pragma unroll
            for (int i = 0; i < 16; i++) z[i] = row[(j + 16 * b + i) * step];
          };
          auto fold = [&](const double* z) {
#pragma unroll
            for (int i = 0; i < 16; i++) acc = ew<OP>(z[i], acc);
          };
          read(x, 0);
          int b = 0;
          for (; b + 2 < nb; b += 2) { read(y, b + 1); fold(x); read(x, b + 2); fold(y); }
          if (nb - b == 2) { read(y, b + 1); fold(x); fold(y); }
          else fold(x);
          j += 16 * nb;
        }
        for (; j < nj; j++) acc = ew<OP>(row[j * step], acc);
      }
    }
    if (tid < nk) a.C[(COLS ? (int64_t)k1 * a.K0 : 0) + kk + tid] = acc;
  }
}

// ---------------------------------------------------------------------------------------------- reduce: cols
// A is [K1, R, K0]; one lane per output (k1, k0), consecutive lanes along K0
template <int OP>
__global__ __launch_bounds__(256) void reduce_cols_kernel(const double* __restrict__ A, double* __restrict__ C, int64_t K1, int64_t R, int64_t K0) {
  const int64_t total = K1 * K0;
  for (int64_t e = blockIdx.x * (int64_t)256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const int64_t k1 = e / K0, k0 = e - k1 * K0;
    const double* p = A + k1 * R * K0 + k0;
    double acc = p[0];
    int64_t r = 1;
    for (; r + 7 < R; r += 8) {
      double x[8];
#pragma unroll
      for (int i = 0; i < 8; i++) x[i] = p[(r + i) * K0];
#pragma unroll
      for (int i = 0; i < 8; i++) acc = ew<OP>(x[i], acc);
    }
    for (; r < R; r++) acc = ew<OP>(p[r * K0], acc);
    C[e] = acc;
  }
}

// ---------------------------------------------------------------------------------------------- reduce: tree (min / max)
// A is [K, R]; workgroup (k, s) folds A[k, s seg .. (s + 1) seg) into P[k, s]. Every lane starts from the piece's first element
// (min and max are idempotent), so no lane is without a value.
template <int OP>
__global__ __launch_bounds__(256) void reduce_tree_kernel(const double* __restrict__ A, double* __restrict__ P, int64_t R, int64_t S, int64_t seg,
                                                          int64_t items) {
  __shared__ double sh[256];
  const int tid = threadIdx.x;
  for (int64_t w = blockIdx.x; w < items; w += gridDim.x) {
    const int64_t k = w / S, s = w - k * S;
    const int64_t lo = s * seg, hi = lo + seg < R ? lo + seg : R;
    const double* p = A + k * R;
    double m0 = p[lo], m1 = m0, m2 = m0, m3 = m0;
    int64_t j = lo + tid;
    for (; j + 768 < hi; j += 1024) {
      const double x0 = p[j], x1 = p[j + 256], x2 = p[j + 512], x3 = p[j + 768];
      m0 = ew<OP>(x0, m0); m1 = ew<OP>(x1, m1); m2 = ew<OP>(x2, m2); m3 = ew<OP>(x3, m3);
    }
    for (; j < hi; j += 256) m0 = ew<OP>(p[j], m0);
    __syncthreads();                                                        // the previous item's reads of sh are done
    sh[tid] = ew<OP>(ew<OP>(m0, m1), ew<OP>(m2, m3));
    __syncthreads();
    for (int d = 128; d > 0; d >>= 1) {
      if (tid < d) sh[tid] = ew<OP>(sh[tid + d], sh[tid]);
      __syncthreads();
    }
    if (tid == 0) P[w] = sh[0];
  }
}

// ---------------------------------------------------------------------------------------------- reduce: elems
// any alternation: kept and reduced axes innermost first, unused ones with extent 1; one lane per output
struct RedElemArgs {
  const double* A; double* C;
  int64_t kn[4], ks[4], rn[4], rs[4];
  int64_t total;
};
template <int OP>
__global__ __launch_bounds__(256) void reduce_elems_kernel(RedElemArgs a) {
  for (int64_t e = blockIdx.x * (int64_t)256 + threadIdx.x; e < a.total; e += (int64_t)gridDim.x * 256) {
    int64_t w = e, off = 0;
#pragma unroll
    for (int d = 0; d < 4; d++) { const int64_t q = w / a.kn[d]; off += (w - q * a.kn[d]) * a.ks[d]; w = q; }
    const double* p = a.A + off;
    double acc = p[0];
    bool first = true;
    for (int64_t i3 = 0; i3 < a.rn[3]; i3++)
      for (int64_t i2 = 0; i2 < a.rn[2]; i2++)
        for (int64_t i1 = 0; i1 < a.rn[1]; i1++) {
          const double* q = p + i3 * a.rs[3] + i2 * a.rs[2] + i1 * a.rs[1];
          for (int64_t i0 = 0; i0 < a.rn[0]; i0++) {
            const double x = q[i0 * a.rs[0]];
            acc = first ? x : ew<OP>(x, acc);
            first = false;
          }
        }
    a.C[e] = acc;
  }
}

// ---------------------------------------------------------------------------------------------- host side
#define EW_BINARY_OPS(X) X(ND4HIP_EW_ADD) X(ND4HIP_EW_SUB) X(ND4HIP_EW_MUL) X(ND4HIP_EW_DIV) X(ND4HIP_EW_MIN) X(ND4HIP_EW_MAX)
#define EW_ALL_OPS(X) EW_BINARY_OPS(X) X(ND4HIP_EW_NEG) X(ND4HIP_EW_ABS) X(EW_COPY)
#define EW_REDUCERS(X) X(ND4HIP_EW_ADD) X(ND4HIP_EW_MUL) X(ND4HIP_EW_MIN) X(ND4HIP_EW_MAX)

struct ZipBox {
  int nd;
  int64_t shape[EW_MAX_ND], as[EW_MAX_ND], bs[EW_MAX_ND], cs[EW_MAX_ND];    // outermost first; cs: row-major strides of C
};

template <int OP, bool VEC>
void launch_zip_dense_op(dim3 grid, hipStream_t st, const double* A, const double* B, double* C, int64_t n, bool a_step, bool b_step) {
  if constexpr (is_unary<OP>()) {
    if (a_step) hipLaunchKernelGGL((zip_dense_kernel<OP, VEC, true, false>), grid, dim3(256), 0, st, A, B, C, n);
    else hipLaunchKernelGGL((zip_dense_kernel<OP, VEC, false, false>), grid, dim3(256), 0, st, A, B, C, n);
  } else {
    if (a_step && b_step) hipLaunchKernelGGL((zip_dense_kernel<OP, VEC, true, true>), grid, dim3(256), 0, st, A, B, C, n);
    else if (a_step) hipLaunchKernelGGL((zip_dense_kernel<OP, VEC, true, false>), grid, dim3(256), 0, st, A, B, C, n);
    else if (b_step) hipLaunchKernelGGL((zip_dense_kernel<OP, VEC, false, true>), grid, dim3(256), 0, st, A, B, C, n);
    else hipLaunchKernelGGL((zip_dense_kernel<OP, VEC, false, false>), grid, dim3(256), 0, st, A, B, C, n);
  }
}

int launch_zip_dense(nd4hip_handle* h, int op, const double* A, const double* B, double* C, int64_t n, bool a_step, bool b_step) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(A), b = reinterpret_cast<uintptr_t>(B), c = reinterpret_cast<uintptr_t>(C);
  const bool vec = n >= 2 && c % 16 == 0 && (!a_step || a % 16 == 0) && (B == nullptr || !b_step || b % 16 == 0);
  const dim3 grid(grid_for(h, ((vec ? n / 2 : n) + 1023) / 1024));
  switch (op) {
#define X(O) case O: \
    if (vec) launch_zip_dense_op<O, true>(grid, h->stream, A, B, C, n, a_step, b_step); \
    else launch_zip_dense_op<O, false>(grid, h->stream, A, B, C, n, a_step, b_step); \
    break;
    EW_ALL_OPS(X)
#undef X
    default: break;
  }
  ND4_HIP(hipGetLastError());
  return 0;
}

int launch_zip_elems(nd4hip_handle* h, int op, const ZipBox& b, const double* A, const double* B, double* C, int64_t total) {
  ZipElemArgs a;
  a.A = A; a.B = B; a.C = C; a.total = total; a.nd = b.nd;
  for (int k = 0; k < EW_MAX_ND; k++) { a.shape[k] = 1; a.as[k] = 0; a.bs[k] = 0; }
  for (int k = 0; k < b.nd; k++) { a.shape[k] = b.shape[b.nd - 1 - k]; a.as[k] = b.as[b.nd - 1 - k]; a.bs[k] = b.bs[b.nd - 1 - k]; }
  const dim3 grid(grid_for(h, (total + 255) / 256));
  const bool small = total < ((int64_t)1 << 32);
  switch (op) {
#define X(O) case O: \
    if (small) hipLaunchKernelGGL((zip_elems_kernel<O, u32>), grid, dim3(256), 0, h->stream, a); \
    else hipLaunchKernelGGL((zip_elems_kernel<O, u64>), grid, dim3(256), 0, h->stream, a); \
    break;
    EW_ALL_OPS(X)
#undef X
    default: break;
  }
  ND4_HIP(hipGetLastError());
  return 0;
}

int launch_zip_rows(nd4hip_handle* h, int op, const ZipBox& b, const double* A, const double* B, double* C, int64_t total) {
  ZipPairArgs a;
  a.A = A; a.B = B; a.C = C; a.nout = 0;
  for (int k = 0; k < EW_OUTER; k++) { a.oshape[k] = 1; a.oas[k] = 0; a.obs[k] = 0; a.ocs[k] = 0; }
  const int ax0 = b.nd - 1, ax1 = b.nd - 2;
  for (int k = b.nd - 3; k >= 0; k--) {
    if (b.shape[k] > INT32_MAX) return launch_zip_elems(h, op, b, A, B, C, total);
    a.oshape[a.nout] = (u32)b.shape[k]; a.oas[a.nout] = b.as[k]; a.obs[a.nout] = b.bs[k]; a.ocs[a.nout] = b.cs[k]; a.nout++;
  }
  a.n0 = b.shape[ax0]; a.a0 = b.as[ax0]; a.b0 = b.bs[ax0];
  if (ax1 >= 0) { a.n1 = b.shape[ax1]; a.a1 = b.as[ax1]; a.b1 = b.bs[ax1]; }
  else { a.n1 = 1; a.a1 = 0; a.b1 = 0; }
  if (a.n0 >= EW_ITEM) { a.R = 1; a.Cc = EW_ITEM; }
  else { a.R = std::min<int64_t>(a.n1, EW_ITEM / a.n0); a.Cc = a.n0; }
  const int64_t nrb = (a.n1 + a.R - 1) / a.R, ncb = (a.n0 + a.Cc - 1) / a.Cc, outer = total / (a.n1 * a.n0);
  const __int128 items = (__int128)outer * nrb * ncb;
  if (nrb > INT32_MAX || ncb > INT32_MAX || outer > INT32_MAX || items > INT32_MAX) return launch_zip_elems(h, op, b, A, B, C, total);
  a.nrb = (u32)nrb; a.ncb = (u32)ncb; a.items = (u32)items;
  const dim3 grid(grid_for(h, a.items));
  switch (op) {
#define X(O) case O: hipLaunchKernelGGL((zip_rows_kernel<O>), grid, dim3(256), 0, h->stream, a); break;
    EW_ALL_OPS(X)
#undef X
    default: break;
  }
  ND4_HIP(hipGetLastError());
  return 0;
}

// 1: the operand is congruent with C; 0: it is one element; -1: neither
int dense_kind(const ZipBox& b, const int64_t* strides) {
  bool same = true, zero = true;
  for (int d = 0; d < b.nd; d++) {
    if (b.shape[d] == 1) continue;
    same = same && strides[d] == b.cs[d];
    zero = zero && strides[d] == 0;
  }
  return zero ? 0 : same ? 1 : -1;
}

int zip_dispatch(nd4hip_handle* h, int op, const ZipBox& b, const double* A, const double* B, double* C, int64_t total) {
  const int ka = dense_kind(b, b.as), kb = B ? dense_kind(b, b.bs) : 0;
  if (ka >= 0 && kb >= 0) return launch_zip_dense(h, op, A, B, C, total, ka, kb);
  const int in = b.nd - 1;
  if (total > EW_SMALL && b.as[in] <= 1 && (!B || b.bs[in] <= 1)) return launch_zip_rows(h, op, b, A, B, C, total);
  return launch_zip_elems(h, op, b, A, B, C, total);
}

bool known_op(int op) { return (op >= ND4HIP_EW_ADD && op <= ND4HIP_EW_MAX) || op == ND4HIP_EW_NEG || op == ND4HIP_EW_ABS; }

// byte ranges [p, p + 8 n) and [q, q + 8 m)
bool bytes_overlap(const void* p, int64_t n, const void* q, int64_t m) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(p), b = reinterpret_cast<uintptr_t>(q);
  return a < b + (uintptr_t)m * 8 && b < a + (uintptr_t)n * 8;
}

template <int RB, bool COLS>
int launch_tile(nd4hip_handle* h, int op, const double* A, double* C, int64_t K1, int64_t R, int64_t K0) {
  TileArgs a;
  a.A = A; a.C = C; a.K1 = K1; a.R = R; a.K0 = K0;
  const int64_t nkb = (K0 + RB - 1) / RB;
  a.nkb = (u32)nkb; a.items = (u32)(K1 * nkb);                               // the caller checked that it fits
  const dim3 grid(grid_for(h, a.items));
  switch (op) {
#define X(O) case O: hipLaunchKernelGGL((reduce_tile_kernel<O, RB, COLS>), grid, dim3(256), 0, h->stream, a); break;
    EW_REDUCERS(X)
#undef X
    default: break;
  }
  ND4_HIP(hipGetLastError());
  return 0;
}

// [K, R], innermost reduced, in the reference's order. A lane's chain of R steps is what a workgroup takes however many outputs
// it folds side by side, so with few outputs a workgroup takes fewer of them: more workgroups hide each other's loads and
// barriers. Not fewer than 8: the kernel's registers let three workgroups share a CU, and a second round of workgroups would
// cost a whole chain more.
int reduce_rows(nd4hip_handle* h, int op, const double* A, double* C, int64_t K, int64_t R) {
  const int64_t cu = h->num_cu;
  if (K == 1) return launch_tile<1, false>(h, op, A, C, 1, R, 1);
  if ((K + 63) / 64 >= 2 * cu) return launch_tile<64, false>(h, op, A, C, 1, R, K);
  if ((K + 15) / 16 >= 2 * cu) return launch_tile<16, false>(h, op, A, C, 1, R, K);
  return launch_tile<8, false>(h, op, A, C, 1, R, K);
}

// [K, R] -> [K] for min / max, whose order is immaterial: every fold is split into S pieces when the outputs alone would not fill
// the chip, and the same kernel folds the [K, S] partials
int reduce_tree(nd4hip_handle* h, int op, const double* A, double* C, int64_t K, int64_t R) {
  auto launch = [&](const double* src, double* dst, int64_t r, int64_t pieces, int64_t seg) {
    const dim3 grid(grid_for(h, K * pieces));
    if (op == ND4HIP_EW_MIN) hipLaunchKernelGGL((reduce_tree_kernel<ND4HIP_EW_MIN>), grid, dim3(256), 0, h->stream, src, dst, r, pieces, seg, K * pieces);
    else hipLaunchKernelGGL((reduce_tree_kernel<ND4HIP_EW_MAX>), grid, dim3(256), 0, h->stream, src, dst, r, pieces, seg, K * pieces);
  };
  const int64_t want = std::min<int64_t>((R + TREE_SEG - 1) / TREE_SEG, std::max<int64_t>(1, (int64_t)h->num_cu * 8 / K));
  const int64_t seg = (R + want - 1) / want, S = (R + seg - 1) / seg;           // S pieces, none empty
  if (S == 1) { launch(A, C, R, 1, R); ND4_HIP(hipGetLastError()); return 0; }
  Nd4WsScope scope(h);
  void* p = nullptr;
  ND4_TRY(nd4_ws_alloc(h, sizeof(double) * (size_t)(K * S) + 64, &p));
  double* P = static_cast<double*>(p);
  launch(A, P, R, S, seg);
  ND4_HIP(hipGetLastError());
  launch(P, C, S, 1, S);
  ND4_HIP(hipGetLastError());
  return 0;
}

}  // namespace

extern "C" int nd4hip_dzip_nd_dev(nd4hip_handle* h, int op, int ndim, const int64_t* shape, const double* A, int64_t a_len, int64_t a_off,
                                  const int64_t* a_strides, const double* B, int64_t b_len, int64_t b_off, const int64_t* b_strides, double* C,
                                  int64_t c_len) {
  ND4_CHECK_ARG(h != nullptr, "nd4hip_dzip_nd: NULL handle");
  ND4_CHECK_ARG(known_op(op), "nd4hip_dzip_nd: unknown op %d", op);
  const bool unary = op >= ND4HIP_EW_NEG;
  ND4_CHECK_ARG(unary == (B == nullptr), "nd4hip_dzip_nd: op %d takes %s", op, unary ? "one operand (B must be NULL)" : "two operands (B is NULL)");
  ND4_CHECK_ARG(ndim >= 0 && ndim <= EW_MAX_ND, "nd4hip_dzip_nd: ndim=%d is not in 0..%d", ndim, EW_MAX_ND);
  ND4_CHECK_ARG(ndim == 0 || (shape && a_strides && (unary || b_strides)), "nd4hip_dzip_nd: NULL shape or strides");
  ND4_CHECK_ARG(A && C, "nd4hip_dzip_nd: NULL pointer");
  ND4_CHECK_ARG(a_len >= 1 && c_len >= 1 && (unary || b_len >= 1) && a_len <= INT64_MAX / 8 && c_len <= INT64_MAX / 8 && (unary || b_len <= INT64_MAX / 8),
                "nd4hip_dzip_nd: bad allocation length");
  ZipBox b;
  b.nd = ndim;
  __int128 count = 1, ahi = a_off, bhi = unary ? 0 : b_off, aread = 1, bread = 1;
  for (int d = 0; d < ndim; d++) {
    ND4_CHECK_ARG(shape[d] >= 1, "nd4hip_dzip_nd: extent %lld of axis %d is less than 1", (long long)shape[d], d);
    ND4_CHECK_ARG(a_strides[d] >= 0 && (unary || b_strides[d] >= 0), "nd4hip_dzip_nd: negative stride on axis %d", d);
    b.shape[d] = shape[d]; b.as[d] = a_strides[d]; b.bs[d] = unary ? 0 : b_strides[d];
    count *= shape[d];
    ND4_CHECK_ARG(count <= (__int128)c_len, "nd4hip_dzip_nd: the box has more elements than C");
    ahi += (__int128)(shape[d] - 1) * b.as[d]; bhi += (__int128)(shape[d] - 1) * b.bs[d];
    if (b.as[d] != 0) aread *= shape[d];
    if (b.bs[d] != 0) bread *= shape[d];
  }
  const int64_t total = (int64_t)count;
  ND4_CHECK_ARG(total == c_len, "nd4hip_dzip_nd: c_len=%lld is not the result's element count %lld", (long long)c_len, (long long)total);
  ND4_CHECK_ARG(a_off >= 0 && ahi < (__int128)a_len, "nd4hip_dzip_nd: the box leaves A [0, %lld)", (long long)a_len);
  ND4_CHECK_ARG(unary || (b_off >= 0 && bhi < (__int128)b_len), "nd4hip_dzip_nd: the box leaves B [0, %lld)", (long long)b_len);
  ND4_CHECK_ARG(!bytes_overlap(C, c_len, A + a_off, (int64_t)ahi - a_off + 1), "nd4hip_dzip_nd: C must not overlap A");
  ND4_CHECK_ARG(unary || !bytes_overlap(C, c_len, B + b_off, (int64_t)bhi - b_off + 1), "nd4hip_dzip_nd: C must not overlap B");
  int64_t s = 1;
  for (int d = ndim - 1; d >= 0; d--) { b.cs[d] = s; s *= b.shape[d]; }
  Nd4DeviceGuard guard(h);
  Nd4Prof prof(h, "zip_nd", 0.0, 8.0 * ((double)total + (double)aread + (unary ? 0.0 : (double)bread)));
  return zip_dispatch(h, op, b, A + a_off, unary ? nullptr : B + b_off, C, total);
}

extern "C" int nd4hip_dreduce_nd_dev(nd4hip_handle* h, int op, int ndim, const int64_t* shape, const int32_t* reduced, const double* A,
                                     int64_t a_len, double* C, int64_t c_len) {
  ND4_CHECK_ARG(h != nullptr, "nd4hip_dreduce_nd: NULL handle");
  ND4_CHECK_ARG(op == ND4HIP_EW_ADD || op == ND4HIP_EW_MUL || op == ND4HIP_EW_MIN || op == ND4HIP_EW_MAX,
                "nd4hip_dreduce_nd: op %d is not a reducer (add, mul, min, max)", op);
  ND4_CHECK_ARG(ndim >= 0 && ndim <= EW_MAX_ND, "nd4hip_dreduce_nd: ndim=%d is not in 0..%d", ndim, EW_MAX_ND);
  ND4_CHECK_ARG(ndim == 0 || (shape && reduced), "nd4hip_dreduce_nd: NULL shape or flags");
  ND4_CHECK_ARG(A && C, "nd4hip_dreduce_nd: NULL pointer");
  ND4_CHECK_ARG(a_len >= 1 && c_len >= 1 && a_len <= INT64_MAX / 8 && c_len <= INT64_MAX / 8, "nd4hip_dreduce_nd: bad allocation length");
  // extent-1 axes dropped, neighbours of one kind merged: n[], red[] alternate, outermost first
  int64_t n[EW_MAX_ND]; bool red[EW_MAX_ND]; int m = 0;
  __int128 count = 1, kept = 1;
  bool any_reduced = false;
  for (int d = 0; d < ndim; d++) {
    ND4_CHECK_ARG(shape[d] >= 1, "nd4hip_dreduce_nd: extent %lld of axis %d is less than 1", (long long)shape[d], d);
    count *= shape[d];
    ND4_CHECK_ARG(count <= (__int128)a_len, "nd4hip_dreduce_nd: the box leaves A [0, %lld)", (long long)a_len);
    const bool r = reduced[d] != 0;
    any_reduced = any_reduced || r;
    if (!r) kept *= shape[d];
    if (shape[d] == 1) continue;
    if (m > 0 && red[m - 1] == r) n[m - 1] *= shape[d];
    else { n[m] = shape[d]; red[m] = r; m++; }
  }
  const int64_t total = (int64_t)count, outs = (int64_t)kept;
  ND4_CHECK_ARG(outs == c_len, "nd4hip_dreduce_nd: c_len=%lld is not the result's element count %lld", (long long)c_len, (long long)outs);
  ND4_CHECK_ARG(!bytes_overlap(C, c_len, A, total), "nd4hip_dreduce_nd: C must not overlap A");
  Nd4DeviceGuard guard(h);
  Nd4Prof prof(h, "reduce_nd", 0.0, 8.0 * ((double)total + (double)outs));
  if (!any_reduced || outs == total) return launch_zip_dense(h, EW_COPY, A, nullptr, C, total, 1, 0);   // nothing is folded: a copy
  const bool tile_fits = outs <= (int64_t)INT32_MAX;
  if (m == 1 || (m == 2 && red[1])) {                                       // [R] or [K, R]
    const int64_t K = m == 1 ? 1 : n[0], R = m == 1 ? n[0] : n[1];
    if ((op == ND4HIP_EW_MIN || op == ND4HIP_EW_MAX) && R >= TREE_MIN) return reduce_tree(h, op, A, C, K, R);
    if (tile_fits) return reduce_rows(h, op, A, C, K, R);
  } else if ((m == 2 && red[0]) || (m == 3 && red[1])) {                    // [R, K0] or [K1, R, K0]
    const int64_t K1 = m == 2 ? 1 : n[0], R = n[m - 2], K0 = n[m - 1];
    if (tile_fits && outs < 64 * 4 * (int64_t)h->num_cu) {
      if (K1 * ((K0 + 63) / 64) >= 2 * (int64_t)h->num_cu) return launch_tile<64, true>(h, op, A, C, K1, R, K0);
      return launch_tile<16, true>(h, op, A, C, K1, R, K0);                  // (128-byte pieces of a row: whole cache lines)
    }
    const dim3 grid(grid_for(h, (outs + 255) / 256));
    switch (op) {
#define X(O) case O: hipLaunchKernelGGL((reduce_cols_kernel<O>), grid, dim3(256), 0, h->stream, A, C, K1, R, K0); break;
      EW_REDUCERS(X)
#undef X
      default: break;
    }
    ND4_HIP(hipGetLastError());
    return 0;
  }
  RedElemArgs a;
  a.A = A; a.C = C; a.total = outs;
  for (int k = 0; k < 4; k++) { a.kn[k] = 1; a.ks[k] = 0; a.rn[k] = 1; a.rs[k] = 0; }
  int nk = 0, nr = 0;
  int64_t s = 1;
  for (int d = m - 1; d >= 0; d--) {                                         // innermost first
    if (red[d]) { a.rn[nr] = n[d]; a.rs[nr] = s; nr++; }
    else { a.kn[nk] = n[d]; a.ks[nk] = s; nk++; }
    s *= n[d];
  }
  const dim3 grid(grid_for(h, (outs + 255) / 256));
  switch (op) {
#define X(O) case O: hipLaunchKernelGGL((reduce_elems_kernel<O>), grid, dim3(256), 0, h->stream, a); break;
    EW_REDUCERS(X)
#undef X
    default: break;
  }
  ND4_HIP(hipGetLastError());
  return 0;
}
