// Strided N-d copy on the device: what NDArray.sliceElems, transpose(...axes), concat and stack come down to once their
// planners (la.py, index.js) have turned them into a box, two offsets and two stride vectors:
//
//   dst[dst_off + sum_d i_d dst_stride_d] = src[src_off + sum_d i_d src_stride_d]     for every i in the box shape[0..nd)
//
// Nothing here computes: elements are opaque 4-byte or 8-byte words moved as integers (NaN payloads, -0 and denormals keep
// their bits). The entry point proves on the host that neither side leaves its allocation and that the two sides do not
// intersect before it launches anything, so no kernel checks an address.
//
// Three kernels, all indexed flat in 64 bits, none with the batch in a grid dimension, at most 8 workgroups per CU:
//   * rows:  a work item is one index of the outer axes times a block of the two innermost axes (whole rows while they are
//            short, pieces of 2048 words of one row otherwise). The item's outer index is decomposed once, from values that are
//            the same in every lane (the outer extents and strides wait in LDS). Rows of at least 256 words are walked without
//            a division, four loads in flight per lane; shorter rows pay one 32-bit division per element. Where the innermost
//            stride is 1 on both sides and lengths, pitches and addresses allow it, the box is rewritten in 16-byte words
//            first (8-byte words for int32 rows that only allow that). Stepped and reversed innermost axes take the same kernel.
//   * tiles: the innermost axis of dst is not the axis on which src has stride 1 (a true axis permutation): 64 x 64 tiles
//            through LDS over that pair of axes, as the transposition of struct.hip, so that both global sides are coalesced;
//            16-byte accesses on both sides for 8-byte words where extents, strides and addresses are even. A box that was
//            rewritten in 16-byte words (complex128 pairs) moves them whole, in 32 x 32 tiles.
//   * elems: one thread per element with up to 8 divisions, 32-bit ones while the box has fewer than 2^32 elements. Small boxes
//            and boxes whose two innermost axes are too small to fill a work item.
#include "nd4hip_internal.h"
#include <algorithm>

namespace {

typedef uint32_t u32;
typedef unsigned long long u64;
typedef ulonglong2 u64x2;

constexpr int GATHER_MAX_ND = 8;
constexpr int GATHER_OUTER = GATHER_MAX_ND - 2;   // axes beside the two that a work item spans
constexpr int GATHER_TILE = 64;                  // 32 for 16-byte words
constexpr int64_t GATHER_ITEM = 2048;             // words per work item of the rows kernel
constexpr int64_t GATHER_SMALL = 1024;            // boxes of at most this many elements take the elems kernel
constexpr int64_t GATHER_ROWS_MIN = 256;          // the two innermost axes must hold this many words for the rows kernel
constexpr int64_t GATHER_TILE_MIN = 16;           // both axes of the pair must be this long for the tiles kernel

inline unsigned grid_for(const nd4hip_handle* h, int64_t items) {
  const int64_t cap = (int64_t)h->num_cu * 8;
  return (unsigned)(items < cap ? (items < 1 ? 1 : items) : cap);
}

// outer axes innermost first; axis 1 and axis 0 are the pair a work item spans (n1 x n0). Unused outer axes have extent 1, stride 0.
struct PairArgs {
  const void* src; void* dst;
  int64_t oss[GATHER_OUTER], ods[GATHER_OUTER];
  int64_t n1, n0, s1s, s0s, s1d, s0d;
  int64_t R, C;                                   // rows x columns per item
  u32 oshape[GATHER_OUTER];
  u32 nrb, ncb, items;                            // blocks per axis, all items: below 2^31, or the box takes the elems kernel
  int nout;
};

// The outer axes wait in LDS, not in 30 scalar registers that would stay live across the item loop (and spill).
struct OuterAxes { int64_t ss[GATHER_OUTER], ds[GATHER_OUTER]; u32 n[GATHER_OUTER]; };
__device__ inline void outer_stage(const PairArgs& a, OuterAxes& o) {
  const int t = threadIdx.x;
  if (t < GATHER_OUTER) { o.ss[t] = a.oss[t]; o.ds[t] = a.ods[t]; o.n[t] = a.oshape[t]; }
  __syncthreads();
}
// the part of the item index beyond the pair -> offsets on both sides; w is the same in every lane
__device__ inline void outer_offsets(const OuterAxes& o, int nout, u32 w, int64_t& so, int64_t& dof) {
  so = 0; dof = 0;
  for (int d = 0; d < nout; d++) {
    const u32 n = o.n[d], q = w / n, i = w - q * n;
    so += (int64_t)i * o.ss[d]; dof += (int64_t)i * o.ds[d];
    w = q;
  }
}

// ---------------------------------------------------------------------------------------------- rows
// UNIT: the innermost stride is 1 on both sides (the row copy); otherwise a stepped or reversed innermost axis
template <typename T, bool UNIT>
__global__ __launch_bounds__(256) void gather_rows_kernel(PairArgs a) {
  __shared__ OuterAxes outer;
  outer_stage(a, outer);
  const int64_t s0s = UNIT ? 1 : a.s0s, s0d = UNIT ? 1 : a.s0d;
  const T* __restrict__ src = static_cast<const T*>(a.src);
  T* __restrict__ dst = static_cast<T*>(a.dst);
  const int tid = threadIdx.x;
  for (u32 w = blockIdx.x; w < a.items; w += gridDim.x) {
    const u32 t = w / a.ncb, cb = w - t * a.ncb, o = t / a.nrb, rb = t - o * a.nrb;
    int64_t so, dof;
    outer_offsets(outer, a.nout, o, so, dof);
    const int64_t r0 = (int64_t)rb * a.R, c0 = (int64_t)cb * a.C;
    const u32 rc = (u32)(a.n1 - r0 < a.R ? a.n1 - r0 : a.R), cc = (u32)(a.n0 - c0 < a.C ? a.n0 - c0 : a.C);
    const T* s = src + so + r0 * a.s1s + c0 * s0s;
    T* d = dst + dof + r0 * a.s1d + c0 * s0d;
    if (rc == 1 || cc >= 256) {
      // row by row, no division; four loads in flight per lane before the first store, so that the item's index arithmetic
      // is paid once per 16 KiB and more
      for (u32 r = 0; r < rc; r++) {
        const T* sr = s + (int64_t)r * a.s1s;
        T* dr = d + (int64_t)r * a.s1d;
        u32 j = tid;
        for (; j + 768 < cc; j += 1024) {
          const T v0 = sr[(int64_t)j * s0s], v1 = sr[(int64_t)(j + 256) * s0s], v2 = sr[(int64_t)(j + 512) * s0s],
                  v3 = sr[(int64_t)(j + 768) * s0s];
          dr[(int64_t)j * s0d] = v0; dr[(int64_t)(j + 256) * s0d] = v1; dr[(int64_t)(j + 512) * s0d] = v2;
          dr[(int64_t)(j + 768) * s0d] = v3;
        }
        for (; j < cc; j += 256) dr[(int64_t)j * s0d] = sr[(int64_t)j * s0s];
      }
    } else {                                                // rc whole rows shorter than the workgroup: one 32-bit division per element
      const u32 n = rc * cc;
      for (u32 x = tid; x < n; x += 256) {
        const u32 r = x / cc, j = x - r * cc;
        d[(int64_t)r * a.s1d + (int64_t)j * s0d] = s[(int64_t)r * a.s1s + (int64_t)j * s0s];
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------- tiles
// axis 1 is the axis on which src has stride 1 (s1s == 1), axis 0 the innermost axis of dst (s0d == 1):
//   dst[i1 s1d + i0] = src[i1 + i0 s0s];   the tile is indexed [i0][i1]
template <typename T, int TS, bool VEC>
__global__ __launch_bounds__(256) void gather_tiles_kernel(PairArgs a) {
  __shared__ T tile[TS][TS + 1];
  __shared__ OuterAxes outer;
  outer_stage(a, outer);
  const T* __restrict__ src = static_cast<const T*>(a.src);
  T* __restrict__ dst = static_cast<T*>(a.dst);
  const int tid = threadIdx.x;
  for (u32 w = blockIdx.x; w < a.items; w += gridDim.x) {
    const u32 t = w / a.ncb, cb = w - t * a.ncb, o = t / a.nrb, rb = t - o * a.nrb;     // cb: tile along axis 1, rb: tile along axis 0
    int64_t so, dof;
    outer_offsets(outer, a.nout, o, so, dof);
    const int64_t p0 = (int64_t)cb * TS, q0 = (int64_t)rb * TS;
    const T* s = src + so;
    T* d = dst + dof;
    __syncthreads();                                       // the previous item's reads of the tile are done
    if constexpr (VEC) {                                   // TS == 64, T = u64
      const int c = (tid & 31) * 2;
      for (int r = tid >> 5; r < TS; r += 8)
        if (q0 + r < a.n0 && p0 + c < a.n1) {              // n1 is even: the pair is inside or outside as one
          const u64x2 v = *reinterpret_cast<const u64x2*>(s + (q0 + r) * a.s0s + p0 + c);
          tile[r][c] = v.x; tile[r][c + 1] = v.y;
        }
    } else {
      const int c = tid % TS;
      for (int r = tid / TS; r < TS; r += 256 / TS)
        if (q0 + r < a.n0 && p0 + c < a.n1) tile[r][c] = s[(q0 + r) * a.s0s + p0 + c];
    }
    __syncthreads();
    if constexpr (VEC) {
      // as in struct.hip: a 32-lane half stores two output rows, word addresses 130 q + (jj | jj+1): banks 4 q and 4 q + 2
      const int l = tid & 63, q = l & 15, rsel = (l >> 4) & 1, i = 2 * (q + 16 * (l >> 5));
      for (int jj = (tid >> 6) * 2 + rsel; jj < TS; jj += 8)
        if (p0 + jj < a.n1 && q0 + i < a.n0) {             // n0 is even
          u64x2 v; v.x = tile[i][jj]; v.y = tile[i + 1][jj];
          *reinterpret_cast<u64x2*>(d + (p0 + jj) * a.s1d + q0 + i) = v;
        }
    } else {
      const int c = tid % TS;
      for (int jj = tid / TS; jj < TS; jj += 256 / TS)
        if (p0 + jj < a.n1 && q0 + c < a.n0) d[(p0 + jj) * a.s1d + q0 + c] = tile[c][jj];
    }
  }
}

// ---------------------------------------------------------------------------------------------- elems
// axes innermost first; unused axes have extent 1
struct ElemArgs {
  const void* src; void* dst;
  int64_t shape[GATHER_MAX_ND], ss[GATHER_MAX_ND], ds[GATHER_MAX_ND];
  int64_t total;
  int nd;
};

template <typename T, typename I>
__global__ __launch_bounds__(256) void gather_elems_kernel(ElemArgs a) {
  const T* __restrict__ src = static_cast<const T*>(a.src);
  T* __restrict__ dst = static_cast<T*>(a.dst);
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < a.total; e += (int64_t)gridDim.x * blockDim.x) {
    I w = (I)e;
    int64_t so = 0, dof = 0;
#pragma unroll
    for (int d = 0; d < GATHER_MAX_ND; d++) {
      if (d >= a.nd) break;
      const I n = (I)a.shape[d], q = w / n, i = w - q * n;
      so += (int64_t)i * a.ss[d]; dof += (int64_t)i * a.ds[d];
      w = q;
    }
    dst[dof] = src[so];
  }
}

// ---------------------------------------------------------------------------------------------- host side
struct Box {
  int nd;
  int64_t shape[GATHER_MAX_ND], ss[GATHER_MAX_ND], ds[GATHER_MAX_ND];     // outermost first, as the caller gave them
};

// lowest and highest element reached from off; false if it leaves [0, len)
bool reach(const Box& b, const int64_t* strides, int64_t off, int64_t len, int64_t* lo_out, int64_t* hi_out) {
  __int128 lo = off, hi = off;
  for (int d = 0; d < b.nd; d++) {
    const __int128 span = (__int128)(b.shape[d] - 1) * strides[d];
    if (span < 0) lo += span; else hi += span;
  }
  if (lo < 0 || hi >= (__int128)len) return false;
  *lo_out = (int64_t)lo; *hi_out = (int64_t)hi;
  return true;
}

// the box in words W times as wide, if the innermost axis has stride 1 on both sides and everything is a multiple of W
bool widen(Box& b, int W, uintptr_t s_addr, uintptr_t d_addr, int elem_bytes) {
  if (b.nd < 1) return false;
  const int in = b.nd - 1;
  if (b.ss[in] != 1 || b.ds[in] != 1 || b.shape[in] % W != 0) return false;
  if (s_addr % (uintptr_t)(W * elem_bytes) != 0 || d_addr % (uintptr_t)(W * elem_bytes) != 0) return false;
  for (int d = 0; d < in; d++)
    if (b.ss[d] % W != 0 || b.ds[d] % W != 0) return false;
  b.shape[in] /= W;
  for (int d = 0; d < in; d++) { b.ss[d] /= W; b.ds[d] /= W; }
  if (b.shape[in] == 1 && b.nd > 1) b.nd--;                 // the row was one wide word: the axis is gone
  return true;
}

template <typename T>
int launch_elems(nd4hip_handle* h, const Box& b, const void* s, void* d, int64_t total) {
  ElemArgs a;
  a.src = s; a.dst = d; a.total = total; a.nd = b.nd;
  for (int k = 0; k < GATHER_MAX_ND; k++) { a.shape[k] = 1; a.ss[k] = 0; a.ds[k] = 0; }
  for (int k = 0; k < b.nd; k++) { a.shape[k] = b.shape[b.nd - 1 - k]; a.ss[k] = b.ss[b.nd - 1 - k]; a.ds[k] = b.ds[b.nd - 1 - k]; }
  const dim3 grid(grid_for(h, (total + 255) / 256));
  if (total < ((int64_t)1 << 32)) hipLaunchKernelGGL((gather_elems_kernel<T, u32>), grid, dim3(256), 0, h->stream, a);
  else hipLaunchKernelGGL((gather_elems_kernel<T, u64>), grid, dim3(256), 0, h->stream, a);
  ND4_HIP(hipGetLastError());
  return 0;
}

// every axis but ax1 and ax0 becomes an outer axis (innermost first)
void pair_args(const Box& b, int ax1, int ax0, const void* s, void* d, PairArgs* a) {
  a->src = s; a->dst = d; a->nout = 0;
  for (int k = 0; k < GATHER_OUTER; k++) { a->oshape[k] = 1; a->oss[k] = 0; a->ods[k] = 0; }
  for (int k = b.nd - 1; k >= 0; k--)
    if (k != ax1 && k != ax0) { a->oshape[a->nout] = (u32)b.shape[k]; a->oss[a->nout] = b.ss[k]; a->ods[a->nout] = b.ds[k]; a->nout++; }
  a->n0 = b.shape[ax0]; a->s0s = b.ss[ax0]; a->s0d = b.ds[ax0];
  if (ax1 >= 0) { a->n1 = b.shape[ax1]; a->s1s = b.ss[ax1]; a->s1d = b.ds[ax1]; }
  else { a->n1 = 1; a->s1s = 0; a->s1d = 0; }
}

// the item count of a pair kernel, or false when it does not fit 31 bits (total does: the caller checked)
bool set_items(PairArgs* a, int64_t nrb, int64_t ncb, int64_t total) {
  const int64_t per = a->n1 * a->n0, outer = total / per;
  if (nrb > INT32_MAX || ncb > INT32_MAX || outer > INT32_MAX) return false;
  const __int128 items = (__int128)outer * nrb * ncb;
  if (items > INT32_MAX) return false;
  a->nrb = (u32)nrb; a->ncb = (u32)ncb; a->items = (u32)items;
  return true;
}

template <typename T>
int launch_rows(nd4hip_handle* h, const Box& b, const void* s, void* d, int64_t total) {
  PairArgs a;
  pair_args(b, b.nd - 2, b.nd - 1, s, d, &a);
  if (a.n0 >= GATHER_ITEM) { a.R = 1; a.C = GATHER_ITEM; }
  else { a.R = std::min<int64_t>(a.n1, GATHER_ITEM / a.n0); a.C = a.n0; }
  if (!set_items(&a, (a.n1 + a.R - 1) / a.R, (a.n0 + a.C - 1) / a.C, total)) return launch_elems<T>(h, b, s, d, total);
  if (a.s0s == 1 && a.s0d == 1) hipLaunchKernelGGL((gather_rows_kernel<T, true>), dim3(grid_for(h, a.items)), dim3(256), 0, h->stream, a);
  else hipLaunchKernelGGL((gather_rows_kernel<T, false>), dim3(grid_for(h, a.items)), dim3(256), 0, h->stream, a);
  ND4_HIP(hipGetLastError());
  return 0;
}

template <typename T, int TS, bool VEC>
int launch_tiles(nd4hip_handle* h, const Box& b, int ax1, const void* s, void* d, int64_t total) {
  PairArgs a;
  pair_args(b, ax1, b.nd - 1, s, d, &a);
  a.R = a.C = TS;
  // nrb: tiles along axis 0; ncb: tiles along axis 1, walked first: consecutive items read on along src
  if (!set_items(&a, (a.n0 + TS - 1) / TS, (a.n1 + TS - 1) / TS, total)) return launch_elems<T>(h, b, s, d, total);
  hipLaunchKernelGGL((gather_tiles_kernel<T, TS, VEC>), dim3(grid_for(h, a.items)), dim3(256), 0, h->stream, a);
  ND4_HIP(hipGetLastError());
  return 0;
}

bool all_even(const Box& b, int ax1) {
  const int in = b.nd - 1;
  if (b.shape[ax1] % 2 || b.shape[in] % 2 || b.ss[in] % 2 || b.ds[ax1] % 2) return false;
  for (int d = 0; d < b.nd; d++)
    if (d != ax1 && d != in && (b.ss[d] % 2 || b.ds[d] % 2)) return false;
  return true;
}

template <typename T>
int dispatch(nd4hip_handle* h, const Box& b, const void* s, void* d, int64_t total, bool vec_tiles) {
  const int in = b.nd - 1;
  if (b.nd == 0 || total <= GATHER_SMALL) return launch_elems<T>(h, b, s, d, total);
  if (!(b.ss[in] == 1 && b.ds[in] == 1) && b.ds[in] == 1 && b.shape[in] >= GATHER_TILE_MIN) {
    for (int p = in - 1; p >= 0; p--)
      if (b.ss[p] == 1 && b.shape[p] >= GATHER_TILE_MIN) {
        if constexpr (sizeof(T) == 8) {
          if (vec_tiles && all_even(b, p)) return launch_tiles<T, GATHER_TILE, true>(h, b, p, s, d, total);
        }
        return launch_tiles<T, (sizeof(T) == 16 ? GATHER_TILE / 2 : GATHER_TILE), false>(h, b, p, s, d, total);
      }
  }
  const int64_t area = b.shape[in] * (b.nd >= 2 ? b.shape[in - 1] : 1);
  if (area >= GATHER_ROWS_MIN) return launch_rows<T>(h, b, s, d, total);
  return launch_elems<T>(h, b, s, d, total);
}

}  // namespace

extern "C" int nd4hip_gather_nd_dev(nd4hip_handle* h, int elem_bytes, int ndim, const int64_t* shape, const void* src, int64_t src_len,
                                    int64_t src_off, const int64_t* src_strides, void* dst, int64_t dst_len, int64_t dst_off,
                                    const int64_t* dst_strides) {
  ND4_CHECK_ARG(h != nullptr, "nd4hip_gather_nd: NULL handle");
  ND4_CHECK_ARG(elem_bytes == 4 || elem_bytes == 8, "nd4hip_gather_nd: elem_bytes=%d is neither 4 nor 8", elem_bytes);
  ND4_CHECK_ARG(ndim >= 0 && ndim <= GATHER_MAX_ND, "nd4hip_gather_nd: ndim=%d is not in 0..%d", ndim, GATHER_MAX_ND);
  ND4_CHECK_ARG(ndim == 0 || (shape && src_strides && dst_strides), "nd4hip_gather_nd: NULL shape or strides");
  ND4_CHECK_ARG(src && dst, "nd4hip_gather_nd: NULL pointer");
  ND4_CHECK_ARG(src_len >= 1 && dst_len >= 1 && src_len <= INT64_MAX / 8 && dst_len <= INT64_MAX / 8, "nd4hip_gather_nd: bad allocation length");
  Box b;
  b.nd = ndim;
  __int128 count = 1;
  for (int d = 0; d < ndim; d++) {
    ND4_CHECK_ARG(shape[d] >= 1, "nd4hip_gather_nd: extent %lld of axis %d is less than 1", (long long)shape[d], d);
    b.shape[d] = shape[d]; b.ss[d] = src_strides[d]; b.ds[d] = dst_strides[d];
    count *= shape[d];
    ND4_CHECK_ARG(count <= (__int128)dst_len, "nd4hip_gather_nd: the box has more elements than dst");
  }
  const int64_t total = (int64_t)count;
  int64_t slo, shi, dlo, dhi;
  ND4_CHECK_ARG(reach(b, b.ss, src_off, src_len, &slo, &shi), "nd4hip_gather_nd: the box leaves src [0, %lld)", (long long)src_len);
  ND4_CHECK_ARG(reach(b, b.ds, dst_off, dst_len, &dlo, &dhi), "nd4hip_gather_nd: the box leaves dst [0, %lld)", (long long)dst_len);
  const uintptr_t sb = reinterpret_cast<uintptr_t>(src), db = reinterpret_cast<uintptr_t>(dst), eb = (uintptr_t)elem_bytes;
  ND4_CHECK_ARG(!(sb + (uintptr_t)slo * eb < db + ((uintptr_t)dhi + 1) * eb && db + (uintptr_t)dlo * eb < sb + ((uintptr_t)shi + 1) * eb),
                "nd4hip_gather_nd: dst must not overlap src");
  Nd4DeviceGuard guard(h);
  Nd4Prof prof(h, "gather_nd", 0.0, 2.0 * (double)elem_bytes * (double)total);
  const char* s = static_cast<const char*>(src) + src_off * elem_bytes;
  char* d = static_cast<char*>(dst) + dst_off * elem_bytes;
  const uintptr_t sa = reinterpret_cast<uintptr_t>(s), da = reinterpret_cast<uintptr_t>(d);
  const bool vec_tiles = sa % 16 == 0 && da % 16 == 0;
  if (elem_bytes == 8) {
    Box w = b;
    if (widen(w, 2, sa, da, 8)) return dispatch<u64x2>(h, w, s, d, total / 2, false);
    return dispatch<u64>(h, b, s, d, total, vec_tiles);
  }
  Box w = b;
  if (widen(w, 4, sa, da, 4)) return dispatch<u64x2>(h, w, s, d, total / 4, false);
  if (widen(w, 2, sa, da, 4)) return dispatch<u64>(h, w, s, d, total / 2, false);
  return dispatch<u32>(h, b, s, d, total, false);
}
