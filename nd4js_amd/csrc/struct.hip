// Structure functions of nd.la on the device: transposition, tril / triu (tri.js:23-42), diag / diag_mat (diag.js:23-88) and
// permute_rows / permute_cols / unpermute_rows / unpermute_cols (permute.js:23-306). Nothing here computes: every element is
// moved as a 64-bit word (NaN payloads, -0, denormals and Inf keep their bits) or filled with +0.0 (all bits zero).
//
// Two regimes per operation, both indexed flat so that no launch depends on the batch fitting a grid dimension:
//   * large members: 64 x 64 tiles through LDS for the transposition (16-byte global accesses on both sides where M, N and the base
//     addresses are even, a 65-word row pitch so that the 8-byte column reads fall on distinct banks), row blocks for the gathers
//     (a row gather is a row copy, a column gather stages its rows in LDS and gathers there);
//   * very many tiny members: one workgroup walks many members (a flat element index, resp. groups of members per work item).
// unpermute_* is a gather through inv[k] = the largest i with P[i] = k (-1: a zero row / column), built with 32-bit integer
// atomicMax in LDS (a work item that holds whole members, M N <= STRUCT_STAGE) or in the handle's workspace (members cut into
// row blocks, maps beyond STRUCT_LDS_MAP): the reference's "a later i overwrites an earlier one",
// without racing stores. An index outside [0, L) raises a flag word and is never turned into an address.
#include "nd4hip_args.h"
#include <algorithm>

namespace {

typedef unsigned long long u64;
typedef ulonglong2 u64x2;

constexpr int STRUCT_TILE = 64;             // transposition tile
constexpr int STRUCT_FLAT_MAX = 1024;       // members of at most this many elements are transposed by the flat form
constexpr int STRUCT_STAGE = 4096;          // 64-bit words of LDS staging per work item of the gathers
constexpr int STRUCT_LDS_MAP = 4096;        // the inverse map of a work item lives in LDS up to this many entries

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
inline unsigned grid_for(const nd4hip_handle* h, int64_t items) {
  const int64_t cap = (int64_t)h->num_cu * 8;
  return (unsigned)(items < cap ? (items < 1 ? 1 : items) : cap);
}

// ---------------------------------------------------------------------------------------------- transposition
// B[b, j, i] = A[b, i, j]; work item = one tile of one member, consecutive items walk a row of tiles
template <bool VEC>
__global__ __launch_bounds__(256) void transpose_tiled_kernel(int64_t batch, int64_t M, int64_t N, const u64* __restrict__ A,
                                                              u64* __restrict__ B, int64_t tm, int64_t tn) {
  __shared__ u64 tile[STRUCT_TILE][STRUCT_TILE + 1];
  const int tid = threadIdx.x;
  const int64_t per = tm * tn, total = batch * per;
  for (int64_t w = blockIdx.x; w < total; w += gridDim.x) {
    const int64_t b = w / per, t = w - b * per, ti = t / tn, tj = t - ti * tn;
    const int64_t i0 = ti * STRUCT_TILE, j0 = tj * STRUCT_TILE;
    const u64* src = A + b * M * N;
    u64* dst = B + b * M * N;
    __syncthreads();                                       // the previous item's reads of the tile are done
    if (VEC) {
      const int c = (tid & 31) * 2;
      for (int r = tid >> 5; r < STRUCT_TILE; r += 8)
        if (i0 + r < M && j0 + c < N) {                    // N is even: the pair is inside or outside as one
          const u64x2 v = *reinterpret_cast<const u64x2*>(src + (i0 + r) * N + j0 + c);
          tile[r][c] = v.x; tile[r][c + 1] = v.y;
        }
    } else {
      const int c = tid & 63;
      for (int r = tid >> 6; r < STRUCT_TILE; r += 4)
        if (i0 + r < M && j0 + c < N) tile[r][c] = src[(i0 + r) * N + j0 + c];
    }
    __syncthreads();
    if (VEC) {
      // a 32-lane half reads two output rows: lanes 0..15 the row pairs (2q, 2q+1) of column jj, lanes 16..31 those of column
      // jj+1: word addresses 130 q + (jj | jj+1), i.e. banks 4 q and 4 q + 2: all distinct
      const int l = tid & 63, q = l & 15, rsel = (l >> 4) & 1, i = 2 * (q + 16 * (l >> 5));
      for (int jj = (tid >> 6) * 2 + rsel; jj < STRUCT_TILE; jj += 8)
        if (j0 + jj < N && i0 + i < M) {                   // M is even
          u64x2 v; v.x = tile[i][jj]; v.y = tile[i + 1][jj];
          *reinterpret_cast<u64x2*>(dst + (j0 + jj) * M + i0 + i) = v;
        }
    } else {
      const int c = tid & 63;
      for (int jj = tid >> 6; jj < STRUCT_TILE; jj += 4)
        if (j0 + jj < N && i0 + c < M) dst[(j0 + jj) * M + i0 + c] = tile[c][jj];
    }
  }
}

// tiny members: one thread per output element over the whole batch (coalesced stores, the strided loads stay inside one member)
__global__ __launch_bounds__(256) void transpose_flat_kernel(int64_t total, int M, int N, const u64* __restrict__ A, u64* __restrict__ B) {
  const int MN = M * N;
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t b = e / MN;
    const int r = (int)(e - b * MN), j = r / M, i = r - j * M;
    B[e] = A[b * MN + i * N + j];
  }
}

// ---------------------------------------------------------------------------------------------- tril / triu
// W = 1: one word per thread and step; W = 2: 16 bytes (N even: both words lie in one row). k is clamped to [-M, N] by the host.
template <int W>
__global__ __launch_bounds__(256) void tri_kernel(int upper, int64_t k, int64_t total, int64_t M, int64_t N, const u64* __restrict__ A,
                                                  u64* __restrict__ B) {
  for (int64_t p = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; p * W < total; p += (int64_t)gridDim.x * blockDim.x) {
    const int64_t e = p * W, row = e / N, j = e - row * N, i = row % M;
    if (W == 2) {
      u64x2 v = reinterpret_cast<const u64x2*>(A)[p];
      if (upper ? i > j - k : i < j - k) v.x = 0;
      if (upper ? i > j + 1 - k : i < j + 1 - k) v.y = 0;
      reinterpret_cast<u64x2*>(B)[p] = v;
    } else {
      const u64 v = A[e];
      B[e] = (upper ? i > j - k : i < j - k) ? 0ull : v;
    }
  }
}

// ---------------------------------------------------------------------------------------------- diag / diag_mat
__global__ __launch_bounds__(256) void diag_kernel(int64_t total, int64_t L, int64_t MN, int64_t N, int64_t a_off, const u64* __restrict__ A,
                                                   u64* __restrict__ d) {
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t b = e / L, i = e - b * L;
    d[e] = A[b * MN + a_off + i * (N + 1)];
  }
}
template <int W>
__global__ __launch_bounds__(256) void diagmat_kernel(int64_t total, int64_t N, const u64* __restrict__ d, u64* __restrict__ Dm) {
  for (int64_t p = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; p * W < total; p += (int64_t)gridDim.x * blockDim.x) {
    const int64_t e = p * W, row = e / N, j = e - row * N, i = row % N;     // row = b N + i is also the index into d
    if (W == 2) {
      u64x2 v; v.x = 0; v.y = 0;
      if (i == j) v.x = d[row];
      if (i == j + 1) v.y = d[row];
      reinterpret_cast<u64x2*>(Dm)[p] = v;
    } else {
      Dm[e] = i == j ? d[row] : 0ull;
    }
  }
}

// ---------------------------------------------------------------------------------------------- (un)permute_rows / _cols
// inv[b, k] = max i with P[b, i] = k for maps too long for LDS; inv is -1 on entry
__global__ __launch_bounds__(256) void inv_build_kernel(int64_t total, int64_t L, const int32_t* __restrict__ P, int64_t sP, int* __restrict__ inv,
                                                        int* __restrict__ flag) {
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t b = t / L, i = t - b * L;
    const int32_t k = P[b * sP + i];
    if ((uint32_t)k < (uint64_t)L) atomicMax(&inv[b * L + k], (int)i);
    else atomicOr(flag, 1);
  }
}

struct PermArgs {
  int64_t batch, M, N;        // N in units of T for the row forms
  const void* A; int64_t sA;  // sA in units of T
  const int32_t* P; int64_t sP;
  const int* inv;             // inverse map in the workspace [batch or 1, L], or NULL
  void* B;
  int* flag;
  int64_t G, RB, nrb;         // members per work item, rows per work item, row blocks per member
  int inverse, lds_map;
};

// Work item = G consecutive members x one block of RB rows. T = u64, or u64x2 for a row gather of even, aligned rows.
// COLS && STAGE: the item's rows go through LDS and the gather happens there (G RB N <= STRUCT_STAGE).
template <typename T, bool COLS, bool STAGE>
__global__ __launch_bounds__(256) void perm_kernel(PermArgs a) {
  __shared__ u64 stage[STAGE ? STRUCT_STAGE : 1];
  __shared__ int inv_l[STRUCT_LDS_MAP];
  const int tid = threadIdx.x;
  const int64_t M = a.M, N = a.N, L = COLS ? N : M;
  const T* A = static_cast<const T*>(a.A);
  T* B = static_cast<T*>(a.B);
  const int64_t groups = (a.batch + a.G - 1) / a.G, items = groups * a.nrb;
  for (int64_t w = blockIdx.x; w < items; w += gridDim.x) {
    const int64_t grp = w / a.nrb, rb = w - grp * a.nrb, b0 = grp * a.G, r0 = rb * a.RB;
    const int gc = (int)(a.batch - b0 < a.G ? a.batch - b0 : a.G);
    const int64_t rc = M - r0 < a.RB ? M - r0 : a.RB;
    __syncthreads();                                       // the previous item is done with LDS
    if (a.inverse && a.lds_map) {
      const int n = gc * (int)L;
      for (int t = tid; t < n; t += 256) inv_l[t] = -1;
      __syncthreads();
      for (int t = tid; t < n; t += 256) {
        const int g = t / (int)L, i = t - g * (int)L;
        const int32_t k = a.P[(b0 + g) * a.sP + i];
        if ((uint32_t)k < (uint64_t)L) atomicMax(&inv_l[g * (int)L + k], i);
        else atomicOr(a.flag, 1);
      }
    }
    if constexpr (STAGE) {
      const int n = gc * (int)(rc * N), per = (int)(rc * N);
      for (int x = tid; x < n; x += 256) {
        const int g = x / per, rem = x - g * per;
        stage[x] = reinterpret_cast<const u64*>(A)[(b0 + g) * a.sA + r0 * N + rem];
      }
    }
    __syncthreads();
    // element (g, r, j) of the item: member b0 + g, row r0 + r, column j
    auto move = [&](int g, int64_t r, int64_t j) {
      const int64_t idx = COLS ? j : r0 + r;
      int32_t m;
      if (!a.inverse) {
        m = a.P[(b0 + g) * a.sP + idx];
        if ((uint32_t)m >= (uint64_t)L) { atomicOr(a.flag, 1); return; }       // never an address
      } else {
        m = a.lds_map ? inv_l[g * (int)L + (int)idx] : a.inv[(a.sP ? b0 + g : 0) * L + idx];
      }
      T v = T();                                            // +0.0
      if (m >= 0) {
        if constexpr (!COLS) v = A[(b0 + g) * a.sA + (int64_t)m * N + j];
        else if constexpr (STAGE) v = stage[((int64_t)g * rc + r) * N + m];
        else v = A[(b0 + g) * a.sA + (r0 + r) * N + m];
      }
      B[((b0 + g) * M + r0 + r) * N + j] = v;
    };
    if (N >= 256) {                                         // long rows: row by row, no division per element
      for (int g = 0; g < gc; g++)
        for (int64_t r = 0; r < rc; r++)
          for (int64_t j = tid; j < N; j += 256) move(g, r, j);
    } else {                                                // short rows: a flat index over the item, which has at most STRUCT_STAGE elements
      const uint32_t n32 = (uint32_t)N, rc32 = (uint32_t)rc, n = (uint32_t)gc * rc32 * n32;
      for (uint32_t x = tid; x < n; x += 256) {
        const uint32_t row = x / n32, g = row / rc32;
        move((int)g, row - g * rc32, x - row * n32);
      }
    }
  }
}

bool overlaps(const void* a, size_t na, const void* b, size_t nb) {
  const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
  return na != 0 && nb != 0 && x < y + nb && y < x + na;
}

// reads the flag word back (synchronises the stream)
int flag_raised(nd4hip_handle* h, const int* flag, int* out) {
  void* hp = nullptr;
  ND4_TRY(nd4_pinned(h, sizeof(int), &hp));
  ND4_HIP(hipMemcpyAsync(hp, flag, sizeof(int), hipMemcpyDeviceToHost, h->stream));
  ND4_HIP(hipStreamSynchronize(h->stream));
  *out = *static_cast<int*>(hp);
  return 0;
}

// enqueues the kernels of one dpermute call; flag is zero on entry
int launch_permute(nd4hip_handle* h, int cols, int inverse, int64_t batch, int64_t M, int64_t N, const double* A, int64_t strideA,
                   const int32_t* P, int64_t strideP, double* B, int* flag) {
  const int64_t L = cols ? N : M;
  void* p = nullptr;
  PermArgs a;
  a.batch = batch; a.M = M; a.N = N; a.A = A; a.sA = strideA; a.P = P; a.sP = strideP; a.inv = nullptr; a.B = B; a.flag = flag;
  a.inverse = inverse ? 1 : 0;
  // work items: whole groups of tiny members, or row blocks of one member
  const int64_t MN = M * N;
  bool stage = false;
  if (MN <= STRUCT_STAGE) {
    const int64_t fill = (batch + (int64_t)h->num_cu * 4 - 1) / ((int64_t)h->num_cu * 4);     // keep every CU busy before growing the groups
    a.G = std::max<int64_t>(1, std::min<int64_t>(STRUCT_STAGE / MN, fill));
    a.RB = M; a.nrb = 1; stage = cols != 0;
  } else {
    a.G = 1;
    a.RB = std::max<int64_t>(1, STRUCT_STAGE / N);
    a.nrb = (M + a.RB - 1) / a.RB;
    stage = cols != 0 && N <= STRUCT_STAGE;
  }
  // the map is built in LDS by the work item that uses it; a member cut into row blocks would rebuild it once per block (at
  // 4096^2, one row per block, unpermute_cols took 107 us that way and takes 87 us with the map in the workspace: DESIGN.md
  // 4.14), so it takes the workspace like a map that does not fit
  a.lds_map = (a.G * L <= STRUCT_LDS_MAP && a.nrb == 1) ? 1 : 0;
  if (inverse && !a.lds_map) {
    const int64_t nP = strideP ? batch : 1;
    ND4_TRY(nd4_ws_alloc(h, (size_t)(nP * L) * sizeof(int), &p));
    int* inv = static_cast<int*>(p);
    ND4_HIP(hipMemsetAsync(inv, 0xFF, (size_t)(nP * L) * sizeof(int), h->stream));
    hipLaunchKernelGGL(inv_build_kernel, dim3(grid_for(h, (nP * L + 255) / 256)), dim3(256), 0, h->stream, nP * L, L, P, strideP, inv, flag);
    ND4_HIP(hipGetLastError());
    a.inv = inv;
  }
  const dim3 grid(grid_for(h, ((batch + a.G - 1) / a.G) * a.nrb));
  if (cols) {
    if (stage) hipLaunchKernelGGL((perm_kernel<u64, true, true>), grid, dim3(256), 0, h->stream, a);
    else hipLaunchKernelGGL((perm_kernel<u64, true, false>), grid, dim3(256), 0, h->stream, a);
  } else if (N % 2 == 0 && strideA % 2 == 0 && aligned16(A) && aligned16(B)) {
    a.N = N / 2; a.sA = strideA / 2;                        // a row is N / 2 16-byte words; rows per item stay as chosen
    hipLaunchKernelGGL((perm_kernel<u64x2, false, false>), grid, dim3(256), 0, h->stream, a);
  } else {
    hipLaunchKernelGGL((perm_kernel<u64, false, false>), grid, dim3(256), 0, h->stream, a);
  }
  ND4_HIP(hipGetLastError());
  return 0;
}

}  // namespace

const char* nd4_permute_name(int cols, int inverse) {
  return inverse ? (cols ? "unpermute_cols" : "unpermute_rows") : (cols ? "permute_cols" : "permute_rows");
}
bool nd4_struct_overlap(const void* in, int64_t in_elems, const void* out, int64_t out_elems) {
  return overlaps(in, (size_t)in_elems * 8, out, (size_t)out_elems * 8);
}

extern "C" int nd4hip_dtranspose_batched_dev(nd4hip_handle* h, int64_t batch, int64_t M, int64_t N, const double* A, double* B) {
  ND4_CHECK_ARG(h != nullptr, "nd4hip_dtranspose_batched: NULL handle");
  ND4_ARGS(nd4_args_dense("dtranspose_batched", {batch, M, N}, {A, B}));
  Nd4DeviceGuard guard(h);
  Nd4Prof prof(h, "dtranspose_batched", 0.0, 16.0 * (double)batch * (double)M * (double)N);
  ND4_CHECK_ARG(!nd4_struct_overlap(A, batch * M * N, B, batch * M * N), "nd4hip_dtranspose_batched: B must not overlap A");
  const u64* a = reinterpret_cast<const u64*>(A);
  u64* b = reinterpret_cast<u64*>(B);
  if (M * N <= STRUCT_FLAT_MAX) {
    const int64_t total = batch * M * N;
    hipLaunchKernelGGL(transpose_flat_kernel, dim3(grid_for(h, (total + 255) / 256)), dim3(256), 0, h->stream, total, (int)M, (int)N, a, b);
  } else {
    const int64_t tm = (M + STRUCT_TILE - 1) / STRUCT_TILE, tn = (N + STRUCT_TILE - 1) / STRUCT_TILE;
    const dim3 grid(grid_for(h, batch * tm * tn));
    if (M % 2 == 0 && N % 2 == 0 && aligned16(A) && aligned16(B))
      hipLaunchKernelGGL(transpose_tiled_kernel<true>, grid, dim3(256), 0, h->stream, batch, M, N, a, b, tm, tn);
    else
      hipLaunchKernelGGL(transpose_tiled_kernel<false>, grid, dim3(256), 0, h->stream, batch, M, N, a, b, tm, tn);
  }
  ND4_HIP(hipGetLastError());
  return 0;
}

extern "C" int nd4hip_dtri_batched_dev(nd4hip_handle* h, int upper, int64_t k, int64_t batch, int64_t M, int64_t N, const double* A, double* B) {
  ND4_CHECK_ARG(h != nullptr, "nd4hip_dtri_batched: NULL handle");
  ND4_ARGS(nd4_args_dense("dtri_batched", {batch, M, N}, {A, B}));
  Nd4DeviceGuard guard(h);
  Nd4Prof prof(h, "dtri_batched", 0.0, 16.0 * (double)batch * (double)M * (double)N);
  ND4_CHECK_ARG(!nd4_struct_overlap(A, batch * M * N, B, batch * M * N), "nd4hip_dtri_batched: B must not overlap A");
  // j - i lies in [-(M-1), N-1]: every k <= -M behaves like -M and every k >= N like N, and j - k cannot overflow
  const int64_t kc = k < -M ? -M : (k > N ? N : k);
  const int64_t total = batch * M * N;
  const u64* a = reinterpret_cast<const u64*>(A);
  u64* b = reinterpret_cast<u64*>(B);
  if (N % 2 == 0 && aligned16(A) && aligned16(B))
    hipLaunchKernelGGL(tri_kernel<2>, dim3(grid_for(h, (total / 2 + 255) / 256)), dim3(256), 0, h->stream, upper ? 1 : 0, kc, total, M, N, a, b);
  else
    hipLaunchKernelGGL(tri_kernel<1>, dim3(grid_for(h, (total + 255) / 256)), dim3(256), 0, h->stream, upper ? 1 : 0, kc, total, M, N, a, b);
  ND4_HIP(hipGetLastError());
  return 0;
}

extern "C" int nd4hip_ddiag_batched_dev(nd4hip_handle* h, int64_t batch, int64_t M, int64_t N, int64_t offset, const double* A, double* d) {
  ND4_CHECK_ARG(h != nullptr, "nd4hip_ddiag_batched: NULL handle");
  ND4_ARGS(nd4_args_diag(batch, M, N, offset, A, d));
  const int64_t L = nd4_diag_length(M, N, offset);
  Nd4DeviceGuard guard(h);
  Nd4Prof prof(h, "ddiag_batched", 0.0, 16.0 * (double)batch * (double)L);
  ND4_CHECK_ARG(!nd4_struct_overlap(A, batch * M * N, d, batch * L), "nd4hip_ddiag_batched: d must not overlap A");
  const int64_t total = batch * L, a_off = offset >= 0 ? offset : -offset * N;
  hipLaunchKernelGGL(diag_kernel, dim3(grid_for(h, (total + 255) / 256)), dim3(256), 0, h->stream, total, L, M * N, N, a_off,
                     reinterpret_cast<const u64*>(A), reinterpret_cast<u64*>(d));
  ND4_HIP(hipGetLastError());
  return 0;
}

extern "C" int nd4hip_ddiagmat_batched_dev(nd4hip_handle* h, int64_t batch, int64_t N, const double* d, double* Dm) {
  ND4_CHECK_ARG(h != nullptr, "nd4hip_ddiagmat_batched: NULL handle");
  ND4_ARGS(nd4_args_dense("ddiagmat_batched", {batch, N}, {d, Dm}));
  Nd4DeviceGuard guard(h);
  Nd4Prof prof(h, "ddiagmat_batched", 0.0, 8.0 * (double)batch * ((double)N + (double)N * (double)N));
  ND4_CHECK_ARG(!nd4_struct_overlap(d, batch * N, Dm, batch * N * N), "nd4hip_ddiagmat_batched: D must not overlap d");
  const int64_t total = batch * N * N;
  if (N % 2 == 0 && aligned16(Dm))
    hipLaunchKernelGGL(diagmat_kernel<2>, dim3(grid_for(h, (total / 2 + 255) / 256)), dim3(256), 0, h->stream, total, N,
                       reinterpret_cast<const u64*>(d), reinterpret_cast<u64*>(Dm));
  else
    hipLaunchKernelGGL(diagmat_kernel<1>, dim3(grid_for(h, (total + 255) / 256)), dim3(256), 0, h->stream, total, N,
                       reinterpret_cast<const u64*>(d), reinterpret_cast<u64*>(Dm));
  ND4_HIP(hipGetLastError());
  return 0;
}

extern "C" int nd4hip_dpermute_batched_dev(nd4hip_handle* h, int cols, int inverse, int64_t batch, int64_t M, int64_t N, const double* A,
                                           int64_t strideA, const int32_t* P, int64_t strideP, double* B) {
  const char* name = nd4_permute_name(cols, inverse);
  ND4_CHECK_ARG(h != nullptr, "nd4hip_dpermute_batched: NULL handle");
  ND4_ARGS(nd4_args_permute(cols, batch, M, N, A, strideA, P, strideP, B));
  const int64_t L = cols ? N : M;
  Nd4DeviceGuard guard(h);
  ND4_CHECK_ARG(!nd4_struct_overlap(A, (strideA ? (batch - 1) * strideA : 0) + M * N, B, batch * M * N),
                "nd4hip_dpermute_batched: B must not overlap A");
  ND4_CHECK_ARG(!overlaps(P, (size_t)((strideP ? (batch - 1) * strideP : 0) + L) * 4, B, (size_t)(batch * M * N) * 8),
                "nd4hip_dpermute_batched: B must not overlap P");
  Nd4WsScope scope(h);
  void* p = nullptr;
  ND4_TRY(nd4_ws_alloc(h, sizeof(int), &p));
  int* flag = static_cast<int*>(p);
  ND4_HIP(hipMemsetAsync(flag, 0, sizeof(int), h->stream));
  {  // the profile brackets the kernels, not the read-back of the flag
    Nd4Prof prof(h, "dpermute_batched", 0.0,
                 8.0 * (double)M * (double)N * (double)(batch + (strideA ? batch : 1)) + 4.0 * (double)L * (double)(strideP ? batch : 1));
    ND4_TRY(launch_permute(h, cols, inverse, batch, M, N, A, strideA, P, strideP, B, flag));
  }
  int raised = 0;
  ND4_TRY(flag_raised(h, flag, &raised));
  ND4_CHECK_ARG(raised == 0, "%s(A,P): P.contains invalid indices.", name);
  return 0;
}
