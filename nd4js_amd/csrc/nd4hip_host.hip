// Host-pointer entry points of include/nd4hip.h (what the N-API shim binds: JS TypedArrays are host memory) on top of the
// *_dev forms, through ONE driver:
//   * the batch axis — the reference's loops over independent matrices (qr.js:43-49, lu.js:34-40, svd_dc.js:918-925,
//     matmul odometer matmul.js:44-70) — is cut into contiguous blocks, one per device of the handle (nd4hip_create_multi),
//     each block driven by its own host thread on its own device, streams and staging: no data-path collective, the only
//     "reductions" (max sweeps, off-norm, rotation count, error code) happen on the host;
//   * inside a block the batch is cut again into chunks that are pipelined: H2D of chunk k+1 and D2H of chunk k-1 run on a copy
//     stream while chunk k computes (two staging sets). Measured on this pool (tools/pcie_bench.hip): pageable host memory
//     moves at the pinned rate (56 GB/s) through hipMemcpyAsync, so the user's buffers are used as they are; the copies block
//     the calling host thread, the kernels do not, which is all the overlap needs;
//   * a single large matmul is pipelined over the ROWS of A and C (B is a broadcast operand).
// Error path: a failing chunk stops the block, the block's streams are synchronised BEFORE its staging returns to the cache.
#include "nd4hip_args.h"
#include <algorithm>
#include <atomic>
#include <climits>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <string>
#include <thread>
#include <vector>

namespace {

constexpr size_t D = sizeof(double);
constexpr size_t ND4_STAGE_CAP = size_t(12) << 30;     // cached staging per device before the cache is trimmed

// Device staging blocks are cached in the handle between calls: every host-pointer call synchronises before it returns, so a
// released block is immediately reusable, and hipMalloc + hipFree (~100 us each, several per call) used to be most of the
// latency of a small call. Best fit among the free blocks that are not more than 4x too large.
struct DevBuf {
  void* p = nullptr;
  nd4hip_handle* h = nullptr;
  int slot = -1;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { release(); }
  void release() {
    if (slot >= 0) h->stage[(size_t)slot].in_use = false;
    else if (p) (void)hipFree(p);
    p = nullptr; slot = -1;
  }
  int alloc(nd4hip_handle* hh, size_t bytes) {
    h = hh;
    if (bytes == 0) bytes = 8;
    int best = -1;
    for (size_t i = 0; i < h->stage.size(); i++) {
      const Nd4Stage& b = h->stage[i];
      if (!b.in_use && b.bytes >= bytes && b.bytes <= 4 * bytes + 4096 && (best < 0 || b.bytes < h->stage[(size_t)best].bytes)) best = (int)i;
    }
    if (best >= 0) { h->stage[(size_t)best].in_use = true; slot = best; p = h->stage[(size_t)best].p; return 0; }
    if (h->stage_bytes + bytes > ND4_STAGE_CAP || h->stage.size() >= 64) {
      bool any_used = false;
      for (const auto& b : h->stage) any_used = any_used || b.in_use;
      if (any_used) { ND4_HIP(hipMalloc(&p, bytes)); slot = -1; return 0; }     // over budget mid-call: an uncached block
      for (auto& b : h->stage) (void)hipFree(b.p);                              // between calls: start the cache afresh
      h->stage.clear(); h->stage_bytes = 0;
    }
    ND4_HIP(hipMalloc(&p, bytes));
    h->stage.push_back(Nd4Stage{p, bytes, true});
    h->stage_bytes += bytes;
    slot = (int)h->stage.size() - 1;
    return 0;
  }
};

// One operand of a batched host-pointer call: `item` elements per batch member, members `stride` elements apart on the host
// (0 = one block shared by all members: uploaded once per device). The device image keeps the same stride.
struct Operand {
  const void* src;      // host source, NULL = not an input
  void* dst;            // host destination, NULL = not an output (src == dst: in place)
  int64_t item;         // elements per batch member
  int64_t stride;       // elements between members (0 = broadcast)
  size_t es;            // bytes per element
};
inline Operand in_op(const void* p, int64_t item, int64_t stride, size_t es = D) { return Operand{p, nullptr, item, stride, es}; }
inline Operand out_op(void* p, int64_t item, size_t es = D) { return Operand{nullptr, p, item, item, es}; }
inline Operand inout_op(void* p, int64_t item, size_t es = D) { return Operand{p, p, item, item, es}; }

// run(hd, dev_index, nb, dptr): nb batch members whose operands start at dptr[i] on device handle hd
using ChunkFn = std::function<int(nd4hip_handle* hd, int dev, int64_t nb, void* const* dptr)>;

struct Plan {
  int64_t min_chunk = 1;                 // never cut a block into chunks smaller than this many members (efficiency of the kernels)
  size_t chunk_bytes = size_t(64) << 20; // target bytes moved per chunk
  int max_chunks = 8;
};

// index, in the caller's batch, of the first member of the chunk whose ChunkFn is running on this thread (for error texts that
// name a member)
thread_local int64_t g_chunk_first = 0;

inline size_t span_bytes(const Operand& o, int64_t nb) { return (size_t)((o.stride ? (nb - 1) * o.stride : 0) + o.item) * o.es; }

// One device's contiguous block [lo, hi) of the batch: chunked, double-buffered.
int run_block(nd4hip_handle* h, int dev, int64_t lo, int64_t hi, const std::vector<Operand>& ops, const ChunkFn& fn, const Plan& plan) {
  Nd4DeviceGuard guard(h);
  const int64_t n = hi - lo;
  if (n <= 0) return 0;
  const size_t nops = ops.size();
  size_t per_item = 0;
  for (const auto& o : ops) if (o.stride) per_item += (size_t)o.item * o.es;
  int64_t nchunks = (int64_t)((per_item * (size_t)n + plan.chunk_bytes - 1) / plan.chunk_bytes);
  if (nchunks > plan.max_chunks) nchunks = plan.max_chunks;
  if (nchunks > n / plan.min_chunk) nchunks = n / plan.min_chunk;
  if (nchunks < 1) nchunks = 1;
  const int64_t per = (n + nchunks - 1) / nchunks;
  nchunks = (n + per - 1) / per;
  const int nsets = nchunks > 1 ? 2 : 1;

  std::vector<DevBuf> bufs(nops * 2);
  auto buf = [&](size_t i, int set) -> DevBuf& { return bufs[i * 2 + (size_t)(ops[i].stride ? set : 0)]; };
  int rc = 0;
  hipStream_t cs = h->copy_stream ? h->copy_stream : h->stream;       // copies; compute goes to h->stream
  auto fail = [&](int code) {
    // the block's copies / kernels may still be using the staging blocks: drain before the DevBufs go back to the cache
    (void)hipStreamSynchronize(cs); (void)hipStreamSynchronize(h->stream);
    return code;
  };
#define BLK_TRY(expr) do { int _rc = (expr); if (_rc != 0) return fail(_rc); } while (0)
#define BLK_HIP(expr) do { hipError_t _e = (expr); if (_e != hipSuccess) return fail(nd4_hip_fail(_e, #expr, __FILE__, __LINE__)); } while (0)
  for (size_t i = 0; i < nops; i++) {
    const Operand& o = ops[i];
    if (o.stride == 0) {
      BLK_TRY(buf(i, 0).alloc(h, span_bytes(o, 1)));
      if (o.src) BLK_HIP(hipMemcpyAsync(buf(i, 0).p, o.src, span_bytes(o, 1), hipMemcpyHostToDevice, cs));
    } else {
      for (int s = 0; s < nsets; s++) BLK_TRY(buf(i, s).alloc(h, span_bytes(o, per)));
    }
  }
  std::vector<void*> dptr(nops);
  auto upload = [&](int64_t c) -> int {
    const int64_t b0 = lo + c * per, nb = (b0 + per <= hi) ? per : hi - b0;
    const int set = (int)(c & 1) % nsets;
    // the set was last used by chunk c-2: its kernels must be done before the inputs are overwritten
    if (c >= 2) ND4_HIP(hipStreamWaitEvent(cs, h->ev_chunk[set], 0));
    for (size_t i = 0; i < nops; i++) {
      const Operand& o = ops[i];
      if (o.stride && o.src)
        ND4_HIP(hipMemcpyAsync(buf(i, set).p, static_cast<const char*>(o.src) + (size_t)(b0 * o.stride) * o.es, span_bytes(o, nb), hipMemcpyHostToDevice, cs));
    }
    ND4_HIP(hipEventRecord(h->ev_in[set], cs));
    return 0;
  };
  auto compute = [&](int64_t c) -> int {
    const int64_t b0 = lo + c * per, nb = (b0 + per <= hi) ? per : hi - b0;
    const int set = (int)(c & 1) % nsets;
    if (cs != h->stream) ND4_HIP(hipStreamWaitEvent(h->stream, h->ev_in[set], 0));
    for (size_t i = 0; i < nops; i++) dptr[i] = buf(i, set).p;
    g_chunk_first = b0;
    ND4_TRY(fn(h, dev, nb, dptr.data()));
    ND4_HIP(hipEventRecord(h->ev_chunk[set], h->stream));
    return 0;
  };
  auto download = [&](int64_t c) -> int {
    const int64_t b0 = lo + c * per, nb = (b0 + per <= hi) ? per : hi - b0;
    const int set = (int)(c & 1) % nsets;
    if (cs != h->stream) ND4_HIP(hipStreamWaitEvent(cs, h->ev_chunk[set], 0));
    for (size_t i = 0; i < nops; i++) {
      const Operand& o = ops[i];
      if (o.dst)
        ND4_HIP(hipMemcpyAsync(static_cast<char*>(o.dst) + (size_t)(b0 * o.stride) * o.es, buf(i, set).p, span_bytes(o, nb), hipMemcpyDeviceToHost, cs));
    }
    return 0;
  };
  // software pipeline: while chunk c computes, the results of chunk c-1 come down and the inputs of chunk c+1 go up (in this
  // order on the copy stream: an in-place operand of set (c+1)&1 must be read out before it is overwritten)
  rc = upload(0);
  for (int64_t c = 0; c < nchunks && rc == 0; c++) {
    rc = compute(c);
    if (rc == 0 && c >= 1) rc = download(c - 1);
    if (rc == 0 && c + 1 < nchunks) rc = upload(c + 1);
  }
  if (rc == 0) rc = download(nchunks - 1);
  if (rc != 0) return fail(rc);
  BLK_HIP(hipStreamSynchronize(cs));
  BLK_HIP(hipStreamSynchronize(h->stream));
  BLK_TRY(nd4_xchg_check(h, "host-pointer entry point"));
#undef BLK_TRY
#undef BLK_HIP
  return 0;
}

// All devices of the handle: contiguous blocks of the batch (remainder to the low devices), one host thread per extra device.
int run_host(nd4hip_handle* h, int64_t batch, const std::vector<Operand>& ops, const ChunkFn& fn, const Plan& plan = Plan()) {
  if (batch <= 0) return 0;
  const int ndev = 1 + (int)h->peers.size();
  const int used = (int)(batch < ndev ? batch : ndev);
  if (used <= 1) return run_block(h, 0, 0, batch, ops, fn, plan);
  std::vector<int> rcs((size_t)used, 0);
  std::vector<std::string> errs((size_t)used);
  std::vector<std::thread> workers;
  const int64_t per = batch / used, rem = batch % used;
  auto edge = [&](int d) { return (int64_t)d * per + (d < rem ? d : rem); };
  for (int d = 1; d < used; d++) {
    workers.emplace_back([&, d] {
      rcs[(size_t)d] = run_block(h->peers[(size_t)d - 1], d, edge(d), edge(d + 1), ops, fn, plan);
      if (rcs[(size_t)d] != 0) errs[(size_t)d] = nd4hip_last_error();         // the error text is thread-local
    });
  }
  rcs[0] = run_block(h, 0, edge(0), edge(1), ops, fn, plan);
  for (auto& w : workers) w.join();
  for (int d = 0; d < used; d++)
    if (rcs[(size_t)d] != 0) { if (d > 0) nd4_set_error("%s (device %d of the handle)", errs[(size_t)d].c_str(), d); return rcs[(size_t)d]; }
  return 0;
}

inline double* P(void* const* d, int i) { return static_cast<double*>(d[i]); }

}  // namespace

// ------------------------------------------------------------------------------------ lifecycle: several devices behind one handle
extern "C" int nd4hip_create_multi(nd4hip_handle** out, const int* device_ids, int n_dev) {
  ND4_CHECK_ARG(out != nullptr, "nd4hip_create_multi: out is NULL");
  *out = nullptr;
  ND4_CHECK_ARG(n_dev >= 1 && n_dev <= 64 && device_ids != nullptr, "nd4hip_create_multi: need 1..64 device ids");
  // ND4HIP_TEST_ALLOW_DUP_DEVICES=1 (tests only): the same device may be listed several times, so that the per-device host threads,
  // the block partition, the merged SVD audit and the first-error-with-its-device hand-off run on a one-GPU box
  const char* dup = getenv("ND4HIP_TEST_ALLOW_DUP_DEVICES");
  if (!(dup && *dup && *dup != '0'))
    for (int i = 0; i < n_dev; i++)
      for (int j = 0; j < i; j++) ND4_CHECK_ARG(device_ids[i] != device_ids[j], "nd4hip_create_multi: device %d listed twice", device_ids[i]);
  nd4hip_handle* h = nullptr;
  ND4_TRY(nd4hip_create(&h, device_ids[0]));
  for (int i = 1; i < n_dev; i++) {
    nd4hip_handle* p = nullptr;
    const int rc = nd4hip_create(&p, device_ids[i]);
    if (rc != 0) { nd4hip_destroy(h); return rc; }
    h->peers.push_back(p);
  }
  *out = h;
  return 0;
}
extern "C" int nd4hip_device_list(nd4hip_handle* h, int* device_ids, int capacity) {
  ND4_CHECK_ARG(h != nullptr, "nd4hip_device_list: NULL handle");
  const int n = 1 + (int)h->peers.size();
  for (int i = 0; i < n && i < capacity && device_ids; i++) device_ids[i] = i == 0 ? h->device : h->peers[(size_t)i - 1]->device;
  return n;
}
// [lo, hi) of a batch of `batch` members that device `index` of an n_dev-device handle processes (exposed for tests / hosts)
extern "C" int nd4hip_partition(int64_t batch, int n_dev, int index, int64_t* lo, int64_t* hi) {
  ND4_CHECK_ARG(batch >= 0 && n_dev >= 1 && index >= 0 && index < n_dev && lo && hi, "nd4hip_partition: bad argument");
  const int used = (int)(batch < n_dev ? batch : n_dev);
  if (index >= used) { *lo = *hi = batch; return 0; }
  const int64_t per = batch / used, rem = batch % used;
  *lo = (int64_t)index * per + (index < rem ? index : rem);
  *hi = (int64_t)(index + 1) * per + (index + 1 < rem ? index + 1 : rem);
  return 0;
}

// ------------------------------------------------------------------------------------ matmul
extern "C" int nd4hip_dgemm_batched(nd4hip_handle* h, int64_t batch, int64_t I, int64_t K, int64_t J,
                                    const double* A, int64_t strideA, const double* B, int64_t strideB, double* C) {
  ND4_CHECK_ARG(h != nullptr, "nd4hip_dgemm_batched: NULL handle");
  ND4_ARGS(nd4_args_gemm("dgemm_batched", true, batch, I, K, J, A, strideA, B, strideB, C));
  if (batch == 1 && K > 0) {
    // one product: the "batch" of the driver is the rows of A and C (a row of C needs its row of A and all of B), so the
    // upload of the next row block and the download of the previous one overlap the MFMA kernel; one device (replicas only)
    Plan plan; plan.min_chunk = 512;
    std::vector<Operand> ops{in_op(A, K, K), in_op(B, K * J, 0), out_op(C, J)};
    ChunkFn fn = [=](nd4hip_handle* hd, int, int64_t rows, void* const* d) {
      return nd4hip_dgemm_batched_dev(hd, 1, rows, K, J, P(d, 0), 0, P(d, 1), 0, P(d, 2));
    };
    return run_block(h, 0, 0, I, ops, fn, plan);
  }
  std::vector<Operand> ops{in_op(A, I * K, strideA), in_op(B, K * J, strideB), out_op(C, I * J)};
  ChunkFn fn = [=](nd4hip_handle* hd, int, int64_t nb, void* const* d) {
    return nd4hip_dgemm_batched_dev(hd, nb, I, K, J, P(d, 0), nb > 1 ? strideA : 0, P(d, 1), nb > 1 ? strideB : 0, P(d, 2));
  };
  return run_host(h, batch, ops, fn);
}

// complex: the same plans as nd4hip_dgemm_batched, with 16-byte elements for the complex operands
extern "C" int nd4hip_zgemm_batched(nd4hip_handle* h, int a_complex, int b_complex, int64_t batch, int64_t I, int64_t K, int64_t J,
                                    const double* A, int64_t strideA, const double* B, int64_t strideB, double* C) {
  ND4_ARGS(nd4_args_gemm("zgemm_batched", a_complex || b_complex, batch, I, K, J, A, strideA, B, strideB, C));
  ND4_CHECK_ARG(h != nullptr, "nd4hip_zgemm_batched: NULL handle");
  const int ac = a_complex ? 1 : 0, bc = b_complex ? 1 : 0;
  const size_t ea = a_complex ? 2 * D : D, eb = b_complex ? 2 * D : D;
  if (batch == 1 && K > 0) {
    // one product: pipelined over the rows of A and C (B is a broadcast operand), one device (replicas only)
    Plan plan; plan.min_chunk = 512;
    std::vector<Operand> ops{in_op(A, K, K, ea), in_op(B, K * J, 0, eb), out_op(C, J, 2 * D)};
    ChunkFn fn = [=](nd4hip_handle* hd, int, int64_t rows, void* const* d) {
      return nd4hip_zgemm_batched_dev(hd, ac, bc, 1, rows, K, J, P(d, 0), 0, P(d, 1), 0, P(d, 2));
    };
    return run_block(h, 0, 0, I, ops, fn, plan);
  }
  std::vector<Operand> ops{in_op(A, I * K, strideA, ea), in_op(B, K * J, strideB, eb), out_op(C, I * J, 2 * D)};
  ChunkFn fn = [=](nd4hip_handle* hd, int, int64_t nb, void* const* d) {
    return nd4hip_zgemm_batched_dev(hd, ac, bc, nb, I, K, J, P(d, 0), nb > 1 ? strideA : 0, P(d, 1), nb > 1 ? strideB : 0, P(d, 2));
  };
  return run_host(h, batch, ops, fn);
}

// ------------------------------------------------------------------------------------ LU
extern "C" int nd4hip_dgetrf_batched(nd4hip_handle* h, int64_t batch, int64_t N, const double* A, double* LU, int32_t* Pv) {
  ND4_CHECK_ARG(h != nullptr, "nd4hip_dgetrf_batched: NULL handle");
  ND4_ARGS(nd4_args_dense("dgetrf_batched", {batch, N}, {A, LU, Pv}));
  std::vector<Operand> ops{in_op(A, N * N, N * N), out_op(LU, N * N), out_op(Pv, N, 4)};
  ChunkFn fn = [=](nd4hip_handle* hd, int, int64_t nb, void* const* d) {
    return nd4hip_dgetrf_batched_dev(hd, nb, N, P(d, 0), P(d, 1), static_cast<int32_t*>(d[2]));
  };
  return run_host(h, batch, ops, fn);
}

// ------------------------------------------------------------------------------------ solves
extern "C" int nd4hip_dgetrs_batched(nd4hip_handle* h, int64_t batch, int64_t N, int64_t J, const double* LU, int64_t strideLU,
                                     const int32_t* Pv, int64_t strideP, const double* Y, int64_t strideY, double* X) {
  ND4_CHECK_ARG(h != nullptr, "nd4hip_dgetrs_batched: NULL handle");
  ND4_ARGS(nd4_args_solve("dgetrs_batched", batch, N, J, {{LU, strideLU, N * N}, {Pv, strideP, N}, {Y, strideY, N * J}}, X));
  std::vector<Operand> ops{in_op(LU, N * N, strideLU), in_op(Pv, N, strideP, 4), in_op(Y, N * J, strideY), out_op(X, N * J)};
  ChunkFn fn = [=](nd4hip_handle* hd, int, int64_t nb, void* const* d) {
    return nd4hip_dgetrs_batched_dev(hd, nb, N, J, P(d, 0), strideLU, static_cast<const int32_t*>(d[1]), strideP, P(d, 2), strideY, P(d, 3));
  };
  return run_host(h, batch, ops, fn);
}
extern "C" int nd4hip_dtrsm_batched(nd4hip_handle* h, int upper, int unit_diag, int64_t batch, int64_t M, int64_t J,
                                    const double* T, int64_t strideT, const double* Y, int64_t strideY, double* X) {
  ND4_CHECK_ARG(h != nullptr, "nd4hip_dtrsm_batched: NULL handle");
  ND4_ARGS(nd4_args_solve("dtrsm_batched", batch, M, J, {{T, strideT, M * M}, {Y, strideY, M * J}}, X));
  std::vector<Operand> ops{in_op(T, M * M, strideT), in_op(Y, M * J, strideY), out_op(X, M * J)};
  ChunkFn fn = [=](nd4hip_handle* hd, int, int64_t nb, void* const* d) {
    return nd4hip_dtrsm_batched_dev(hd, upper, unit_diag, nb, M, J, P(d, 0), strideT, P(d, 1), strideY, P(d, 2));
  };
  return run_host(h, batch, ops, fn);
}

// ---- least squares from a factorisation: qr_lstsq (qr.js:186-273), svd_lstsq / svd_solve (svd.js:66-228)
extern "C" int nd4hip_dqrls_batched(nd4hip_handle* h, int64_t batch, int64_t N, int64_t M, int64_t I, int64_t J,
                                    const double* Q, int64_t strideQ, const double* R, int64_t strideR,
                                    const double* Y, int64_t strideY, double* X) {
  ND4_CHECK_ARG(h != nullptr, "nd4hip_dqrls_batched: NULL handle");
  ND4_ARGS(nd4_args_factor_ls("dqrls_batched", true, batch, N, M, I, J, {{Q, strideQ, N * M}, {R, strideR, M * I}, {Y, strideY, N * J}}, X));
  if (N == 0 || M == 0) { memset(X, 0, D * (size_t)(batch * I * J)); return 0; }
  std::vector<Operand> ops{in_op(Q, N * M, strideQ), in_op(R, M * I, strideR), in_op(Y, N * J, strideY), out_op(X, I * J)};
  ChunkFn fn = [=](nd4hip_handle* hd, int, int64_t nb, void* const* d) {
    return nd4hip_dqrls_batched_dev(hd, nb, N, M, I, J, P(d, 0), strideQ, P(d, 1), strideR, P(d, 2), strideY, P(d, 3));
  };
  return run_host(h, batch, ops, fn);
}
extern "C" int nd4hip_dsvdls_batched(nd4hip_handle* h, int64_t batch, int64_t N, int64_t M, int64_t I, int64_t J,
                                     const double* U, int64_t strideU, const double* sv, int64_t strideSv,
                                     const double* V, int64_t strideV, const double* Y, int64_t strideY, double* X) {
  ND4_CHECK_ARG(h != nullptr, "nd4hip_dsvdls_batched: NULL handle");
  ND4_ARGS(nd4_args_factor_ls("dsvdls_batched", false, batch, N, M, I, J,
                              {{U, strideU, N * M}, {sv, strideSv, M}, {V, strideV, M * I}, {Y, strideY, N * J}}, X));
  if (N == 0 || M == 0) { memset(X, 0, D * (size_t)(batch * I * J)); return 0; }
  const size_t nS = (size_t)(strideSv ? (batch - 1) * strideSv + M : M);
  for (size_t i = 0; i < nS; i++) ND4_CHECK_ARG(std::isfinite(sv[i]), "svd_solve(): NaN or Infinity encountered.");   // svd.js:171-172
  std::vector<Operand> ops{in_op(U, N * M, strideU), in_op(sv, M, strideSv), in_op(V, M * I, strideV), in_op(Y, N * J, strideY), out_op(X, I * J)};
  ChunkFn fn = [=](nd4hip_handle* hd, int, int64_t nb, void* const* d) {
    return nd4hip_dsvdls_batched_dev(hd, nb, N, M, I, J, P(d, 0), strideU, P(d, 1), strideSv, P(d, 2), strideV, P(d, 3), strideY, P(d, 4));
  };
  return run_host(h, batch, ops, fn);
}

// ---- Cholesky / LDL^T
extern "C" int nd4hip_dpotrf_batched(nd4hip_handle* h, int64_t batch, int64_t N, const double* S, double* L) {
  ND4_CHECK_ARG(h != nullptr, "nd4hip_dpotrf_batched: NULL handle");
  ND4_ARGS(nd4_args_dense("dpotrf_batched", {batch, N}, {S, L}));
  std::vector<Operand> ops{in_op(S, N * N, N * N), out_op(L, N * N)};
  ChunkFn fn = [=](nd4hip_handle* hd, int, int64_t nb, void* const* d) { return nd4hip_dpotrf_batched_dev(hd, nb, N, P(d, 0), P(d, 1)); };
  return run_host(h, batch, ops, fn);
}
extern "C" int nd4hip_dpotrs_batched(nd4hip_handle* h, int64_t batch, int64_t N, int64_t J, const double* L, int64_t strideL,
                                     const double* Y, int64_t strideY, double* X) {
  ND4_CHECK_ARG(h != nullptr, "nd4hip_dpotrs_batched: NULL handle");
  ND4_ARGS(nd4_args_solve("dpotrs_batched", batch, N, J, {{L, strideL, N * N}, {Y, strideY, N * J}}, X));
  std::vector<Operand> ops{in_op(L, N * N, strideL), in_op(Y, N * J, strideY), out_op(X, N * J)};
  ChunkFn fn = [=](nd4hip_handle* hd, int, int64_t nb, void* const* d) {
    return nd4hip_dpotrs_batched_dev(hd, nb, N, J, P(d, 0), strideL, P(d, 1), strideY, P(d, 2));
  };
  return run_host(h, batch, ops, fn);
}
extern "C" int nd4hip_dldltrf_batched(nd4hip_handle* h, int64_t batch, int64_t N, const double* S, double* LD) {
  ND4_CHECK_ARG(h != nullptr, "nd4hip_dldltrf_batched: NULL handle");
  ND4_ARGS(nd4_args_dense("dldltrf_batched", {batch, N}, {S, LD}));
  std::vector<Operand> ops{in_op(S, N * N, N * N), out_op(LD, N * N)};
  ChunkFn fn = [=](nd4hip_handle* hd, int, int64_t nb, void* const* d) { return nd4hip_dldltrf_batched_dev(hd, nb, N, P(d, 0), P(d, 1)); };
  return run_host(h, batch, ops, fn);
}
extern "C" int nd4hip_dldltrs_batched(nd4hip_handle* h, int64_t batch, int64_t N, int64_t J, const double* LD, int64_t strideLD,
                                      const double* Y, int64_t strideY, double* X) {
  ND4_CHECK_ARG(h != nullptr, "nd4hip_dldltrs_batched: NULL handle");
  ND4_ARGS(nd4_args_solve("dldltrs_batched", batch, N, J, {{LD, strideLD, N * N}, {Y, strideY, N * J}}, X));
  std::vector<Operand> ops{in_op(LD, N * N, strideLD), in_op(Y, N * J, strideY), out_op(X, N * J)};
  ChunkFn fn = [=](nd4hip_handle* hd, int, int64_t nb, void* const* d) {
    return nd4hip_dldltrs_batched_dev(hd, nb, N, J, P(d, 0), strideLD, P(d, 1), strideY, P(d, 2));
  };
  return run_host(h, batch, ops, fn);
}

// ---- pivoted LDL^T (pldlp.js)
extern "C" int nd4hip_dsytrf_bk_batched_ex(nd4hip_handle* h, int64_t batch, int64_t N, const double* S, double* LD, int32_t* Pv, int tier) {
  ND4_ARGS(nd4_args_sytrf_bk(batch, N, S, LD, Pv, tier));
  ND4_CHECK_ARG(h != nullptr, "nd4hip_dsytrf_bk_batched: NULL handle");
  // AUTO is decided once, by the whole batch: the chunks and devices below must not each choose their own tier
  const int t = nd4_sytrf_bk_tier(h, batch, N, tier);
  std::vector<Operand> ops{in_op(S, N * N, N * N), out_op(LD, N * N), out_op(Pv, N, 4)};
  // a singular member does not stop the others: every chunk runs and comes back, the lowest singular member is reported at the end
  std::atomic<int64_t> worst(INT64_MAX);
  ChunkFn fn = [=, &worst](nd4hip_handle* hd, int, int64_t nb, void* const* d) {
    int64_t bad = INT64_MAX;
    const int rc = nd4_sytrf_bk_run(hd, nb, N, P(d, 0), P(d, 1), static_cast<int32_t*>(d[2]), t, g_chunk_first, &bad);
    if (rc != ND4HIP_ERR_SINGULAR) return rc;
    for (int64_t seen = worst.load(); bad < seen && !worst.compare_exchange_weak(seen, bad);) {}
    return 0;
  };
  ND4_TRY(run_host(h, batch, ops, fn));
  if (worst.load() != INT64_MAX) {
    nd4_set_error("_pldlp_decomp(M,N, LD,LD_off, P,P_off): Zero column or NaN encountered. (matrix %lld)", (long long)worst.load());
    return ND4HIP_ERR_SINGULAR;
  }
  return 0;
}
extern "C" int nd4hip_dsytrf_bk_batched(nd4hip_handle* h, int64_t batch, int64_t N, const double* S, double* LD, int32_t* Pv) {
  return nd4hip_dsytrf_bk_batched_ex(h, batch, N, S, LD, Pv, ND4HIP_PLDLP_TIER_AUTO);
}
extern "C" int nd4hip_dsytrs_bk_batched(nd4hip_handle* h, int64_t batch, int64_t N, int64_t J, const double* LD, int64_t strideLD,
                                        const int32_t* Pv, int64_t strideP, const double* Y, int64_t strideY, double* X) {
  ND4_ARGS(nd4_args_solve("dsytrs_bk_batched", batch, N, J, {{LD, strideLD, N * N}, {Pv, strideP, N}, {Y, strideY, N * J}}, X));
  {  // pldlp_p's checks (pldlp.js:408-435), before any device work
    std::vector<char> seen((size_t)N);
    for (int64_t b = 0; b < (strideP ? batch : 1); b++) {
      const int32_t* p = Pv + b * strideP;
      std::fill(seen.begin(), seen.end(), 0);
      for (int64_t i = N; i-- > 0;) {
        int64_t q = p[i];
        if (q < 0) {
          ND4_CHECK_ARG(i > 0 && p[i - 1] >= 0, "pldlp_solve(LD,P,y): P is invalid.");
          q = ~q;
        }
        ND4_CHECK_ARG(q >= 0 && q < N, "pldlp_solve(LD,P,y): P contains out-of-bounds indices.");
        ND4_CHECK_ARG(!seen[(size_t)q], "pldlp_solve(LD,P,y): P contains duplicate indices.");
        seen[(size_t)q] = 1;
      }
    }
  }
  ND4_CHECK_ARG(h != nullptr, "nd4hip_dsytrs_bk_batched: NULL handle");
  std::vector<Operand> ops{in_op(LD, N * N, strideLD), in_op(Pv, N, strideP, 4), in_op(Y, N * J, strideY), out_op(X, N * J)};
  ChunkFn fn = [=](nd4hip_handle* hd, int, int64_t nb, void* const* d) {
    return nd4hip_dsytrs_bk_batched_dev(hd, nb, N, J, P(d, 0), strideLD, static_cast<const int32_t*>(d[1]), strideP, P(d, 2), strideY, P(d, 3));
  };
  return run_host(h, batch, ops, fn);
}

// ---- structure functions (tri.js:23-42, diag.js:23-88, permute.js:23-306): pure data movement, sharded like every batched call
extern "C" int nd4hip_dtranspose_batched(nd4hip_handle* h, int64_t batch, int64_t M, int64_t N, const double* A, double* B) {
  ND4_CHECK_ARG(h != nullptr, "nd4hip_dtranspose_batched: NULL handle");
  ND4_ARGS(nd4_args_dense("dtranspose_batched", {batch, M, N}, {A, B}));
  ND4_CHECK_ARG(!nd4_struct_overlap(A, batch * M * N, B, batch * M * N), "nd4hip_dtranspose_batched: B must not overlap A");
  std::vector<Operand> ops{in_op(A, M * N, M * N), out_op(B, M * N)};
  ChunkFn fn = [=](nd4hip_handle* hd, int, int64_t nb, void* const* d) { return nd4hip_dtranspose_batched_dev(hd, nb, M, N, P(d, 0), P(d, 1)); };
  return run_host(h, batch, ops, fn);
}
extern "C" int nd4hip_dtri_batched(nd4hip_handle* h, int upper, int64_t k, int64_t batch, int64_t M, int64_t N, const double* A, double* B) {
  ND4_CHECK_ARG(h != nullptr, "nd4hip_dtri_batched: NULL handle");
  ND4_ARGS(nd4_args_dense("dtri_batched", {batch, M, N}, {A, B}));
  ND4_CHECK_ARG(!nd4_struct_overlap(A, batch * M * N, B, batch * M * N), "nd4hip_dtri_batched: B must not overlap A");
  std::vector<Operand> ops{in_op(A, M * N, M * N), out_op(B, M * N)};
  ChunkFn fn = [=](nd4hip_handle* hd, int, int64_t nb, void* const* d) { return nd4hip_dtri_batched_dev(hd, upper, k, nb, M, N, P(d, 0), P(d, 1)); };
  return run_host(h, batch, ops, fn);
}
extern "C" int nd4hip_ddiag_batched(nd4hip_handle* h, int64_t batch, int64_t M, int64_t N, int64_t offset, const double* A, double* dg) {
  ND4_CHECK_ARG(h != nullptr, "nd4hip_ddiag_batched: NULL handle");
  ND4_ARGS(nd4_args_diag(batch, M, N, offset, A, dg));
  const int64_t L = nd4_diag_length(M, N, offset);
  ND4_CHECK_ARG(!nd4_struct_overlap(A, batch * M * N, dg, batch * L), "nd4hip_ddiag_batched: d must not overlap A");
  std::vector<Operand> ops{in_op(A, M * N, M * N), out_op(dg, L)};
  ChunkFn fn = [=](nd4hip_handle* hd, int, int64_t nb, void* const* d) { return nd4hip_ddiag_batched_dev(hd, nb, M, N, offset, P(d, 0), P(d, 1)); };
  return run_host(h, batch, ops, fn);
}
extern "C" int nd4hip_ddiagmat_batched(nd4hip_handle* h, int64_t batch, int64_t N, const double* dg, double* Dm) {
  ND4_CHECK_ARG(h != nullptr, "nd4hip_ddiagmat_batched: NULL handle");
  ND4_ARGS(nd4_args_dense("ddiagmat_batched", {batch, N}, {dg, Dm}));
  ND4_CHECK_ARG(!nd4_struct_overlap(dg, batch * N, Dm, batch * N * N), "nd4hip_ddiagmat_batched: D must not overlap d");
  std::vector<Operand> ops{in_op(dg, N, N), out_op(Dm, N * N)};
  ChunkFn fn = [=](nd4hip_handle* hd, int, int64_t nb, void* const* d) { return nd4hip_ddiagmat_batched_dev(hd, nb, N, P(d, 0), P(d, 1)); };
  return run_host(h, batch, ops, fn);
}
extern "C" int nd4hip_dpermute_batched(nd4hip_handle* h, int cols, int inverse, int64_t batch, int64_t M, int64_t N, const double* A,
                                       int64_t strideA, const int32_t* Pv, int64_t strideP, double* B) {
  ND4_CHECK_ARG(h != nullptr, "nd4hip_dpermute_batched: NULL handle");
  ND4_ARGS(nd4_args_permute(cols, batch, M, N, A, strideA, Pv, strideP, B));
  const int64_t L = cols ? N : M;
  ND4_CHECK_ARG(!nd4_struct_overlap(A, (strideA ? (batch - 1) * strideA : 0) + M * N, B, batch * M * N),
                "nd4hip_dpermute_batched: B must not overlap A");
  // the indices are checked on the device, where they are used: a bad one fails its chunk with the reference's text
  std::vector<Operand> ops{in_op(A, M * N, strideA), in_op(Pv, L, strideP, 4), out_op(B, M * N)};
  ChunkFn fn = [=](nd4hip_handle* hd, int, int64_t nb, void* const* d) {
    return nd4hip_dpermute_batched_dev(hd, cols, inverse, nb, M, N, P(d, 0), strideA, static_cast<const int32_t*>(d[1]), strideP, P(d, 2));
  };
  return run_host(h, batch, ops, fn);
}

// ---- bidiag_decomp (bidiag.js:245-319), hessenberg_decomp (hessenberg.js:89-115)
extern "C" int nd4hip_dgebrd_batched(nd4hip_handle* h, int64_t batch, int64_t M, int64_t N, const double* A, double* U, double* B, double* V) {
  ND4_CHECK_ARG(h != nullptr, "nd4hip_dgebrd_batched: NULL handle");
  ND4_ARGS(nd4_args_dense("dgebrd_batched", {batch, M, N}, {A, U, B, V}));
  const int64_t K = M < N ? M : N, J = M >= N ? K : K + 1;
  std::vector<Operand> ops{in_op(A, M * N, M * N), out_op(U, M * K), out_op(B, K * J), out_op(V, J * N)};
  ChunkFn fn = [=](nd4hip_handle* hd, int, int64_t nb, void* const* d) { return nd4hip_dgebrd_batched_dev(hd, nb, M, N, P(d, 0), P(d, 1), P(d, 2), P(d, 3)); };
  return run_host(h, batch, ops, fn);
}
extern "C" int nd4hip_dgehrd_batched(nd4hip_handle* h, int64_t batch, int64_t N, const double* A, double* U, double* H) {
  ND4_CHECK_ARG(h != nullptr, "nd4hip_dgehrd_batched: NULL handle");
  ND4_ARGS(nd4_args_dense("dgehrd_batched", {batch, N}, {A, U, H}));
  std::vector<Operand> ops{in_op(A, N * N, N * N), out_op(U, N * N), out_op(H, N * N)};
  ChunkFn fn = [=](nd4hip_handle* hd, int, int64_t nb, void* const* d) { return nd4hip_dgehrd_batched_dev(hd, nb, N, P(d, 0), P(d, 1), P(d, 2)); };
  return run_host(h, batch, ops, fn);
}

// ------------------------------------------------------------------------------------ QR
extern "C" int nd4hip_dgeqrf_q_batched(nd4hip_handle* h, int64_t batch, int64_t M, int64_t N, const double* A, double* Q, double* R) {
  ND4_CHECK_ARG(h != nullptr, "nd4hip_dgeqrf_q_batched: NULL handle");
  ND4_ARGS(nd4_args_dense("dgeqrf_q_batched", {batch, M, N}, {A, Q, R}));
  const int64_t L = M < N ? M : N;
  std::vector<Operand> ops{in_op(A, M * N, M * N), out_op(Q, M * L), out_op(R, L * N)};
  ChunkFn fn = [=](nd4hip_handle* hd, int, int64_t nb, void* const* d) { return nd4hip_dgeqrf_q_batched_dev(hd, nb, M, N, P(d, 0), P(d, 1), P(d, 2)); };
  return run_host(h, batch, ops, fn);
}
extern "C" int nd4hip_dgeqrf_full_batched(nd4hip_handle* h, int64_t batch, int64_t M, int64_t N, const double* A, double* Q, double* R) {
  ND4_CHECK_ARG(h != nullptr, "nd4hip_dgeqrf_full_batched: NULL handle");
  ND4_ARGS(nd4_args_dense("dgeqrf_full_batched", {batch, M, N}, {A, Q, R}));
  std::vector<Operand> ops{in_op(A, M * N, M * N), out_op(Q, M * M), out_op(R, M * N)};
  ChunkFn fn = [=](nd4hip_handle* hd, int, int64_t nb, void* const* d) { return nd4hip_dgeqrf_full_batched_dev(hd, nb, M, N, P(d, 0), P(d, 1), P(d, 2)); };
  return run_host(h, batch, ops, fn);
}
extern "C" int nd4hip_dgeqrf_qty_batched(nd4hip_handle* h, int64_t batch, int64_t M, int64_t N, int64_t L, double* A, double* Y) {
  ND4_CHECK_ARG(h != nullptr, "nd4hip_dgeqrf_qty_batched: NULL handle");
  ND4_ARGS(nd4_args_geqrf_qty(batch, M, N, L, A, Y));
  std::vector<Operand> ops{inout_op(A, M * N)};
  if (L > 0) ops.push_back(inout_op(Y, M * L));
  ChunkFn fn = [=](nd4hip_handle* hd, int, int64_t nb, void* const* d) {
    return nd4hip_dgeqrf_qty_batched_dev(hd, nb, M, N, L, P(d, 0), L > 0 ? P(d, 1) : nullptr);
  };
  return run_host(h, batch, ops, fn);
}

// ------------------------------------------------------------------------------------ column-pivoted QR
extern "C" int nd4hip_dgeqp3_batched(nd4hip_handle* h, int64_t batch, int64_t M, int64_t N, const double* A, double* Q, double* R, int32_t* Pv) {
  ND4_CHECK_ARG(h != nullptr, "nd4hip_dgeqp3_batched: NULL handle");
  ND4_ARGS(nd4_args_dense("dgeqp3_batched", {batch, M, N}, {A, Q, R, Pv}));
  const int64_t L = M < N ? M : N;
  std::vector<Operand> ops{in_op(A, M * N, M * N), out_op(Q, M * L), out_op(R, L * N), out_op(Pv, N, 4)};
  ChunkFn fn = [=](nd4hip_handle* hd, int, int64_t nb, void* const* d) {
    return nd4hip_dgeqp3_batched_dev(hd, nb, M, N, P(d, 0), P(d, 1), P(d, 2), static_cast<int32_t*>(d[3]));
  };
  return run_host(h, batch, ops, fn);
}
extern "C" int nd4hip_dgeqp3_full_batched(nd4hip_handle* h, int64_t batch, int64_t M, int64_t N, const double* A, double* Q, double* R, int32_t* Pv) {
  ND4_CHECK_ARG(h != nullptr, "nd4hip_dgeqp3_full_batched: NULL handle");
  ND4_ARGS(nd4_args_dense("dgeqp3_full_batched", {batch, M, N}, {A, Q, R, Pv}));
  std::vector<Operand> ops{in_op(A, M * N, M * N), out_op(Q, M * M), out_op(R, M * N), out_op(Pv, N, 4)};
  ChunkFn fn = [=](nd4hip_handle* hd, int, int64_t nb, void* const* d) {
    return nd4hip_dgeqp3_full_batched_dev(hd, nb, M, N, P(d, 0), P(d, 1), P(d, 2), static_cast<int32_t*>(d[3]));
  };
  return run_host(h, batch, ops, fn);
}

namespace {
// _rrqr_rank throws on a non-finite partial norm (rrqr.js:78-79); the kernels mark such a matrix with rank -1
int qp3_rank_verdict(const int32_t* rank, int64_t batch) {
  for (int64_t b = 0; b < batch; b++)
    ND4_CHECK_ARG(rank[b] >= 0, "Infinity or NaN encountered during rank estimation.");
  return 0;
}
}  // namespace

extern "C" int nd4hip_dqp3rank_batched(nd4hip_handle* h, int64_t batch, int64_t M, int64_t N, const double* R, int32_t* rank) {
  ND4_CHECK_ARG(h != nullptr, "nd4hip_dqp3rank_batched: NULL handle");
  ND4_ARGS(nd4_args_qp3rank(batch, M, N, R, rank));
  if (M == 0 || N == 0) { memset(rank, 0, sizeof(int32_t) * (size_t)batch); return 0; }
  std::vector<Operand> ops{in_op(R, M * N, M * N), out_op(rank, 1, 4)};
  ChunkFn fn = [=](nd4hip_handle* hd, int, int64_t nb, void* const* d) {
    return nd4hip_dqp3rank_batched_dev(hd, nb, M, N, P(d, 0), static_cast<int32_t*>(d[1]));
  };
  ND4_TRY(run_host(h, batch, ops, fn));
  return qp3_rank_verdict(rank, batch);
}

extern "C" int nd4hip_dqp3ls_batched(nd4hip_handle* h, int64_t batch, int64_t N, int64_t M, int64_t I, int64_t J,
                                     const double* Q, int64_t strideQ, const double* R, int64_t strideR, const int32_t* Pv, int64_t strideP,
                                     const double* Y, int64_t strideY, double* X, int32_t* rank) {
  ND4_CHECK_ARG(h != nullptr, "nd4hip_dqp3ls_batched: NULL handle");
  ND4_ARGS(nd4_args_qp3ls(batch, N, M, I, J, Q, strideQ, R, strideR, Pv, strideP, Y, strideY, X));
  // the rank-only shape (I = 0 or J = 0) is staged like every other, so this form needs its four inputs there too
  ND4_CHECK_ARG(Q && R && Pv && Y, "nd4hip_dqp3ls_batched: NULL pointer");
  // the reference's un-permutation refuses indices that do not form a permutation (rrqr.js:560-563)
  {
    std::vector<char> seen((size_t)I);
    for (int64_t b = 0; b < (strideP ? batch : 1); b++) {
      std::fill(seen.begin(), seen.end(), 0);
      for (int64_t i = 0; i < I; i++) {
        const int32_t k = Pv[b * strideP + i];
        ND4_CHECK_ARG(k >= 0 && k < I && !seen[(size_t)k], "rrqr_lstsq(Q,R,P,y): Invalid indices in P.");
        seen[(size_t)k] = 1;
      }
    }
  }
  std::vector<int32_t> own;
  if (!rank) { own.resize((size_t)batch); rank = own.data(); }
  std::vector<Operand> ops{in_op(Q, N * M, strideQ), in_op(R, M * I, strideR), in_op(Pv, I, strideP, 4), in_op(Y, N * J, strideY),
                           out_op(X, I * J), out_op(rank, 1, 4)};
  ChunkFn fn = [=](nd4hip_handle* hd, int, int64_t nb, void* const* d) {
    return nd4hip_dqp3ls_batched_dev(hd, nb, N, M, I, J, P(d, 0), strideQ, P(d, 1), strideR, static_cast<const int32_t*>(d[2]), strideP,
                                     P(d, 3), strideY, P(d, 4), static_cast<int32_t*>(d[5]));
  };
  ND4_TRY(run_host(h, batch, ops, fn));
  return qp3_rank_verdict(rank, batch);
}

// ------------------------------------------------------------------------------------ strong rank-revealing QR
namespace {
// the decision kernel marks a non-finite scale (srrqr.js:592-593 throws 'Assertion failed: ' + SCALE) and the swap cap
int srrqr_rank_verdict(const int32_t* rank, int64_t batch) {
  for (int64_t b = 0; b < batch; b++) {
    ND4_CHECK_ARG(rank[b] != -1, "Assertion failed: Infinity");
    ND4_CHECK_ARG(rank[b] != -3, "Assertion failed: NaN");
    if (rank[b] < 0) { nd4_set_error("srrqr_decomp_full(A,opt): the swap limit was reached."); return ND4HIP_ERR_NOCONV; }
  }
  return 0;
}
}  // namespace

extern "C" int nd4hip_dsrrqr_batched(nd4hip_handle* h, int64_t batch, int64_t M, int64_t N, const double* A, double dtol, double ztol,
                                     double* Q, double* R, int32_t* Pv, int32_t* rank) {
  ND4_CHECK_ARG(h != nullptr, "nd4hip_dsrrqr_batched: NULL handle");
  ND4_ARGS(nd4_args_srrqr(batch, M, N, A, dtol, ztol, Q, R, Pv, rank));
  if (M == 0 || N == 0) {                                    // nothing to decide: P = identity, rank 0, Q = I
    for (int64_t b = 0; b < batch; b++) {
      rank[b] = 0;
      for (int64_t j = 0; j < N; j++) Pv[b * N + j] = (int32_t)j;
      for (int64_t i = 0; i < M * M; i++) Q[b * M * M + i] = (i % (M + 1) == 0) ? 1.0 : 0.0;
    }
    return 0;
  }
  std::vector<Operand> ops{in_op(A, M * N, M * N), out_op(Q, M * M), out_op(R, M * N), out_op(Pv, N, 4), out_op(rank, 1, 4)};
  ChunkFn fn = [=](nd4hip_handle* hd, int, int64_t nb, void* const* d) {
    return nd4hip_dsrrqr_batched_dev(hd, nb, M, N, P(d, 0), dtol, ztol, P(d, 1), P(d, 2), static_cast<int32_t*>(d[3]),
                                     static_cast<int32_t*>(d[4]));
  };
  ND4_TRY(run_host(h, batch, ops, fn));
  return srrqr_rank_verdict(rank, batch);
}

// ------------------------------------------------------------------------------------ URV
extern "C" int nd4hip_durv_batched(nd4hip_handle* h, int64_t batch, int64_t M, int64_t N, const double* A, double* U, double* R, double* V,
                                   int32_t* rank) {
  ND4_CHECK_ARG(h != nullptr, "nd4hip_durv_batched: NULL handle");
  ND4_ARGS(nd4_args_urv(batch, M, N, A, U, R, V, rank));
  if (M == 0 || N == 0) {                                    // rank 0, U = I, V = I
    for (int64_t b = 0; b < batch; b++) {
      rank[b] = 0;
      for (int64_t i = 0; i < M * M; i++) U[b * M * M + i] = (i % (M + 1) == 0) ? 1.0 : 0.0;
      for (int64_t i = 0; i < N * N; i++) V[b * N * N + i] = (i % (N + 1) == 0) ? 1.0 : 0.0;
    }
    return 0;
  }
  std::vector<Operand> ops{in_op(A, M * N, M * N), out_op(U, M * M), out_op(R, M * N), out_op(V, N * N), out_op(rank, 1, 4)};
  ChunkFn fn = [=](nd4hip_handle* hd, int, int64_t nb, void* const* d) {
    return nd4hip_durv_batched_dev(hd, nb, M, N, P(d, 0), P(d, 1), P(d, 2), P(d, 3), static_cast<int32_t*>(d[4]));
  };
  ND4_TRY(run_host(h, batch, ops, fn));
  return srrqr_rank_verdict(rank, batch);
}

extern "C" int nd4hip_durvls_batched(nd4hip_handle* h, int64_t batch, int64_t I, int64_t J, int64_t K, int64_t L, int64_t Jc,
                                     const double* U, int64_t strideU, const double* R, int64_t strideR, const double* V, int64_t strideV,
                                     const int32_t* rank, int64_t strideRank, const double* Y, int64_t strideY, double* X) {
  ND4_CHECK_ARG(h != nullptr, "nd4hip_durvls_batched: NULL handle");
  ND4_ARGS(nd4_args_urvls(batch, I, J, K, L, Jc, U, strideU, R, strideR, V, strideV, rank, strideRank, Y, strideY, X));
  std::vector<Operand> ops{in_op(U, I * J, strideU), in_op(R, J * K, strideR), in_op(V, K * L, strideV), in_op(rank, 1, strideRank, 4),
                           in_op(Y, I * Jc, strideY), out_op(X, L * Jc)};
  ChunkFn fn = [=](nd4hip_handle* hd, int, int64_t nb, void* const* d) {
    return nd4hip_durvls_batched_dev(hd, nb, I, J, K, L, Jc, P(d, 0), strideU, P(d, 1), strideR, P(d, 2), strideV,
                                     static_cast<const int32_t*>(d[3]), strideRank, P(d, 4), strideY, P(d, 5));
  };
  return run_host(h, batch, ops, fn);
}

// ------------------------------------------------------------------------------------ det, slogdet, det_tri, slogdet_tri, norm
namespace {
// the Givens tiers mark a matrix where the reference's _giv_rot_qr asserts (_giv_rot.js:34: 'Assertion failed: ' + NaN)
int det_verdict(const double* D, int64_t batch) {
  for (int64_t b = 0; b < batch; b++) {
    uint64_t bits;
    std::memcpy(&bits, D + b, sizeof bits);
    ND4_CHECK_ARG(bits != (uint64_t)ND4HIP_DET_ASSERT_NAN_BITS, "Assertion failed: NaN");
  }
  return 0;
}
}  // namespace

extern "C" int nd4hip_ddet_batched(nd4hip_handle* h, int64_t batch, int64_t M, int64_t N, const double* A, double* det) {
  ND4_CHECK_ARG(h != nullptr, "nd4hip_ddet_batched: NULL handle");
  ND4_ARGS(nd4_args_det("ddet_batched", false, batch, M, N, A, det, nullptr));
  std::vector<Operand> ops{in_op(A, M * N, M * N), out_op(det, 1)};
  ChunkFn fn = [=](nd4hip_handle* hd, int, int64_t nb, void* const* d) { return nd4hip_ddet_batched_dev(hd, nb, M, N, P(d, 0), P(d, 1)); };
  ND4_TRY(run_host(h, batch, ops, fn));
  return det_verdict(det, batch);
}

extern "C" int nd4hip_dslogdet_batched(nd4hip_handle* h, int64_t batch, int64_t M, int64_t N, const double* A, double* sign, double* logdet) {
  ND4_CHECK_ARG(h != nullptr, "nd4hip_dslogdet_batched: NULL handle");
  ND4_ARGS(nd4_args_det("dslogdet_batched", true, batch, M, N, A, sign, logdet));
  std::vector<Operand> ops{in_op(A, M * N, M * N), out_op(sign, 1), out_op(logdet, 1)};
  ChunkFn fn = [=](nd4hip_handle* hd, int, int64_t nb, void* const* d) {
    return nd4hip_dslogdet_batched_dev(hd, nb, M, N, P(d, 0), P(d, 1), P(d, 2));
  };
  ND4_TRY(run_host(h, batch, ops, fn));
  return det_verdict(sign, batch);
}

extern "C" int nd4hip_ddettri_batched(nd4hip_handle* h, int64_t batch, int64_t N, const double* A, double* det) {
  ND4_CHECK_ARG(h != nullptr, "nd4hip_ddettri_batched: NULL handle");
  ND4_ARGS(nd4_args_det("ddettri_batched", false, batch, N, N, A, det, nullptr));
  std::vector<Operand> ops{in_op(A, N * N, N * N), out_op(det, 1)};
  ChunkFn fn = [=](nd4hip_handle* hd, int, int64_t nb, void* const* d) { return nd4hip_ddettri_batched_dev(hd, nb, N, P(d, 0), P(d, 1)); };
  return run_host(h, batch, ops, fn);
}

extern "C" int nd4hip_dslogdettri_batched(nd4hip_handle* h, int64_t batch, int64_t N, const double* A, double* sign, double* logdet) {
  ND4_CHECK_ARG(h != nullptr, "nd4hip_dslogdettri_batched: NULL handle");
  ND4_ARGS(nd4_args_det("dslogdettri_batched", true, batch, N, N, A, sign, logdet));
  std::vector<Operand> ops{in_op(A, N * N, N * N), out_op(sign, 1), out_op(logdet, 1)};
  ChunkFn fn = [=](nd4hip_handle* hd, int, int64_t nb, void* const* d) {
    return nd4hip_dslogdettri_batched_dev(hd, nb, N, P(d, 0), P(d, 1), P(d, 2));
  };
  return run_host(h, batch, ops, fn);
}

extern "C" int nd4hip_dnrmfro(nd4hip_handle* h, int64_t n, const double* A, double* out) {
  ND4_CHECK_ARG(h != nullptr, "nd4hip_dnrmfro: NULL handle");
  ND4_ARGS(nd4_args_nrmfro(n, A, out));
  if (n == 0) { *out = 0.0; return 0; }
  std::vector<Operand> ops{in_op(A, n, n), out_op(out, 1)};     // one "matrix" of n elements
  ChunkFn fn = [=](nd4hip_handle* hd, int, int64_t, void* const* d) { return nd4hip_dnrmfro_dev(hd, n, P(d, 0), P(d, 1)); };
  return run_host(h, 1, ops, fn);
}

// ------------------------------------------------------------------------------------ schur_eigenvals, schur_eigen, eigen_balance_pre / _post
// the _dev forms read the device flags back and return the reference's message; run_host hands the first failing chunk's code on
extern "C" int nd4hip_dtreval_batched(nd4hip_handle* h, int64_t batch, int64_t N, const double* T, double* Lam) {
  ND4_CHECK_ARG(h != nullptr, "nd4hip_dtreval_batched: NULL handle");
  ND4_ARGS(nd4_args_ev("dtreval_batched", EV_MAX_N, batch, N, {T, Lam}));
  std::vector<Operand> ops{in_op(T, N * N, N * N), out_op(Lam, 2 * N)};
  ChunkFn fn = [=](nd4hip_handle* hd, int, int64_t nb, void* const* d) { return nd4hip_dtreval_batched_dev(hd, nb, N, P(d, 0), P(d, 1)); };
  return run_host(h, batch, ops, fn);
}

extern "C" int nd4hip_dtrevc_batched(nd4hip_handle* h, int64_t batch, int64_t N, const double* Q, const double* T, double* Lam, double* V) {
  ND4_CHECK_ARG(h != nullptr, "nd4hip_dtrevc_batched: NULL handle");
  ND4_ARGS(nd4_args_ev("dtrevc_batched", EV_MAX_N, batch, N, {Q, T, Lam, V}));
  std::vector<Operand> ops{in_op(Q, N * N, N * N), in_op(T, N * N, N * N), out_op(Lam, 2 * N), out_op(V, 2 * N * N)};
  ChunkFn fn = [=](nd4hip_handle* hd, int, int64_t nb, void* const* d) {
    return nd4hip_dtrevc_batched_dev(hd, nb, N, P(d, 0), P(d, 1), P(d, 2), P(d, 3));
  };
  return run_host(h, batch, ops, fn);
}

extern "C" int nd4hip_dgebal_batched(nd4hip_handle* h, int64_t batch, int64_t N, double p, const double* A, double* D, double* B) {
  ND4_CHECK_ARG(h != nullptr, "nd4hip_dgebal_batched: NULL handle");
  ND4_ARGS(nd4_args_gebal(batch, N, p, A, D, B));
  std::vector<Operand> ops{in_op(A, N * N, N * N), out_op(D, N), out_op(B, N * N)};
  ChunkFn fn = [=](nd4hip_handle* hd, int, int64_t nb, void* const* d) { return nd4hip_dgebal_batched_dev(hd, nb, N, p, P(d, 0), P(d, 1), P(d, 2)); };
  return run_host(h, batch, ops, fn);
}

extern "C" int nd4hip_zgebak_batched(nd4hip_handle* h, int64_t batch, int64_t N, const double* Dv, const double* V, double* W) {
  ND4_CHECK_ARG(h != nullptr, "nd4hip_zgebak_batched: NULL handle");
  ND4_ARGS(nd4_args_gebak(false, batch, N, Dv, V, W));
  std::vector<Operand> ops{in_op(Dv, N, N), in_op(V, 2 * N * N, 2 * N * N), out_op(W, 2 * N * N)};
  ChunkFn fn = [=](nd4hip_handle* hd, int, int64_t nb, void* const* d) { return nd4hip_zgebak_batched_dev(hd, nb, N, P(d, 0), P(d, 1), P(d, 2)); };
  return run_host(h, batch, ops, fn);
}

// ------------------------------------------------------------------------------------ schur_decomp, eigen, eigenvals
namespace {
// the largest of the devices' sweep counts (each device's host thread writes its own slot)
struct SweepMax {
  std::vector<int> per;
  explicit SweepMax(nd4hip_handle* h) : per(1 + h->peers.size(), 0) {}
  void note(int dev, int sw) { if (sw > per[(size_t)dev]) per[(size_t)dev] = sw; }
  int max() const { int m = 0; for (int x : per) if (x > m) m = x; return m; }
};
}  // namespace

extern "C" int nd4hip_dhseqr_batched_ex(nd4hip_handle* h, int64_t batch, int64_t N, const double* U, const double* H, double* Q, double* T,
                                        int* sweeps_out, int tier) {
  ND4_CHECK_ARG(h != nullptr, "nd4hip_dhseqr_batched: NULL handle");
  if (sweeps_out) *sweeps_out = 0;
  ND4_ARGS(nd4_args_hseqr(batch, N, U, H, Q, T, tier));
  SweepMax sweeps(h);
  std::vector<Operand> ops{in_op(U, N * N, N * N), in_op(H, N * N, N * N), out_op(Q, N * N), out_op(T, N * N)};
  ChunkFn fn = [&, N, tier](nd4hip_handle* hd, int dev, int64_t nb, void* const* d) {
    int sw = 0;
    const int rc = nd4hip_dhseqr_batched_ex_dev(hd, nb, N, P(d, 0), P(d, 1), P(d, 2), P(d, 3), &sw, tier);
    sweeps.note(dev, sw);
    return rc;
  };
  const int rc = run_host(h, batch, ops, fn);
  if (sweeps_out) *sweeps_out = sweeps.max();
  return rc;
}
extern "C" int nd4hip_dhseqr_batched(nd4hip_handle* h, int64_t batch, int64_t N, const double* U, const double* H, double* Q, double* T,
                                     int* sweeps_out) {
  return nd4hip_dhseqr_batched_ex(h, batch, N, U, H, Q, T, sweeps_out, ND4HIP_SCHUR_TIER_AUTO);
}

extern "C" int nd4hip_dgees_batched(nd4hip_handle* h, int64_t batch, int64_t N, const double* A, double* Q, double* T, int* sweeps_out) {
  ND4_CHECK_ARG(h != nullptr, "nd4hip_dgees_batched: NULL handle");
  if (sweeps_out) *sweeps_out = 0;
  ND4_ARGS(nd4_args_ev("dgees_batched", INT64_MAX, batch, N, {A, Q, T}));
  SweepMax sweeps(h);
  std::vector<Operand> ops{in_op(A, N * N, N * N), out_op(Q, N * N), out_op(T, N * N)};
  ChunkFn fn = [&, N](nd4hip_handle* hd, int dev, int64_t nb, void* const* d) {
    int sw = 0;
    const int rc = nd4hip_dgees_batched_dev(hd, nb, N, P(d, 0), P(d, 1), P(d, 2), &sw);
    sweeps.note(dev, sw);
    return rc;
  };
  const int rc = run_host(h, batch, ops, fn);
  if (sweeps_out) *sweeps_out = sweeps.max();
  return rc;
}

extern "C" int nd4hip_dgeev_batched(nd4hip_handle* h, int64_t batch, int64_t N, const double* A, double* Lam, double* V) {
  ND4_CHECK_ARG(h != nullptr, "nd4hip_dgeev_batched: NULL handle");
  ND4_ARGS(nd4_args_ev("dgeev_batched", INT64_MAX, batch, N, {A, Lam}));
  std::vector<Operand> ops{in_op(A, N * N, N * N), out_op(Lam, 2 * N)};
  if (V) ops.push_back(out_op(V, 2 * N * N));
  const bool vecs = V != nullptr;
  ChunkFn fn = [=](nd4hip_handle* hd, int, int64_t nb, void* const* d) {
    return nd4hip_dgeev_batched_dev(hd, nb, N, P(d, 0), P(d, 1), vecs ? P(d, 2) : nullptr);
  };
  return run_host(h, batch, ops, fn);
}

// ------------------------------------------------------------------------------------ SVD
extern "C" int nd4hip_dgesvdj_batched(nd4hip_handle* h, int64_t batch, int64_t M, int64_t N, const double* A,
                                      double* U, double* sv, double* V, int* sweeps_out, double* offnorm_out) {
  ND4_CHECK_ARG(h != nullptr, "nd4hip_dgesvdj_batched: NULL handle");
  if (sweeps_out) *sweeps_out = 0;
  if (offnorm_out) *offnorm_out = 0.0;
  ND4_ARGS(nd4_args_dense("dgesvdj_batched", {batch, M, N}, {A, U, sv, V}));
  const int64_t L = M < N ? M : N;
  const int ndev = 1 + (int)h->peers.size();
  // per-device audit (each device's host thread writes its own slot); reduced on the host afterwards — this is the R1
  // "health" reduction of SURVEY.md §8(e), and with host-side results it needs no collective
  std::vector<int> sweeps((size_t)ndev, 0);
  std::vector<double> off((size_t)ndev, 0.0);
  std::vector<unsigned long long> rot((size_t)ndev, 0);
  std::vector<Operand> ops{in_op(A, M * N, M * N), out_op(U, M * L), out_op(sv, L), out_op(V, L * N)};
  ChunkFn fn = [&, M, N](nd4hip_handle* hd, int dev, int64_t nb, void* const* d) {
    int sw = 0; double of = 0.0;
    ND4_TRY(nd4hip_dgesvdj_batched_dev(hd, nb, M, N, P(d, 0), P(d, 1), P(d, 2), P(d, 3), &sw, &of));
    if (sw > sweeps[(size_t)dev]) sweeps[(size_t)dev] = sw;
    if (of > off[(size_t)dev]) off[(size_t)dev] = of;
    rot[(size_t)dev] += hd->svd_rotations;
    return 0;
  };
  // a Jacobi batch below ~100 matrices leaves most of the chip idle: chunks stay large, small batches are not cut at all
  Plan plan; plan.min_chunk = 128; plan.chunk_bytes = size_t(256) << 20;
  ND4_TRY(run_host(h, batch, ops, fn, plan));
  int sw = 0; double of = 0.0; unsigned long long r = 0;
  for (int d = 0; d < ndev; d++) { if (sweeps[(size_t)d] > sw) sw = sweeps[(size_t)d]; if (off[(size_t)d] > of) of = off[(size_t)d]; r += rot[(size_t)d]; }
  h->svd_sweeps = sw; h->svd_offnorm = of; h->svd_rotations = r;
  if (sweeps_out) *sweeps_out = sw;
  if (offnorm_out) *offnorm_out = of;
  return 0;
}

// svd_decomp by divide & conquer and the bidiagonal solver (svd_dc.hip)
extern "C" int nd4hip_dgesdd_batched(nd4hip_handle* h, int64_t batch, int64_t M, int64_t N, const double* A, double* U, double* sv, double* V) {
  ND4_CHECK_ARG(h != nullptr, "nd4hip_dgesdd_batched: NULL handle");
  ND4_ARGS(nd4_args_dense("dgesdd_batched", {batch, M, N}, {A, U, sv, V}));
  const int64_t L = M < N ? M : N;
  std::vector<Operand> ops{in_op(A, M * N, M * N), out_op(U, M * L), out_op(sv, L), out_op(V, L * N)};
  ChunkFn fn = [=](nd4hip_handle* hd, int, int64_t nb, void* const* d) { return nd4hip_dgesdd_batched_dev(hd, nb, M, N, P(d, 0), P(d, 1), P(d, 2), P(d, 3)); };
  return run_host(h, batch, ops, fn);
}
extern "C" int nd4hip_dbdsdc_batched(nd4hip_handle* h, int64_t batch, int64_t K, int64_t J, const double* d, const double* e,
                                     double* U2, double* sv, double* V2) {
  ND4_CHECK_ARG(h != nullptr, "nd4hip_dbdsdc_batched: NULL handle");
  ND4_ARGS(nd4_args_bdsdc(batch, K, J, d, e, U2, sv, V2));
  // the operands in the order d, U2, sv, V2, [e]; 1 x 1: there is no super-diagonal to move
  std::vector<Operand> ops{in_op(d, K, K), out_op(U2, K * K), out_op(sv, K), out_op(V2, J * J)};
  const int ie = J >= 2 ? (int)ops.size() : -1;
  if (J >= 2) ops.push_back(in_op(e, J - 1, J - 1));
  ChunkFn fn = [=](nd4hip_handle* hd, int, int64_t nb, void* const* p) {
    return nd4hip_dbdsdc_batched_dev(hd, nb, K, J, P(p, 0), ie >= 0 ? P(p, ie) : nullptr, P(p, 1), P(p, 2), P(p, 3));
  };
  return run_host(h, batch, ops, fn);
}

// selected singular triplets (bdsvdx.hip); U2 = V2 = NULL (U = V = NULL): the values alone; fallback = NULL: not wanted; e is not moved for J = 1
extern "C" int nd4hip_dbdsvdx_batched_host(nd4hip_handle* h, int64_t batch, int64_t K, int64_t J, int64_t i0, int64_t i1, const double* d,
                                           const double* e, double* U2, double* sv, double* V2, int32_t* fallback) {
  ND4_ARGS(nd4_args_bdsvdx(batch, K, J, i0, i1, d, e, U2, sv, V2));
  ND4_CHECK_ARG(h != nullptr, "nd4hip_dbdsvdx_batched: NULL handle");
  const int64_t k = i1 - i0;
  // the operands in the order d, sv, [e], [U2, V2], [fallback]
  std::vector<Operand> ops{in_op(d, K, K), out_op(sv, k)};
  const int ie = J >= 2 ? (int)ops.size() : -1;
  if (J >= 2) ops.push_back(in_op(e, J - 1, J - 1));
  const int iu = U2 ? (int)ops.size() : -1;
  if (U2) { ops.push_back(out_op(U2, K * k)); ops.push_back(out_op(V2, k * J)); }
  const int ifb = fallback ? (int)ops.size() : -1;
  if (fallback) ops.push_back(out_op(fallback, 1, 4));
  ChunkFn fn = [=](nd4hip_handle* hd, int, int64_t nb, void* const* p) {
    return nd4hip_dbdsvdx_batched_dev(hd, nb, K, J, i0, i1, P(p, 0), ie >= 0 ? P(p, ie) : nullptr, iu >= 0 ? P(p, iu) : nullptr, P(p, 1),
                                      iu >= 0 ? P(p, iu + 1) : nullptr, ifb >= 0 ? static_cast<int32_t*>(p[ifb]) : nullptr);
  };
  return run_host(h, batch, ops, fn);
}
extern "C" int nd4hip_dgesvdx_batched_host(nd4hip_handle* h, int64_t batch, int64_t M, int64_t N, int64_t i0, int64_t i1, const double* A, double* U,
                                           double* sv, double* V, int32_t* fallback) {
  ND4_ARGS(nd4_args_gesvdx(batch, M, N, i0, i1, A, U, sv, V));
  ND4_CHECK_ARG(h != nullptr, "nd4hip_dgesvdx_batched: NULL handle");
  const int64_t k = i1 - i0;
  // the operands in the order A, sv, [U, V], [fallback]
  std::vector<Operand> ops{in_op(A, M * N, M * N), out_op(sv, k)};
  const int iu = U ? (int)ops.size() : -1;
  if (U) { ops.push_back(out_op(U, M * k)); ops.push_back(out_op(V, k * N)); }
  const int ifb = fallback ? (int)ops.size() : -1;
  if (fallback) ops.push_back(out_op(fallback, 1, 4));
  ChunkFn fn = [=](nd4hip_handle* hd, int, int64_t nb, void* const* p) {
    return nd4hip_dgesvdx_batched_dev(hd, nb, M, N, i0, i1, P(p, 0), iu >= 0 ? P(p, iu) : nullptr, P(p, 1), iu >= 0 ? P(p, iu + 1) : nullptr,
                                      ifb >= 0 ? static_cast<int32_t*>(p[ifb]) : nullptr);
  };
  return run_host(h, batch, ops, fn);
}

// eigen_sym / eigenvals_sym (syev.hip); V = NULL: the values alone
extern "C" int nd4hip_dsyevd_batched(nd4hip_handle* h, int64_t batch, int64_t N, const double* S, double* lambda, double* V) {
  ND4_CHECK_ARG(h != nullptr, "nd4hip_dsyevd_batched: NULL handle");
  ND4_ARGS(nd4_args_syev("dsyevd_batched", false, batch, N, S, lambda));
  // the operands that are wanted, in the order S, lambda, [V]
  std::vector<Operand> ops{in_op(S, N * N, N * N), out_op(lambda, N)};
  const int iv = V ? (int)ops.size() : -1;
  if (V) ops.push_back(out_op(V, N * N));
  ChunkFn fn = [=](nd4hip_handle* hd, int, int64_t nb, void* const* d) {
    return nd4hip_dsyevd_batched_dev(hd, nb, N, P(d, 0), P(d, 1), iv >= 0 ? P(d, iv) : nullptr);
  };
  return run_host(h, batch, ops, fn);
}

// the same with algo = 'jacobi' (syevj.hip); V = NULL: the values alone; sweeps = NULL: not wanted
extern "C" int nd4hip_dsyevj_batched(nd4hip_handle* h, int64_t batch, int64_t N, const double* S, double* lambda, double* V, int32_t* sweeps) {
  ND4_CHECK_ARG(h != nullptr, "nd4hip_dsyevj_batched: NULL handle");
  ND4_ARGS(nd4_args_syev("dsyevj_batched", true, batch, N, S, lambda));
  // the operands that are wanted, in the order S, lambda, [V], [sweeps]
  std::vector<Operand> ops{in_op(S, N * N, N * N), out_op(lambda, N)};
  const int iv = V ? (int)ops.size() : -1;
  if (V) ops.push_back(out_op(V, N * N));
  const int is = sweeps ? (int)ops.size() : -1;
  if (sweeps) ops.push_back(out_op(sweeps, 1, 4));
  ChunkFn fn = [=](nd4hip_handle* hd, int, int64_t nb, void* const* d) {
    return nd4hip_dsyevj_batched_dev(hd, nb, N, P(d, 0), P(d, 1), iv >= 0 ? P(d, iv) : nullptr, is >= 0 ? static_cast<int32_t*>(d[is]) : nullptr);
  };
  return run_host(h, batch, ops, fn);
}

// selected eigenpairs by bisection and inverse iteration (syevx.hip); Z, V = NULL: the values alone; e is not moved for N = 1
extern "C" int nd4hip_dstcnt_batched_host(nd4hip_handle* h, int64_t batch, int64_t N, int64_t M, const double* d, const double* e, const double* x,
                                          int32_t* count) {
  ND4_ARGS(nd4_args_stcnt(batch, N, M, d, e, x, count));
  ND4_CHECK_ARG(h != nullptr, "nd4hip_dstcnt_batched: NULL handle");
  // the operands in the order d, x, count, [e]
  std::vector<Operand> ops{in_op(d, N, N), in_op(x, M, M), out_op(count, M, 4)};
  const int ie = N >= 2 ? (int)ops.size() : -1;
  if (N >= 2) ops.push_back(in_op(e, N - 1, N - 1));
  ChunkFn fn = [=](nd4hip_handle* hd, int, int64_t nb, void* const* p) {
    return nd4hip_dstcnt_batched_dev(hd, nb, N, M, P(p, 0), ie >= 0 ? P(p, ie) : nullptr, P(p, 1), static_cast<int32_t*>(p[2]));
  };
  return run_host(h, batch, ops, fn);
}
extern "C" int nd4hip_dstevx_batched_host(nd4hip_handle* h, int64_t batch, int64_t N, int64_t i0, int64_t i1, const double* d, const double* e,
                                          double* lambda, double* Z) {
  ND4_ARGS(nd4_args_stevx(batch, N, i0, i1, d, e, lambda));
  ND4_CHECK_ARG(h != nullptr, "nd4hip_dstevx_batched: NULL handle");
  const int64_t k = i1 - i0;
  // the operands in the order d, lambda, [e], [Z]
  std::vector<Operand> ops{in_op(d, N, N), out_op(lambda, k)};
  const int ie = N >= 2 ? (int)ops.size() : -1;
  if (N >= 2) ops.push_back(in_op(e, N - 1, N - 1));
  const int iz = Z ? (int)ops.size() : -1;
  if (Z) ops.push_back(out_op(Z, k * N));
  ChunkFn fn = [=](nd4hip_handle* hd, int, int64_t nb, void* const* p) {
    return nd4hip_dstevx_batched_dev(hd, nb, N, i0, i1, P(p, 0), ie >= 0 ? P(p, ie) : nullptr, P(p, 1), iz >= 0 ? P(p, iz) : nullptr);
  };
  return run_host(h, batch, ops, fn);
}
extern "C" int nd4hip_dsyevx_batched_host(nd4hip_handle* h, int64_t batch, int64_t N, int64_t i0, int64_t i1, const double* S, double* lambda,
                                          double* V) {
  ND4_ARGS(nd4_args_syevx(batch, N, i0, i1, S, lambda));
  ND4_CHECK_ARG(h != nullptr, "nd4hip_dsyevx_batched: NULL handle");
  const int64_t k = i1 - i0;
  // the operands that are wanted, in the order S, lambda, [V]
  std::vector<Operand> ops{in_op(S, N * N, N * N), out_op(lambda, k)};
  const int iv = V ? (int)ops.size() : -1;
  if (V) ops.push_back(out_op(V, N * k));
  ChunkFn fn = [=](nd4hip_handle* hd, int, int64_t nb, void* const* p) {
    return nd4hip_dsyevx_batched_dev(hd, nb, N, i0, i1, P(p, 0), P(p, 1), iv >= 0 ? P(p, iv) : nullptr);
  };
  return run_host(h, batch, ops, fn);
}

// symmetric tridiagonal reduction, its Q and the eigen routes on them (sytrd.hip); tau and e are not moved for N = 1; V = NULL: the
// values alone
extern "C" int nd4hip_dsytrd_batched_host(nd4hip_handle* h, int64_t batch, int64_t N, const double* S, double* F, double* tau, double* d, double* e) {
  ND4_ARGS(nd4_args_sytrd(batch, N, S, F, tau, d, e));
  ND4_CHECK_ARG(h != nullptr, "nd4hip_dsytrd_batched: NULL handle");
  // the operands in the order S, F, d, [tau, e]
  std::vector<Operand> ops{in_op(S, N * N, N * N), out_op(F, N * N), out_op(d, N)};
  if (N >= 2) { ops.push_back(out_op(tau, N - 1)); ops.push_back(out_op(e, N - 1)); }
  ChunkFn fn = [=](nd4hip_handle* hd, int, int64_t nb, void* const* p) {
    return nd4hip_dsytrd_batched_dev(hd, nb, N, P(p, 0), P(p, 1), N >= 2 ? P(p, 3) : nullptr, P(p, 2), N >= 2 ? P(p, 4) : nullptr);
  };
  return run_host(h, batch, ops, fn);
}
extern "C" int nd4hip_dormtr_batched_host(nd4hip_handle* h, int64_t batch, int64_t N, int64_t K, int transpose, const double* F,
                                          const double* tau, double* Z) {
  ND4_ARGS(nd4_args_ormtr(batch, N, K, transpose, F, tau, Z));
  ND4_CHECK_ARG(h != nullptr, "nd4hip_dormtr_batched: NULL handle");
  // the operands in the order F, Z, [tau]
  std::vector<Operand> ops{in_op(F, N * N, N * N), inout_op(Z, N * K)};
  if (N >= 2) ops.push_back(in_op(tau, N - 1, N - 1));
  ChunkFn fn = [=](nd4hip_handle* hd, int, int64_t nb, void* const* p) {
    return nd4hip_dormtr_batched_dev(hd, nb, N, K, transpose, P(p, 0), N >= 2 ? P(p, 2) : nullptr, P(p, 1));
  };
  return run_host(h, batch, ops, fn);
}
extern "C" int nd4hip_dsyevd_tr_batched_host(nd4hip_handle* h, int64_t batch, int64_t N, const double* S, double* lambda, double* V) {
  ND4_ARGS(nd4_args_syevd_tr(batch, N, S, lambda));
  ND4_CHECK_ARG(h != nullptr, "nd4hip_dsyevd_tr_batched: NULL handle");
  // the operands that are wanted, in the order S, lambda, [V]
  std::vector<Operand> ops{in_op(S, N * N, N * N), out_op(lambda, N)};
  const int iv = V ? (int)ops.size() : -1;
  if (V) ops.push_back(out_op(V, N * N));
  ChunkFn fn = [=](nd4hip_handle* hd, int, int64_t nb, void* const* p) {
    return nd4hip_dsyevd_tr_batched_dev(hd, nb, N, P(p, 0), P(p, 1), iv >= 0 ? P(p, iv) : nullptr);
  };
  return run_host(h, batch, ops, fn);
}
extern "C" int nd4hip_dsyevx_tr_batched_host(nd4hip_handle* h, int64_t batch, int64_t N, int64_t i0, int64_t i1, const double* S, double* lambda,
                                             double* V) {
  ND4_ARGS(nd4_args_syevx_tr(batch, N, i0, i1, S, lambda));
  ND4_CHECK_ARG(h != nullptr, "nd4hip_dsyevx_tr_batched: NULL handle");
  const int64_t k = i1 - i0;
  // the operands that are wanted, in the order S, lambda, [V]
  std::vector<Operand> ops{in_op(S, N * N, N * N), out_op(lambda, k)};
  const int iv = V ? (int)ops.size() : -1;
  if (V) ops.push_back(out_op(V, N * k));
  ChunkFn fn = [=](nd4hip_handle* hd, int, int64_t nb, void* const* p) {
    return nd4hip_dsyevx_tr_batched_dev(hd, nb, N, i0, i1, P(p, 0), P(p, 1), iv >= 0 ? P(p, iv) : nullptr);
  };
  return run_host(h, batch, ops, fn);
}

// Hermitian tridiagonal reduction, its Q and the eigen routes on them (hetrd.hip): complex operands move as elements of 2 D bytes; tau
// and e are not moved for N = 1; V = NULL: the values alone
extern "C" int nd4hip_zhetrd_batched_host(nd4hip_handle* h, int64_t batch, int64_t N, const double* H, double* F, double* tau, double* d, double* e) {
  ND4_ARGS(nd4_args_hetrd(batch, N, H, F, tau, d, e));
  ND4_CHECK_ARG(h != nullptr, "nd4hip_zhetrd_batched: NULL handle");
  // the operands in the order H, F, d, [tau, e]
  std::vector<Operand> ops{in_op(H, N * N, N * N, 2 * D), out_op(F, N * N, 2 * D), out_op(d, N)};
  if (N >= 2) { ops.push_back(out_op(tau, N - 1, 2 * D)); ops.push_back(out_op(e, N - 1)); }
  ChunkFn fn = [=](nd4hip_handle* hd, int, int64_t nb, void* const* p) {
    return nd4hip_zhetrd_batched_dev(hd, nb, N, P(p, 0), P(p, 1), N >= 2 ? P(p, 3) : nullptr, P(p, 2), N >= 2 ? P(p, 4) : nullptr);
  };
  return run_host(h, batch, ops, fn);
}
extern "C" int nd4hip_zunmtr_batched_host(nd4hip_handle* h, int64_t batch, int64_t N, int64_t K, int adjoint, const double* F, const double* tau,
                                          double* Z) {
  ND4_ARGS(nd4_args_unmtr(batch, N, K, adjoint, F, tau, Z));
  ND4_CHECK_ARG(h != nullptr, "nd4hip_zunmtr_batched: NULL handle");
  // the operands in the order F, Z, [tau]
  std::vector<Operand> ops{in_op(F, N * N, N * N, 2 * D), inout_op(Z, N * K, 2 * D)};
  if (N >= 2) ops.push_back(in_op(tau, N - 1, N - 1, 2 * D));
  ChunkFn fn = [=](nd4hip_handle* hd, int, int64_t nb, void* const* p) {
    return nd4hip_zunmtr_batched_dev(hd, nb, N, K, adjoint, P(p, 0), N >= 2 ? P(p, 2) : nullptr, P(p, 1));
  };
  return run_host(h, batch, ops, fn);
}
extern "C" int nd4hip_zheevd_batched_host(nd4hip_handle* h, int64_t batch, int64_t N, const double* H, double* lambda, double* V) {
  ND4_ARGS(nd4_args_heevd(batch, N, H, lambda));
  ND4_CHECK_ARG(h != nullptr, "nd4hip_zheevd_batched: NULL handle");
  // the operands that are wanted, in the order H, lambda, [V]
  std::vector<Operand> ops{in_op(H, N * N, N * N, 2 * D), out_op(lambda, N)};
  const int iv = V ? (int)ops.size() : -1;
  if (V) ops.push_back(out_op(V, N * N, 2 * D));
  ChunkFn fn = [=](nd4hip_handle* hd, int, int64_t nb, void* const* p) {
    return nd4hip_zheevd_batched_dev(hd, nb, N, P(p, 0), P(p, 1), iv >= 0 ? P(p, iv) : nullptr);
  };
  return run_host(h, batch, ops, fn);
}
extern "C" int nd4hip_zheevx_batched_host(nd4hip_handle* h, int64_t batch, int64_t N, int64_t i0, int64_t i1, const double* H, double* lambda,
                                          double* V) {
  ND4_ARGS(nd4_args_heevx(batch, N, i0, i1, H, lambda));
  ND4_CHECK_ARG(h != nullptr, "nd4hip_zheevx_batched: NULL handle");
  const int64_t k = i1 - i0;
  // the operands that are wanted, in the order H, lambda, [V]
  std::vector<Operand> ops{in_op(H, N * N, N * N, 2 * D), out_op(lambda, k)};
  const int iv = V ? (int)ops.size() : -1;
  if (V) ops.push_back(out_op(V, N * k, 2 * D));
  ChunkFn fn = [=](nd4hip_handle* hd, int, int64_t nb, void* const* p) {
    return nd4hip_zheevx_batched_dev(hd, nb, N, i0, i1, P(p, 0), P(p, 1), iv >= 0 ? P(p, iv) : nullptr);
  };
  return run_host(h, batch, ops, fn);
}

// The eigenpairs in a value interval (syevx.hip). bounds, the inputs and range travel through the driver. lambda and
// the vectors do not: a chunk computes them into kcap-wide staging of its own and brings down the kmax columns it found, no more,
// straight to their place in the caller's arrays. The padding up to the kmax of the whole call is then written on the host, from
// range. bounds are host memory here, so NaN and lo > hi are refused before anything is moved.
namespace {
struct IntervalCall {
  int64_t N, kcap;
  double *lambda, *vectors;          // the caller's; vectors may be NULL
  bool by_rows;                      // vectors [batch, kcap, N] (dstevxv), else [batch, N, kcap]
  std::atomic<int64_t> kmax{0};      // the largest of the chunks, which may run on several threads
};
// kc columns of nb members: from kcap-wide device staging to the same columns of the kcap-wide host array `host` (the chunk's part)
int interval_download(nd4hip_handle* hd, int64_t nb, int64_t rows, int64_t kcap, int64_t kc, bool by_rows, const void* dev, double* host) {
  if (kc == 0) return 0;
  if (kc == kcap) { ND4_HIP(hipMemcpyAsync(host, dev, (size_t)(nb * rows * kcap) * D, hipMemcpyDeviceToHost, hd->stream)); return 0; }
  const size_t unit = (size_t)(by_rows ? rows : 1) * D, height = (size_t)(by_rows ? nb : nb * rows);
  ND4_HIP(hipMemcpy2DAsync(host, (size_t)kcap * unit, dev, (size_t)kcap * unit, (size_t)kc * unit, height, hipMemcpyDeviceToHost, hd->stream));
  return 0;
}
// one chunk: `dev_call(lambda_dev, vectors_dev, &kc)` runs the _dev form on the staging, then the kc columns come down
template <class DevCall> int interval_chunk(nd4hip_handle* hd, int64_t nb, IntervalCall* c, DevCall dev_call) {
  const int64_t first = g_chunk_first;
  DevBuf dl, dv;
  ND4_TRY(dl.alloc(hd, (size_t)(nb * c->kcap) * D));
  if (c->vectors) ND4_TRY(dv.alloc(hd, (size_t)(nb * c->N * c->kcap) * D));
  int64_t kc = 0;
  ND4_TRY(dev_call(static_cast<double*>(dl.p), c->vectors ? static_cast<double*>(dv.p) : nullptr, &kc));
  ND4_TRY(interval_download(hd, nb, 1, c->kcap, kc, false, dl.p, c->lambda + first * c->kcap));
  if (c->vectors) ND4_TRY(interval_download(hd, nb, c->N, c->kcap, kc, c->by_rows, dv.p, c->vectors + first * c->N * c->kcap));
  ND4_HIP(hipStreamSynchronize(hd->stream));                 // before the staging goes back to the cache
  int64_t seen = c->kmax.load();
  while (kc > seen && !c->kmax.compare_exchange_weak(seen, kc)) {}
  return 0;
}
// NaN / zeros in the columns k_b .. kmax - 1 of every member, on the host
void interval_pad(const IntervalCall& c, int64_t batch, const int32_t* range, int64_t kmax) {
  for (int64_t b = 0; b < batch; ++b) {
    const int64_t kb = range[2 * b + 1] - range[2 * b];
    for (int64_t j = kb; j < kmax; ++j) {
      c.lambda[b * c.kcap + j] = std::nan("");
      if (!c.vectors) continue;
      if (c.by_rows) std::fill_n(c.vectors + (b * c.kcap + j) * c.N, c.N, 0.0);
      else for (int64_t i = 0; i < c.N; ++i) c.vectors[(b * c.N + i) * c.kcap + j] = 0.0;
    }
  }
}
int syevxv_host(nd4hip_handle* h, bool tridiag, int64_t batch, int64_t N, int64_t kcap, const double* bounds, const double* S, double* lambda,
                double* V, int32_t* range, int64_t* kmax) {
  const char* op = tridiag ? "dsyevxv_tr_batched" : "dsyevxv_batched";
  ND4_ARGS(nd4_args_syevxv(tridiag, batch, N, kcap, bounds, S, lambda, range, kmax));
  ND4_CHECK_ARG(h != nullptr, "nd4hip_%s: NULL handle", op);
  ND4_TRY(nd4_args_bounds(op, batch, bounds));
  IntervalCall call{N, kcap, lambda, V, false};
  // the operands in the order bounds, S, range
  std::vector<Operand> ops{in_op(bounds, 2, 2), in_op(S, N * N, N * N), out_op(range, 2, 4)};
  ChunkFn fn = [=, &call](nd4hip_handle* hd, int, int64_t nb, void* const* p) {
    return interval_chunk(hd, nb, &call, [=](double* ld, double* vd, int64_t* kc) {
      return (tridiag ? nd4hip_dsyevxv_tr_batched_dev : nd4hip_dsyevxv_batched_dev)(hd, nb, N, kcap, P(p, 0), P(p, 1), ld, vd,
                                                                                  static_cast<int32_t*>(p[2]), kc);
    });
  };
  ND4_TRY(run_host(h, batch, ops, fn));
  *kmax = call.kmax.load();
  interval_pad(call, batch, range, *kmax);
  return 0;
}
}  // namespace
extern "C" int nd4hip_dstevxv_batched_host(nd4hip_handle* h, int64_t batch, int64_t N, int64_t kcap, const double* bounds, const double* d,
                                           const double* e, double* lambda, double* Z, int32_t* range, int64_t* kmax) {
  ND4_ARGS(nd4_args_stevxv(batch, N, kcap, bounds, d, e, lambda, range, kmax));
  ND4_CHECK_ARG(h != nullptr, "nd4hip_dstevxv_batched: NULL handle");
  ND4_TRY(nd4_args_bounds("dstevxv_batched", batch, bounds));
  IntervalCall call{N, kcap, lambda, Z, true};
  // the operands in the order bounds, d, range, [e]
  std::vector<Operand> ops{in_op(bounds, 2, 2), in_op(d, N, N), out_op(range, 2, 4)};
  const int ie = N >= 2 ? (int)ops.size() : -1;
  if (N >= 2) ops.push_back(in_op(e, N - 1, N - 1));
  ChunkFn fn = [=, &call](nd4hip_handle* hd, int, int64_t nb, void* const* p) {
    return interval_chunk(hd, nb, &call, [=](double* ld, double* zd, int64_t* kc) {
      return nd4hip_dstevxv_batched_dev(hd, nb, N, kcap, P(p, 0), P(p, 1), ie >= 0 ? P(p, ie) : nullptr, ld, zd, static_cast<int32_t*>(p[2]), kc);
    });
  };
  ND4_TRY(run_host(h, batch, ops, fn));
  *kmax = call.kmax.load();
  interval_pad(call, batch, range, *kmax);
  return 0;
}
extern "C" int nd4hip_dsyevxv_batched_host(nd4hip_handle* h, int64_t batch, int64_t N, int64_t kcap, const double* bounds, const double* S,
                                           double* lambda, double* V, int32_t* range, int64_t* kmax) {
  return syevxv_host(h, false, batch, N, kcap, bounds, S, lambda, V, range, kmax);
}
extern "C" int nd4hip_dsyevxv_tr_batched_host(nd4hip_handle* h, int64_t batch, int64_t N, int64_t kcap, const double* bounds, const double* S,
                                              double* lambda, double* V, int32_t* range, int64_t* kmax) {
  return syevxv_host(h, true, batch, N, kcap, bounds, S, lambda, V, range, kmax);
}

// eigen_sym_gen / eigenvals_sym_gen (sygv.hip); X = NULL: the values alone; sweeps = NULL: not wanted; strideB = 0: one B, uploaded
// once per device
extern "C" int nd4hip_dsygvd_batched(nd4hip_handle* h, int algo, int64_t batch, int64_t N, const double* A, const double* B, int64_t strideB,
                                     double* lambda, double* X, int32_t* sweeps) {
  ND4_ARGS(nd4_args_sygvd(algo, batch, N, A, B, strideB, lambda));
  ND4_CHECK_ARG(h != nullptr, "nd4hip_dsygvd_batched: NULL handle");
  if (algo == 0) sweeps = nullptr;
  // the operands that are wanted, in the order A, B, lambda, [X], [sweeps]
  std::vector<Operand> ops{in_op(A, N * N, N * N), in_op(B, N * N, strideB), out_op(lambda, N)};
  const int ix = X ? (int)ops.size() : -1;
  if (X) ops.push_back(out_op(X, N * N));
  const int is = sweeps ? (int)ops.size() : -1;
  if (sweeps) ops.push_back(out_op(sweeps, 1, 4));
  ChunkFn fn = [=](nd4hip_handle* hd, int, int64_t nb, void* const* d) {
    return nd4_sygvd_run(hd, algo, nb, N, P(d, 0), P(d, 1), strideB, P(d, 2), ix >= 0 ? P(d, ix) : nullptr,
                         is >= 0 ? static_cast<int32_t*>(d[is]) : nullptr, g_chunk_first);
  };
  return run_host(h, batch, ops, fn);
}

// the same with the selectors of step 3. select 0 and 1 are plain operands; select 2 is an interval call (see IntervalCall above):
// lambda and X stay out of the driver and come down kmax columns wide
extern "C" int nd4hip_dsygvx_batched_host(nd4hip_handle* h, int reduction, int select, int64_t batch, int64_t N, int64_t i0, int64_t i1,
                                     int64_t kcap, const double* bounds, const double* A, const double* B, int64_t strideB, double* lambda,
                                     double* X, int32_t* range, int64_t* kmax) {
  ND4_ARGS(nd4_args_sygvx(reduction, select, batch, N, i0, i1, kcap, bounds, A, B, strideB, lambda, range, kmax));
  ND4_CHECK_ARG(h != nullptr, "nd4hip_dsygvx_batched: NULL handle");
  if (select == 2) {
    ND4_TRY(nd4_args_bounds("dsygvx_batched", batch, bounds));
    IntervalCall call{N, kcap, lambda, X, false};
    // the operands in the order bounds, A, B, range
    std::vector<Operand> ops{in_op(bounds, 2, 2), in_op(A, N * N, N * N), in_op(B, N * N, strideB), out_op(range, 2, 4)};
    ChunkFn fn = [=, &call](nd4hip_handle* hd, int, int64_t nb, void* const* p) {
      const int64_t first = g_chunk_first;
      return interval_chunk(hd, nb, &call, [=](double* ld, double* xd, int64_t* kc) {
        return nd4_sygvx_run(hd, reduction, 2, nb, N, 0, 0, kcap, P(p, 0), P(p, 1), P(p, 2), strideB, ld, xd, static_cast<int32_t*>(p[3]), kc, first);
      });
    };
    ND4_TRY(run_host(h, batch, ops, fn));
    *kmax = call.kmax.load();
    interval_pad(call, batch, range, *kmax);
    return 0;
  }
  const int64_t K = select == 1 ? i1 - i0 : N;
  // the operands that are wanted, in the order A, B, lambda, [X]
  std::vector<Operand> ops{in_op(A, N * N, N * N), in_op(B, N * N, strideB), out_op(lambda, K)};
  const int ix = X ? (int)ops.size() : -1;
  if (X) ops.push_back(out_op(X, N * K));
  ChunkFn fn = [=](nd4hip_handle* hd, int, int64_t nb, void* const* p) {
    return nd4_sygvx_run(hd, reduction, select, nb, N, i0, i1, 0, nullptr, P(p, 0), P(p, 1), strideB, P(p, 2), ix >= 0 ? P(p, ix) : nullptr, nullptr,
                         nullptr, g_chunk_first);
  };
  return run_host(h, batch, ops, fn);
}

extern "C" int nd4hip_dsygst_batched(nd4hip_handle* h, int64_t batch, int64_t N, const double* A, const double* L, int64_t strideL, double* C) {
  ND4_ARGS(nd4_args_sygst(batch, N, A, L, strideL, C));
  ND4_CHECK_ARG(h != nullptr, "nd4hip_dsygst_batched: NULL handle");
  std::vector<Operand> ops{in_op(A, N * N, N * N), in_op(L, N * N, strideL), out_op(C, N * N)};
  ChunkFn fn = [=](nd4hip_handle* hd, int, int64_t nb, void* const* d) { return nd4hip_dsygst_batched_dev(hd, nb, N, P(d, 0), P(d, 1), strideL, P(d, 2)); };
  return run_host(h, batch, ops, fn);
}

// Hermitian Cholesky, the complex triangular solves and eigen_herm_gen (hegv.hip): complex operands move as elements of 2 D bytes;
// strideL / strideB = 0: one L or B, uploaded once per device; X = NULL: the values alone
extern "C" int nd4hip_zpotrf_batched_host(nd4hip_handle* h, int64_t batch, int64_t N, const double* H, double* L) {
  ND4_ARGS(nd4_args_zpotrf(batch, N, H, L));
  ND4_CHECK_ARG(h != nullptr, "nd4hip_zpotrf_batched: NULL handle");
  std::vector<Operand> ops{in_op(H, N * N, N * N, 2 * D), out_op(L, N * N, 2 * D)};
  ChunkFn fn = [=](nd4hip_handle* hd, int, int64_t nb, void* const* p) { return nd4_zpotrf_run(hd, nb, N, P(p, 0), P(p, 1), g_chunk_first); };
  return run_host(h, batch, ops, fn);
}
extern "C" int nd4hip_zpotrs_batched_host(nd4hip_handle* h, int64_t batch, int64_t N, int64_t K, const double* L, int64_t strideL,
                                          const double* Y, double* X) {
  ND4_ARGS(nd4_args_zpotrs(batch, N, K, L, strideL, Y, X));
  ND4_CHECK_ARG(h != nullptr, "nd4hip_zpotrs_batched: NULL handle");
  std::vector<Operand> ops{in_op(L, N * N, strideL, 2 * D), in_op(Y, N * K, N * K, 2 * D), out_op(X, N * K, 2 * D)};
  ChunkFn fn = [=](nd4hip_handle* hd, int, int64_t nb, void* const* p) {
    return nd4hip_zpotrs_batched_dev(hd, nb, N, K, P(p, 0), strideL, P(p, 1), P(p, 2));
  };
  return run_host(h, batch, ops, fn);
}
extern "C" int nd4hip_ztrsm_batched_host(nd4hip_handle* h, int64_t batch, int64_t N, int64_t K, int adjoint, const double* L, int64_t strideL,
                                         double* X) {
  ND4_ARGS(nd4_args_ztrsm(batch, N, K, adjoint, L, strideL, X));
  ND4_CHECK_ARG(h != nullptr, "nd4hip_ztrsm_batched: NULL handle");
  std::vector<Operand> ops{in_op(L, N * N, strideL, 2 * D), inout_op(X, N * K, 2 * D)};
  ChunkFn fn = [=](nd4hip_handle* hd, int, int64_t nb, void* const* p) {
    return nd4hip_ztrsm_batched_dev(hd, nb, N, K, adjoint, P(p, 0), strideL, P(p, 1));
  };
  return run_host(h, batch, ops, fn);
}
extern "C" int nd4hip_zhegst_batched_host(nd4hip_handle* h, int64_t batch, int64_t N, const double* A, const double* L, int64_t strideL,
                                          double* C) {
  ND4_ARGS(nd4_args_zhegst(batch, N, A, L, strideL, C));
  ND4_CHECK_ARG(h != nullptr, "nd4hip_zhegst_batched: NULL handle");
  std::vector<Operand> ops{in_op(A, N * N, N * N, 2 * D), in_op(L, N * N, strideL, 2 * D), out_op(C, N * N, 2 * D)};
  ChunkFn fn = [=](nd4hip_handle* hd, int, int64_t nb, void* const* p) { return nd4hip_zhegst_batched_dev(hd, nb, N, P(p, 0), P(p, 1), strideL, P(p, 2)); };
  return run_host(h, batch, ops, fn);
}
extern "C" int nd4hip_zhegvd_batched_host(nd4hip_handle* h, int64_t batch, int64_t N, const double* A, const double* B, int64_t strideB,
                                          double* lambda, double* X) {
  ND4_ARGS(nd4_args_zhegvd(batch, N, A, B, strideB, lambda));
  ND4_CHECK_ARG(h != nullptr, "nd4hip_zhegvd_batched: NULL handle");
  // the operands that are wanted, in the order A, B, lambda, [X]
  std::vector<Operand> ops{in_op(A, N * N, N * N, 2 * D), in_op(B, N * N, strideB, 2 * D), out_op(lambda, N)};
  const int ix = X ? (int)ops.size() : -1;
  if (X) ops.push_back(out_op(X, N * N, 2 * D));
  ChunkFn fn = [=](nd4hip_handle* hd, int, int64_t nb, void* const* p) {
    return nd4_zhegvd_run(hd, nb, N, P(p, 0), P(p, 1), strideB, P(p, 2), ix >= 0 ? P(p, ix) : nullptr, g_chunk_first);
  };
  return run_host(h, batch, ops, fn);
}
extern "C" int nd4hip_zhegvx_batched_host(nd4hip_handle* h, int64_t batch, int64_t N, int64_t i0, int64_t i1, const double* A, const double* B,
                                          int64_t strideB, double* lambda, double* X) {
  ND4_ARGS(nd4_args_zhegvx(batch, N, i0, i1, A, B, strideB, lambda));
  ND4_CHECK_ARG(h != nullptr, "nd4hip_zhegvx_batched: NULL handle");
  const int64_t k = i1 - i0;
  // the operands that are wanted, in the order A, B, lambda, [X]
  std::vector<Operand> ops{in_op(A, N * N, N * N, 2 * D), in_op(B, N * N, strideB, 2 * D), out_op(lambda, k)};
  const int ix = X ? (int)ops.size() : -1;
  if (X) ops.push_back(out_op(X, N * k, 2 * D));
  ChunkFn fn = [=](nd4hip_handle* hd, int, int64_t nb, void* const* p) {
    return nd4_zhegvx_run(hd, nb, N, i0, i1, P(p, 0), P(p, 1), strideB, P(p, 2), ix >= 0 ? P(p, ix) : nullptr, g_chunk_first);
  };
  return run_host(h, batch, ops, fn);
}
