// Stand-alone host check of csrc/zgetrf.hip: the argument checkers of its three operations (nd4hip_args.h), the tier choice, the LDS
// requests for every N in 1 .. 2048, and the pass arithmetic for every N and a range of batches, for AddressSanitizer + UBSan on the
// CPU. Nothing is launched and no device is needed: the few library functions that zgetrf.hip's drivers would call are stubs that
// fail. Build and run from the repository root:
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         -fsanitize=address,undefined tools/zlu_host_check.hip nd4js_amd/csrc/zgetrf.hip -o zlu_host_check && ./zlu_host_check
#include "../nd4js_amd/csrc/nd4hip_args.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>

static char g_err[256];
void nd4_set_error(const char* fmt, ...) { va_list ap; va_start(ap, fmt); vsnprintf(g_err, sizeof g_err, fmt, ap); va_end(ap); }
int nd4_hip_fail(hipError_t, const char*, const char*, int) { return ND4HIP_ERR_HIP; }
int nd4_ws_alloc(nd4hip_handle*, size_t, void**) { return ND4HIP_ERR_HIP; }
int nd4_pinned(nd4hip_handle*, size_t, void**) { return ND4HIP_ERR_HIP; }
Nd4WsScope::Nd4WsScope(nd4hip_handle* hh) : h(hh), nblocks(0), used_last(0), generation(0) {}
Nd4WsScope::~Nd4WsScope() {}

#define EXPECT(cond) do { if (!(cond)) { std::printf("FAILED line %d: %s (last error: %s)\n", __LINE__, #cond, g_err); return 1; } } while (0)

int main() {
  alignas(16) double buf[4];
  int32_t ibuf[4];
  const void *P = buf, *Z = nullptr;
  // the order of the checks: negative extent, N <= 2048, stride, empty call, NULL pointer
  EXPECT(nd4_args_zgetrf(-1, 4096, Z, Z, Z) == ND4HIP_ERR_ARG && std::strstr(g_err, "nd4hip_zgetrf_batched: negative extent"));
  EXPECT(nd4_args_zgetrf(0, 2049, Z, Z, Z) == ND4HIP_ERR_ARG && std::strstr(g_err, "nd4hip_zgetrf_batched: N <= 2048"));
  EXPECT(nd4_args_zgetrf(0, 5, Z, Z, Z) == ND4_ARGS_EMPTY && nd4_args_zgetrf(3, 0, Z, Z, Z) == ND4_ARGS_EMPTY);
  EXPECT(nd4_args_zgetrf(1, 1, P, P, P) == ND4_ARGS_GO && nd4_args_zgetrf(1, 2, P, Z, P) == ND4HIP_ERR_ARG && nd4_args_zgetrf(1, 2, Z, P, P) == ND4HIP_ERR_ARG);
  EXPECT(nd4_args_zgetrf(1, 2, P, P, Z) == ND4HIP_ERR_ARG && std::strstr(g_err, "nd4hip_zgetrf_batched: NULL pointer"));
  EXPECT(nd4_args_zgetrs(2, 3, 2, P, 9, P, 3, P, 6, P) == ND4_ARGS_GO && nd4_args_zgetrs(2, 3, 2, P, 0, P, 0, P, 0, P) == ND4_ARGS_GO);
  EXPECT(nd4_args_zgetrs(2, 3, 2, P, 8, P, 3, P, 6, P) == ND4HIP_ERR_ARG && std::strstr(g_err, "nd4hip_zgetrs_batched: a stride must be 0 or at least"));
  EXPECT(nd4_args_zgetrs(2, 3, 2, P, 9, P, 2, P, 6, P) == ND4HIP_ERR_ARG && nd4_args_zgetrs(2, 3, 2, P, 9, P, 3, P, 5, P) == ND4HIP_ERR_ARG);
  EXPECT(nd4_args_zgetrs(2, 3, -2, P, 9, P, 3, P, 6, P) == ND4HIP_ERR_ARG && std::strstr(g_err, "negative extent"));
  EXPECT(nd4_args_zgetrs(2, 2049, 0, Z, 0, Z, 0, Z, 0, Z) == ND4HIP_ERR_ARG && std::strstr(g_err, "N <= 2048"));
  EXPECT(nd4_args_zgetrs(2, 3, 0, Z, 9, Z, 3, Z, 0, Z) == ND4_ARGS_EMPTY && nd4_args_zgetrs(0, 3, 2, Z, 9, Z, 3, Z, 6, Z) == ND4_ARGS_EMPTY);
  EXPECT(nd4_args_zgetrs(2, 3, 2, Z, 9, P, 3, P, 6, P) == ND4HIP_ERR_ARG && nd4_args_zgetrs(2, 3, 2, P, 9, Z, 3, P, 6, P) == ND4HIP_ERR_ARG);
  EXPECT(nd4_args_zgetrs(2, 3, 2, P, 9, P, 3, Z, 6, P) == ND4HIP_ERR_ARG && nd4_args_zgetrs(2, 3, 2, P, 9, P, 3, P, 6, Z) == ND4HIP_ERR_ARG);
  EXPECT(nd4_args_zgesv(1, 2049, 1, P, P, P) == ND4HIP_ERR_ARG && std::strstr(g_err, "nd4hip_zgesv_batched: N <= 2048"));
  EXPECT(nd4_args_zgesv(1, 4, -1, P, P, P) == ND4HIP_ERR_ARG && nd4_args_zgesv(1, 4, 0, Z, Z, Z) == ND4_ARGS_EMPTY && nd4_args_zgesv(0, 4, 1, Z, Z, Z) == ND4_ARGS_EMPTY);
  EXPECT(nd4_args_zgesv(1, 4, 1, P, P, P) == ND4_ARGS_GO && nd4_args_zgesv(1, 4, 1, Z, P, P) == ND4HIP_ERR_ARG && nd4_args_zgesv(1, 4, 1, P, Z, P) == ND4HIP_ERR_ARG);
  EXPECT(nd4_args_zgesv(1, 4, 1, P, P, Z) == ND4HIP_ERR_ARG && std::strstr(g_err, "nd4hip_zgesv_batched: NULL pointer"));
  // tiers and their LDS over every N the entry points admit; 163840 B is the CU's LDS
  const size_t LDS = 163840;
  int64_t cap = 0;
  for (int64_t N = 1; N <= 2048; ++N) {
    const int tier = nd4_zgetrf_tier(N);
    EXPECT(tier == (N <= 16 ? 0 : N <= 64 ? 1 : 2));
    if (tier <= 1) cap = N;
    const size_t lds = nd4_zgetrf_lds(N);
    EXPECT(lds % 16 == 0 && lds <= LDS);
    if (tier <= 1) EXPECT(lds == 16 * (size_t)(N * (N | 1) + N * 65));   // zgetrs_small: LU at pitch N | 1 and 64 right-hand sides at pitch 65
    else EXPECT(lds == 16 * (size_t)(2 * 64 * 65));                      // a diagonal block and 64 columns or right-hand sides
  }
  EXPECT(cap == 64 && nd4_zgetrf_lds(64) == 133120);
  // passes: every member is taken once, a pass fits a grid dimension, zsolve's LU workspace stays within 1 GiB
  const int64_t batches[] = {1, 2, 31, 32, 33, 511, 512, 513, 32767, 32768, 32769, 65535, 65536, 70000, 1000000};
  for (int64_t N = 1; N <= 2048; ++N)
    for (int64_t batch : batches)
      for (int with_lu = 0; with_lu < 2; ++with_lu) {
        const int64_t chunk = nd4_zgetrf_chunk(batch, N, with_lu != 0);
        EXPECT(chunk >= 1 && chunk <= batch && chunk <= 32768);
        if (with_lu) EXPECT((size_t)chunk * (size_t)(N * N) * 16 <= ((size_t)1 << 30));
        else EXPECT(chunk == (batch < 32768 ? batch : 32768));
        int64_t seen = 0, passes = 0;
        for (int64_t b0 = 0; b0 < batch; b0 += chunk) { seen += batch - b0 < chunk ? batch - b0 : chunk; ++passes; }
        EXPECT(seen == batch && passes == (batch + chunk - 1) / chunk);
      }
  EXPECT(nd4_zgetrf_chunk(1000, 2048, true) == 16 && nd4_zgetrf_chunk(1000, 512, true) == 256 && nd4_zgetrf_chunk(70000, 4, true) == 32768);
  // the drivers' refusals, and their stop at the stub allocator before anything is launched
  nd4hip_handle h;
  EXPECT(nd4_zgetrf(&h, 1, 2049, buf, buf, ibuf, nullptr) == ND4HIP_ERR_ARG && nd4_zgetrf(&h, 1, 0, buf, buf, ibuf, nullptr) == ND4HIP_ERR_ARG);
  EXPECT(nd4_zgetrf(&h, 1, 4, buf + 1, buf, ibuf, nullptr) == ND4HIP_ERR_ARG && std::strstr(g_err, "16-byte aligned"));
  EXPECT(nd4_zgetrf(&h, 1, 4, buf, buf, ibuf, nullptr) == ND4HIP_ERR_HIP && nd4_zgetrf(&h, 3, 65, buf, buf, ibuf, ibuf) == ND4HIP_ERR_HIP);
  EXPECT(nd4_zgetrs(&h, 1, 2049, 1, buf, 0, ibuf, 0, buf, 0, buf) == ND4HIP_ERR_ARG && nd4_zgetrs(&h, 1, 4, 1, buf, 0, ibuf, 0, buf + 1, 0, buf) == ND4HIP_ERR_ARG);
  EXPECT(nd4_args_zgetrs(1, 4, (int64_t)65535 * 64 + 1, P, 16, P, 4, P, 0, P) == ND4HIP_ERR_ARG && std::strstr(g_err, "nd4hip_zgetrs_batched: K exceeds"));
  EXPECT(nd4_args_zgesv(1, 4, (int64_t)65535 * 64 + 1, P, P, P) == ND4HIP_ERR_ARG && std::strstr(g_err, "nd4hip_zgesv_batched: K exceeds"));
  EXPECT(nd4_args_zgesv(1, 4, (int64_t)65535 * 64, P, P, P) == ND4_ARGS_GO);
  EXPECT(nd4_zgesv(&h, 1, 2049, 1, buf, buf, buf, 0, nullptr) == ND4HIP_ERR_ARG && nd4_zgesv(&h, 1, 4, 1, buf, buf, buf + 1, 0, nullptr) == ND4HIP_ERR_ARG);
  EXPECT(nd4_zgesv(&h, 2, 4, 1, buf, buf, buf, 0, nullptr) == ND4HIP_ERR_HIP);
  std::printf("zlu host check ok\n");
  return 0;
}
