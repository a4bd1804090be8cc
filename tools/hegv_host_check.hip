// Stand-alone host check of csrc/hegv.hip: the argument checkers of its six operations (nd4hip_args.h), the tier choice, the LDS
// requests for every N in 1 .. 2048, and the pass and workspace arithmetic for every N and a range of batches, for AddressSanitizer
// + UBSan on the CPU. Nothing is launched and no device is needed: the few library functions that hegv.hip's drivers would call are
// stubs that fail. Build and run from the repository root:
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         -fsanitize=address,undefined tools/hegv_host_check.hip nd4js_amd/csrc/hegv.hip -o hegv_host_check && ./hegv_host_check
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
int nd4_zheevd(nd4hip_handle*, int64_t, int64_t, const double*, double*, double*) { return ND4HIP_ERR_HIP; }
int nd4_zheevx(nd4hip_handle*, int64_t, int64_t, int64_t, int64_t, const double*, double*, double*) { return ND4HIP_ERR_HIP; }

#define EXPECT(cond) do { if (!(cond)) { std::printf("FAILED line %d: %s (last error: %s)\n", __LINE__, #cond, g_err); return 1; } } while (0)

int main() {
  double buf[4];
  const void *P = buf, *Z = nullptr;
  // the order of the checks: negative extent, subset / selector, N <= 2048, stride, empty call, NULL pointer
  EXPECT(nd4_args_zpotrf(-1, 4096, Z, Z) == ND4HIP_ERR_ARG && std::strstr(g_err, "nd4hip_zpotrf_batched: negative extent"));
  EXPECT(nd4_args_zpotrf(0, 2049, Z, Z) == ND4HIP_ERR_ARG && std::strstr(g_err, "nd4hip_zpotrf_batched: N <= 2048"));
  EXPECT(nd4_args_zpotrf(0, 5, Z, Z) == ND4_ARGS_EMPTY && nd4_args_zpotrf(3, 0, Z, Z) == ND4_ARGS_EMPTY);
  EXPECT(nd4_args_zpotrf(1, 1, P, P) == ND4_ARGS_GO && nd4_args_zpotrf(1, 2, P, Z) == ND4HIP_ERR_ARG && nd4_args_zpotrf(1, 2, Z, P) == ND4HIP_ERR_ARG);
  EXPECT(nd4_args_zpotrs(1, 3, 2, P, 9, P, P) == ND4_ARGS_GO && nd4_args_zpotrs(4, 3, 2, P, 0, P, P) == ND4_ARGS_GO);
  EXPECT(nd4_args_zpotrs(1, 3, 2, P, 8, P, P) == ND4HIP_ERR_ARG && std::strstr(g_err, "nd4hip_zpotrs_batched: strideL must be N*N or 0"));
  EXPECT(nd4_args_zpotrs(1, 3, 2, P, 9, Z, P) == ND4HIP_ERR_ARG && nd4_args_zpotrs(1, 3, 2, P, 9, P, Z) == ND4HIP_ERR_ARG);
  EXPECT(nd4_args_zpotrs(1, 3, 2, Z, 9, P, P) == ND4HIP_ERR_ARG && std::strstr(g_err, "nd4hip_zpotrs_batched: NULL pointer"));
  EXPECT(nd4_args_zpotrs(1, 3, 0, Z, 9, Z, Z) == ND4_ARGS_EMPTY && nd4_args_zpotrs(1, 2049, 0, Z, 0, Z, Z) == ND4HIP_ERR_ARG);
  EXPECT(nd4_args_ztrsm(1, 4, 1, 2, P, 16, P) == ND4HIP_ERR_ARG && std::strstr(g_err, "nd4hip_ztrsm_batched: adjoint must be 0 or 1"));
  EXPECT(nd4_args_ztrsm(1, 4, 1, 1, P, 16, P) == ND4_ARGS_GO && nd4_args_ztrsm(1, 4, -1, 1, P, 16, P) == ND4HIP_ERR_ARG);
  EXPECT(nd4_args_ztrsm(1, 4, 1, 0, P, 15, P) == ND4HIP_ERR_ARG && nd4_args_ztrsm(0, 4, 1, 0, Z, 16, Z) == ND4_ARGS_EMPTY);
  EXPECT(nd4_args_zhegst(1, 2049, P, P, 0, P) == ND4HIP_ERR_ARG && std::strstr(g_err, "nd4hip_zhegst_batched: N <= 2048"));
  EXPECT(nd4_args_zhegst(2, 3, P, P, 9, P) == ND4_ARGS_GO && nd4_args_zhegst(2, 3, P, P, 3, P) == ND4HIP_ERR_ARG);
  EXPECT(nd4_args_zhegst(2, 3, P, Z, 9, P) == ND4HIP_ERR_ARG && nd4_args_zhegst(2, 0, Z, Z, 0, Z) == ND4_ARGS_EMPTY);
  EXPECT(nd4_args_zhegvd(1, 2049, P, P, 0, P) == ND4HIP_ERR_ARG && nd4_args_zhegvd(1, 0, Z, Z, 0, Z) == ND4_ARGS_EMPTY);
  EXPECT(nd4_args_zhegvd(2, 2, P, P, 4, P) == ND4_ARGS_GO && nd4_args_zhegvd(2, 2, P, P, 0, P) == ND4_ARGS_GO);
  EXPECT(nd4_args_zhegvd(2, 2, P, P, 5, P) == ND4HIP_ERR_ARG && std::strstr(g_err, "nd4hip_zhegvd_batched: strideB must be N*N or 0"));
  EXPECT(nd4_args_zhegvd(2, 2, P, P, 4, Z) == ND4HIP_ERR_ARG && std::strstr(g_err, "nd4hip_zhegvd_batched: NULL pointer"));
  EXPECT(nd4_args_zhegvd(-2, 2, P, P, 4, P) == ND4HIP_ERR_ARG && std::strstr(g_err, "negative extent"));
  EXPECT(nd4_args_zhegvx(1, 4, 3, 2, P, P, 16, P) == ND4HIP_ERR_ARG && std::strstr(g_err, "nd4hip_zhegvx_batched: subset must satisfy"));
  EXPECT(nd4_args_zhegvx(1, 2049, 0, 2050, P, P, 0, P) == ND4HIP_ERR_ARG && std::strstr(g_err, "subset must satisfy"));
  EXPECT(nd4_args_zhegvx(1, 2049, 0, 1, P, P, 0, P) == ND4HIP_ERR_ARG && std::strstr(g_err, "N <= 2048"));
  EXPECT(nd4_args_zhegvx(1, 4, 2, 2, Z, Z, 16, Z) == ND4_ARGS_EMPTY && nd4_args_zhegvx(1, 4, 0, 4, P, P, 16, P) == ND4_ARGS_GO);
  EXPECT(nd4_args_zhegvx(1, 4, 0, 4, P, Z, 16, P) == ND4HIP_ERR_ARG && std::strstr(g_err, "NULL pointer"));
  // tiers and their LDS over every N the entry points admit; 163840 B is the CU's LDS
  const size_t LDS = 163840;
  int64_t cap = 0;
  for (int64_t N = 1; N <= 2048; ++N) {
    const int tier = nd4_hegv_tier(N);
    EXPECT(tier == (N <= 64 ? 0 : 1));
    if (tier == 0) cap = N;
    const size_t lds = nd4_hegv_lds(N);
    EXPECT(lds % 16 == 0 && lds <= LDS);
    if (tier == 0) {
      // hegst_small's two tiles at pitch N | 1, and ztrsm_small's L with 64 right-hand sides at pitch 65: both inside the request
      EXPECT(lds >= 16 * (size_t)(2 * N * (N | 1)) && lds == 16 * (size_t)(N * (N | 1) + N * 65));
    } else {
      EXPECT(lds == 16 * (size_t)(2 * 64 * 65));   // a diagonal block and 64 rows or right-hand sides
    }
  }
  EXPECT(cap == 64 && nd4_hegv_lds(64) == 133120 && 16 * (size_t)(2 * 64 * 65) == 133120);
  // passes: every member is taken once, a pass's N^2 workspace stays within 1 GiB of 16-byte elements, a pass fits a grid dimension
  const int64_t batches[] = {1, 2, 31, 32, 33, 511, 512, 513, 15887, 15888, 32767, 32768, 32769, 65535, 65536, 70000, 1000000};
  for (int64_t N = 1; N <= 2048; ++N)
    for (int64_t batch : batches) {
      const int64_t chunk = nd4_hegv_chunk(batch, N);
      EXPECT(chunk >= 1 && chunk <= batch && chunk <= 32768);
      EXPECT((size_t)chunk * (size_t)(N * N) * 16 <= ((size_t)1 << 30));
      EXPECT(chunk == batch || (size_t)(chunk + 1) * (size_t)(N * N) * 16 > ((size_t)1 << 30) || chunk == 32768);
      if (N <= 45) EXPECT(chunk == (batch < 32768 ? batch : 32768));
      int64_t seen = 0, passes = 0;
      for (int64_t b0 = 0; b0 < batch; b0 += chunk) { seen += batch - b0 < chunk ? batch - b0 : chunk; ++passes; }
      EXPECT(seen == batch && passes == (batch + chunk - 1) / chunk);
    }
  EXPECT(nd4_hegv_chunk(1000, 2048) == 16 && nd4_hegv_chunk(1000, 512) == 256 && nd4_hegv_chunk(70000, 4) == 32768 && nd4_hegv_chunk(70000, 64) == 16384);
  // the drivers stop at the stub allocator, before anything is launched
  nd4hip_handle h;
  EXPECT(nd4_zpotrf(&h, 1, 4, buf, buf, 0) == ND4HIP_ERR_HIP);
  EXPECT(nd4_zhegst(&h, 1, 65, buf, buf, 0, buf) == ND4HIP_ERR_HIP);
  EXPECT(nd4_zhegvx(&h, true, 0, 4, 1, 4, buf, buf, 0, buf, buf, 0) == ND4HIP_ERR_HIP);
  EXPECT(nd4_zhegvx(&h, false, 0, 1, 2, 1, buf, buf, 1, buf, nullptr, 0) == ND4HIP_ERR_HIP);
  EXPECT(nd4_ztrsm(&h, 0, 1, 4, (int64_t)65536 * 64, buf, 16, buf) == ND4HIP_ERR_ARG && std::strstr(g_err, "right-hand sides"));
  std::printf("hegv host check ok\n");
  return 0;
}
