// Stand-alone host check of csrc/zgehrd.hip and csrc/zhseqr.hip: the six argument checkers (nd4hip_args.h), the tier choices, the LDS
// requests and the workspace and pass arithmetic for every N, and the drivers' refusals, for AddressSanitizer + UBSan on the CPU.
// Nothing is launched and no device is needed: the library functions that the drivers would call are stubs that fail. Build and run
// from the repository root:
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         -fsanitize=address,undefined tools/zeig_host_check.hip nd4js_amd/csrc/zgehrd.hip nd4js_amd/csrc/zhseqr.hip -o zeig_host_check && ./zeig_host_check
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
int nd4_zunmtr(nd4hip_handle*, int64_t, int64_t, int64_t, bool, const double*, const double*, double*) { return ND4HIP_ERR_HIP; }
int zlu_update_launch(nd4hip_handle*, int64_t, const ZluUpd&) { return ND4HIP_ERR_HIP; }
int64_t nd4_zunmtr_ws_elems(int64_t N, int64_t K) { return N <= 96 ? 0 : 2 * N * 64 + 2 * 64 * 64 + 2 * 64 * K; }   // hetrd.hip's
int nd4_zgemm(nd4hip_handle*, bool, int64_t, int64_t, int64_t, int64_t, const double*, int64_t, const double*, int64_t, double*) { return ND4HIP_ERR_HIP; }

#define EXPECT(cond) do { if (!(cond)) { std::printf("FAILED line %d: %s (last error: %s)\n", __LINE__, #cond, g_err); return 1; } } while (0)

int main() {
  alignas(16) double buf[4];
  const void *P = buf, *Z = nullptr;
  // the order of the checks: selectors, negative extent, the shape, empty call, NULL pointer
  EXPECT(nd4_args_zgehrd(-1, 4, Z, Z, Z) == ND4HIP_ERR_ARG && std::strstr(g_err, "nd4hip_zgehrd_batched: negative extent"));
  EXPECT(nd4_args_zgehrd(0, 2049, Z, Z, Z) == ND4HIP_ERR_ARG && std::strstr(g_err, "N <= 2048") && nd4_args_zgehrd(0, 4, Z, Z, Z) == ND4_ARGS_EMPTY);
  EXPECT(nd4_args_zgehrd(1, 4, P, P, P) == ND4_ARGS_GO && nd4_args_zgehrd(1, 4, P, P, Z) == ND4HIP_ERR_ARG && nd4_args_zgehrd(1, 1, P, P, Z) == ND4_ARGS_GO);
  EXPECT(nd4_args_zunmhr(1, 4, 2, 2, P, P, P) == ND4HIP_ERR_ARG && std::strstr(g_err, "adjoint must be 0 or 1"));
  EXPECT(nd4_args_zunmhr(1, 4, 2, 1, P, P, P) == ND4_ARGS_GO && nd4_args_zunmhr(1, 4, 0, 0, Z, Z, Z) == ND4_ARGS_EMPTY && nd4_args_zunmhr(1, 2049, 2, 0, P, P, P) == ND4HIP_ERR_ARG);
  EXPECT(nd4_args_zunmhr(1, 4, 2, 0, P, P, Z) == ND4HIP_ERR_ARG && nd4_args_zunmhr(1, 4, (int64_t)65535 * 64 + 1, 0, P, P, P) == ND4HIP_ERR_ARG);
  EXPECT(nd4_args_zhseqr(1, 4, 1, P, P, P, P) == ND4_ARGS_GO && nd4_args_zhseqr(1, 4, 0, Z, P, Z, P) == ND4_ARGS_GO && nd4_args_zhseqr(1, 4, 0, P, P, P, P) == ND4HIP_ERR_ARG);
  EXPECT(nd4_args_zhseqr(1, 4, 2, P, P, P, P) == ND4HIP_ERR_ARG && nd4_args_zhseqr(1, 1025, 1, P, P, P, P) == ND4HIP_ERR_ARG && std::strstr(g_err, "N <= 1024"));
  EXPECT(nd4_args_zgees(1, 4, P, P, P) == ND4_ARGS_GO && nd4_args_zgees(1, 4, P, Z, P) == ND4HIP_ERR_ARG && nd4_args_zgees(1, 1025, P, P, P) == ND4HIP_ERR_ARG);
  EXPECT(nd4_args_ztrevc(1, 4, P, P, P, P) == ND4_ARGS_GO && nd4_args_ztrevc(1, 4, P, P, P, Z) == ND4HIP_ERR_ARG && nd4_args_ztrevc(2, 0, Z, Z, Z, Z) == ND4_ARGS_EMPTY);
  EXPECT(nd4_args_zgeev(1, 4, P, P, Z) == ND4_ARGS_GO && nd4_args_zgeev(1, 4, P, Z, P) == ND4HIP_ERR_ARG && nd4_args_zgeev(1, 1025, P, P, P) == ND4HIP_ERR_ARG);
  // tiers: what each kernel keeps in LDS fits 163840 B; the edges of the file headers
  const size_t LDS = 163840;
  for (int64_t N = 1; N <= 2048; ++N) {
    const size_t small = 16 * (size_t)(N * (N | 1) + 7 * N + 256) + 96;
    EXPECT(nd4_zgehrd_tier(N) == (small <= LDS ? 0 : 1) && nd4_zgehrd_lds(N) == (small <= LDS ? small : 48 * (size_t)N) && nd4_zgehrd_lds(N) <= LDS);
    EXPECT(nd4_zgehrd_ws_elems(N) == (small <= LDS ? 0 : 6 * N + 2 * ((N + 63) / 64) * N));
    if (N > 1024) continue;
    const int rows = nd4_zhseqr_tile_rows(N), tier = nd4_zhseqr_tier(N);
    EXPECT(rows == (tier ? 256 : N <= 16 ? 16 : N <= 32 ? 32 : 64));
    EXPECT(nd4_zhseqr_lds(N) == 24 * (size_t)N + 528 * (size_t)rows + (tier ? 0 : 16 * (size_t)(N * (N | 1))) && nd4_zhseqr_lds(N) <= LDS);
  }
  EXPECT(nd4_zgehrd_tier(95) == 0 && nd4_zgehrd_tier(96) == 1 && nd4_zgehrd_lds(95) == 159232 && nd4_zgehrd_lds(2048) == 98304);
  EXPECT(nd4_ztrevc_tier(1) == 0 && nd4_ztrevc_tier(64) == 0 && nd4_ztrevc_tier(65) == 1 && nd4_ztrevc_tier(1024) == 1);
  EXPECT(nd4_zeig_chunk(70000, 0) == 32768 && nd4_zeig_chunk(5, 2 * 1024 * 1024) == 5 && nd4_zeig_chunk(100, 2 * 1024 * 1024) == 32);
  EXPECT(nd4_zhseqr_tier(89) == 0 && nd4_zhseqr_tier(90) == 1 && nd4_zhseqr_lds(89) == 162664 && nd4_zhseqr_lds(1024) == 159744);
  // passes: every member is taken once, a pass fits a grid dimension and its workspace about 1 GiB (one member may exceed it)
  const int64_t batches[] = {1, 2, 33, 32767, 32768, 32769, 70000, 1000000};
  for (int64_t N : {(int64_t)4, (int64_t)95, (int64_t)96, (int64_t)700, (int64_t)2048})
    for (int64_t batch : batches)
      for (int64_t extra : {(int64_t)0, N * N, 3 * N * N + N}) {
        const int64_t chunk = nd4_zgehrd_chunk(batch, N, extra);
        EXPECT(chunk >= 1 && chunk <= batch && chunk <= 32768);
        if (chunk > 1 && extra) EXPECT((size_t)chunk * (size_t)(extra + nd4_zgehrd_ws_elems(N)) * 16 <= ((size_t)1 << 30));
        int64_t seen = 0;
        for (int64_t b0 = 0; b0 < batch; b0 += chunk) seen += batch - b0 < chunk ? batch - b0 : chunk;
        EXPECT(seen == batch);
      }
  // the drivers' refusals, and their stop at the stub allocator before anything is launched
  nd4hip_handle h;
  EXPECT(nd4_zgehrd_run(&h, 1, 2049, buf, buf, buf, "x: A", 0, nullptr) == ND4HIP_ERR_ARG && nd4_zgehrd_run(&h, 1, 4, buf, buf, buf, "x: A", 0, nullptr) == ND4HIP_ERR_HIP);
  EXPECT(nd4_zunmhr(&h, 1, 4, 2, true, buf + 1, buf, buf) == ND4HIP_ERR_ARG && std::strstr(g_err, "16-byte aligned"));
  EXPECT(nd4_zunmhr(&h, 3, 1, 2, false, buf, buf, buf) == 0 && nd4_zunmhr(&h, 1, 200, 2, false, buf, buf, buf) == ND4HIP_ERR_HIP);
  EXPECT(nd4_zhseqr_run(&h, 1, 1025, buf, buf, buf, buf, true, "x: H", 0, nullptr) == ND4HIP_ERR_ARG && nd4_zhseqr_run(&h, 1, 4, buf, buf, buf, buf, true, "x: H", 0, nullptr) == ND4HIP_ERR_HIP);
  EXPECT(nd4_zgees_run(&h, 1, 4, buf, buf + 1, buf, "x: A", 0, nullptr) == ND4HIP_ERR_ARG && nd4_zgees_run(&h, 1, 200, buf, buf, buf, "x: A", 0, nullptr) == ND4HIP_ERR_HIP);
  EXPECT(nd4_ztrevc_run(&h, 1, 4, buf, buf, buf, buf, "x: T", 0, nullptr) == ND4HIP_ERR_HIP && nd4_zgeev_run(&h, 1, 4, buf, buf, nullptr, "x: A", 0, nullptr) == ND4HIP_ERR_HIP);
  EXPECT(nd4_zgeev_run(&h, 1, 1025, buf, buf, buf, "x: A", 0, nullptr) == ND4HIP_ERR_ARG);
  std::printf("zeig host check ok\n");
  return 0;
}
