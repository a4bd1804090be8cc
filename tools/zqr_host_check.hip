// Stand-alone host check of csrc/zgeqrf.hip: the argument checkers of its four operations (nd4hip_args.h), the tier choice and the LDS
// requests for every 1 <= N <= M <= 2048 that can change them, and the pass arithmetic, for AddressSanitizer + UBSan on the CPU.
// Nothing is launched and no device is needed: the few library functions that the drivers would call are stubs that fail. Build and
// run from the repository root:
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         -fsanitize=address,undefined tools/zqr_host_check.hip nd4js_amd/csrc/zgeqrf.hip nd4js_amd/csrc/zgetrf.hip -o zqr_host_check && ./zqr_host_check
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
  const void *P = buf, *Z = nullptr;
  // the order of the checks: selector and strides, negative extent, the shape, K, empty call, NULL pointer
  EXPECT(nd4_args_zgeqrf(-1, 4, 3, Z, Z, Z) == ND4HIP_ERR_ARG && std::strstr(g_err, "nd4hip_zgeqrf_batched: negative extent"));
  EXPECT(nd4_args_zgeqrf(0, 2049, 3, Z, Z, Z) == ND4HIP_ERR_ARG && std::strstr(g_err, "N <= M <= 2048"));
  EXPECT(nd4_args_zgeqrf(0, 3, 4, Z, Z, Z) == ND4HIP_ERR_ARG && nd4_args_zgeqrf(0, 4, 3, Z, Z, Z) == ND4_ARGS_EMPTY && nd4_args_zgeqrf(2, 4, 0, Z, Z, Z) == ND4_ARGS_EMPTY);
  EXPECT(nd4_args_zgeqrf(1, 4, 3, P, P, P) == ND4_ARGS_GO && nd4_args_zgeqrf(1, 4, 3, P, P, Z) == ND4HIP_ERR_ARG && std::strstr(g_err, "NULL pointer"));
  EXPECT(nd4_args_zungqr(1, 4, 4, P, P, P) == ND4_ARGS_GO && nd4_args_zungqr(1, 4, 5, P, P, P) == ND4HIP_ERR_ARG && nd4_args_zungqr(1, 4, 4, P, Z, P) == ND4HIP_ERR_ARG);
  EXPECT(nd4_args_zunmqr(2, 4, 3, 2, 0, P, 12, P, 3, P) == ND4_ARGS_GO && nd4_args_zunmqr(2, 4, 3, 2, 1, P, 0, P, 0, P) == ND4_ARGS_GO);
  EXPECT(nd4_args_zunmqr(2, 4, 3, 2, 2, P, 12, P, 3, P) == ND4HIP_ERR_ARG && std::strstr(g_err, "adjoint must be 0 or 1"));
  EXPECT(nd4_args_zunmqr(2, 4, 3, 2, 0, P, 12, P, 0, P) == ND4HIP_ERR_ARG && nd4_args_zunmqr(2, 4, 3, 2, 0, P, 13, P, 3, P) == ND4HIP_ERR_ARG);
  EXPECT(nd4_args_zunmqr(2, 4, 3, 0, 0, Z, 12, Z, 3, Z) == ND4_ARGS_EMPTY && nd4_args_zunmqr(2, 4, 3, (int64_t)65535 * 64 + 1, 0, P, 12, P, 3, P) == ND4HIP_ERR_ARG);
  EXPECT(nd4_args_zgels(2, 4, 3, 2, P, 12, Z, P, P) == ND4_ARGS_GO && nd4_args_zgels(2, 4, 3, 2, P, 0, P, P, P) == ND4_ARGS_GO);
  EXPECT(nd4_args_zgels(2, 4, 3, 2, P, 0, Z, P, P) == ND4HIP_ERR_ARG && std::strstr(g_err, "strideA must be M*N"));
  EXPECT(nd4_args_zgels(2, 4, 3, 2, P, 12, Z, Z, P) == ND4HIP_ERR_ARG && nd4_args_zgels(2, 4, 3, 2, P, 12, Z, P, Z) == ND4HIP_ERR_ARG);
  // tiers: the factorisation fits 163840 B and M <= 152, where the tile of zqr_apply_q fits for every N
  const size_t LDS = 163840;
  for (int64_t N = 1; N <= 2048; ++N)
    for (int64_t M = N; M <= 2048; M += (M < 160 || M % 256 > 253) ? 1 : 97) {
      const size_t fac = 16 * (size_t)(M * (N | 1) + M + 5 * N + 256) + 96, app = 16 * (size_t)(66 * M + N);
      EXPECT(nd4_zgeqrf_tier(M, N) == (fac <= LDS && M <= 152 ? 0 : 1) && (M > 152 || app <= LDS));
      EXPECT(nd4_zgeqrf_lds(M, N) == (nd4_zgeqrf_tier(M, N) == 0 ? (fac > app ? fac : app) : 0) && nd4_zgeqrf_lds(M, N) <= LDS);
    }
  EXPECT(nd4_zgeqrf_tier(96, 96) == 0 && nd4_zgeqrf_tier(97, 97) == 1 && nd4_zgeqrf_tier(152, 1) == 0 && nd4_zgeqrf_tier(153, 1) == 1);
  // passes: every member is taken once, a pass fits a grid dimension and its workspace 1 GiB (one member may exceed it)
  const int64_t batches[] = {1, 2, 33, 32767, 32768, 32769, 70000, 1000000};
  const int64_t shapes[][2] = {{4, 4}, {96, 96}, {153, 17}, {700, 130}, {2048, 256}, {2048, 2048}};
  for (const auto& s : shapes)
    for (int64_t batch : batches)
      for (int64_t extra : {(int64_t)0, s[0] * s[1] + s[1], 2 * s[0] * s[1] + s[1] + 1}) {
        const int64_t chunk = nd4_zgeqrf_chunk(batch, s[0], s[1], s[1], extra);
        EXPECT(chunk >= 1 && chunk <= batch && chunk <= 32768);
        if (chunk > 1 && extra) EXPECT((size_t)chunk * (size_t)extra * 16 <= ((size_t)1 << 30));
        int64_t seen = 0;
        for (int64_t b0 = 0; b0 < batch; b0 += chunk) seen += batch - b0 < chunk ? batch - b0 : chunk;
        EXPECT(seen == batch);
      }
  EXPECT(nd4_zgeqrf_chunk(70000, 4, 4, 4, 0) == 32768 && nd4_zgeqrf_chunk(5, 2048, 2048, 2048, 0) == 5);
  // the drivers' refusals, and their stop at the stub allocator before anything is launched
  nd4hip_handle h;
  EXPECT(nd4_zgeqrf(&h, 1, 3, 4, buf, buf, buf) == ND4HIP_ERR_ARG && nd4_zgeqrf(&h, 1, 2049, 4, buf, buf, buf) == ND4HIP_ERR_ARG);
  EXPECT(nd4_zgeqrf(&h, 1, 4, 3, buf + 1, buf, buf) == ND4HIP_ERR_ARG && std::strstr(g_err, "16-byte aligned"));
  EXPECT(nd4_zgeqrf(&h, 1, 200, 40, buf, buf, buf) == ND4HIP_ERR_HIP && nd4_zungqr(&h, 1, 4, 3, buf, buf, buf) == ND4HIP_ERR_HIP);
  EXPECT(nd4_zunmqr(&h, 1, 200, 40, 2, true, buf, 0, buf, 0, buf) == ND4HIP_ERR_HIP && nd4_zgels(&h, 1, 4, 3, 1, buf, 12, nullptr, buf, buf, nullptr, 0, nullptr) == ND4HIP_ERR_HIP);
  EXPECT(nd4_zgels(&h, 1, 4, 5, 1, buf, 20, nullptr, buf, buf, nullptr, 0, nullptr) == ND4HIP_ERR_ARG);
  std::printf("zqr host check ok\n");
  return 0;
}
