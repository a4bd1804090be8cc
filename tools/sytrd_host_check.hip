// Stand-alone host check of csrc/sytrd.hip: the argument checkers of its four operations (nd4hip_args.h), the tier choice and the
// LDS / workspace arithmetic, for AddressSanitizer + UBSan on the CPU. Nothing is launched and no device is needed: the few library
// functions that sytrd.hip's launchers would call are stubs that fail. Build and run from the repository root:
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         -fsanitize=address,undefined tools/sytrd_host_check.hip nd4js_amd/csrc/sytrd.hip -o sytrd_host_check && ./sytrd_host_check
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
int nd4_gemm(nd4hip_handle*, bool, bool, int64_t, int64_t, int64_t, double, const double*, int64_t, int64_t, const double*, int64_t, int64_t, double,
             double*, int64_t, int64_t, int64_t) { return ND4HIP_ERR_HIP; }

#define EXPECT(cond) do { if (!(cond)) { std::printf("FAILED line %d: %s (last error: %s)\n", __LINE__, #cond, g_err); return 1; } } while (0)

int main() {
  double buf[4];
  const void *P = buf, *Z = nullptr;
  // the order of the checks: negative extent, N <= 2048, selector / subset, empty call, NULL pointer
  EXPECT(nd4_args_sytrd(-1, 4096, Z, Z, Z, Z, Z) == ND4HIP_ERR_ARG && std::strstr(g_err, "negative extent"));
  EXPECT(nd4_args_sytrd(0, 2049, Z, Z, Z, Z, Z) == ND4HIP_ERR_ARG && std::strstr(g_err, "N <= 2048"));
  EXPECT(nd4_args_sytrd(0, 5, Z, Z, Z, Z, Z) == ND4_ARGS_EMPTY && nd4_args_sytrd(3, 0, Z, Z, Z, Z, Z) == ND4_ARGS_EMPTY);
  EXPECT(nd4_args_sytrd(1, 1, P, P, Z, P, Z) == ND4_ARGS_GO && nd4_args_sytrd(1, 2, P, P, Z, P, P) == ND4HIP_ERR_ARG);
  EXPECT(nd4_args_sytrd(1, 2, P, P, P, P, P) == ND4_ARGS_GO && nd4_args_sytrd(1, 2, P, Z, P, P, P) == ND4HIP_ERR_ARG);
  EXPECT(nd4_args_ormtr(1, 2049, 1, 7, Z, Z, Z) == ND4HIP_ERR_ARG && std::strstr(g_err, "N <= 2048"));
  EXPECT(nd4_args_ormtr(0, 4, 1, 7, Z, Z, Z) == ND4HIP_ERR_ARG && std::strstr(g_err, "transpose must be 0 or 1"));
  EXPECT(nd4_args_ormtr(1, 4, 0, 1, Z, Z, Z) == ND4_ARGS_EMPTY && nd4_args_ormtr(1, 4, 2, 0, P, Z, P) == ND4HIP_ERR_ARG);
  EXPECT(nd4_args_ormtr(1, 1, 2, 1, P, Z, P) == ND4_ARGS_GO && nd4_args_ormtr(1, 4, -2, 0, P, P, P) == ND4HIP_ERR_ARG);
  EXPECT(nd4_args_syevd_tr(1, 2049, P, P) == ND4HIP_ERR_ARG && nd4_args_syevd_tr(1, 0, Z, Z) == ND4_ARGS_EMPTY && nd4_args_syevd_tr(2, 2, P, P) == ND4_ARGS_GO);
  EXPECT(nd4_args_syevd_tr(2, 2, P, Z) == ND4HIP_ERR_ARG && std::strstr(g_err, "nd4hip_dsyevd_tr_batched: NULL pointer"));
  EXPECT(nd4_args_syevx_tr(1, 4, 3, 2, P, P) == ND4HIP_ERR_ARG && std::strstr(g_err, "subset must satisfy"));
  EXPECT(nd4_args_syevx_tr(1, 4, 2, 2, Z, Z) == ND4_ARGS_EMPTY && nd4_args_syevx_tr(1, 4, 0, 4, P, P) == ND4_ARGS_GO);
  // tiers and their arithmetic over every N the entry points admit
  for (int64_t N = 1; N <= 2048; ++N) {
    const int tier = nd4_sytrd_tier(N);
    EXPECT(tier == (N <= 128 ? 0 : 1));
    const size_t lds = nd4_sytrd_lds(N);
    EXPECT(lds % 8 == 0 && lds <= 160 * 1024);                 // the CU's LDS
    if (tier == 0) EXPECT(lds >= 8 * (size_t)(N * (N | 1) + 2 * N + 264));
    else EXPECT(lds == 8 * (size_t)(7 * N + 4));
    const int64_t nblk = nd4_sytrd_blocks(N);
    EXPECT(nblk >= 1 && (nblk - 1) * 64 < N && N <= nblk * 64);
    EXPECT(nd4_sytrd_ws_doubles(N) == (size_t)(N * (6 + 2 * nblk)));
  }
  EXPECT(nd4_sytrd_lds(128) == 8 * (size_t)(128 * 129 + 3 * 128 + 264) && nd4_sytrd_lds(129) == 8 * (size_t)(7 * 129 + 4));
  // the launchers refuse what the entry points never pass on, before anything is allocated or launched
  nd4hip_handle h;
  EXPECT(nd4_ormtr(&h, 1, 2049, 1, false, buf, buf, buf) == ND4HIP_ERR_ARG && nd4_ormtr(&h, 0, 4, 1, false, buf, buf, buf) == ND4HIP_ERR_ARG);
  EXPECT(nd4_ormtr(&h, 1, 2, 5, true, buf, buf, buf) == 0);     // N <= 2: Q = I, nothing to do
  EXPECT(nd4_sytrd_run(&h, 1, 4, buf, buf, buf, buf, buf) == ND4HIP_ERR_HIP);   // the stub allocator fails first
  std::printf("sytrd host check ok\n");
  return 0;
}
