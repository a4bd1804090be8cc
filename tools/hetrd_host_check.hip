// Stand-alone host check of csrc/hetrd.hip: the argument checkers of its four operations (nd4hip_args.h), the tier choice and the
// LDS / workspace arithmetic for every N in 1 .. 2048, for AddressSanitizer + UBSan on the CPU. Nothing is launched and no device is
// needed: the few library functions that hetrd.hip's launchers would call are stubs that fail. Build and run from the repository root:
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         -fsanitize=address,undefined tools/hetrd_host_check.hip nd4js_amd/csrc/hetrd.hip -o hetrd_host_check && ./hetrd_host_check
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
int nd4_zgemm(nd4hip_handle*, bool, int64_t, int64_t, int64_t, int64_t, const double*, int64_t, const double*, int64_t, double*) { return ND4HIP_ERR_HIP; }
int nd4_stevx(nd4hip_handle*, int64_t, int64_t, int64_t, int64_t, const double*, const double*, double*, double*) { return ND4HIP_ERR_HIP; }

#define EXPECT(cond) do { if (!(cond)) { std::printf("FAILED line %d: %s (last error: %s)\n", __LINE__, #cond, g_err); return 1; } } while (0)

int main() {
  double buf[4];
  const void *P = buf, *Z = nullptr;
  // the order of the checks: negative extent, subset, N <= 2048, selector, empty call, NULL pointer
  EXPECT(nd4_args_hetrd(-1, 4096, Z, Z, Z, Z, Z) == ND4HIP_ERR_ARG && std::strstr(g_err, "negative extent"));
  EXPECT(nd4_args_hetrd(0, 2049, Z, Z, Z, Z, Z) == ND4HIP_ERR_ARG && std::strstr(g_err, "nd4hip_zhetrd_batched: N <= 2048"));
  EXPECT(nd4_args_hetrd(0, 5, Z, Z, Z, Z, Z) == ND4_ARGS_EMPTY && nd4_args_hetrd(3, 0, Z, Z, Z, Z, Z) == ND4_ARGS_EMPTY);
  EXPECT(nd4_args_hetrd(1, 1, P, P, Z, P, Z) == ND4_ARGS_GO && nd4_args_hetrd(1, 2, P, P, Z, P, P) == ND4HIP_ERR_ARG);
  EXPECT(nd4_args_hetrd(1, 2, P, P, P, P, P) == ND4_ARGS_GO && nd4_args_hetrd(1, 2, P, Z, P, P, P) == ND4HIP_ERR_ARG);
  EXPECT(nd4_args_hetrd(1, 2, Z, P, P, P, P) == ND4HIP_ERR_ARG && nd4_args_hetrd(1, 2, P, P, P, Z, P) == ND4HIP_ERR_ARG);
  EXPECT(nd4_args_unmtr(1, 2049, 1, 7, Z, Z, Z) == ND4HIP_ERR_ARG && std::strstr(g_err, "N <= 2048"));
  EXPECT(nd4_args_unmtr(0, 4, 1, 7, Z, Z, Z) == ND4HIP_ERR_ARG && std::strstr(g_err, "adjoint must be 0 or 1"));
  EXPECT(nd4_args_unmtr(1, 4, 0, 1, Z, Z, Z) == ND4_ARGS_EMPTY && nd4_args_unmtr(1, 4, 2, 0, P, Z, P) == ND4HIP_ERR_ARG);
  EXPECT(nd4_args_unmtr(1, 1, 2, 1, P, Z, P) == ND4_ARGS_GO && nd4_args_unmtr(1, 4, -2, 0, P, P, P) == ND4HIP_ERR_ARG);
  EXPECT(nd4_args_heevd(1, 2049, P, P) == ND4HIP_ERR_ARG && nd4_args_heevd(1, 0, Z, Z) == ND4_ARGS_EMPTY && nd4_args_heevd(2, 2, P, P) == ND4_ARGS_GO);
  EXPECT(nd4_args_heevd(2, 2, P, Z) == ND4HIP_ERR_ARG && std::strstr(g_err, "nd4hip_zheevd_batched: NULL pointer"));
  EXPECT(nd4_args_heevd(-2, 2, P, P) == ND4HIP_ERR_ARG && std::strstr(g_err, "negative extent"));
  EXPECT(nd4_args_heevx(1, 4, 3, 2, P, P) == ND4HIP_ERR_ARG && std::strstr(g_err, "nd4hip_zheevx_batched: subset must satisfy"));
  EXPECT(nd4_args_heevx(1, 2049, 0, 2050, P, P) == ND4HIP_ERR_ARG && std::strstr(g_err, "subset must satisfy"));
  EXPECT(nd4_args_heevx(1, 2049, 0, 1, P, P) == ND4HIP_ERR_ARG && std::strstr(g_err, "N <= 2048"));
  EXPECT(nd4_args_heevx(1, 4, 2, 2, Z, Z) == ND4_ARGS_EMPTY && nd4_args_heevx(1, 4, 0, 4, P, P) == ND4_ARGS_GO);
  EXPECT(nd4_args_heevx(1, 4, 0, 4, P, Z) == ND4HIP_ERR_ARG && std::strstr(g_err, "NULL pointer"));
  // tiers and their arithmetic over every N the entry points admit; 163840 B is the CU's LDS
  const size_t LDS = 163840;
  int64_t cap = 0;
  for (int64_t N = 1; N <= 2048; ++N) {
    const int tier = nd4_hetrd_tier(N);
    EXPECT(tier == (N <= 96 ? 0 : 1));
    if (tier == 0) cap = N;
    const size_t lds = nd4_hetrd_lds(N), zlds = nd4_zunmtr_lds(N);
    EXPECT(lds % 16 == 0 && lds <= LDS && zlds % 16 == 0 && zlds <= LDS);
    if (tier == 0) {
      // the square at an odd pitch, v, w, the 2 x 128 partial sums, 8 doubles and 4 words of reductions: all inside the request
      EXPECT(lds >= 16 * (size_t)(N * (N | 1) + 2 * N + 256) + 8 * 8 + 8 * 4);
      EXPECT(zlds == 16 * (size_t)(64 * N + 3 * N));
    } else {
      EXPECT(lds == 16 * (size_t)(3 * N + 512) + 64 && zlds == 0);
    }
    const int64_t nblk = nd4_hetrd_blocks(N);
    EXPECT(nblk >= 1 && (nblk - 1) * 64 < N && N <= nblk * 64);
    EXPECT(nd4_hetrd_ws_bytes(N) == (size_t)(N * (16 + 16 * (4 + 2 * nblk))));
  }
  EXPECT(cap == 96);
  EXPECT(nd4_hetrd_lds(96) == 16 * (size_t)(96 * 97 + 2 * 96 + 264) && nd4_hetrd_lds(96) == 156288 && nd4_hetrd_lds(97) == 16 * (size_t)(3 * 97 + 512) + 64);
  // the layout of tier A would fit N = 98 and no further: the cap is the round number below
  EXPECT(16 * (size_t)(98 * 99 + 2 * 98 + 264) <= LDS && 16 * (size_t)(99 * 99 + 2 * 99 + 264) > LDS);
  // the launchers refuse what the entry points never pass on, before anything is allocated or launched
  nd4hip_handle h;
  EXPECT(nd4_zunmtr(&h, 1, 2049, 1, false, buf, buf, buf) == ND4HIP_ERR_ARG && nd4_zunmtr(&h, 0, 4, 1, false, buf, buf, buf) == ND4HIP_ERR_ARG);
  EXPECT(nd4_zunmtr(&h, 1, 1, 5, true, buf, buf, buf) == 0);    // N = 1: Q = I, nothing to do
  EXPECT(nd4_hetrd(&h, 1, 2049, buf, buf, buf, buf, buf, nullptr, true, nullptr) == ND4HIP_ERR_ARG);
  EXPECT(nd4_hetrd(&h, 32769, 4, buf, buf, buf, buf, buf, nullptr, true, nullptr) == ND4HIP_ERR_ARG);
  EXPECT(nd4_hetrd_run(&h, 1, 4, buf, buf, buf, buf, buf) == ND4HIP_ERR_HIP);   // the stub allocator fails first
  EXPECT(nd4_zheevx(&h, 1, 2049, 0, 1, buf, buf, buf) == ND4HIP_ERR_ARG);
  EXPECT(nd4_zheevx(&h, 1, 4, 0, 2, buf, buf, buf) == ND4HIP_ERR_HIP);
  std::printf("hetrd host check ok\n");
  return 0;
}
