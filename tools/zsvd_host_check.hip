// Stand-alone host check of csrc/zgebrd.hip: the argument checkers of its three operations (nd4hip_args.h), the tier choice, the LDS
// requests and the QR-first rule for every 1 <= N <= M <= 2048 that can change them, and the pass arithmetic, for AddressSanitizer +
// UBSan on the CPU. Nothing is launched and no device is needed: the library functions that the drivers would call are stubs that
// fail. Build and run from the repository root:
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         -fsanitize=address,undefined tools/zsvd_host_check.hip nd4js_amd/csrc/zgebrd.hip -o zsvd_host_check && ./zsvd_host_check
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
int nd4_zgeqrf(nd4hip_handle*, int64_t, int64_t, int64_t, const double*, double*, double*) { return ND4HIP_ERR_HIP; }
int nd4_zunmqr(nd4hip_handle*, int64_t, int64_t, int64_t, int64_t, bool, const double*, int64_t, const double*, int64_t, double*) { return ND4HIP_ERR_HIP; }
int nd4_bdsdc_rows(nd4hip_handle*, int64_t, int64_t, int64_t, const double*, const double*, double*, double*, double*) { return ND4HIP_ERR_HIP; }
int nd4_bdsvdx(nd4hip_handle*, int64_t, int64_t, int64_t, int64_t, int64_t, const double*, const double*, double*, double*, double*, int32_t*) {
  return ND4HIP_ERR_HIP;
}
int nd4_hetrd_rows_to_columns(nd4hip_handle*, int64_t, int, int, const double*, double*) { return ND4HIP_ERR_HIP; }

#define EXPECT(cond) do { if (!(cond)) { std::printf("FAILED line %d: %s (last error: %s)\n", __LINE__, #cond, g_err); return 1; } } while (0)

int main() {
  alignas(16) double buf[4];
  const void *P = buf, *Z = nullptr;
  // the order of the checks: selectors, negative extent, strides, the shape, the subset, empty call, NULL pointer
  EXPECT(nd4_args_zgebrd(-1, 4, 3, Z, Z, Z, Z, Z, Z) == ND4HIP_ERR_ARG && std::strstr(g_err, "nd4hip_zgebrd_batched: negative extent"));
  EXPECT(nd4_args_zgebrd(0, 2049, 3, Z, Z, Z, Z, Z, Z) == ND4HIP_ERR_ARG && std::strstr(g_err, "N <= M <= 2048"));
  EXPECT(nd4_args_zgebrd(0, 3, 4, Z, Z, Z, Z, Z, Z) == ND4HIP_ERR_ARG && nd4_args_zgebrd(0, 4, 3, Z, Z, Z, Z, Z, Z) == ND4_ARGS_EMPTY);
  EXPECT(nd4_args_zgebrd(1, 4, 3, P, P, P, P, P, P) == ND4_ARGS_GO && nd4_args_zgebrd(1, 4, 3, P, P, P, P, P, Z) == ND4HIP_ERR_ARG);
  EXPECT(nd4_args_zgebrd(1, 4, 1, P, P, P, P, P, Z) == ND4_ARGS_GO && nd4_args_zgebrd(1, 4, 3, P, P, Z, P, P, P) == ND4HIP_ERR_ARG);
  EXPECT(nd4_args_zunmbr_p(2, 4, 3, 2, 0, P, 12, P, 3, P) == ND4_ARGS_GO && nd4_args_zunmbr_p(2, 4, 3, 2, 1, P, 0, P, 0, P) == ND4_ARGS_GO);
  EXPECT(nd4_args_zunmbr_p(2, 4, 3, 2, 2, P, 12, P, 3, P) == ND4HIP_ERR_ARG && std::strstr(g_err, "adjoint must be 0 or 1"));
  EXPECT(nd4_args_zunmbr_p(2, 4, 3, 2, 0, P, 12, P, 0, P) == ND4HIP_ERR_ARG && nd4_args_zunmbr_p(2, 4, 3, 2, 0, P, 13, P, 3, P) == ND4HIP_ERR_ARG);
  EXPECT(nd4_args_zunmbr_p(2, 3, 4, 2, 0, P, 12, P, 4, P) == ND4HIP_ERR_ARG && nd4_args_zunmbr_p(2, 4, 3, 0, 0, Z, 12, Z, 3, Z) == ND4_ARGS_EMPTY);
  EXPECT(nd4_args_zgesdd(1, 4, 3, 0, 3, 1, P, P, P, P) == ND4_ARGS_GO && nd4_args_zgesdd(1, 3, 4, 1, 2, 0, P, Z, P, Z) == ND4_ARGS_GO);
  EXPECT(nd4_args_zgesdd(1, 2049, 3, 0, 3, 1, P, P, P, P) == ND4HIP_ERR_ARG && nd4_args_zgesdd(1, 3, 2049, 0, 3, 1, P, P, P, P) == ND4HIP_ERR_ARG);
  EXPECT(nd4_args_zgesdd(1, 4, 3, 0, 4, 1, P, P, P, P) == ND4HIP_ERR_ARG && std::strstr(g_err, "subset must satisfy"));
  EXPECT(nd4_args_zgesdd(1, 4, 3, 2, 2, 1, Z, Z, Z, Z) == ND4_ARGS_EMPTY && nd4_args_zgesdd(1, 4, 3, 0, 3, 2, P, P, P, P) == ND4HIP_ERR_ARG);
  EXPECT(nd4_args_zgesdd(1, 4, 3, 0, 3, 1, P, Z, P, P) == ND4HIP_ERR_ARG && nd4_args_zgesdd(1, 4, 3, 0, 3, 0, P, P, P, Z) == ND4HIP_ERR_ARG);
  // tiers: the member, v, z, w, u and the partial dot products fit 163840 B; above, the column of L_k and w, u of R_k
  const size_t LDS = 163840;
  for (int64_t N = 1; N <= 2048; ++N)
    for (int64_t M = N; M <= 2048; M += (M < 160 || M % 256 > 253) ? 1 : 97) {
      const size_t small = 16 * (size_t)(M * (N | 1) + 2 * M + 6 * N + 256) + 96, big = 16 * (size_t)M > 32 * (size_t)N ? 16 * (size_t)M : 32 * (size_t)N;
      EXPECT(nd4_zgebrd_tier(M, N) == (small <= LDS ? 0 : 1));
      EXPECT(nd4_zgebrd_lds(M, N) == (small <= LDS ? small : big) && nd4_zgebrd_lds(M, N) <= LDS);
      EXPECT(nd4_zgesdd_qr_first(M, N) == (M > N && 3 * M >= 5 * N));
    }
  EXPECT(nd4_zgebrd_tier(95, 95) == 0 && nd4_zgebrd_tier(96, 96) == 1 && nd4_zgebrd_tier(2048, 1) == 0 && nd4_zgebrd_tier(2048, 3) == 1);
  EXPECT(nd4_zgebrd_lds(2048, 2048) == 65536 && !nd4_zgesdd_qr_first(100, 70) && nd4_zgesdd_qr_first(150, 60) && !nd4_zgesdd_qr_first(7, 7));
  // passes: every member is taken once, a pass fits a grid dimension and its workspace about 1 GiB (one member may exceed it)
  const int64_t batches[] = {1, 2, 33, 32767, 32768, 32769, 70000, 1000000};
  const int64_t shapes[][2] = {{4, 4}, {95, 95}, {96, 96}, {700, 130}, {2048, 256}, {2048, 2048}};
  for (const auto& s : shapes)
    for (int64_t batch : batches)
      for (int64_t extra : {(int64_t)0, s[0] * s[1] + s[1], 4 * s[0] * s[1] + 4 * s[1]}) {
        const int64_t chunk = nd4_zgebrd_chunk(batch, s[0], s[1], extra);
        EXPECT(chunk >= 1 && chunk <= batch && chunk <= 32768);
        if (chunk > 1 && extra) EXPECT((size_t)chunk * (size_t)extra * 16 <= ((size_t)1 << 30));
        int64_t seen = 0;
        for (int64_t b0 = 0; b0 < batch; b0 += chunk) seen += batch - b0 < chunk ? batch - b0 : chunk;
        EXPECT(seen == batch);
      }
  EXPECT(nd4_zgebrd_chunk(70000, 4, 4, 0) == 32768 && nd4_zgebrd_chunk(5, 2048, 2048, 0) == 5);
  // the drivers' refusals, and their stop at the stub allocator before anything is launched
  nd4hip_handle h;
  EXPECT(nd4_zgebrd(&h, 1, 3, 4, buf, buf, buf, buf, buf, buf, "x") == ND4HIP_ERR_ARG && nd4_zgebrd(&h, 1, 2049, 4, buf, buf, buf, buf, buf, buf, "x") == ND4HIP_ERR_ARG);
  EXPECT(nd4_zgebrd(&h, 1, 4, 3, buf + 1, buf, buf, buf, buf, buf, "x") == ND4HIP_ERR_ARG && std::strstr(g_err, "16-byte aligned"));
  EXPECT(nd4_zgebrd(&h, 1, 200, 140, buf, buf, buf, buf, buf, buf, "x") == ND4HIP_ERR_HIP && nd4_zgebrd(&h, 1, 4, 3, buf, buf, buf, buf, buf, buf, "x") == ND4HIP_ERR_HIP);
  EXPECT(nd4_zunmbr_p(&h, 1, 4, 3, 2, true, buf, 12, buf, 3, buf) == ND4HIP_ERR_HIP && nd4_zunmbr_p(&h, 1, 3, 4, 2, true, buf, 12, buf, 4, buf) == ND4HIP_ERR_ARG);
  EXPECT(nd4_zunmbr_p(&h, 3, 4, 1, 2, false, buf, 0, buf, 0, buf) == 0);   // P = I: nothing to do
  EXPECT(nd4_zgesdd(&h, 1, 4, 3, 0, 3, buf, buf, buf, buf) == ND4HIP_ERR_HIP && nd4_zgesdd(&h, 1, 3, 2049, 0, 3, buf, buf, buf, buf) == ND4HIP_ERR_ARG);
  std::printf("zsvd host check ok\n");
  return 0;
}
