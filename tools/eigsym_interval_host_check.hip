// Stand-alone host check of the interval forms of csrc/syevx.hip: their argument checkers (nd4hip_args.h), the
// bounds check of the host forms, kmax from the ranges that are read back, the kcap refusal and the grid arithmetic, for
// AddressSanitizer + UBSan on the CPU. The workspace sizes are not covered: they are written where they are allocated (stx_solve,
// stx_interval), as products of batch, N and kmax in size_t, and no host function computes them apart from the allocation.
// Nothing is launched and no device is needed: the library functions that syevx.hip's launchers would call are stubs that fail.
// Build and run from the repository root:
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=undefined -fsanitize=address,undefined tools/eigsym_interval_host_check.hip \
//         nd4js_amd/csrc/syevx.hip -o eigsym_interval_host_check && ./eigsym_interval_host_check
#include "../nd4js_amd/csrc/syev_internal.h"
#include "../nd4js_amd/csrc/nd4hip_args.h"
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

static char g_err[256];
void nd4_set_error(const char* fmt, ...) { va_list ap; va_start(ap, fmt); vsnprintf(g_err, sizeof g_err, fmt, ap); va_end(ap); }
int nd4_hip_fail(hipError_t, const char*, const char*, int) { return ND4HIP_ERR_HIP; }
int nd4_ws_alloc(nd4hip_handle*, size_t, void**) { return ND4HIP_ERR_HIP; }
int nd4_pinned(nd4hip_handle*, size_t, void**) { return ND4HIP_ERR_HIP; }
Nd4WsScope::Nd4WsScope(nd4hip_handle* hh) : h(hh), nblocks(0), used_last(0), generation(0) {}
Nd4WsScope::~Nd4WsScope() {}
int nd4_gemm(nd4hip_handle*, bool, bool, int64_t, int64_t, int64_t, double, const double*, int64_t, int64_t, const double*, int64_t, int64_t, double,
             double*, int64_t, int64_t, int64_t) { return ND4HIP_ERR_HIP; }
int nd4_gehrd(nd4hip_handle*, int64_t, int64_t, const double*, double*, double*) { return ND4HIP_ERR_HIP; }
int nd4_ormtr(nd4hip_handle*, int64_t, int64_t, int64_t, bool, const double*, const double*, double*) { return ND4HIP_ERR_HIP; }
int nd4_transpose(nd4hip_handle*, int64_t, int64_t, const double*, int64_t, double*, int64_t, int64_t, int64_t, int64_t) { return ND4HIP_ERR_HIP; }
int nd4_syev_symm(nd4hip_handle*, int64_t, int, const double*, double*, u64*) { return ND4HIP_ERR_HIP; }
int nd4_sytrd(nd4hip_handle*, int64_t, int64_t, const double*, double*, double*, double*, double*, u64*, bool, int*) { return ND4HIP_ERR_HIP; }
int nd4_sytrf_bk_tier(const nd4hip_handle*, int64_t, int64_t, int) { return 0; }

#define EXPECT(cond) do { if (!(cond)) { std::printf("FAILED line %d: %s (last error: %s)\n", __LINE__, #cond, g_err); return 1; } } while (0)

int main() {
  double buf[8] = {0};
  int64_t km = -1;
  const void *P = buf, *Z = nullptr, *K = &km;
  // the order of the checks: negative extent (kcap included), N <= 2048, empty call, NULL pointer
  EXPECT(nd4_args_stevxv(-1, 4096, 1, Z, Z, Z, Z, Z, Z) == ND4HIP_ERR_ARG && std::strstr(g_err, "nd4hip_dstevxv_batched: negative extent"));
  EXPECT(nd4_args_stevxv(1, 4, -1, P, P, P, P, P, K) == ND4HIP_ERR_ARG && std::strstr(g_err, "negative extent"));
  EXPECT(nd4_args_stevxv(0, 2049, 1, Z, Z, Z, Z, Z, Z) == ND4HIP_ERR_ARG && std::strstr(g_err, "N <= 2048"));
  EXPECT(nd4_args_stevxv(0, 5, 5, Z, Z, Z, Z, Z, Z) == ND4_ARGS_EMPTY && nd4_args_stevxv(3, 0, 0, Z, Z, Z, Z, Z, Z) == ND4_ARGS_EMPTY);
  EXPECT(nd4_args_stevxv(1, 1, 1, P, P, Z, P, P, K) == ND4_ARGS_GO && nd4_args_stevxv(1, 2, 1, P, P, Z, P, P, K) == ND4HIP_ERR_ARG);
  EXPECT(nd4_args_stevxv(1, 2, 2, P, P, P, P, P, Z) == ND4HIP_ERR_ARG && std::strstr(g_err, "nd4hip_dstevxv_batched: NULL pointer"));
  EXPECT(nd4_args_stevxv(1, 2, 0, P, P, P, Z, P, K) == ND4_ARGS_GO && nd4_args_stevxv(1, 2, 1, P, P, P, Z, P, K) == ND4HIP_ERR_ARG);
  for (int tr = 0; tr < 2; ++tr) {
    const char* name = tr ? "nd4hip_dsyevxv_tr_batched" : "nd4hip_dsyevxv_batched";
    EXPECT(nd4_args_syevxv(tr, 1, 2049, 1, P, P, P, P, K) == ND4HIP_ERR_ARG && std::strstr(g_err, name) && std::strstr(g_err, "N <= 2048"));
    EXPECT(nd4_args_syevxv(tr, 1, 0, 0, Z, Z, Z, Z, Z) == ND4_ARGS_EMPTY && nd4_args_syevxv(tr, 2, 3, 3, P, P, P, P, K) == ND4_ARGS_GO);
    EXPECT(nd4_args_syevxv(tr, 2, 3, 3, P, P, P, Z, K) == ND4HIP_ERR_ARG && std::strstr(g_err, name) && std::strstr(g_err, "NULL pointer"));
    EXPECT(nd4_args_syevxv(tr, 2, 3, 0, P, P, Z, P, K) == ND4_ARGS_GO);
  }
  // eigen_sym_gen's selectors: reduction, select, extents (kcap only for an interval), subset, N, strideB, empty, pointers
  EXPECT(nd4_args_sygvx(2, 0, 1, 4, 0, 0, 0, Z, P, P, 16, P, Z, Z) == ND4HIP_ERR_ARG && std::strstr(g_err, "reduction must be 0"));
  EXPECT(nd4_args_sygvx(0, 3, 1, 4, 0, 0, 0, Z, P, P, 16, P, Z, Z) == ND4HIP_ERR_ARG && std::strstr(g_err, "select must be 0"));
  EXPECT(nd4_args_sygvx(0, 0, 1, 4, 7, 3, -1, Z, P, P, 16, P, Z, Z) == ND4_ARGS_GO);          // i0, i1, kcap: not looked at for select 0
  EXPECT(nd4_args_sygvx(0, 2, 1, 4, 0, 0, -1, P, P, P, 16, P, P, K) == ND4HIP_ERR_ARG && std::strstr(g_err, "negative extent"));
  EXPECT(nd4_args_sygvx(1, 1, 1, 4, 3, 2, 0, Z, P, P, 16, P, Z, Z) == ND4HIP_ERR_ARG && std::strstr(g_err, "subset must satisfy"));
  EXPECT(nd4_args_sygvx(1, 1, 1, 2049, 0, 1, 0, Z, P, P, 0, P, Z, Z) == ND4HIP_ERR_ARG && std::strstr(g_err, "N <= 2048"));
  EXPECT(nd4_args_sygvx(1, 1, 1, 4, 0, 1, 0, Z, P, P, 15, P, Z, Z) == ND4HIP_ERR_ARG && std::strstr(g_err, "strideB must be N*N or 0"));
  EXPECT(nd4_args_sygvx(1, 1, 1, 4, 2, 2, 0, Z, Z, Z, 0, Z, Z, Z) == ND4_ARGS_EMPTY && nd4_args_sygvx(0, 2, 0, 4, 0, 0, 4, Z, Z, Z, 0, Z, Z, Z) == ND4_ARGS_EMPTY);
  EXPECT(nd4_args_sygvx(1, 1, 1, 4, 0, 2, 0, Z, P, P, 0, P, Z, Z) == ND4_ARGS_GO && nd4_args_sygvx(1, 1, 1, 4, 0, 2, 0, Z, P, Z, 0, P, Z, Z) == ND4HIP_ERR_ARG);
  EXPECT(nd4_args_sygvx(0, 2, 1, 4, 0, 0, 4, P, P, P, 16, P, P, K) == ND4_ARGS_GO && nd4_args_sygvx(0, 2, 1, 4, 0, 0, 0, P, P, P, 16, Z, P, K) == ND4_ARGS_GO);
  EXPECT(nd4_args_sygvx(0, 2, 1, 4, 0, 0, 4, Z, P, P, 16, P, P, K) == ND4HIP_ERR_ARG && nd4_args_sygvx(0, 2, 1, 4, 0, 0, 4, P, P, P, 16, P, Z, K) == ND4HIP_ERR_ARG);
  EXPECT(nd4_args_sygvx(0, 2, 1, 4, 0, 0, 4, P, P, P, 16, P, P, Z) == ND4HIP_ERR_ARG && std::strstr(g_err, "nd4hip_dsygvx_batched: NULL pointer"));
  // the bounds of the host forms: NaN and lo > hi are refused, +-Infinity and lo = hi are not
  const double inf = std::numeric_limits<double>::infinity(), nan = std::nan("");
  std::vector<double> bounds{-inf, inf, 1.0, 1.0, -2.0, inf, -inf, -inf};
  EXPECT(nd4_args_bounds("dstevxv_batched", 4, bounds.data()) == ND4_ARGS_GO);
  bounds[5] = nan;
  EXPECT(nd4_args_bounds("dstevxv_batched", 4, bounds.data()) == ND4HIP_ERR_ARG && std::strstr(g_err, "interval contains NaN"));
  EXPECT(nd4_args_bounds("dstevxv_batched", 2, bounds.data()) == ND4_ARGS_GO);
  bounds[5] = -2.5;
  EXPECT(nd4_args_bounds("dsyevxv_batched", 4, bounds.data()) == ND4HIP_ERR_ARG && std::strstr(g_err, "nd4hip_dsyevxv_batched: interval must satisfy lo <= hi"));
  // kmax from the ranges of a batch, and what it refuses: a range outside 0 <= i0 <= i1 <= N (lo > hi in device memory)
  for (int64_t batch = 1; batch <= 300; batch += 13) {
    std::vector<int32_t> range((size_t)(2 * batch));
    int64_t want = 0;
    for (int64_t b = 0; b < batch; ++b) {
      const int32_t i0 = (int32_t)((b * 7) % 41), k = (int32_t)((b * b + 3 * batch) % (41 - i0 + 1));
      range[(size_t)(2 * b)] = i0; range[(size_t)(2 * b + 1)] = i0 + k;
      want = k > want ? k : want;
    }
    km = -1;
    EXPECT(nd4_interval_kmax("dstevxv_batched", batch, 41, range.data(), &km) == ND4_ARGS_GO && km == want);
    EXPECT(nd4_args_kcap("dstevxv_batched", want, km) == ND4_ARGS_GO && nd4_args_kcap("dstevxv_batched", 41, km) == ND4_ARGS_GO);
    if (want > 0) EXPECT(nd4_args_kcap("dstevxv_batched", want - 1, km) == ND4HIP_ERR_ARG && std::strstr(g_err, "kcap = ") && std::strstr(g_err, "is less than"));
    range[(size_t)(2 * (batch / 2) + 1)] = range[(size_t)(2 * (batch / 2))] - 1;
    EXPECT(nd4_interval_kmax("dstevxv_batched", batch, 41, range.data(), &km) == ND4HIP_ERR_ARG && std::strstr(g_err, "lo <= hi"));
    range[(size_t)(2 * (batch / 2) + 1)] = 42;
    EXPECT(nd4_interval_kmax("dstevxv_batched", batch, 41, range.data(), &km) == ND4HIP_ERR_ARG);
  }
  const int32_t none[4] = {0, 0, 41, 41};
  EXPECT(nd4_interval_kmax("dstevxv_batched", 2, 41, none, &km) == ND4_ARGS_GO && km == 0 && nd4_args_kcap("dstevxv_batched", 0, km) == ND4_ARGS_GO);
  // the grids: every selected value, vector and output element has a lane, and no workgroup is launched without one
  for (int64_t k = 1; k <= 2048; ++k) {
    const int64_t nb = nd4_stx_bisect_blocks(k);
    EXPECT(nb >= 1 && (nb - 1) * 256 < k && k <= nb * 256);
    for (int64_t batch : {1, 5, 1024, 32768}) {
      const int64_t ns = nd4_stx_solve_blocks(batch, k), nr = nd4_stx_ragged_blocks(batch, 2048, k);
      EXPECT((ns - 1) * 64 < batch * k && batch * k <= ns * 64);
      EXPECT((nr - 1) * 256 < batch * 2048 * k && batch * 2048 * k <= nr * 256);
      EXPECT(nd4_stx_ragged_blocks(batch, 1, k) * 256 >= batch * k);
    }
  }
  // the launchers refuse what the entry points never pass on, before anything is allocated or launched; otherwise the stub allocator
  // fails first, and kmax is not written
  nd4hip_handle h;
  int32_t range[2] = {-1, -1};
  km = -5;
  EXPECT(nd4_stevxv(&h, 1, 2049, 1, buf, buf, buf, buf, buf, range, &km) == ND4HIP_ERR_ARG && std::strstr(g_err, "nd4hip_dstevxv_batched: extent out of range"));
  EXPECT(nd4_stevxv(&h, 32769, 4, 1, buf, buf, buf, buf, buf, range, &km) == ND4HIP_ERR_ARG);
  EXPECT(nd4_syevxv(&h, false, 1, 2049, 1, buf, buf, buf, buf, range, &km) == ND4HIP_ERR_ARG && std::strstr(g_err, "nd4hip_dsyevxv_batched: extent out of range"));
  EXPECT(nd4_syevxv(&h, true, 32769, 4, 1, buf, buf, buf, buf, range, &km) == ND4HIP_ERR_ARG && std::strstr(g_err, "nd4hip_dsyevxv_tr_batched"));
  EXPECT(nd4_stevxv(&h, 1, 4, 4, buf, buf, buf, buf, buf, range, &km) == ND4HIP_ERR_HIP);
  EXPECT(nd4_syevxv(&h, false, 1, 4, 4, buf, buf, buf, buf, range, &km) == ND4HIP_ERR_HIP && nd4_syevxv(&h, true, 2, 1, 1, buf, buf, buf, buf, range, &km) == ND4HIP_ERR_HIP);
  EXPECT(km == -5 && range[0] == -1 && range[1] == -1);
  std::printf("eigsym interval host check ok\n");
  return 0;
}
