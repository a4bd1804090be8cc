// Stand-alone host check of the selected-triplet SVD (csrc/bdsvdx.hip): the argument checkers of nd4hip_args.h, the
// order, LDS and workspace arithmetic for every K and J the entry points admit, the index arithmetic of the Golub-Kahan interleave
// and of the strided diagonals of the dense route, the grids, and the launchers' refusals, for AddressSanitizer + UBSan on the CPU.
// Nothing is launched and no device is needed: what bdsvdx.hip's launchers would call are stubs that fail.
// Build and run from the repository root:
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=undefined -fsanitize=address,undefined tools/bdsvdx_host_check.hip \
//         nd4js_amd/csrc/bdsvdx.hip -o bdsvdx_host_check && ./bdsvdx_host_check
#include "../nd4js_amd/csrc/syev_internal.h"
#include "../nd4js_amd/csrc/nd4hip_args.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

static char g_err[256];
static int g_allocs = 0;
void nd4_set_error(const char* fmt, ...) { va_list ap; va_start(ap, fmt); vsnprintf(g_err, sizeof g_err, fmt, ap); va_end(ap); }
int nd4_hip_fail(hipError_t, const char*, const char*, int) { return ND4HIP_ERR_HIP; }
int nd4_ws_alloc(nd4hip_handle*, size_t, void**) { ++g_allocs; return ND4HIP_ERR_HIP; }
int nd4_pinned(nd4hip_handle*, size_t, void**) { return ND4HIP_ERR_HIP; }
int nd4_xchg_check(nd4hip_handle*, const char*) { return ND4HIP_ERR_HIP; }
Nd4WsScope::Nd4WsScope(nd4hip_handle* hh) : h(hh), nblocks(0), used_last(0), generation(0) {}
Nd4WsScope::~Nd4WsScope() {}
int nd4_gemm(nd4hip_handle*, bool, bool, int64_t, int64_t, int64_t, double, const double*, int64_t, int64_t, const double*, int64_t, int64_t, double,
             double*, int64_t, int64_t, int64_t) { return ND4HIP_ERR_HIP; }
int nd4_transpose(nd4hip_handle*, int64_t, int64_t, const double*, int64_t, double*, int64_t, int64_t, int64_t, int64_t) { return ND4HIP_ERR_HIP; }
int nd4_gebrd(nd4hip_handle*, int64_t, int64_t, int64_t, const double*, double*, double*, double*) { return ND4HIP_ERR_HIP; }
int nd4_svd_scale_begin(nd4hip_handle*, int64_t, int64_t, const double*, unsigned long long*) { return ND4HIP_ERR_HIP; }
int nd4_svd_scale_apply(nd4hip_handle*, int64_t, int64_t, const double*, double*, const unsigned long long*) { return ND4HIP_ERR_HIP; }
int nd4_svd_scale_undo(nd4hip_handle*, int64_t, int64_t, double*, const unsigned long long*) { return ND4HIP_ERR_HIP; }
int nd4_bdsdc_rows(nd4hip_handle*, int64_t, int64_t, int64_t, const double*, const double*, double*, double*, double*) { return ND4HIP_ERR_HIP; }
int nd4_stx_vectors(nd4hip_handle*, int64_t, int, int, int, const int*, const double*, const double*, const double*, const int*, const double*, double*) {
  return ND4HIP_ERR_HIP;
}
int nd4_stx_read_flags(nd4hip_handle*, const int*, size_t, const int**) { return ND4HIP_ERR_HIP; }
int nd4_sytrf_bk_tier(const nd4hip_handle*, int64_t, int64_t, int) { return 0; }

#define EXPECT(cond) do { if (!(cond)) { std::printf("FAILED line %d: %s (last error: %s)\n", __LINE__, #cond, g_err); return 1; } } while (0)

int main() {
  double buf[8] = {0};
  int32_t ibuf[4] = {0};
  const void *P = buf, *Z = nullptr;
  // dbdsvdx: negative extent, shape, subset, K <= 2048, empty call, NULL pointer, the vectors together
  EXPECT(nd4_args_bdsvdx(-1, 4096, 9, 7, 3, Z, Z, Z, Z, Z) == ND4HIP_ERR_ARG && std::strstr(g_err, "nd4hip_dbdsvdx_batched: negative extent"));
  EXPECT(nd4_args_bdsvdx(1, -1, -1, 0, 0, P, P, P, P, P) == ND4HIP_ERR_ARG && std::strstr(g_err, "negative extent"));
  EXPECT(nd4_args_bdsvdx(1, 4, 6, 0, 1, P, P, P, P, P) == ND4HIP_ERR_ARG && std::strstr(g_err, "B must be K x K or K x (K+1)"));
  EXPECT(nd4_args_bdsvdx(1, 4, 3, 0, 1, P, P, P, P, P) == ND4HIP_ERR_ARG);
  EXPECT(nd4_args_bdsvdx(1, 4, 4, 3, 2, P, P, P, P, P) == ND4HIP_ERR_ARG && std::strstr(g_err, "subset must satisfy 0 <= i0 <= i1 <= K"));
  EXPECT(nd4_args_bdsvdx(1, 4, 5, -1, 2, P, P, P, P, P) == ND4HIP_ERR_ARG && nd4_args_bdsvdx(1, 4, 5, 0, 5, P, P, P, P, P) == ND4HIP_ERR_ARG);
  EXPECT(nd4_args_bdsvdx(1, 2049, 2050, 0, 1, P, P, P, P, P) == ND4HIP_ERR_ARG && std::strstr(g_err, "K <= 2048"));
  EXPECT(nd4_args_bdsvdx(1, 2049, 2050, 0, 2050, P, P, P, P, P) == ND4HIP_ERR_ARG && std::strstr(g_err, "subset must satisfy"));
  EXPECT(nd4_args_bdsvdx(0, 4, 4, 0, 1, Z, Z, Z, Z, Z) == ND4_ARGS_EMPTY && nd4_args_bdsvdx(2, 0, 0, 0, 0, Z, Z, Z, Z, Z) == ND4_ARGS_EMPTY);
  EXPECT(nd4_args_bdsvdx(2, 4, 5, 3, 3, Z, Z, Z, Z, Z) == ND4_ARGS_EMPTY && nd4_args_bdsvdx(2, 0, 1, 0, 0, Z, Z, Z, Z, Z) == ND4_ARGS_EMPTY);
  EXPECT(nd4_args_bdsvdx(1, 1, 1, 0, 1, P, Z, Z, P, Z) == ND4_ARGS_GO && nd4_args_bdsvdx(1, 1, 2, 0, 1, P, Z, Z, P, Z) == ND4HIP_ERR_ARG);
  EXPECT(nd4_args_bdsvdx(1, 2, 2, 0, 1, Z, P, P, P, P) == ND4HIP_ERR_ARG && nd4_args_bdsvdx(1, 2, 2, 0, 1, P, P, P, Z, P) == ND4HIP_ERR_ARG);
  EXPECT(std::strstr(g_err, "nd4hip_dbdsvdx_batched: NULL pointer"));
  EXPECT(nd4_args_bdsvdx(1, 2, 2, 0, 1, P, P, P, P, Z) == ND4HIP_ERR_ARG && std::strstr(g_err, "U2 and V2 go together"));
  EXPECT(nd4_args_bdsvdx(1, 2, 2, 0, 1, P, P, Z, P, P) == ND4HIP_ERR_ARG && nd4_args_bdsvdx(1, 2048, 2049, 0, 2048, P, P, P, P, P) == ND4_ARGS_GO);
  // dgesvdx: negative extent, subset against min(M, N), min(M, N) <= 2048, empty call, NULL pointer, the vectors together
  EXPECT(nd4_args_gesvdx(1, 3, -2, 0, 0, P, P, P, P) == ND4HIP_ERR_ARG && std::strstr(g_err, "nd4hip_dgesvdx_batched: negative extent"));
  EXPECT(nd4_args_gesvdx(1, 4, 7, 0, 5, P, P, P, P) == ND4HIP_ERR_ARG && std::strstr(g_err, "0 <= i0 <= i1 <= min(M, N)"));
  EXPECT(nd4_args_gesvdx(1, 7, 4, 0, 5, P, P, P, P) == ND4HIP_ERR_ARG && nd4_args_gesvdx(1, 7, 4, 2, 1, P, P, P, P) == ND4HIP_ERR_ARG);
  EXPECT(nd4_args_gesvdx(1, 2049, 30000, 0, 1, P, P, P, P) == ND4HIP_ERR_ARG && std::strstr(g_err, "min(M, N) <= 2048"));
  EXPECT(nd4_args_gesvdx(1, 2048, 30000, 0, 2048, P, P, P, P) == ND4_ARGS_GO && nd4_args_gesvdx(1, 30000, 2048, 2047, 2048, P, Z, P, Z) == ND4_ARGS_GO);
  EXPECT(nd4_args_gesvdx(0, 3, 3, 0, 1, Z, Z, Z, Z) == ND4_ARGS_EMPTY && nd4_args_gesvdx(1, 0, 3, 0, 0, Z, Z, Z, Z) == ND4_ARGS_EMPTY);
  EXPECT(nd4_args_gesvdx(1, 3, 0, 0, 0, Z, Z, Z, Z) == ND4_ARGS_EMPTY && nd4_args_gesvdx(1, 3, 3, 1, 1, Z, Z, Z, Z) == ND4_ARGS_EMPTY);
  EXPECT(nd4_args_gesvdx(1, 3, 3, 0, 1, Z, P, P, P) == ND4HIP_ERR_ARG && nd4_args_gesvdx(1, 3, 3, 0, 1, P, P, Z, P) == ND4HIP_ERR_ARG);
  EXPECT(std::strstr(g_err, "nd4hip_dgesvdx_batched: NULL pointer"));
  EXPECT(nd4_args_gesvdx(1, 3, 3, 0, 1, P, P, P, Z) == ND4HIP_ERR_ARG && std::strstr(g_err, "U and V go together"));
  // every K and J: the order, what is staged in LDS (at most 4096 squares, 32 KB), and every index the kernels form. The interleave
  // is walked on real arrays of exactly K, J - 1 and K + J entries, so that an index past an end is the sanitizer's to report.
  for (int64_t K = 1; K <= 2048; ++K)
    for (int64_t J = K; J <= K + 1; ++J) {
      const int64_t n = nd4_bdx_order(K, J), no = nd4_bdx_offdiagonals(K, J);
      EXPECT(n == K + J && no == n - 1 && no <= 4096 && nd4_bdx_lds_bytes(K, J) == 8 * (size_t)no && nd4_bdx_lds_bytes(K, J) <= 32768);
      std::vector<double> d((size_t)K, 1.0), e((size_t)(J - 1), 2.0), z((size_t)n, 0.0);
      int64_t nd = 0, ne = 0;
      for (int64_t i = 0; i < no; ++i) {                        // bdx_off: d_{i/2} for even i, e_{i/2} for odd i
        if (i & 1) { z[(size_t)i] += e[(size_t)(i >> 1)]; ++ne; } else { z[(size_t)i] += d[(size_t)(i >> 1)]; ++nd; }
      }
      EXPECT(nd == K && ne == J - 1);
      double su = 0.0, sv = 0.0;                                // bdx_split: u = the odd entries, v = the even entries
      for (int64_t i = 0; i < K; ++i) su += z[(size_t)(2 * i + 1)];
      for (int64_t i = 0; i < J; ++i) sv += z[(size_t)(2 * i)];
      EXPECT(su == 2.0 * (double)(J - 1) && sv == (double)K);   // every e once in u's places, every d once in v's, z[n - 1] = 0
      // the dense route reads the diagonals of B_b [m, Jb] in place: d at i (Jb + 1), e at 1 + i (Jb + 1), members m Jb apart
      const int64_t m = K, Jb = J;
      EXPECT((m - 1) * (Jb + 1) < m * Jb && (Jb < 2 || 1 + (Jb - 2) * (Jb + 1) < m * Jb));
      for (int64_t k : {(int64_t)1, K / 2 + 1, K}) {
        EXPECT(nd4_bdx_vector_doubles(1, K, J, k) == (size_t)(5 * k * n));
        EXPECT(nd4_bdx_vector_doubles(32768, K, J, k) / 32768 == (size_t)(5 * k * n));   // no wrap in size_t at the largest chunk
        const int64_t nb = nd4_stx_bisect_blocks(k);
        EXPECT(nb >= 1 && (nb - 1) * 256 < k && k <= nb * 256);
      }
    }
  // the launchers refuse what the entry points never pass on, before anything is allocated; otherwise the stub allocator fails first
  nd4hip_handle h;
  EXPECT(nd4_bdsvdx(&h, 1, 2049, 2049, 0, 1, buf, buf, buf, buf, buf, ibuf) == ND4HIP_ERR_ARG && std::strstr(g_err, "nd4hip_dbdsvdx_batched: extent out of range"));
  EXPECT(nd4_bdsvdx(&h, 1, 4, 6, 0, 1, buf, buf, buf, buf, buf, ibuf) == ND4HIP_ERR_ARG && nd4_bdsvdx(&h, 32769, 4, 4, 0, 1, buf, buf, buf, buf, buf, ibuf) == ND4HIP_ERR_ARG);
  EXPECT(nd4_bdsvdx(&h, 0, 4, 4, 0, 1, buf, buf, buf, buf, buf, ibuf) == ND4HIP_ERR_ARG && nd4_bdsvdx(&h, 1, 0, 0, 0, 0, buf, buf, buf, buf, buf, ibuf) == ND4HIP_ERR_ARG);
  EXPECT(nd4_gesvdx(&h, 1, 2049, 4000, 0, 1, buf, buf, buf, buf, ibuf) == ND4HIP_ERR_ARG && std::strstr(g_err, "nd4hip_dgesvdx_batched: extent out of range"));
  EXPECT(nd4_gesvdx(&h, 32769, 4, 4, 0, 1, buf, buf, buf, buf, ibuf) == ND4HIP_ERR_ARG && nd4_gesvdx(&h, 1, 0, 4, 0, 0, buf, buf, buf, buf, ibuf) == ND4HIP_ERR_ARG);
  EXPECT(g_allocs == 0);
  EXPECT(nd4_bdsvdx(&h, 1, 4, 5, 0, 4, buf, buf, buf, buf, buf, ibuf) == ND4HIP_ERR_HIP && nd4_bdsvdx(&h, 2, 1, 1, 0, 1, buf, nullptr, nullptr, buf, nullptr, nullptr) == ND4HIP_ERR_HIP);
  EXPECT(nd4_gesvdx(&h, 1, 4, 7, 0, 4, buf, buf, buf, buf, ibuf) == ND4HIP_ERR_HIP && nd4_gesvdx(&h, 3, 7, 4, 1, 2, buf, nullptr, buf, nullptr, nullptr) == ND4HIP_ERR_HIP);
  EXPECT(g_allocs == 4 && ibuf[0] == 0 && buf[0] == 0.0);
  std::printf("bdsvdx host check ok\n");
  return 0;
}
