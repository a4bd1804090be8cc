// extern "C" entry points of include/nd4hip.h: the *_dev (device pointer) forms. The host-pointer forms that the N-API shim
// binds live in nd4hip_host.hip; the argument checks that the two forms of an operation share, in nd4hip_args.h.
#include "nd4hip_args.h"
#include <cmath>
#include <cstdlib>

namespace {

constexpr size_t D = sizeof(double);

// The kernels carry the batch in gridDim.y/z (<= 65535): longer batches run in chunks of ND4_CHUNK matrices. `b0` is the
// first matrix of the chunk, `nb` its length; strides that are 0 (broadcast operand) stay 0.
constexpr int64_t ND4_CHUNK = 32768;
#define ND4_FOR_CHUNKS(batch) for (int64_t b0 = 0, nb = 0; (nb = ((batch) - b0 < ND4_CHUNK ? (batch) - b0 : ND4_CHUNK)) > 0; b0 += nb)

// The kernels raise flag words where the reference throws. One small read-back decides: `count` ints from the device into the
// handle's pinned buffer on h->stream, synchronised; *host stays valid until the next nd4_pinned of the handle.
int read_flags(nd4hip_handle* h, const int* flags, size_t count, const int** host) {
  void* hp = nullptr;
  ND4_TRY(nd4_pinned(h, sizeof(int) * count, &hp));
  ND4_HIP(hipMemcpyAsync(hp, flags, sizeof(int) * count, hipMemcpyDeviceToHost, h->stream));
  ND4_HIP(hipStreamSynchronize(h->stream));
  *host = static_cast<const int*>(hp);
  return 0;
}

// algorithmic flop conventions of SURVEY.md 8(d) for nd4hip_profile_last
inline double nd4_flops_qr(int64_t M, int64_t N) {          // with explicit Q: 4 (M N^2 - N^3 / 3) for M >= N, 8/3 N^3 when square
  const double m = (double)M, n = (double)N;
  return M >= N ? 4.0 * (m * n * n - n * n * n / 3.0) : 2.0 * n * m * m - 2.0 / 3.0 * m * m * m + 4.0 / 3.0 * m * m * m;
}
inline double nd4_flops_svd(int64_t M, int64_t N) {         // Golub-Reinsch count with U, sv, V: 21 N^3 when square
  const double m = (double)(M >= N ? M : N), n = (double)(M >= N ? N : M);
  return 4.0 * m * m * n + 8.0 * m * n * n + 9.0 * n * n * n;
}

// column-pivoted QR: the pivot pass touches every trailing element once per step (dot 2 + update 2 + norm 2 flops), then the QR
// with explicit Q of the permuted matrix
inline double nd4_flops_qp3(int64_t M, int64_t N) {
  const double m = (double)M, n = (double)N, k = (double)(M < N ? M : N);
  return 6.0 * (k * m * n - (m + n) * k * (k - 1.0) / 2.0 + (k - 1.0) * k * (2.0 * k - 1.0) / 6.0) + nd4_flops_qr(M, N);
}

}  // namespace

// ------------------------------------------------------------------------------------ matmul
extern "C" int nd4hip_dgemm_batched_dev(nd4hip_handle* h, int64_t batch, int64_t I, int64_t K, int64_t J,
                                        const double* A, int64_t strideA, const double* B, int64_t strideB, double* C) {
  ND4_CHECK_ARG(h != nullptr, "nd4hip_dgemm_batched: NULL handle");
  Nd4DeviceGuard guard(h);
  Nd4Prof prof(h, "dgemm_batched", (double)(2.0 * batch * I * K * J), (double)(8.0 * (double)(batch * I * J + (strideA ? batch : 1) * I * K + (strideB ? batch : 1) * K * J)));
  ND4_ARGS(nd4_args_gemm("dgemm_batched", true, batch, I, K, J, A, strideA, B, strideB, C));
  ND4_FOR_CHUNKS(batch) {
    ND4_TRY(nd4_gemm(h, false, false, I, J, K, 1.0, A + b0 * strideA, K, strideA, B + b0 * strideB, J, strideB,
                     0.0, C + b0 * I * J, J, I * J, nb));
  }
  return 0;
}

extern "C" int nd4hip_zgemm_batched_dev(nd4hip_handle* h, int a_complex, int b_complex, int64_t batch, int64_t I, int64_t K, int64_t J,
                                        const double* A, int64_t strideA, const double* B, int64_t strideB, double* C) {
  // the argument checks come first: they need no handle (and are testable without a device)
  ND4_ARGS(nd4_args_gemm("zgemm_batched", a_complex || b_complex, batch, I, K, J, A, strideA, B, strideB, C));
  ND4_CHECK_ARG(h != nullptr, "nd4hip_zgemm_batched: NULL handle");
  Nd4DeviceGuard guard(h);
  const double ea = a_complex ? 2.0 : 1.0, eb = b_complex ? 2.0 : 1.0;     // doubles per element
  Nd4Prof prof(h, "zgemm_batched", (double)((a_complex && b_complex ? 8.0 : 4.0) * batch * I * K * J),
               8.0 * (2.0 * batch * I * J + ea * (strideA ? batch : 1) * I * K + eb * (strideB ? batch : 1) * K * J));
  ND4_FOR_CHUNKS(batch) {
    if (!a_complex)   // RC: A (I x K) times the K x 2J real view of B, into the I x 2J real view of C: the reference's products
      ND4_TRY(nd4_gemm(h, false, false, I, 2 * J, K, 1.0, A + b0 * strideA, K, strideA, B + 2 * b0 * strideB, 2 * J, 2 * strideB,
                       0.0, C + 2 * b0 * I * J, 2 * J, 2 * I * J, nb));
    else
      ND4_TRY(nd4_zgemm(h, b_complex != 0, nb, I, K, J, A + 2 * b0 * strideA, strideA,
                      B + (b_complex ? 2 : 1) * b0 * strideB, strideB, C + 2 * b0 * I * J));
  }
  return 0;
}

extern "C" int nd4hip_dgemm_ex_dev(nd4hip_handle* h, int transA, int transB, int64_t M, int64_t N, int64_t K,
                                   double alpha, const double* A, int64_t lda, const double* B, int64_t ldb,
                                   double beta, double* C, int64_t ldc) {
  ND4_CHECK_ARG(h != nullptr, "nd4hip_dgemm_ex: NULL handle");
  Nd4DeviceGuard guard(h);
  Nd4Prof prof(h, "dgemm_ex", (double)(2.0 * M * N * K), (double)(8.0 * (double)(M * K + K * N + M * N)));
  ND4_CHECK_ARG(M >= 0 && N >= 0 && K >= 0, "nd4hip_dgemm_ex: negative extent");
  ND4_CHECK_ARG(lda >= (transA ? M : K) && ldb >= (transB ? K : N) && ldc >= N, "nd4hip_dgemm_ex: leading dimension too small");
  if (M == 0 || N == 0) return 0;
  return nd4_gemm(h, transA != 0, transB != 0, M, N, K, alpha, A, lda, 0, B, ldb, 0, beta, C, ldc, 0, 1);
}

// ------------------------------------------------------------------------------------ LU
extern "C" int nd4hip_dgetrf_batched_dev(nd4hip_handle* h, int64_t batch, int64_t N, const double* A, double* LU, int32_t* P) {
  ND4_CHECK_ARG(h != nullptr, "nd4hip_dgetrf_batched: NULL handle");
  Nd4DeviceGuard guard(h);
  Nd4Prof prof(h, "dgetrf_batched", (double)(2.0 / 3.0 * batch * N * N * N), (double)(16.0 * batch * N * N));
  ND4_ARGS(nd4_args_dense("dgetrf_batched", {batch, N}, {A, LU, P}));
  ND4_FOR_CHUNKS(batch) ND4_TRY(nd4_getrf(h, nb, N, A + b0 * N * N, LU + b0 * N * N, P + b0 * N));
  return 0;
}

// ------------------------------------------------------------------------------------ solves
namespace {
// X[b] = Y[b*strideY] for every batch member (strideY = 0: the same Y for all)
int copy_rhs(nd4hip_handle* h, int64_t batch, int64_t rows, int64_t J, const double* Y, int64_t strideY, double* X) {
  return nd4_copy_matrix(h, rows, J, Y, J, X, J, batch, strideY, rows * J);
}
}  // namespace

extern "C" int nd4hip_dgetrs_batched_dev(nd4hip_handle* h, int64_t batch, int64_t N, int64_t J, const double* LU, int64_t strideLU,
                                         const int32_t* P, int64_t strideP, const double* Y, int64_t strideY, double* X) {
  ND4_CHECK_ARG(h != nullptr, "nd4hip_dgetrs_batched: NULL handle");
  Nd4DeviceGuard guard(h);
  Nd4Prof prof(h, "dgetrs_batched", (double)(2.0 * batch * N * N * J), (double)(8.0 * batch * (double)(N * N + 2 * N * J)));
  ND4_ARGS(nd4_args_solve("dgetrs_batched", batch, N, J, {{LU, strideLU, N * N}, {P, strideP, N}, {Y, strideY, N * J}}, X));
  ND4_FOR_CHUNKS(batch) ND4_TRY(nd4_getrs(h, nb, N, J, LU + b0 * strideLU, strideLU, P + b0 * strideP, strideP, Y + b0 * strideY, strideY, X + b0 * N * J));
  return 0;
}

extern "C" int nd4hip_dtrsm_batched_dev(nd4hip_handle* h, int upper, int unit_diag, int64_t batch, int64_t M, int64_t J,
                                        const double* T, int64_t strideT, const double* Y, int64_t strideY, double* X) {
  ND4_CHECK_ARG(h != nullptr, "nd4hip_dtrsm_batched: NULL handle");
  Nd4DeviceGuard guard(h);
  Nd4Prof prof(h, "dtrsm_batched", (double)(1.0 * batch * M * M * J), (double)(8.0 * batch * (double)(M * M / 2 + 2 * M * J)));
  ND4_ARGS(nd4_args_solve("dtrsm_batched", batch, M, J, {{T, strideT, M * M}, {Y, strideY, M * J}}, X));
  if (X != Y || strideY != M * J) ND4_TRY(copy_rhs(h, batch, M, J, Y, strideY, X));
  ND4_FOR_CHUNKS(batch) ND4_TRY(nd4_trsm(h, upper != 0, unit_diag != 0, nb, M, J, T + b0 * strideT, strideT, X + b0 * M * J));
  return 0;
}

// ---- least squares from a factorisation: qr_lstsq (qr.js:186-273), svd_lstsq / svd_solve (svd.js:66-228)
extern "C" int nd4hip_dqrls_batched_dev(nd4hip_handle* h, int64_t batch, int64_t N, int64_t M, int64_t I, int64_t J,
                                        const double* Q, int64_t strideQ, const double* R, int64_t strideR,
                                        const double* Y, int64_t strideY, double* X) {
  ND4_CHECK_ARG(h != nullptr, "nd4hip_dqrls_batched: NULL handle");
  Nd4DeviceGuard guard(h);
  Nd4Prof prof(h, "dqrls_batched", (double)(0.0), (double)(0.0));
  ND4_ARGS(nd4_args_factor_ls("dqrls_batched", true, batch, N, M, I, J, {{Q, strideQ, N * M}, {R, strideR, M * I}, {Y, strideY, N * J}}, X));
  if (N == 0 || M == 0) { ND4_HIP(hipMemsetAsync(X, 0, D * (size_t)(batch * I * J), h->stream)); return 0; }
  ND4_FOR_CHUNKS(batch) ND4_TRY(nd4_qrls(h, nb, N, M, I, J, Q + b0 * strideQ, strideQ, R + b0 * strideR, strideR, Y + b0 * strideY, strideY, X + b0 * I * J));
  return 0;
}

extern "C" int nd4hip_dsvdls_batched_dev(nd4hip_handle* h, int64_t batch, int64_t N, int64_t M, int64_t I, int64_t J,
                                         const double* U, int64_t strideU, const double* sv, int64_t strideSv,
                                         const double* V, int64_t strideV, const double* Y, int64_t strideY, double* X) {
  ND4_CHECK_ARG(h != nullptr, "nd4hip_dsvdls_batched: NULL handle");
  Nd4DeviceGuard guard(h);
  Nd4Prof prof(h, "dsvdls_batched", (double)(0.0), (double)(0.0));
  ND4_ARGS(nd4_args_factor_ls("dsvdls_batched", false, batch, N, M, I, J,
                              {{U, strideU, N * M}, {sv, strideSv, M}, {V, strideV, M * I}, {Y, strideY, N * J}}, X));
  if (N == 0 || M == 0) { ND4_HIP(hipMemsetAsync(X, 0, D * (size_t)(batch * I * J), h->stream)); return 0; }
  ND4_FOR_CHUNKS(batch) ND4_TRY(nd4_svdls(h, nb, N, M, I, J, U + b0 * strideU, strideU, sv + b0 * strideSv, strideSv, V + b0 * strideV, strideV,
                                          Y + b0 * strideY, strideY, X + b0 * I * J));
  return 0;
}

// ---- Cholesky: cholesky_decomp (cholesky.js:51-71), cholesky_solve (:74-150)   
extern "C" int nd4hip_dpotrf_batched_dev(nd4hip_handle* h, int64_t batch, int64_t N, const double* S, double* L) {
  ND4_CHECK_ARG(h != nullptr, "nd4hip_dpotrf_batched: NULL handle");
  Nd4DeviceGuard guard(h);
  Nd4Prof prof(h, "dpotrf_batched", (double)(batch * N * N * N / 3.0), (double)(16.0 * batch * N * N));
  ND4_ARGS(nd4_args_dense("dpotrf_batched", {batch, N}, {S, L}));
  Nd4WsScope scope(h);
  void* p = nullptr;
  ND4_TRY(nd4_ws_alloc(h, sizeof(int) * (size_t)batch, &p));
  int* flags = static_cast<int*>(p);
  ND4_FOR_CHUNKS(batch) ND4_TRY(nd4_potrf(h, nb, N, S + b0 * N * N, L + b0 * N * N, flags + b0));
  // the reference throws on the first NaN pivot (cholesky.js:43-44): one small read-back decides it
  const int* host = nullptr;
  ND4_TRY(read_flags(h, flags, (size_t)batch, &host));
  for (int64_t b = 0; b < batch; b++)
    if (host[b]) { nd4_set_error("Matrix contains NaNs or is (near) singular."); return ND4HIP_ERR_SINGULAR; }
  return 0;
}
extern "C" int nd4hip_dpotrs_batched_dev(nd4hip_handle* h, int64_t batch, int64_t N, int64_t J, const double* L, int64_t strideL,
                                         const double* Y, int64_t strideY, double* X) {
  ND4_CHECK_ARG(h != nullptr, "nd4hip_dpotrs_batched: NULL handle");
  Nd4DeviceGuard guard(h);
  Nd4Prof prof(h, "dpotrs_batched", (double)(2.0 * batch * N * N * J), (double)(8.0 * batch * (double)(N * N + 2 * N * J)));
  ND4_ARGS(nd4_args_solve("dpotrs_batched", batch, N, J, {{L, strideL, N * N}, {Y, strideY, N * J}}, X));
  ND4_FOR_CHUNKS(batch) ND4_TRY(nd4_potrs(h, nb, N, J, L + b0 * strideL, strideL, Y + b0 * strideY, strideY, X + b0 * N * J));
  return 0;
}

// ---- LDL^T: ldl_decomp (ldl.js:67-90), ldl_solve (:133-201)   
extern "C" int nd4hip_dldltrf_batched_dev(nd4hip_handle* h, int64_t batch, int64_t N, const double* S, double* LD) {
  ND4_CHECK_ARG(h != nullptr, "nd4hip_dldltrf_batched: NULL handle");
  Nd4DeviceGuard guard(h);
  Nd4Prof prof(h, "dldltrf_batched", (double)(batch * N * N * N / 3.0), (double)(16.0 * batch * N * N));
  ND4_ARGS(nd4_args_dense("dldltrf_batched", {batch, N}, {S, LD}));
  ND4_FOR_CHUNKS(batch) ND4_TRY(nd4_ldltrf(h, nb, N, S + b0 * N * N, LD + b0 * N * N));
  return 0;
}
extern "C" int nd4hip_dldltrs_batched_dev(nd4hip_handle* h, int64_t batch, int64_t N, int64_t J, const double* LD, int64_t strideLD,
                                          const double* Y, int64_t strideY, double* X) {
  ND4_CHECK_ARG(h != nullptr, "nd4hip_dldltrs_batched: NULL handle");
  Nd4DeviceGuard guard(h);
  Nd4Prof prof(h, "dldltrs_batched", (double)(2.0 * batch * N * N * J), (double)(8.0 * batch * (double)(N * N + 2 * N * J)));
  ND4_ARGS(nd4_args_solve("dldltrs_batched", batch, N, J, {{LD, strideLD, N * N}, {Y, strideY, N * J}}, X));
  ND4_FOR_CHUNKS(batch) ND4_TRY(nd4_ldltrs(h, nb, N, J, LD + b0 * strideLD, strideLD, Y + b0 * strideY, strideY, X + b0 * N * J));
  return 0;
}

// ---- pivoted LDL^T: pldlp_decomp (pldlp.js:191-222), pldlp_solve (:519-604)
int nd4_sytrf_bk_run(nd4hip_handle* h, int64_t batch, int64_t N, const double* S, double* LD, int32_t* P, int tier, int64_t member0,
                     int64_t* first_bad) {
  // the argument checks come first: they need no handle (and are testable without a device)
  ND4_ARGS(nd4_args_sytrf_bk(batch, N, S, LD, P, tier));
  ND4_CHECK_ARG(h != nullptr, "nd4hip_dsytrf_bk_batched: NULL handle");
  Nd4DeviceGuard guard(h);
  Nd4Prof prof(h, "dsytrf_bk_batched", (double)(batch * N * N * N / 3.0), (double)(16.0 * batch * N * N));
  const int t = nd4_sytrf_bk_tier(h, batch, N, tier);
  Nd4WsScope scope(h);
  void* p = nullptr;
  ND4_TRY(nd4_ws_alloc(h, sizeof(int) * (size_t)batch, &p));
  int* flags = static_cast<int*>(p);
  ND4_HIP(hipMemsetAsync(flags, 0, sizeof(int) * (size_t)batch, h->stream));
  ND4_TRY(nd4_sytrf_bk(h, batch, N, S, LD, P, flags, t));
  // the reference throws at the first zero column or NaN (pldlp.js:148-149): one small read-back decides it
  const int* host = nullptr;
  ND4_TRY(read_flags(h, flags, (size_t)batch, &host));
  for (int64_t b = 0; b < batch; b++)
    if (host[b]) {
      nd4_set_error("_pldlp_decomp(M,N, LD,LD_off, P,P_off): Zero column or NaN encountered. (matrix %lld)", (long long)(member0 + b));
      if (first_bad) *first_bad = member0 + b;
      return ND4HIP_ERR_SINGULAR;
    }
  return 0;
}
extern "C" int nd4hip_dsytrf_bk_batched_ex_dev(nd4hip_handle* h, int64_t batch, int64_t N, const double* S, double* LD, int32_t* P, int tier) {
  return nd4_sytrf_bk_run(h, batch, N, S, LD, P, tier, 0, nullptr);
}
extern "C" int nd4hip_dsytrf_bk_batched_dev(nd4hip_handle* h, int64_t batch, int64_t N, const double* S, double* LD, int32_t* P) {
  return nd4_sytrf_bk_run(h, batch, N, S, LD, P, ND4HIP_PLDLP_TIER_AUTO, 0, nullptr);
}
extern "C" int nd4hip_dsytrf_bk_tier(nd4hip_handle* h, int64_t batch, int64_t N, int tier) {
  ND4_CHECK_ARG(h != nullptr, "nd4hip_dsytrf_bk_tier: NULL handle");
  ND4_ARGS(nd4_args_sytrf_bk_tier("dsytrf_bk_tier", batch, N, tier));
  return nd4_sytrf_bk_tier(h, batch, N, tier);
}
extern "C" int nd4hip_dsytrf_bk_limits(int* lds_max_n, int* global_max_n, int* grid_tile) {
  nd4_sytrf_bk_limits(lds_max_n, global_max_n, grid_tile);
  return 0;
}
extern "C" int nd4hip_dsytrs_bk_batched_dev(nd4hip_handle* h, int64_t batch, int64_t N, int64_t J, const double* LD, int64_t strideLD,
                                            const int32_t* P, int64_t strideP, const double* Y, int64_t strideY, double* X) {
  // the argument checks come first: they need no handle (and are testable without a device)
  ND4_ARGS(nd4_args_solve("dsytrs_bk_batched", batch, N, J, {{LD, strideLD, N * N}, {P, strideP, N}, {Y, strideY, N * J}}, X));
  ND4_CHECK_ARG(h != nullptr, "nd4hip_dsytrs_bk_batched: NULL handle");
  Nd4DeviceGuard guard(h);
  Nd4Prof prof(h, "dsytrs_bk_batched", (double)(2.0 * batch * N * N * J), (double)(8.0 * batch * (double)(N * N + 2 * N * J)));
  Nd4WsScope scope(h);
  void* p = nullptr;
  ND4_TRY(nd4_ws_alloc(h, sizeof(int), &p));
  int* flag = static_cast<int*>(p);
  ND4_HIP(hipMemsetAsync(flag, 0, sizeof(int), h->stream));
  ND4_FOR_CHUNKS(batch) ND4_TRY(nd4_sytrs_bk(h, nb, N, J, LD + b0 * strideLD, strideLD, P + b0 * strideP, strideP, Y + b0 * strideY, strideY,
                                             X + b0 * N * J, flag));
  const int* host = nullptr;
  ND4_TRY(read_flags(h, flag, 1, &host));
  ND4_CHECK_ARG(host[0] == 0, "pldlp_solve(LD,P,y): P contains out-of-bounds indices.");
  return 0;
}

// ---- bidiag_decomp (bidiag.js:245-319)   
extern "C" int nd4hip_dgebrd_batched_dev(nd4hip_handle* h, int64_t batch, int64_t M, int64_t N, const double* A, double* U, double* B, double* V) {
  ND4_CHECK_ARG(h != nullptr, "nd4hip_dgebrd_batched: NULL handle");
  Nd4DeviceGuard guard(h);
  Nd4Prof prof(h, "dgebrd_batched", (double)(batch * nd4_flops_qr(M, N)), (double)(8.0 * batch * (double)(2 * M * N + M * M + N * N)));
  ND4_ARGS(nd4_args_dense("dgebrd_batched", {batch, M, N}, {A, U, B, V}));
  { const int64_t K = M < N ? M : N, Jb = M >= N ? K : K + 1;
    ND4_FOR_CHUNKS(batch) ND4_TRY(nd4_gebrd(h, nb, M, N, A + b0 * M * N, U + b0 * M * K, B + b0 * K * Jb, V + b0 * Jb * N)); }
  return 0;
}

// ---- hessenberg_decomp (hessenberg.js:89-115)   
extern "C" int nd4hip_dgehrd_batched_dev(nd4hip_handle* h, int64_t batch, int64_t N, const double* A, double* U, double* H) {
  ND4_CHECK_ARG(h != nullptr, "nd4hip_dgehrd_batched: NULL handle");
  Nd4DeviceGuard guard(h);
  Nd4Prof prof(h, "dgehrd_batched", (double)(14.0 / 3.0 * batch * N * N * N), (double)(24.0 * batch * N * N));
  ND4_ARGS(nd4_args_dense("dgehrd_batched", {batch, N}, {A, U, H}));
  ND4_FOR_CHUNKS(batch) ND4_TRY(nd4_gehrd(h, nb, N, A + b0 * N * N, U + b0 * N * N, H + b0 * N * N));
  return 0;
}

// ------------------------------------------------------------------------------------ QR
extern "C" int nd4hip_dgeqrf_q_batched_dev(nd4hip_handle* h, int64_t batch, int64_t M, int64_t N, const double* A, double* Q, double* R) {
  ND4_CHECK_ARG(h != nullptr, "nd4hip_dgeqrf_q_batched: NULL handle");
  Nd4DeviceGuard guard(h);
  Nd4Prof prof(h, "dgeqrf_q_batched", (double)(batch * nd4_flops_qr(M, N)), (double)(8.0 * batch * (double)(M * N + (M + N) * (M < N ? M : N))));
  ND4_ARGS(nd4_args_dense("dgeqrf_q_batched", {batch, M, N}, {A, Q, R}));
  { const int64_t L = M < N ? M : N;
    ND4_FOR_CHUNKS(batch) ND4_TRY(nd4_geqrf_q(h, nb, M, N, A + b0 * M * N, Q + b0 * M * L, R + b0 * L * N)); }
  return 0;
}

// qr_decomp_full (qr.js:27-77) for every shape: Q [M, M], R [M, N]
extern "C" int nd4hip_dgeqrf_full_batched_dev(nd4hip_handle* h, int64_t batch, int64_t M, int64_t N, const double* A, double* Q, double* R) {
  ND4_CHECK_ARG(h != nullptr, "nd4hip_dgeqrf_full_batched: NULL handle");
  Nd4DeviceGuard guard(h);
  Nd4Prof prof(h, "dgeqrf_full_batched", (double)(batch * nd4_flops_qr(M, N)), (double)(8.0 * batch * (double)(2 * M * N + M * M)));
  ND4_ARGS(nd4_args_dense("dgeqrf_full_batched", {batch, M, N}, {A, Q, R}));
  ND4_FOR_CHUNKS(batch) ND4_TRY(nd4_geqrf_q_ex(h, nb, M, N, A + b0 * M * N, Q + b0 * M * M, R + b0 * M * N, true));
  return 0;
}

// _qr_decomp_inplace (qr.js:146-183): A [M, N] <- R, Y [M, L] <- Q^T Y with the full (M x M) Q
extern "C" int nd4hip_dgeqrf_qty_batched_dev(nd4hip_handle* h, int64_t batch, int64_t M, int64_t N, int64_t L, double* A, double* Y) {
  ND4_CHECK_ARG(h != nullptr, "nd4hip_dgeqrf_qty_batched: NULL handle");
  Nd4DeviceGuard guard(h);
  Nd4Prof prof(h, "dgeqrf_qty_batched", (double)(batch * nd4_flops_qr(M, N)), (double)(16.0 * batch * (double)(M * N + M * L)));
  ND4_ARGS(nd4_args_geqrf_qty(batch, M, N, L, A, Y));
  Nd4WsScope scope(h);
  void* p = nullptr;
  ND4_TRY(nd4_ws_alloc(h, D * (size_t)batch * (size_t)(M * M + M * N + M * L), &p));
  double* Q = static_cast<double*>(p);
  double* R = Q + (size_t)batch * M * M;
  double* Yt = R + (size_t)batch * M * N;
  ND4_TRY(nd4_geqrf_q_ex(h, batch, M, N, A, Q, R, true));
  ND4_HIP(hipMemcpyAsync(A, R, D * (size_t)(batch * M * N), hipMemcpyDeviceToDevice, h->stream));
  if (L > 0) {
    ND4_TRY(nd4_gemm(h, true, false, M, L, M, 1.0, Q, M, M * M, Y, L, M * L, 0.0, Yt, L, M * L, batch));
    ND4_HIP(hipMemcpyAsync(Y, Yt, D * (size_t)(batch * M * L), hipMemcpyDeviceToDevice, h->stream));
  }
  return 0;
}

// ------------------------------------------------------------------------------------ column-pivoted QR
// rrqr_decomp (rrqr.js:278-395): Q [M, L], R [L, N], P [N]; rrqr_decomp_full (:88-184): Q [M, M], R [M, N], P [N]
static int geqp3_dev(nd4hip_handle* h, const char* name, bool full, int64_t batch, int64_t M, int64_t N, const double* A, double* Q,
                     double* R, int32_t* P) {
  ND4_CHECK_ARG(h != nullptr, "nd4hip_%s: NULL handle", name);
  Nd4DeviceGuard guard(h);
  const int64_t L = M < N ? M : N, qc = full ? M : L, rr = full ? M : L;
  Nd4Prof prof(h, name, (double)batch * nd4_flops_qp3(M, N), 8.0 * batch * (double)(M * N + M * qc + rr * N) + 4.0 * batch * (double)N);
  ND4_ARGS(nd4_args_dense(name, {batch, M, N}, {A, Q, R, P}));
  ND4_FOR_CHUNKS(batch) ND4_TRY(nd4_geqp3(h, nb, M, N, A + b0 * M * N, Q + b0 * M * qc, R + b0 * rr * N, P + b0 * N, full));
  return 0;
}
extern "C" int nd4hip_dgeqp3_batched_dev(nd4hip_handle* h, int64_t batch, int64_t M, int64_t N, const double* A, double* Q, double* R, int32_t* P) {
  return geqp3_dev(h, "dgeqp3_batched", false, batch, M, N, A, Q, R, P);
}
extern "C" int nd4hip_dgeqp3_full_batched_dev(nd4hip_handle* h, int64_t batch, int64_t M, int64_t N, const double* A, double* Q, double* R, int32_t* P) {
  return geqp3_dev(h, "dgeqp3_full_batched", true, batch, M, N, A, Q, R, P);
}

// srrqr_decomp_full (srrqr.js:58-802): Q [M, M], R [M, N], P [N], rank []
extern "C" int nd4hip_dsrrqr_batched_dev(nd4hip_handle* h, int64_t batch, int64_t M, int64_t N, const double* A, double dtol, double ztol,
                                         double* Q, double* R, int32_t* P, int32_t* rank) {
  ND4_CHECK_ARG(h != nullptr, "nd4hip_dsrrqr_batched: NULL handle");
  Nd4DeviceGuard guard(h);
  Nd4Prof prof(h, "dsrrqr_batched", (double)batch * nd4_flops_qp3(M, N), 8.0 * batch * (double)(M * N + M * M + M * N) + 4.0 * batch * (double)(N + 1));
  ND4_ARGS(nd4_args_srrqr(batch, M, N, A, dtol, ztol, Q, R, P, rank));
  ND4_FOR_CHUNKS(batch) ND4_TRY(nd4_srrqr(h, nb, M, N, A ? A + b0 * M * N : nullptr, dtol, ztol, Q ? Q + b0 * M * M : nullptr,
                                          R ? R + b0 * M * N : nullptr, P + b0 * N, rank + b0));
  return 0;
}

// urv_decomp_full (urv.js:100-135): U [M, M], R [M, N], V [N, N], rank []
extern "C" int nd4hip_durv_batched_dev(nd4hip_handle* h, int64_t batch, int64_t M, int64_t N, const double* A, double* U, double* R,
                                       double* V, int32_t* rank) {
  ND4_CHECK_ARG(h != nullptr, "nd4hip_durv_batched: NULL handle");
  Nd4DeviceGuard guard(h);
  Nd4Prof prof(h, "durv_batched", (double)batch * (nd4_flops_qp3(M, N) + nd4_flops_qr(N, M < N ? M : N)),
               8.0 * batch * (double)(2 * M * N + M * M + N * N) + 4.0 * batch);
  ND4_ARGS(nd4_args_urv(batch, M, N, A, U, R, V, rank));
  if (N == 0) {
    ND4_HIP(hipMemsetAsync(rank, 0, sizeof(int32_t) * (size_t)batch, h->stream));
    if (M > 0) ND4_TRY(nd4_set_identity(h, M, M, U, M, batch, M * M));
    return 0;
  }
  ND4_FOR_CHUNKS(batch) ND4_TRY(nd4_urv(h, nb, M, N, A ? A + b0 * M * N : nullptr, U ? U + b0 * M * M : nullptr, R ? R + b0 * M * N : nullptr,
                                        V + b0 * N * N, rank + b0));
  return 0;
}

// urv_lstsq (urv.js:138-323): U [I, J], R [J, K], V [K, L], rank [], Y [I, Jc] -> X [L, Jc]; strides in elements, 0 = broadcast
extern "C" int nd4hip_durvls_batched_dev(nd4hip_handle* h, int64_t batch, int64_t I, int64_t J, int64_t K, int64_t L, int64_t Jc,
                                         const double* U, int64_t strideU, const double* R, int64_t strideR, const double* V, int64_t strideV,
                                         const int32_t* rank, int64_t strideRank, const double* Y, int64_t strideY, double* X) {
  ND4_CHECK_ARG(h != nullptr, "nd4hip_durvls_batched: NULL handle");
  Nd4DeviceGuard guard(h);
  const int64_t Lr = J < K ? J : K;
  Nd4Prof prof(h, "durvls_batched", (double)batch * (2.0 * Lr * I * Jc + (double)Lr * Lr * Jc + 2.0 * Lr * L * Jc),
               8.0 * batch * (double)(I * J + J * K + K * L + I * Jc + L * Jc));
  ND4_ARGS(nd4_args_urvls(batch, I, J, K, L, Jc, U, strideU, R, strideR, V, strideV, rank, strideRank, Y, strideY, X));
  ND4_FOR_CHUNKS(batch) ND4_TRY(nd4_urvls(h, nb, I, J, K, L, Jc, U + b0 * strideU, strideU, R + b0 * strideR, strideR, V + b0 * strideV, strideV,
                                          rank + b0 * strideRank, strideRank, Y + b0 * strideY, strideY, X + b0 * L * Jc));
  return 0;
}

// det / slogdet (det.js:95-106): det [batch] or sign, logdet [batch] of A [M, N], M >= N
namespace {
bool det_force_qr() { const char* e = getenv("ND4HIP_DET_FORCE_QR"); return e && *e && *e != '0'; }   // read per call

int det_dev(nd4hip_handle* h, const char* op, bool log_form, int64_t batch, int64_t M, int64_t N, const double* A, double* D, double* L) {
  ND4_CHECK_ARG(h != nullptr, "nd4hip_%s: NULL handle", op);
  Nd4DeviceGuard guard(h);
  const double m = (double)M, n = (double)N;
  Nd4Prof prof(h, op, (double)batch * 2.0 * (m * n * n - n * n * n / 3.0), 8.0 * batch * (double)(M * N + (log_form ? 2 : 1)));
  ND4_ARGS(nd4_args_det(op, log_form, batch, M, N, A, D, L));
  const bool force = det_force_qr();
  if (N == 0 || (M == N && N <= 64 && !force)) return nd4_det(h, log_form, batch, M, N, A, D, L, false);   // one launch, any batch
  ND4_FOR_CHUNKS(batch) ND4_TRY(nd4_det(h, log_form, nb, M, N, A + b0 * M * N, D + b0, log_form ? L + b0 : nullptr, force));
  return 0;
}

int dettri_dev(nd4hip_handle* h, const char* op, bool log_form, int64_t batch, int64_t N, const double* A, double* D, double* L) {
  ND4_CHECK_ARG(h != nullptr, "nd4hip_%s: NULL handle", op);
  Nd4DeviceGuard guard(h);
  Nd4Prof prof(h, op, (double)batch * N, 8.0 * batch * (double)(N + (log_form ? 2 : 1)));
  ND4_ARGS(nd4_args_det(op, log_form, batch, N, N, A, D, L));          // the square case of det's rules
  return nd4_dettri(h, log_form, batch, N, A, N * N, D, L);
}
}  // namespace

extern "C" int nd4hip_ddet_batched_dev(nd4hip_handle* h, int64_t batch, int64_t M, int64_t N, const double* A, double* det) {
  return det_dev(h, "ddet_batched", false, batch, M, N, A, det, nullptr);
}
extern "C" int nd4hip_dslogdet_batched_dev(nd4hip_handle* h, int64_t batch, int64_t M, int64_t N, const double* A, double* sign, double* logdet) {
  return det_dev(h, "dslogdet_batched", true, batch, M, N, A, sign, logdet);
}
// det_tri / slogdet_tri (det.js:24-92): the diagonal rule on A [N, N]
extern "C" int nd4hip_ddettri_batched_dev(nd4hip_handle* h, int64_t batch, int64_t N, const double* A, double* det) {
  return dettri_dev(h, "ddettri_batched", false, batch, N, A, det, nullptr);
}
extern "C" int nd4hip_dslogdettri_batched_dev(nd4hip_handle* h, int64_t batch, int64_t N, const double* A, double* sign, double* logdet) {
  return dettri_dev(h, "dslogdettri_batched", true, batch, N, A, sign, logdet);
}
// norm(A) 'fro' (norm.js:22-85): one double into the device pointer out
extern "C" int nd4hip_dnrmfro_dev(nd4hip_handle* h, int64_t n, const double* A, double* out) {
  ND4_CHECK_ARG(h != nullptr, "nd4hip_dnrmfro: NULL handle");
  Nd4DeviceGuard guard(h);
  Nd4Prof prof(h, "dnrmfro", 3.0 * (double)n, 8.0 * (double)n + 8.0);
  ND4_ARGS(nd4_args_nrmfro(n, A, out));
  if (n == 0) { ND4_HIP(hipMemsetAsync(out, 0, sizeof(double), h->stream)); return 0; }
  return nd4_nrmfro(h, n, A, out);
}

// ---- schur_eigenvals / schur_eigen (schur.js:31-370), eigen_balance_pre / _post (eigen.js:91-270)
namespace {
// the reference throws at the first matrix that trips; the kernels raise a flag word per matrix instead: one small read-back
int ev_verdict(nd4hip_handle* h, const int* flags, int64_t batch) {
  const int* host = nullptr;
  ND4_TRY(read_flags(h, flags, (size_t)batch, &host));
  for (int64_t b = 0; b < batch; b++) {
    ND4_CHECK_ARG(!(host[b] & ND4HIP_EV_FLAG_ASSERT), "Assertion failed.");
    ND4_CHECK_ARG(!(host[b] & ND4HIP_EV_FLAG_REAL2X2), "schur_eigenvals(T): T must not contain real eigenvalued 2x2 blocks.");
    ND4_CHECK_ARG(!(host[b] & ND4HIP_EV_FLAG_NAN), "NaN encountered.");
    ND4_CHECK_ARG(!(host[b] & ND4HIP_EV_FLAG_SWEEPS), "nd4hip_dgebal_batched: no fixed point after 1024 sweeps.");
  }
  return 0;
}
int ev_flags(nd4hip_handle* h, int64_t batch, int** flags) {
  void* p = nullptr;
  ND4_TRY(nd4_ws_alloc(h, sizeof(int) * (size_t)batch, &p));
  *flags = static_cast<int*>(p);
  ND4_HIP(hipMemsetAsync(p, 0, sizeof(int) * (size_t)batch, h->stream));
  return 0;
}
}  // namespace

extern "C" int nd4hip_dtreval_batched_dev(nd4hip_handle* h, int64_t batch, int64_t N, const double* T, double* Lam) {
  ND4_CHECK_ARG(h != nullptr, "nd4hip_dtreval_batched: NULL handle");
  Nd4DeviceGuard guard(h);
  Nd4Prof prof(h, "dtreval_batched", 8.0 * (double)batch * N, 8.0 * (double)batch * 5.0 * N);
  ND4_ARGS(nd4_args_ev("dtreval_batched", EV_MAX_N, batch, N, {T, Lam}));
  Nd4WsScope scope(h);
  int* flags = nullptr;
  ND4_TRY(ev_flags(h, batch, &flags));
  ND4_TRY(nd4_trevals(h, batch, N, T, Lam, nullptr, flags));
  return ev_verdict(h, flags, batch);
}

extern "C" int nd4hip_dtrevc_batched_dev(nd4hip_handle* h, int64_t batch, int64_t N, const double* Q, const double* T, double* Lam, double* V) {
  ND4_CHECK_ARG(h != nullptr, "nd4hip_dtrevc_batched: NULL handle");
  Nd4DeviceGuard guard(h);
  const double n = (double)N;
  Nd4Prof prof(h, "dtrevc_batched", (double)batch * (4.0 / 3.0 * n * n * n + 4.0 * n * n * n), 8.0 * (double)batch * (4.0 * n * n + 2.0 * n));
  ND4_ARGS(nd4_args_ev("dtrevc_batched", EV_MAX_N, batch, N, {Q, T, Lam, V}));
  Nd4WsScope scope(h);
  int* flags = nullptr;
  ND4_TRY(ev_flags(h, batch, &flags));
  ND4_FOR_CHUNKS(batch) ND4_TRY(nd4_trevc(h, nb, N, Q + b0 * N * N, T + b0 * N * N, Lam + 2 * b0 * N, V + 2 * b0 * N * N, flags + b0));
  return ev_verdict(h, flags, batch);
}

extern "C" int nd4hip_dgebal_batched_dev(nd4hip_handle* h, int64_t batch, int64_t N, double p, const double* A, double* D, double* B) {
  ND4_CHECK_ARG(h != nullptr, "nd4hip_dgebal_batched: NULL handle");
  Nd4DeviceGuard guard(h);
  Nd4Prof prof(h, "dgebal_batched", 6.0 * (double)batch * N * N, 8.0 * (double)batch * (4.0 * N * N + N));   // per sweep; two sweeps are typical
  ND4_ARGS(nd4_args_gebal(batch, N, p, A, D, B));
  Nd4WsScope scope(h);
  int* flags = nullptr;
  ND4_TRY(ev_flags(h, batch, &flags));
  ND4_FOR_CHUNKS(batch) ND4_TRY(nd4_gebal(h, nb, N, p, A + b0 * N * N, D + b0 * N, B + b0 * N * N, flags + b0));
  return ev_verdict(h, flags, batch);
}

extern "C" int nd4hip_zgebak_batched_dev(nd4hip_handle* h, int64_t batch, int64_t N, const double* D, const double* V, double* W) {
  ND4_CHECK_ARG(h != nullptr, "nd4hip_zgebak_batched: NULL handle");
  Nd4DeviceGuard guard(h);
  Nd4Prof prof(h, "zgebak_batched", 10.0 * (double)batch * N * N, 8.0 * (double)batch * (8.0 * N * N + N));
  ND4_ARGS(nd4_args_gebak(true, batch, N, D, V, W));
  ND4_FOR_CHUNKS(batch) ND4_TRY(nd4_gebak(h, nb, N, D + b0 * N, V + 2 * b0 * N * N, W + 2 * b0 * N * N));
  return 0;
}

// ---- schur_decomp (schur.js:372-683), eigen / eigenvals (eigen.js:33-88)
namespace {
// flag words and sweep counts of the batch in one read-back; *sweeps_max (may be NULL) receives the largest count
int hseqr_verdict(nd4hip_handle* h, const int* fs, int64_t batch, int* sweeps_max) {
  const int* host = nullptr;
  ND4_TRY(read_flags(h, fs, 2 * (size_t)batch, &host));
  int mx = 0;
  for (int64_t b = 0; b < batch; b++) if (host[batch + b] > mx) mx = host[batch + b];
  if (sweeps_max) *sweeps_max = mx;
  for (int64_t b = 0; b < batch; b++) {
    ND4_CHECK_ARG(!(host[b] & ND4HIP_EV_FLAG_ASSERT), "Assertion failed.");
    if (host[b] & ND4HIP_EV_FLAG_NOCONV) {
      nd4_set_error("nd4hip_dhseqr_batched: no convergence after 30 max(10, n) sweeps of one francis_qr call.");
      return ND4HIP_ERR_NOCONV;
    }
  }
  return 0;
}
}  // namespace

extern "C" int nd4hip_dhseqr_batched_ex_dev(nd4hip_handle* h, int64_t batch, int64_t N, const double* U, const double* H, double* Q, double* T,
                                            int* sweeps_out, int tier) {
  ND4_CHECK_ARG(h != nullptr, "nd4hip_dhseqr_batched: NULL handle");
  Nd4DeviceGuard guard(h);
  const double n = (double)N;
  Nd4Prof prof(h, "dhseqr_batched", 25.0 * (double)batch * n * n * n, 8.0 * (double)batch * 4.0 * n * n);
  if (sweeps_out) *sweeps_out = 0;
  ND4_ARGS(nd4_args_hseqr(batch, N, U, H, Q, T, tier));
  Nd4WsScope scope(h);
  void* p = nullptr;
  ND4_TRY(nd4_ws_alloc(h, sizeof(int) * 2 * (size_t)batch, &p));                  // flag words, then sweep counts
  int* fs = static_cast<int*>(p);
  ND4_HIP(hipMemsetAsync(fs, 0, sizeof(int) * 2 * (size_t)batch, h->stream));
  const int64_t chunk = nd4_hseqr_chunk(N);
  for (int64_t b0 = 0; b0 < batch; b0 += chunk) {
    const int64_t nb = batch - b0 < chunk ? batch - b0 : chunk;
    ND4_TRY(nd4_hseqr(h, nb, N, U + b0 * N * N, H + b0 * N * N, Q + b0 * N * N, T + b0 * N * N, fs + b0, fs + batch + b0, tier));
  }
  return hseqr_verdict(h, fs, batch, sweeps_out);
}
extern "C" int nd4hip_dhseqr_batched_dev(nd4hip_handle* h, int64_t batch, int64_t N, const double* U, const double* H, double* Q, double* T,
                                         int* sweeps_out) {
  return nd4hip_dhseqr_batched_ex_dev(h, batch, N, U, H, Q, T, sweeps_out, ND4HIP_SCHUR_TIER_AUTO);
}

extern "C" int nd4hip_dgees_batched_dev(nd4hip_handle* h, int64_t batch, int64_t N, const double* A, double* Q, double* T, int* sweeps_out) {
  ND4_CHECK_ARG(h != nullptr, "nd4hip_dgees_batched: NULL handle");
  Nd4DeviceGuard guard(h);
  const double n = (double)N;
  Nd4Prof prof(h, "dgees_batched", (25.0 + 14.0 / 3.0) * (double)batch * n * n * n, 8.0 * (double)batch * 3.0 * n * n);
  if (sweeps_out) *sweeps_out = 0;
  ND4_ARGS(nd4_args_ev("dgees_batched", INT64_MAX, batch, N, {A, Q, T}));
  ND4_TRY(nd4hip_dgehrd_batched_dev(h, batch, N, A, Q, T));
  return nd4hip_dhseqr_batched_dev(h, batch, N, Q, T, Q, T, sweeps_out);
}

extern "C" int nd4hip_dgeev_batched_dev(nd4hip_handle* h, int64_t batch, int64_t N, const double* A, double* Lam, double* V) {
  ND4_CHECK_ARG(h != nullptr, "nd4hip_dgeev_batched: NULL handle");
  Nd4DeviceGuard guard(h);
  const double n = (double)N;
  Nd4Prof prof(h, "dgeev_batched", (25.0 + 14.0 / 3.0 + (V ? 16.0 / 3.0 : 0.0)) * (double)batch * n * n * n, 8.0 * (double)batch * (V ? 3.0 : 1.0) * n * n);
  ND4_ARGS(nd4_args_ev("dgeev_batched", INT64_MAX, batch, N, {A, Lam}));
  // eigen.js:33-88 per chunk, the intermediates in the workspace: D [N], B, Q, T [N, N] and the eigenvectors before zgebak
  const int64_t chunk = nd4_hseqr_chunk(N);
  for (int64_t b0 = 0; b0 < batch; b0 += chunk) {
    const int64_t nb = batch - b0 < chunk ? batch - b0 : chunk;
    Nd4WsScope scope(h);
    void *pd = nullptr, *pb = nullptr, *pq = nullptr, *pt = nullptr, *pv = nullptr;
    ND4_TRY(nd4_ws_alloc(h, sizeof(double) * (size_t)(nb * N), &pd));
    ND4_TRY(nd4_ws_alloc(h, sizeof(double) * (size_t)(nb * N * N), &pb));
    ND4_TRY(nd4_ws_alloc(h, sizeof(double) * (size_t)(nb * N * N), &pq));
    ND4_TRY(nd4_ws_alloc(h, sizeof(double) * (size_t)(nb * N * N), &pt));
    if (V) ND4_TRY(nd4_ws_alloc(h, 2 * sizeof(double) * (size_t)(nb * N * N), &pv));
    double *D = static_cast<double*>(pd), *B = static_cast<double*>(pb), *Q = static_cast<double*>(pq), *T = static_cast<double*>(pt),
           *X = static_cast<double*>(pv);
    ND4_TRY(nd4hip_dgebal_batched_dev(h, nb, N, 2.0, A + b0 * N * N, D, B));
    ND4_TRY(nd4hip_dgees_batched_dev(h, nb, N, B, Q, T, nullptr));
    if (!V) { ND4_TRY(nd4hip_dtreval_batched_dev(h, nb, N, T, Lam + 2 * b0 * N)); continue; }
    ND4_TRY(nd4hip_dtrevc_batched_dev(h, nb, N, Q, T, Lam + 2 * b0 * N, X));
    ND4_TRY(nd4hip_zgebak_batched_dev(h, nb, N, D, X, V + 2 * b0 * N * N));
  }
  return 0;
}

// rrqr_rank (rrqr.js:398-414): rank [batch] of R [M, N]; -1 marks a matrix whose partial norms are not finite
extern "C" int nd4hip_dqp3rank_batched_dev(nd4hip_handle* h, int64_t batch, int64_t M, int64_t N, const double* R, int32_t* rank) {
  ND4_CHECK_ARG(h != nullptr, "nd4hip_dqp3rank_batched: NULL handle");
  Nd4DeviceGuard guard(h);
  const int64_t L = M < N ? M : N;
  Nd4Prof prof(h, "dqp3rank_batched", 3.0 * batch * (double)(L * N - L * (L - 1) / 2), 8.0 * batch * (double)(L * N - L * (L - 1) / 2) + 4.0 * batch);
  ND4_ARGS(nd4_args_qp3rank(batch, M, N, R, rank));
  ND4_FOR_CHUNKS(batch) ND4_TRY(nd4_qp3rank(h, nb, M, N, R + b0 * M * N, M * N, rank + b0));
  return 0;
}

// rrqr_lstsq (rrqr.js:447-580): Q [N, M], R [M, I], P [I], Y [N, J] -> X [I, J]; rank [batch] (may be NULL) as dqp3rank
extern "C" int nd4hip_dqp3ls_batched_dev(nd4hip_handle* h, int64_t batch, int64_t N, int64_t M, int64_t I, int64_t J,
                                         const double* Q, int64_t strideQ, const double* R, int64_t strideR, const int32_t* P, int64_t strideP,
                                         const double* Y, int64_t strideY, double* X, int32_t* rank) {
  ND4_CHECK_ARG(h != nullptr, "nd4hip_dqp3ls_batched: NULL handle");
  Nd4DeviceGuard guard(h);
  const int64_t L = M < I ? M : I;
  Nd4Prof prof(h, "dqp3ls_batched", (double)batch * (2.0 * L * N * J + (double)L * L * J),
               8.0 * (double)((strideQ ? batch : 1) * N * M + (strideR ? batch : 1) * M * I + (strideY ? batch : 1) * N * J + batch * I * J));
  ND4_ARGS(nd4_args_qp3ls(batch, N, M, I, J, Q, strideQ, R, strideR, P, strideP, Y, strideY, X));
  if (I == 0 || J == 0) {
    if (rank) ND4_FOR_CHUNKS(batch) ND4_TRY(nd4_qp3rank(h, nb, M, I, R ? R + b0 * strideR : nullptr, strideR, rank + b0));
    return 0;
  }
  ND4_FOR_CHUNKS(batch) ND4_TRY(nd4_qp3ls(h, nb, N, M, I, J, Q + b0 * strideQ, strideQ, R + b0 * strideR, strideR, P + b0 * strideP, strideP,
                                          Y + b0 * strideY, strideY, X + b0 * I * J, rank ? rank + b0 : nullptr));
  return 0;
}

// ------------------------------------------------------------------------------------ SVD
extern "C" int nd4hip_dgesvdj_batched_dev(nd4hip_handle* h, int64_t batch, int64_t M, int64_t N, const double* A,
                                          double* U, double* sv, double* V, int* sweeps_out, double* offnorm_out) {
  ND4_CHECK_ARG(h != nullptr, "nd4hip_dgesvdj_batched: NULL handle");
  Nd4DeviceGuard guard(h);
  Nd4Prof prof(h, "dgesvdj_batched", (double)(batch * nd4_flops_svd(M, N)), (double)(8.0 * batch * (double)(M * N + (M + N + 1) * (M < N ? M : N))));
  if (sweeps_out) *sweeps_out = 0;
  if (offnorm_out) *offnorm_out = 0.0;
  ND4_ARGS(nd4_args_dense("dgesvdj_batched", {batch, M, N}, {A, U, sv, V}));
  {
    const int64_t L = M < N ? M : N;
    int sweeps = 0; double off = 0.0; unsigned long long rot = 0;
    ND4_FOR_CHUNKS(batch) {
      int sw = 0; double of = 0.0;
      ND4_TRY(nd4_gesvdj(h, nb, M, N, A + b0 * M * N, U + b0 * M * L, sv + b0 * L, V + b0 * L * N, &sw, &of));
      if (sw > sweeps) sweeps = sw;
      if (of > off) off = of;
      rot += h->svd_rotations;
    }
    h->svd_sweeps = sweeps; h->svd_offnorm = off; h->svd_rotations = rot;
    if (sweeps_out) *sweeps_out = sweeps;
    if (offnorm_out) *offnorm_out = off;
  }
  return 0;
}

// ---- svd_decomp by divide & conquer (svd_dc.js:883-932) and its bidiagonal solver (svd_dc.hip)
extern "C" int nd4hip_dbdsdc_levels(int64_t n, int32_t* nodes, int64_t capacity) {
  ND4_CHECK_ARG(n >= 2 && n <= (1 << 20), "nd4hip_dbdsdc_levels: 2 <= n <= 2^20 columns");
  ND4_CHECK_ARG(capacity >= 0 && (nodes || capacity == 0), "nd4hip_dbdsdc_levels: NULL nodes");
  return nd4_bdsdc_plan(n, nodes, capacity);
}

extern "C" int nd4hip_dbdsdc_batched_dev(nd4hip_handle* h, int64_t batch, int64_t K, int64_t J, const double* d, const double* e,
                                         double* U2, double* sv, double* V2) {
  ND4_CHECK_ARG(h != nullptr, "nd4hip_dbdsdc_batched: NULL handle");
  Nd4DeviceGuard guard(h);
  // the merges: about 2 K^3 flops each for U and for V over the whole tree
  Nd4Prof prof(h, "dbdsdc_batched", 4.0 * batch * (double)K * K * K, 8.0 * batch * (double)(2 * K + J - 1 + K * K + J * J));
  ND4_ARGS(nd4_args_bdsdc(batch, K, J, d, e, U2, sv, V2));
  ND4_FOR_CHUNKS(batch) ND4_TRY(nd4_bdsdc_rows(h, nb, K, J, d + b0 * K, e ? e + b0 * (J - 1) : nullptr, U2 + b0 * K * K, sv + b0 * K, V2 + b0 * J * J));
  return 0;
}

extern "C" int nd4hip_dgesdd_batched_dev(nd4hip_handle* h, int64_t batch, int64_t M, int64_t N, const double* A,
                                         double* U, double* sv, double* V) {
  ND4_CHECK_ARG(h != nullptr, "nd4hip_dgesdd_batched: NULL handle");
  Nd4DeviceGuard guard(h);
  Nd4Prof prof(h, "svd_dc", (double)(batch * nd4_flops_svd(M, N)), (double)(8.0 * batch * (double)(M * N + (M + N + 1) * (M < N ? M : N))));
  ND4_ARGS(nd4_args_dense("dgesdd_batched", {batch, M, N}, {A, U, sv, V}));
  { const int64_t L = M < N ? M : N;
    ND4_FOR_CHUNKS(batch) ND4_TRY(nd4_gesdd(h, nb, M, N, A + b0 * M * N, U + b0 * M * L, sv + b0 * L, V + b0 * L * N)); }
  return 0;
}

extern "C" int nd4hip_dgesdd_last_stages(nd4hip_handle* h, double* ms, int capacity) {
  ND4_CHECK_ARG(h != nullptr && (ms != nullptr || capacity <= 0), "nd4hip_dgesdd_last_stages: NULL argument");
  for (int i = 0; i < capacity && i < ND4HIP_DC_STAGES; ++i) ms[i] = h->dc_stage_ms[i];
  return ND4HIP_DC_STAGES;
}

// ---- selected singular triplets (bdsvdx.hip). The argument checks come first: they need no handle. Algorithmic flops:
// a Sturm count of the Golub-Kahan matrix is 3 (K + J), a bisection about 55 of them per value, an inverse iteration 13 (K + J) per
// vector and round; dgesvdx: 8/3 m^2 (3 n - m) for the bidiagonalisation with U_b and V_b, 2 m k (m + n) for the two products
extern "C" int nd4hip_dbdsvdx_batched_dev(nd4hip_handle* h, int64_t batch, int64_t K, int64_t J, int64_t i0, int64_t i1, const double* d,
                                          const double* e, double* U2, double* sv, double* V2, int32_t* fallback) {
  ND4_ARGS(nd4_args_bdsvdx(batch, K, J, i0, i1, d, e, U2, sv, V2));
  ND4_CHECK_ARG(h != nullptr, "nd4hip_dbdsvdx_batched: NULL handle");
  Nd4DeviceGuard guard(h);
  const int64_t k = i1 - i0, n = K + J;
  Nd4Prof prof(h, "dbdsvdx_batched", batch * (double)k * n * (165.0 + (U2 ? 39.0 : 0.0)), 8.0 * batch * (double)(n - 1 + k + (U2 ? k * n : 0)));
  ND4_FOR_CHUNKS(batch)
    ND4_TRY(nd4_bdsvdx(h, nb, K, J, i0, i1, d + b0 * K, e ? e + b0 * (J - 1) : nullptr, U2 ? U2 + b0 * K * k : nullptr, sv + b0 * k,
                       V2 ? V2 + b0 * k * J : nullptr, fallback ? fallback + b0 : nullptr));
  return 0;
}
extern "C" int nd4hip_dgesvdx_batched_dev(nd4hip_handle* h, int64_t batch, int64_t M, int64_t N, int64_t i0, int64_t i1, const double* A, double* U,
                                          double* sv, double* V, int32_t* fallback) {
  ND4_ARGS(nd4_args_gesvdx(batch, M, N, i0, i1, A, U, sv, V));
  ND4_CHECK_ARG(h != nullptr, "nd4hip_dgesvdx_batched: NULL handle");
  Nd4DeviceGuard guard(h);
  const int64_t k = i1 - i0;
  const double m = (double)(M < N ? M : N), n = (double)(M < N ? N : M);
  Nd4Prof prof(h, "dgesvdx_batched", batch * (8.0 / 3.0 * m * m * (3.0 * n - m) + (U ? 2.0 * m * k * (m + n) : 0.0)),
               8.0 * batch * (double)(M * N + k + (U ? (M + N) * k : 0)));
  ND4_FOR_CHUNKS(batch)
    ND4_TRY(nd4_gesvdx(h, nb, M, N, i0, i1, A + b0 * M * N, U ? U + b0 * M * k : nullptr, sv + b0 * k, V ? V + b0 * k * N : nullptr,
                       fallback ? fallback + b0 : nullptr));
  return 0;
}
extern "C" int nd4hip_dgesvdx_last_stages(nd4hip_handle* h, double* ms, int capacity) {
  ND4_CHECK_ARG(h != nullptr && (ms != nullptr || capacity <= 0), "nd4hip_dgesvdx_last_stages: NULL argument");
  for (int i = 0; i < capacity && i < ND4HIP_SVDX_STAGES; ++i) ms[i] = h->svdx_stage_ms[i];
  return ND4HIP_SVDX_STAGES;
}

// ---- eigen_sym / eigenvals_sym (syev.hip). Algorithmic flops per matrix: 10/3 N^3 for the reduction with U (4/3 N^3 for T, 2 N^3
// for U), 2 N^3 for the eigenvector half of the solver's merges, 2 N^3 for V = U V2^T; without V the last term drops out
extern "C" int nd4hip_dsyevd_batched_dev(nd4hip_handle* h, int64_t batch, int64_t N, const double* S, double* lambda, double* V) {
  ND4_CHECK_ARG(h != nullptr, "nd4hip_dsyevd_batched: NULL handle");
  Nd4DeviceGuard guard(h);
  const double n3 = (double)N * N * N;
  Nd4Prof prof(h, "dsyevd_batched", batch * ((10.0 / 3.0 + 2.0 + (V ? 2.0 : 0.0)) * n3), 8.0 * batch * (double)(N * N / 2 + N + (V ? N * N : 0)));
  ND4_ARGS(nd4_args_syev("dsyevd_batched", false, batch, N, S, lambda));
  ND4_FOR_CHUNKS(batch) ND4_TRY(nd4_syevd(h, nb, N, S + b0 * N * N, lambda + b0 * N, V ? V + b0 * N * N : nullptr));
  return 0;
}

// ---- eigen_sym / eigenvals_sym, algo = 'jacobi' (syevj.hip). The sweep count is not known beforehand: the profile counts 8 sweeps
// (what a dense matrix of N <= 128 needs, give or take two) of 4 N^3 flops for S (2 x 2 blocks of the lower triangle, two
// rotations each) and 4 N^3 for V^T
extern "C" int nd4hip_dsyevj_batched_dev(nd4hip_handle* h, int64_t batch, int64_t N, const double* S, double* lambda, double* V, int32_t* sweeps) {
  ND4_CHECK_ARG(h != nullptr, "nd4hip_dsyevj_batched: NULL handle");
  Nd4DeviceGuard guard(h);
  const double n3 = (double)N * N * N;
  Nd4Prof prof(h, "syevj", batch * 8.0 * (V ? 8.0 : 4.0) * n3, 8.0 * batch * (double)(N * N / 2 + N + (V ? N * N : 0)));
  ND4_ARGS(nd4_args_syev("dsyevj_batched", true, batch, N, S, lambda));
  ND4_FOR_CHUNKS(batch) ND4_TRY(nd4_syevj(h, nb, N, S + b0 * N * N, lambda + b0 * N, V ? V + b0 * N * N : nullptr, sweeps ? sweeps + b0 : nullptr));
  return 0;
}

// ---- selected eigenpairs by bisection and inverse iteration (syevx.hip). The argument checks come first: they need no handle.
// Algorithmic flops: a Sturm count is 3 N; a bisection takes about 55 of them per value; an inverse iteration is 13 N per vector and
// round; dsyevx: 10/3 N^3 for the reduction with U and 2 N^2 k for V = U Z^T
extern "C" int nd4hip_dstcnt_batched_dev(nd4hip_handle* h, int64_t batch, int64_t N, int64_t M, const double* d, const double* e, const double* x,
                                         int32_t* count) {
  ND4_ARGS(nd4_args_stcnt(batch, N, M, d, e, x, count));
  ND4_CHECK_ARG(h != nullptr, "nd4hip_dstcnt_batched: NULL handle");
  Nd4DeviceGuard guard(h);
  Nd4Prof prof(h, "dstcnt_batched", 3.0 * batch * (double)N * M, 8.0 * batch * (double)(2 * N + M) + 4.0 * batch * (double)M);
  const int64_t ne = N > 1 ? N - 1 : 0;
  ND4_FOR_CHUNKS(batch) ND4_TRY(nd4_stcnt(h, nb, N, M, d + b0 * N, e ? e + b0 * ne : nullptr, x + b0 * M, count + b0 * M));
  return 0;
}
extern "C" int nd4hip_dstevx_batched_dev(nd4hip_handle* h, int64_t batch, int64_t N, int64_t i0, int64_t i1, const double* d, const double* e,
                                         double* lambda, double* Z) {
  ND4_ARGS(nd4_args_stevx(batch, N, i0, i1, d, e, lambda));
  ND4_CHECK_ARG(h != nullptr, "nd4hip_dstevx_batched: NULL handle");
  Nd4DeviceGuard guard(h);
  const int64_t k = i1 - i0, ne = N > 1 ? N - 1 : 0;
  Nd4Prof prof(h, "dstevx_batched", batch * (double)k * N * (165.0 + (Z ? 39.0 : 0.0)), 8.0 * batch * (double)(2 * N + k + (Z ? k * N : 0)));
  ND4_FOR_CHUNKS(batch)
    ND4_TRY(nd4_stevx(h, nb, N, i0, i1, d + b0 * N, e ? e + b0 * ne : nullptr, lambda + b0 * k, Z ? Z + b0 * k * N : nullptr));
  return 0;
}
extern "C" int nd4hip_dsyevx_batched_dev(nd4hip_handle* h, int64_t batch, int64_t N, int64_t i0, int64_t i1, const double* S, double* lambda,
                                         double* V) {
  ND4_ARGS(nd4_args_syevx(batch, N, i0, i1, S, lambda));
  ND4_CHECK_ARG(h != nullptr, "nd4hip_dsyevx_batched: NULL handle");
  Nd4DeviceGuard guard(h);
  const int64_t k = i1 - i0;
  const double n2 = (double)N * N;
  Nd4Prof prof(h, "dsyevx_batched", batch * (10.0 / 3.0 * n2 * N + (V ? 2.0 * n2 * k : 0.0)), 8.0 * batch * (double)(N * N / 2 + k + (V ? N * k : 0)));
  ND4_FOR_CHUNKS(batch) ND4_TRY(nd4_syevx(h, nb, N, i0, i1, S + b0 * N * N, lambda + b0 * k, V ? V + b0 * N * k : nullptr));
  return 0;
}
extern "C" int nd4hip_dsyevx_last_stages(nd4hip_handle* h, double* ms, int capacity) {
  ND4_CHECK_ARG(h != nullptr && (ms != nullptr || capacity <= 0), "nd4hip_dsyevx_last_stages: NULL argument");
  for (int i = 0; i < capacity && i < ND4HIP_SYEVX_STAGES; ++i) ms[i] = h->syevx_stage_ms[i];
  return ND4HIP_SYEVX_STAGES;
}

// ---- symmetric tridiagonal reduction, its Q and the eigen routes on them (sytrd.hip). The argument checks come
// first: they need no handle. Flops: 4/3 N^3 for the reduction, 2 N^2 K for Q Z; the eigen routes add the solver's 2 N^3 (dsyevd)
extern "C" int nd4hip_dsytrd_batched_dev(nd4hip_handle* h, int64_t batch, int64_t N, const double* S, double* F, double* tau, double* d, double* e) {
  ND4_ARGS(nd4_args_sytrd(batch, N, S, F, tau, d, e));
  ND4_CHECK_ARG(h != nullptr, "nd4hip_dsytrd_batched: NULL handle");
  Nd4DeviceGuard guard(h);
  const double n2 = (double)N * N;
  Nd4Prof prof(h, "dsytrd_batched", batch * (4.0 / 3.0 * n2 * N), 8.0 * batch * (double)(N * N / 2 + N * N + 3 * N));
  const int64_t ne = N > 1 ? N - 1 : 0;
  ND4_FOR_CHUNKS(batch)
    ND4_TRY(nd4_sytrd_run(h, nb, N, S + b0 * N * N, F + b0 * N * N, tau ? tau + b0 * ne : nullptr, d + b0 * N, e ? e + b0 * ne : nullptr));
  return 0;
}
extern "C" int nd4hip_dormtr_batched_dev(nd4hip_handle* h, int64_t batch, int64_t N, int64_t K, int transpose, const double* F,
                                         const double* tau, double* Z) {
  ND4_ARGS(nd4_args_ormtr(batch, N, K, transpose, F, tau, Z));
  ND4_CHECK_ARG(h != nullptr, "nd4hip_dormtr_batched: NULL handle");
  Nd4DeviceGuard guard(h);
  Nd4Prof prof(h, "dormtr_batched", batch * (2.0 * N * (double)N * K), 8.0 * batch * (double)(N * N / 2 + 2 * N * K));
  const int64_t ne = N > 1 ? N - 1 : 0;
  ND4_FOR_CHUNKS(batch) ND4_TRY(nd4_ormtr(h, nb, N, K, transpose != 0, F + b0 * N * N, tau ? tau + b0 * ne : nullptr, Z + b0 * N * K));
  return 0;
}
extern "C" int nd4hip_dsyevd_tr_batched_dev(nd4hip_handle* h, int64_t batch, int64_t N, const double* S, double* lambda, double* V) {
  ND4_ARGS(nd4_args_syevd_tr(batch, N, S, lambda));
  ND4_CHECK_ARG(h != nullptr, "nd4hip_dsyevd_tr_batched: NULL handle");
  Nd4DeviceGuard guard(h);
  const double n3 = (double)N * N * N;
  Nd4Prof prof(h, "dsyevd_tr_batched", batch * ((4.0 / 3.0 + 2.0 + (V ? 2.0 : 0.0)) * n3), 8.0 * batch * (double)(N * N / 2 + N + (V ? N * N : 0)));
  ND4_FOR_CHUNKS(batch) ND4_TRY(nd4_syevd_tr(h, nb, N, S + b0 * N * N, lambda + b0 * N, V ? V + b0 * N * N : nullptr));
  return 0;
}
extern "C" int nd4hip_dsyevx_tr_batched_dev(nd4hip_handle* h, int64_t batch, int64_t N, int64_t i0, int64_t i1, const double* S, double* lambda,
                                            double* V) {
  ND4_ARGS(nd4_args_syevx_tr(batch, N, i0, i1, S, lambda));
  ND4_CHECK_ARG(h != nullptr, "nd4hip_dsyevx_tr_batched: NULL handle");
  Nd4DeviceGuard guard(h);
  const int64_t k = i1 - i0;
  const double n2 = (double)N * N;
  Nd4Prof prof(h, "dsyevx_tr_batched", batch * (4.0 / 3.0 * n2 * N + (V ? 2.0 * n2 * k : 0.0)), 8.0 * batch * (double)(N * N / 2 + k + (V ? N * k : 0)));
  ND4_FOR_CHUNKS(batch) ND4_TRY(nd4_syevx_tr(h, nb, N, i0, i1, S + b0 * N * N, lambda + b0 * k, V ? V + b0 * N * k : nullptr));
  return 0;
}

// ---- Hermitian tridiagonal reduction, its Q and the eigen routes on them (hetrd.hip): complex128 operands as
// interleaved doubles. The argument checks come first: they need no handle. Flops are real ones: four times the real routes' counts
// where the operands are complex (16/3 N^3 for the reduction, 8 N^2 K for Q Z); the real solver's 2 N^3 stay
extern "C" int nd4hip_zhetrd_batched_dev(nd4hip_handle* h, int64_t batch, int64_t N, const double* H, double* F, double* tau, double* d, double* e) {
  ND4_ARGS(nd4_args_hetrd(batch, N, H, F, tau, d, e));
  ND4_CHECK_ARG(h != nullptr, "nd4hip_zhetrd_batched: NULL handle");
  Nd4DeviceGuard guard(h);
  const double n2 = (double)N * N;
  Nd4Prof prof(h, "zhetrd_batched", batch * (16.0 / 3.0 * n2 * N), 16.0 * batch * (double)(N * N / 2 + N * N + 2 * N));
  const int64_t ne = N > 1 ? N - 1 : 0;
  ND4_FOR_CHUNKS(batch)
    ND4_TRY(nd4_hetrd_run(h, nb, N, H + 2 * b0 * N * N, F + 2 * b0 * N * N, tau ? tau + 2 * b0 * ne : nullptr, d + b0 * N, e ? e + b0 * ne : nullptr));
  return 0;
}
extern "C" int nd4hip_zunmtr_batched_dev(nd4hip_handle* h, int64_t batch, int64_t N, int64_t K, int adjoint, const double* F, const double* tau,
                                         double* Z) {
  ND4_ARGS(nd4_args_unmtr(batch, N, K, adjoint, F, tau, Z));
  ND4_CHECK_ARG(h != nullptr, "nd4hip_zunmtr_batched: NULL handle");
  Nd4DeviceGuard guard(h);
  Nd4Prof prof(h, "zunmtr_batched", batch * (8.0 * N * (double)N * K), 16.0 * batch * (double)(N * N / 2 + 2 * N * K));
  const int64_t ne = N > 1 ? N - 1 : 0;
  ND4_FOR_CHUNKS(batch)
    ND4_TRY(nd4_zunmtr(h, nb, N, K, adjoint != 0, F + 2 * b0 * N * N, tau ? tau + 2 * b0 * ne : nullptr, Z + 2 * b0 * N * K));
  return 0;
}
extern "C" int nd4hip_zheevd_batched_dev(nd4hip_handle* h, int64_t batch, int64_t N, const double* H, double* lambda, double* V) {
  ND4_ARGS(nd4_args_heevd(batch, N, H, lambda));
  ND4_CHECK_ARG(h != nullptr, "nd4hip_zheevd_batched: NULL handle");
  Nd4DeviceGuard guard(h);
  const double n3 = (double)N * N * N;
  Nd4Prof prof(h, "zheevd_batched", batch * ((16.0 / 3.0 + 2.0 + (V ? 8.0 : 0.0)) * n3), 8.0 * batch * (double)(N * N + N + (V ? 2 * N * N : 0)));
  ND4_FOR_CHUNKS(batch) ND4_TRY(nd4_zheevd(h, nb, N, H + 2 * b0 * N * N, lambda + b0 * N, V ? V + 2 * b0 * N * N : nullptr));
  return 0;
}
extern "C" int nd4hip_zheevx_batched_dev(nd4hip_handle* h, int64_t batch, int64_t N, int64_t i0, int64_t i1, const double* H, double* lambda,
                                         double* V) {
  ND4_ARGS(nd4_args_heevx(batch, N, i0, i1, H, lambda));
  ND4_CHECK_ARG(h != nullptr, "nd4hip_zheevx_batched: NULL handle");
  Nd4DeviceGuard guard(h);
  const int64_t k = i1 - i0;
  const double n2 = (double)N * N;
  Nd4Prof prof(h, "zheevx_batched", batch * (16.0 / 3.0 * n2 * N + (V ? 8.0 * n2 * k : 0.0)), 8.0 * batch * (double)(N * N + k + (V ? 2 * N * k : 0)));
  ND4_FOR_CHUNKS(batch) ND4_TRY(nd4_zheevx(h, nb, N, i0, i1, H + 2 * b0 * N * N, lambda + b0 * k, V ? V + 2 * b0 * N * k : nullptr));
  return 0;
}

// ---- the eigenpairs in a value interval (syevx.hip). The argument checks come first: they need no handle. How many
// values an interval holds is not known when the profile opens: it counts the reduction and the two Sturm counts per member.
namespace {
// `run(b0, nb, &kmax_of_the_chunk)` for every chunk of the batch; *kmax is the largest; where the chunks found different kmax the
// padding of every member is extended to it
template <class Run>
int interval_chunks(nd4hip_handle* h, int64_t batch, int64_t N, int64_t kcap, const int32_t* range, double* lambda, double* vectors, bool by_rows,
                    int64_t* kmax, Run run) {
  int64_t km = 0; bool uneven = false;
  *kmax = 0;
  ND4_FOR_CHUNKS(batch) {
    int64_t kc = 0;
    ND4_TRY(run(b0, nb, &kc));
    uneven = uneven || (b0 > 0 && kc != km);
    km = kc > km ? kc : km;
  }
  *kmax = km;
  if (uneven) {
    ND4_TRY(nd4_stxv_pad(h, batch, N, kcap, km, range, lambda, vectors, by_rows));
    ND4_HIP(hipStreamSynchronize(h->stream));
  }
  return 0;
}
int syevxv_dev(nd4hip_handle* h, bool tridiag, int64_t batch, int64_t N, int64_t kcap, const double* bounds, const double* S, double* lambda,
               double* V, int32_t* range, int64_t* kmax) {
  ND4_ARGS(nd4_args_syevxv(tridiag, batch, N, kcap, bounds, S, lambda, range, kmax));
  ND4_CHECK_ARG(h != nullptr, "nd4hip_%s: NULL handle", tridiag ? "dsyevxv_tr_batched" : "dsyevxv_batched");
  Nd4DeviceGuard guard(h);
  const double n2 = (double)N * N;
  Nd4Prof prof(h, tridiag ? "dsyevxv_tr_batched" : "dsyevxv_batched", batch * ((tridiag ? 4.0 : 10.0) / 3.0 * n2 * N + 6.0 * N),
               8.0 * batch * (double)(N * N / 2 + 2) + 8.0 * batch);
  return interval_chunks(h, batch, N, kcap, range, lambda, V, false, kmax, [&](int64_t b0, int64_t nb, int64_t* kc) {
    return nd4_syevxv(h, tridiag, nb, N, kcap, bounds + 2 * b0, S + b0 * N * N, lambda + b0 * kcap, V ? V + b0 * N * kcap : nullptr, range + 2 * b0, kc);
  });
}
}  // namespace
extern "C" int nd4hip_dstevxv_batched_dev(nd4hip_handle* h, int64_t batch, int64_t N, int64_t kcap, const double* bounds, const double* d,
                                          const double* e, double* lambda, double* Z, int32_t* range, int64_t* kmax) {
  ND4_ARGS(nd4_args_stevxv(batch, N, kcap, bounds, d, e, lambda, range, kmax));
  ND4_CHECK_ARG(h != nullptr, "nd4hip_dstevxv_batched: NULL handle");
  Nd4DeviceGuard guard(h);
  Nd4Prof prof(h, "dstevxv_batched", 6.0 * batch * (double)N, 8.0 * batch * (double)(2 * N + 2) + 8.0 * batch);
  const int64_t ne = N > 1 ? N - 1 : 0;
  return interval_chunks(h, batch, N, kcap, range, lambda, Z, true, kmax, [&](int64_t b0, int64_t nb, int64_t* kc) {
    return nd4_stevxv(h, nb, N, kcap, bounds + 2 * b0, d + b0 * N, e ? e + b0 * ne : nullptr, lambda + b0 * kcap, Z ? Z + b0 * kcap * N : nullptr,
                      range + 2 * b0, kc);
  });
}
extern "C" int nd4hip_dsyevxv_batched_dev(nd4hip_handle* h, int64_t batch, int64_t N, int64_t kcap, const double* bounds, const double* S,
                                          double* lambda, double* V, int32_t* range, int64_t* kmax) {
  return syevxv_dev(h, false, batch, N, kcap, bounds, S, lambda, V, range, kmax);
}
extern "C" int nd4hip_dsyevxv_tr_batched_dev(nd4hip_handle* h, int64_t batch, int64_t N, int64_t kcap, const double* bounds, const double* S,
                                             double* lambda, double* V, int32_t* range, int64_t* kmax) {
  return syevxv_dev(h, true, batch, N, kcap, bounds, S, lambda, V, range, kmax);
}

// ---- eigen_sym_gen / eigenvals_sym_gen (sygv.hip). Flops: the solver's count above, (1/3 + 2) N^3 for L = chol(B) and the two
// triangular solves of C = L^-1 A L^-T, N^3 for X = L^-T Y
int nd4_sygvd_run(nd4hip_handle* h, int algo, int64_t batch, int64_t N, const double* A, const double* B, int64_t strideB, double* lambda,
                  double* X, int32_t* sweeps, int64_t member0) {
  // the argument checks come first: they need no handle (and are testable without a device)
  ND4_ARGS(nd4_args_sygvd(algo, batch, N, A, B, strideB, lambda));
  ND4_CHECK_ARG(h != nullptr, "nd4hip_dsygvd_batched: NULL handle");
  Nd4DeviceGuard guard(h);
  const double n3 = (double)N * N * N;
  const double solver = algo == 1 ? 8.0 * (X ? 8.0 : 4.0) : 10.0 / 3.0 + 2.0 + (X ? 2.0 : 0.0);
  Nd4Prof prof(h, "dsygvd_batched", batch * ((solver + 1.0 / 3.0 + 2.0 + (X ? 1.0 : 0.0)) * n3),
               8.0 * ((double)(batch + (strideB ? batch : 1)) * (double)(N * N / 2) + batch * (double)(N + (X ? N * N : 0))));
  return nd4_sygvd(h, algo, batch, N, A, B, strideB, lambda, X, algo == 1 ? sweeps : nullptr, member0);
}
extern "C" int nd4hip_dsygvd_batched_dev(nd4hip_handle* h, int algo, int64_t batch, int64_t N, const double* A, const double* B,
                                         int64_t strideB, double* lambda, double* X, int32_t* sweeps) {
  return nd4_sygvd_run(h, algo, batch, N, A, B, strideB, lambda, X, sweeps, 0);
}
// the same with the selectors of step 3 (nd4_sygvx). Flops as above for what is known when the profile opens: the reduction of C
// by either route, the solver's 2 N^3 (+ 2 N^3 with X) for select 0, 2 N^2 k for the vectors of a subset
int nd4_sygvx_run(nd4hip_handle* h, int reduction, int select, int64_t batch, int64_t N, int64_t i0, int64_t i1, int64_t kcap,
                  const double* bounds, const double* A, const double* B, int64_t strideB, double* lambda, double* X, int32_t* range,
                  int64_t* kmax, int64_t member0) {
  ND4_ARGS(nd4_args_sygvx(reduction, select, batch, N, i0, i1, kcap, bounds, A, B, strideB, lambda, range, kmax));
  ND4_CHECK_ARG(h != nullptr, "nd4hip_dsygvx_batched: NULL handle");
  Nd4DeviceGuard guard(h);
  const double n3 = (double)N * N * N, k = select == 1 ? (double)(i1 - i0) : 0.0;
  const double solver = (reduction ? 4.0 : 10.0) / 3.0 + (select == 0 ? 2.0 + (X ? 2.0 : 0.0) : X ? 3.0 * k / N : 0.0);
  Nd4Prof prof(h, "dsygvx_batched", batch * ((solver + 1.0 / 3.0 + 2.0) * n3),
               8.0 * ((double)(batch + (strideB ? batch : 1)) * (double)(N * N / 2) + batch * (double)N));
  const Nd4SygvSel sel{reduction, select, select == 1 ? i0 : 0, select == 1 ? i1 : 0, select == 2 ? kcap : 0, select == 2 ? bounds : nullptr,
                       select == 2 ? range : nullptr, select == 2 ? kmax : nullptr};
  return nd4_sygvx(h, 0, sel, batch, N, A, B, strideB, lambda, X, nullptr, member0);
}
extern "C" int nd4hip_dsygvx_batched_dev(nd4hip_handle* h, int reduction, int select, int64_t batch, int64_t N, int64_t i0, int64_t i1,
                                         int64_t kcap, const double* bounds, const double* A, const double* B, int64_t strideB,
                                         double* lambda, double* X, int32_t* range, int64_t* kmax) {
  return nd4_sygvx_run(h, reduction, select, batch, N, i0, i1, kcap, bounds, A, B, strideB, lambda, X, range, kmax, 0);
}
extern "C" int nd4hip_dsygst_batched_dev(nd4hip_handle* h, int64_t batch, int64_t N, const double* A, const double* L, int64_t strideL,
                                         double* C) {
  // the argument checks come first: they need no handle (and are testable without a device)
  ND4_ARGS(nd4_args_sygst(batch, N, A, L, strideL, C));
  ND4_CHECK_ARG(h != nullptr, "nd4hip_dsygst_batched: NULL handle");
  Nd4DeviceGuard guard(h);
  Nd4Prof prof(h, "dsygst_batched", batch * 2.0 * (double)N * N * N, 8.0 * batch * 2.0 * (double)(N * N));
  return nd4_sygst(h, batch, N, A, L, strideL, C);
}

// ---- herm_cholesky_decomp / herm_cholesky_solve / ztril_solve / herm_gen_reduce / eigen_herm_gen (hegv.hip). The argument
// checks come first: they need no handle. Real flops: 4/3 N^3 for L = chol(B), 8 N^3 for the two-sided reduction, 4 N^2 k for the
// back-transformation of k columns, on top of eigen_herm's count for the same N
int nd4_zpotrf_run(nd4hip_handle* h, int64_t batch, int64_t N, const double* H, double* L, int64_t member0) {
  ND4_ARGS(nd4_args_zpotrf(batch, N, H, L));
  ND4_CHECK_ARG(h != nullptr, "nd4hip_zpotrf_batched: NULL handle");
  Nd4DeviceGuard guard(h);
  Nd4Prof prof(h, "zpotrf_batched", batch * (4.0 / 3.0 * (double)N * N * N), 16.0 * batch * 1.5 * (double)(N * N));
  return nd4_zpotrf(h, batch, N, H, L, member0);
}
extern "C" int nd4hip_zpotrf_batched_dev(nd4hip_handle* h, int64_t batch, int64_t N, const double* H, double* L) {
  return nd4_zpotrf_run(h, batch, N, H, L, 0);
}
extern "C" int nd4hip_zpotrs_batched_dev(nd4hip_handle* h, int64_t batch, int64_t N, int64_t K, const double* L, int64_t strideL,
                                         const double* Y, double* X) {
  ND4_ARGS(nd4_args_zpotrs(batch, N, K, L, strideL, Y, X));
  ND4_CHECK_ARG(h != nullptr, "nd4hip_zpotrs_batched: NULL handle");
  Nd4DeviceGuard guard(h);
  Nd4Prof prof(h, "zpotrs_batched", batch * (8.0 * N * (double)N * K), 16.0 * batch * (double)(N * N / 2 + 2 * N * K));
  if (Y != X) ND4_HIP(hipMemcpyAsync(X, Y, 16 * (size_t)batch * N * K, hipMemcpyDeviceToDevice, h->stream));   // the solve is made in place
  return nd4_ztrsm(h, 2, batch, N, K, L, strideL, X);
}
extern "C" int nd4hip_ztrsm_batched_dev(nd4hip_handle* h, int64_t batch, int64_t N, int64_t K, int adjoint, const double* L, int64_t strideL,
                                        double* X) {
  ND4_ARGS(nd4_args_ztrsm(batch, N, K, adjoint, L, strideL, X));
  ND4_CHECK_ARG(h != nullptr, "nd4hip_ztrsm_batched: NULL handle");
  Nd4DeviceGuard guard(h);
  Nd4Prof prof(h, "ztrsm_batched", batch * (4.0 * N * (double)N * K), 16.0 * batch * (double)(N * N / 2 + 2 * N * K));
  return nd4_ztrsm(h, adjoint ? 1 : 0, batch, N, K, L, strideL, X);
}
extern "C" int nd4hip_zhegst_batched_dev(nd4hip_handle* h, int64_t batch, int64_t N, const double* A, const double* L, int64_t strideL,
                                         double* C) {
  ND4_ARGS(nd4_args_zhegst(batch, N, A, L, strideL, C));
  ND4_CHECK_ARG(h != nullptr, "nd4hip_zhegst_batched: NULL handle");
  Nd4DeviceGuard guard(h);
  Nd4Prof prof(h, "zhegst_batched", batch * 8.0 * (double)N * N * N, 16.0 * batch * 2.0 * (double)(N * N));
  return nd4_zhegst(h, batch, N, A, L, strideL, C);
}
int nd4_zhegvd_run(nd4hip_handle* h, int64_t batch, int64_t N, const double* A, const double* B, int64_t strideB, double* lambda, double* X,
                   int64_t member0) {
  ND4_ARGS(nd4_args_zhegvd(batch, N, A, B, strideB, lambda));
  ND4_CHECK_ARG(h != nullptr, "nd4hip_zhegvd_batched: NULL handle");
  Nd4DeviceGuard guard(h);
  const double n3 = (double)N * N * N;
  Nd4Prof prof(h, "zhegvd_batched", batch * ((16.0 / 3.0 + 2.0 + (X ? 8.0 : 0.0) + 4.0 / 3.0 + 8.0 + (X ? 4.0 : 0.0)) * n3),
               8.0 * batch * (double)(4 * N * N + N + (X ? 2 * N * N : 0)));
  return nd4_zhegvx(h, true, 0, N, batch, N, A, B, strideB, lambda, X, member0);
}
extern "C" int nd4hip_zhegvd_batched_dev(nd4hip_handle* h, int64_t batch, int64_t N, const double* A, const double* B, int64_t strideB,
                                         double* lambda, double* X) {
  return nd4_zhegvd_run(h, batch, N, A, B, strideB, lambda, X, 0);
}
int nd4_zhegvx_run(nd4hip_handle* h, int64_t batch, int64_t N, int64_t i0, int64_t i1, const double* A, const double* B, int64_t strideB,
                   double* lambda, double* X, int64_t member0) {
  ND4_ARGS(nd4_args_zhegvx(batch, N, i0, i1, A, B, strideB, lambda));
  ND4_CHECK_ARG(h != nullptr, "nd4hip_zhegvx_batched: NULL handle");
  Nd4DeviceGuard guard(h);
  const int64_t k = i1 - i0;
  const double n2 = (double)N * N;
  Nd4Prof prof(h, "zhegvx_batched", batch * ((16.0 / 3.0 + 4.0 / 3.0 + 8.0) * n2 * N + (X ? (8.0 + 4.0) * n2 * k : 0.0)),
               8.0 * batch * (double)(4 * N * N + k + (X ? 2 * N * k : 0)));
  return nd4_zhegvx(h, false, i0, i1, batch, N, A, B, strideB, lambda, X, member0);
}
extern "C" int nd4hip_zhegvx_batched_dev(nd4hip_handle* h, int64_t batch, int64_t N, int64_t i0, int64_t i1, const double* A, const double* B,
                                         int64_t strideB, double* lambda, double* X) {
  return nd4_zhegvx_run(h, batch, N, i0, i1, A, B, strideB, lambda, X, 0);
}

extern "C" int nd4hip_dsyevd_last_stages(nd4hip_handle* h, double* ms, int capacity) {
  ND4_CHECK_ARG(h != nullptr && (ms != nullptr || capacity <= 0), "nd4hip_dsyevd_last_stages: NULL argument");
  for (int i = 0; i < capacity && i < ND4HIP_SYEV_STAGES; ++i) ms[i] = h->syev_stage_ms[i];
  return ND4HIP_SYEV_STAGES;
}

extern "C" int nd4hip_dgeqr2_panel_batched_dev(nd4hip_handle* h, int64_t batch, int64_t M, int64_t b, double* A, double* V, double* T) {
  ND4_CHECK_ARG(h != nullptr, "nd4hip_dgeqr2_panel_batched: NULL handle");
  Nd4DeviceGuard guard(h);
  Nd4Prof prof(h, "dgeqr2_panel_batched", (double)(2.0 * batch * M * b * b), (double)(16.0 * batch * M * b));
  ND4_CHECK_ARG(b == 16, "nd4hip_dgeqr2_panel_batched: the panel width is 16");
  ND4_CHECK_ARG(batch >= 0 && batch <= 65535 && M >= 1 && M <= 2048, "nd4hip_dgeqr2_panel_batched: 1 <= M <= 2048 rows, batch <= 65535");
  if (batch == 0) return 0;
  ND4_CHECK_ARG(A && V && T, "nd4hip_dgeqr2_panel_batched: NULL pointer");
  return nd4_geqr2_panel(h, (int)batch, (int)M, A, V, T);
}

extern "C" int nd4hip_dgesvdj_last_info(nd4hip_handle* h, int* sweeps, unsigned long long* rotations, double* offnorm) {
  ND4_CHECK_ARG(h != nullptr, "nd4hip_dgesvdj_last_info: NULL handle");
  if (sweeps) *sweeps = h->svd_sweeps;
  if (rotations) *rotations = h->svd_rotations;
  if (offnorm) *offnorm = h->svd_offnorm;
  return 0;
}
