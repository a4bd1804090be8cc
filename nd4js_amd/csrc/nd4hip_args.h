// Argument validation of the C ABI, written once per operation. The host-pointer form (nd4hip_host.hip) and the device-pointer
// form (nd4hip_api.hip, struct.hip) of an operation call the same checker at the place where their checks stand, through ND4_ARGS:
//     ND4_ARGS(nd4_args_solve("dgetrs_batched", batch, N, J, {{LU, strideLU, N * N}, {P, strideP, N}, {Y, strideY, N * J}}, X));
// A checker sees extents, strides, selectors and pointers (only to compare them with NULL: what they point to may be host or
// device memory), never the handle. It answers ND4HIP_ERR_ARG with the error text set, ND4_ARGS_EMPTY when the call has nothing
// to do and returns 0, or ND4_ARGS_GO. The texts are part of the contract: many are the reference's own, and the Python and JS
// layers turn them into exceptions by matching them. What reads host memory (the permutation scans, isfinite(sv), the overlap
// tests of the structure functions) or does work for an empty shape (zero and identity fills) stays in the form it belongs to.
// A new operation adds its checker here, not a list of ND4_CHECK_ARG in each form.
#pragma once
#include "nd4hip_internal.h"
#include <cstdint>
#include <initializer_list>

enum { ND4_ARGS_GO = 0, ND4_ARGS_EMPTY = 1 };
#define ND4_ARGS(call) do { const int _a = (call); if (_a != ND4_ARGS_GO) return _a == ND4_ARGS_EMPTY ? 0 : _a; } while (0)

constexpr int64_t EV_MAX_N = 32768;         // the eigenvector and balancing kernels index a matrix with 32-bit products of N

// a batched operand for the stride rule: members `stride` elements apart, 0 = one block for all, else at least `item`
struct Nd4Strided { const void* p; int64_t stride, item; };
using Nd4Extents = std::initializer_list<int64_t>;
using Nd4Ptrs = std::initializer_list<const void*>;

inline bool nd4_none_negative(Nd4Extents e) { for (int64_t x : e) if (x < 0) return false; return true; }
inline bool nd4_any_zero(Nd4Extents e) { for (int64_t x : e) if (x == 0) return true; return false; }
inline bool nd4_none_null(Nd4Ptrs p) { for (const void* x : p) if (!x) return false; return true; }
inline bool nd4_none_null(std::initializer_list<Nd4Strided> s) { for (const Nd4Strided& x : s) if (!x.p) return false; return true; }
inline bool nd4_strides_fit(std::initializer_list<Nd4Strided> s) {
  for (const Nd4Strided& x : s) if (x.stride != 0 && x.stride < x.item) return false;
  return true;
}
#define ND4_STRIDE_TEXT "nd4hip_%s: a stride must be 0 or at least the size of one operand"

// ---- dense operands, one per batch member: every extent >= 0, nothing to do when one is 0, every pointer needed
// (dgetrf, dpotrf, dldltrf, dgebrd, dgehrd, dgeqrf_q, dgeqrf_full, dgeqp3, dgeqp3_full, dgesvdj, dgesdd, dtranspose, dtri, ddiagmat)
inline int nd4_args_dense(const char* op, Nd4Extents extents, Nd4Ptrs ptrs) {
  ND4_CHECK_ARG(nd4_none_negative(extents), "nd4hip_%s: negative extent", op);
  if (nd4_any_zero(extents)) return ND4_ARGS_EMPTY;
  ND4_CHECK_ARG(nd4_none_null(ptrs), "nd4hip_%s: NULL pointer", op);
  return ND4_ARGS_GO;
}
// _qr_decomp_inplace: L = 0 columns of Y still factorises A
inline int nd4_args_geqrf_qty(int64_t batch, int64_t M, int64_t N, int64_t L, const void* A, const void* Y) {
  ND4_CHECK_ARG(batch >= 0 && M >= 0 && N >= 0 && L >= 0, "nd4hip_dgeqrf_qty_batched: negative extent");
  if (batch == 0 || M == 0 || N == 0) return ND4_ARGS_EMPTY;
  ND4_CHECK_ARG(A && (Y || L == 0), "nd4hip_dgeqrf_qty_batched: NULL pointer");
  return ND4_ARGS_GO;
}

// ---- matmul; `complex_ok`: true for dgemm, a_complex || b_complex for zgemm
inline int nd4_args_gemm(const char* op, bool complex_ok, int64_t batch, int64_t I, int64_t K, int64_t J, const void* A, int64_t strideA,
                         const void* B, int64_t strideB, const void* C) {
  ND4_CHECK_ARG(complex_ok, "nd4hip_%s: at least one operand must be complex", op);
  ND4_CHECK_ARG(batch >= 0 && I >= 0 && K >= 0 && J >= 0, "nd4hip_%s: negative extent", op);
  ND4_CHECK_ARG(strideA == 0 || strideA >= I * K, "nd4hip_%s: strideA must be 0 or >= I*K", op);
  ND4_CHECK_ARG(strideB == 0 || strideB >= K * J, "nd4hip_%s: strideB must be 0 or >= K*J", op);
  if (batch == 0 || I == 0 || J == 0) return ND4_ARGS_EMPTY;
  ND4_CHECK_ARG(C && (K == 0 || (A && B)), "nd4hip_%s: NULL matrix pointer", op);   // K = 0: nothing is read, C = 0
  return ND4_ARGS_GO;
}

// ---- solves with a factorisation: N x N factors and their N-vectors, an N x J right-hand side, X [batch, N, J]
// (dgetrs, dtrsm, dpotrs, dldltrs, dsytrs_bk)
inline int nd4_args_solve(const char* op, int64_t batch, int64_t N, int64_t J, std::initializer_list<Nd4Strided> in, const void* X) {
  ND4_CHECK_ARG(batch >= 0 && N >= 0 && J >= 0, "nd4hip_%s: negative extent", op);
  ND4_CHECK_ARG(nd4_strides_fit(in), ND4_STRIDE_TEXT, op);
  if (batch == 0 || N == 0 || J == 0) return ND4_ARGS_EMPTY;
  ND4_CHECK_ARG(nd4_none_null(in) && X, "nd4hip_%s: NULL pointer", op);
  return ND4_ARGS_GO;
}
// ---- qr_lstsq (`qr`: I <= N, qr.js:209) and svd_lstsq: factors of an N x I matrix through M, Y [N, J] -> X [I, J]. N = 0 or
// M = 0 leaves X = 0 to the caller and needs X alone
inline int nd4_args_factor_ls(const char* op, bool qr, int64_t batch, int64_t N, int64_t M, int64_t I, int64_t J,
                              std::initializer_list<Nd4Strided> in, const void* X) {
  ND4_CHECK_ARG(batch >= 0 && N >= 0 && M >= 0 && I >= 0 && J >= 0, "nd4hip_%s: negative extent", op);
  ND4_CHECK_ARG(!qr || I <= N, "qr_lstsq(Q,R,y): Under-determined systems not supported. Use rrqr instead.");
  ND4_CHECK_ARG(nd4_strides_fit(in), ND4_STRIDE_TEXT, op);
  if (batch == 0 || I == 0 || J == 0) return ND4_ARGS_EMPTY;
  ND4_CHECK_ARG(X != nullptr, "nd4hip_%s: NULL pointer", op);
  ND4_CHECK_ARG(N == 0 || M == 0 || nd4_none_null(in), "nd4hip_%s: NULL pointer", op);
  return ND4_ARGS_GO;
}

// ---- pivoted LDL^T; a tier other than AUTO must be able to take N (nd4_sytrf_bk_tier needs no handle for that)
// (`op`: dsytrf_bk_batched, or dsytrf_bk_tier for the query of the tier alone)
inline int nd4_args_sytrf_bk_tier(const char* op, int64_t batch, int64_t N, int tier) {
  ND4_CHECK_ARG(batch >= 0 && N >= 0, "nd4hip_%s: negative extent", op);
  ND4_CHECK_ARG(tier >= ND4HIP_PLDLP_TIER_AUTO && tier <= ND4HIP_PLDLP_TIER_GRID, "nd4hip_%s: unknown tier %d", op, tier);
  ND4_CHECK_ARG(tier == ND4HIP_PLDLP_TIER_AUTO || nd4_sytrf_bk_tier(nullptr, batch, N, tier) != 0,
                "nd4hip_%s: tier %d is not available at N = %lld", op, tier, (long long)N);
  return ND4_ARGS_GO;
}
inline int nd4_args_sytrf_bk(int64_t batch, int64_t N, const void* S, const void* LD, const void* P, int tier) {
  ND4_TRY(nd4_args_sytrf_bk_tier("dsytrf_bk_batched", batch, N, tier));
  if (batch == 0 || N == 0) return ND4_ARGS_EMPTY;
  ND4_CHECK_ARG(S && LD && P, "nd4hip_dsytrf_bk_batched: NULL pointer");
  return ND4_ARGS_GO;
}

// ---- structure functions (the overlap tests follow in each form: the host forms apply them to host addresses)
inline int64_t nd4_diag_length(int64_t M, int64_t N, int64_t offset) {      // of diagonal `offset`, -M < offset < N, of an M x N matrix
  const int64_t rows = offset < 0 ? M + offset : M, cols = offset > 0 ? N - offset : N;
  return rows < cols ? rows : cols;
}
inline int nd4_args_diag(int64_t batch, int64_t M, int64_t N, int64_t offset, const void* A, const void* d) {
  ND4_CHECK_ARG(batch >= 0 && M >= 0 && N >= 0, "nd4hip_ddiag_batched: negative extent");
  ND4_CHECK_ARG(offset > -M && offset < N, "nd4hip_ddiag_batched: offset=%lld out of the shape [%lld,%lld]", (long long)offset, (long long)M,
                (long long)N);
  if (batch == 0 || nd4_diag_length(M, N, offset) <= 0) return ND4_ARGS_EMPTY;
  ND4_CHECK_ARG(A && d, "nd4hip_ddiag_batched: NULL pointer");
  return ND4_ARGS_GO;
}
inline int nd4_args_permute(int cols, int64_t batch, int64_t M, int64_t N, const void* A, int64_t strideA, const void* P, int64_t strideP,
                            const void* B) {
  ND4_CHECK_ARG(batch >= 0 && M >= 0 && N >= 0, "nd4hip_dpermute_batched: negative extent");
  ND4_CHECK_ARG(M <= INT32_MAX && N <= INT32_MAX, "nd4hip_dpermute_batched: M and N must fit int32 (P is int32)");
  ND4_CHECK_ARG(nd4_strides_fit({{A, strideA, M * N}, {P, strideP, cols ? N : M}}), ND4_STRIDE_TEXT, "dpermute_batched");
  if (batch == 0 || M == 0 || N == 0) return ND4_ARGS_EMPTY;
  ND4_CHECK_ARG(A && P && B, "nd4hip_dpermute_batched: NULL pointer");
  return ND4_ARGS_GO;
}

// ---- strong rank-revealing QR, URV: an empty matrix still gets its P, rank and identity factors, so only batch = 0 is empty
inline int nd4_args_srrqr(int64_t batch, int64_t M, int64_t N, const void* A, double dtol, double ztol, const void* Q, const void* R,
                          const void* P, const void* rank) {
  ND4_CHECK_ARG(batch >= 0 && M >= 0 && N >= 0, "nd4hip_dsrrqr_batched: negative extent");
  ND4_CHECK_ARG(dtol >= 1.0, "srrqr_decomp_full(A,opt): Invalid opt.dtol: %s. Must be >=1.", dtol != dtol ? "NaN" : "a value below 1");
  ND4_CHECK_ARG(dtol <= 1.79769313486231570e308, "Assertion failed. Invalid dtol: Infinity.");
  ND4_CHECK_ARG(!(ztol != ztol), "srrqr_decomp_full(A,opt): invalid opt.ztol: NaN. Must be non-negative number.");
  ND4_CHECK_ARG(ztol <= 1.79769313486231570e308, "Assertion failed. Invalid ztol: Infinity.");
  if (batch == 0) return ND4_ARGS_EMPTY;
  ND4_CHECK_ARG(P && rank && (Q || M == 0) && ((A && R) || M * N == 0), "nd4hip_dsrrqr_batched: NULL pointer");
  return ND4_ARGS_GO;
}
inline int nd4_args_urv(int64_t batch, int64_t M, int64_t N, const void* A, const void* U, const void* R, const void* V, const void* rank) {
  ND4_CHECK_ARG(batch >= 0 && M >= 0 && N >= 0, "nd4hip_durv_batched: negative extent");
  if (batch == 0) return ND4_ARGS_EMPTY;
  ND4_CHECK_ARG(rank && (U || M == 0) && (V || N == 0) && ((A && R) || M * N == 0), "nd4hip_durv_batched: NULL pointer");
  return ND4_ARGS_GO;
}
// urv_lstsq: U [I, J], R [J, K], V [K, L], rank [] (stride 0 or 1), Y [I, Jc] -> X [L, Jc]; urv.js asserts J <= I and K <= L
inline int nd4_args_urvls(int64_t batch, int64_t I, int64_t J, int64_t K, int64_t L, int64_t Jc, const void* U, int64_t strideU, const void* R,
                          int64_t strideR, const void* V, int64_t strideV, const void* rank, int64_t strideRank, const void* Y,
                          int64_t strideY, const void* X) {
  ND4_CHECK_ARG(batch >= 0 && I >= 0 && J >= 0 && K >= 0 && L >= 0 && Jc >= 0, "nd4hip_durvls_batched: negative extent");
  ND4_CHECK_ARG(J <= I && K <= L, "Assertion failed.");
  ND4_CHECK_ARG(nd4_strides_fit({{U, strideU, I * J}, {R, strideR, J * K}, {V, strideV, K * L}, {Y, strideY, I * Jc}}) &&
                (strideRank == 0 || strideRank == 1), ND4_STRIDE_TEXT, "durvls_batched");
  if (batch == 0 || L * Jc == 0) return ND4_ARGS_EMPTY;
  ND4_CHECK_ARG(U && R && V && rank && Y && X, "nd4hip_durvls_batched: NULL pointer");
  return ND4_ARGS_GO;
}

// ---- det / slogdet of A [M, N], M >= N (`log_form`: sign and logdet in D and L), det_tri / slogdet_tri of A [N, N], norm:
// an empty matrix has a determinant and a norm, so the outputs are always needed
inline int nd4_args_det(const char* op, bool log_form, int64_t batch, int64_t M, int64_t N, const void* A, const void* D, const void* L) {
  ND4_CHECK_ARG(batch >= 0 && M >= 0 && N >= 0, "nd4hip_%s: negative extent", op);
  ND4_CHECK_ARG(M >= N, log_form ? "det_tri(A): A must be square matrices." : "det_tri(a): a must be square matrices.");
  if (batch == 0) return ND4_ARGS_EMPTY;
  ND4_CHECK_ARG(D && (L || !log_form) && (A || M * N == 0), "nd4hip_%s: NULL pointer", op);
  return ND4_ARGS_GO;
}
inline int nd4_args_nrmfro(int64_t n, const void* A, const void* out) {
  ND4_CHECK_ARG(n >= 0, "nd4hip_dnrmfro: negative extent");
  ND4_CHECK_ARG(out && (A || n == 0), "nd4hip_dnrmfro: NULL pointer");
  return ND4_ARGS_GO;
}

// ---- N x N problems of the nonsymmetric eigen chain; `max_n`: EV_MAX_N for dtreval, dtrevc, dgebal and zgebak, none (INT64_MAX)
// for dhseqr, dgees and dgeev
inline int nd4_args_ev(const char* op, int64_t max_n, int64_t batch, int64_t N, Nd4Ptrs ptrs, const char* null_text = "NULL pointer") {
  ND4_CHECK_ARG(batch >= 0 && N >= 0 && N <= max_n, "nd4hip_%s: extent out of range", op);
  if (batch == 0 || N == 0) return ND4_ARGS_EMPTY;
  ND4_CHECK_ARG(nd4_none_null(ptrs), "nd4hip_%s: %s", op, null_text);
  return ND4_ARGS_GO;
}
inline int nd4_args_gebal(int64_t batch, int64_t N, double p, const void* A, const void* D, const void* B) {
  ND4_CHECK_ARG(p >= 1.0, "nd4hip_dgebal_batched: p must be >= 1");
  return nd4_args_ev("dgebal_batched", EV_MAX_N, batch, N, {A, D, B});
}
// `on_device`: the kernel reads V while it writes W, so the device form refuses V == W. The host form has no such rule: it stages
// V and W in separate device blocks, and in-place use of one host buffer is legitimate there.
inline int nd4_args_gebak(bool on_device, int64_t batch, int64_t N, const void* D, const void* V, const void* W) {
  return nd4_args_ev("zgebak_batched", EV_MAX_N, batch, N, {D, V, on_device && V == W ? nullptr : W},
                     on_device ? "NULL or aliased pointer" : "NULL pointer");
}
inline int nd4_args_hseqr(int64_t batch, int64_t N, const void* U, const void* H, const void* Q, const void* T, int tier) {
  ND4_CHECK_ARG(batch >= 0 && N >= 0, "nd4hip_dhseqr_batched: extent out of range");
  ND4_CHECK_ARG(tier >= ND4HIP_SCHUR_TIER_AUTO && tier <= ND4HIP_SCHUR_TIER_GLOBAL, "nd4hip_dhseqr_batched: unknown tier %d", tier);
  if (batch == 0 || N == 0) return ND4_ARGS_EMPTY;
  ND4_CHECK_ARG(U && H && Q && T, "nd4hip_dhseqr_batched: NULL pointer");
  return ND4_ARGS_GO;
}

// ---- rank and least squares of a pivoted QR: an empty R has rank 0, so only batch = 0 is empty
inline int nd4_args_qp3rank(int64_t batch, int64_t M, int64_t N, const void* R, const void* rank) {
  ND4_CHECK_ARG(batch >= 0 && M >= 0 && N >= 0, "nd4hip_dqp3rank_batched: negative extent");
  if (batch == 0) return ND4_ARGS_EMPTY;
  ND4_CHECK_ARG(rank && (R || M == 0 || N == 0), "nd4hip_dqp3rank_batched: NULL pointer");
  return ND4_ARGS_GO;
}
// I = 0 or J = 0 leaves the rank alone to be computed (X is empty): the pointers are the caller's business then
inline int nd4_args_qp3ls(int64_t batch, int64_t N, int64_t M, int64_t I, int64_t J, const void* Q, int64_t strideQ, const void* R,
                          int64_t strideR, const void* P, int64_t strideP, const void* Y, int64_t strideY, const void* X) {
  ND4_CHECK_ARG(batch >= 0 && N >= 0 && M >= 0 && I >= 0 && J >= 0, "nd4hip_dqp3ls_batched: negative extent");
  ND4_CHECK_ARG(nd4_strides_fit({{Q, strideQ, N * M}, {R, strideR, M * I}, {P, strideP, I}, {Y, strideY, N * J}}), ND4_STRIDE_TEXT, "dqp3ls_batched");
  if (batch == 0) return ND4_ARGS_EMPTY;
  ND4_CHECK_ARG(I == 0 || J == 0 || (Q && R && P && Y && X), "nd4hip_dqp3ls_batched: NULL pointer");
  return ND4_ARGS_GO;
}

// ---- the bidiagonal solver of the divide & conquer SVD: B is K x J, J = K or K + 1; e has J - 1 entries
inline int nd4_args_bdsdc(int64_t batch, int64_t K, int64_t J, const void* d, const void* e, const void* U2, const void* sv, const void* V2) {
  ND4_CHECK_ARG(batch >= 0 && K >= 0, "nd4hip_dbdsdc_batched: negative extent");
  ND4_CHECK_ARG(J == K || J == K + 1, "nd4hip_dbdsdc_batched: B must be K x K or K x (K+1)");
  if (batch == 0 || K == 0) return ND4_ARGS_EMPTY;
  ND4_CHECK_ARG(d && (e || J < 2) && U2 && sv && V2, "nd4hip_dbdsdc_batched: NULL pointer");
  return ND4_ARGS_GO;
}

// ---- selected singular triplets (bdsvdx.hip): the vectors go together and are optional, as is `fallback`; e is not read for J = 1
inline int nd4_args_bdsvdx(int64_t batch, int64_t K, int64_t J, int64_t i0, int64_t i1, const void* d, const void* e, const void* U2,
                           const void* sv, const void* V2) {
  ND4_CHECK_ARG(batch >= 0 && K >= 0, "nd4hip_dbdsvdx_batched: negative extent");
  ND4_CHECK_ARG(J == K || J == K + 1, "nd4hip_dbdsvdx_batched: B must be K x K or K x (K+1)");
  ND4_CHECK_ARG(0 <= i0 && i0 <= i1 && i1 <= K, "nd4hip_dbdsvdx_batched: subset must satisfy 0 <= i0 <= i1 <= K");
  ND4_CHECK_ARG(K <= 2048, "nd4hip_dbdsvdx_batched: K <= 2048");
  if (batch == 0 || K == 0 || i0 == i1) return ND4_ARGS_EMPTY;
  ND4_CHECK_ARG(d && (e || J < 2) && sv, "nd4hip_dbdsvdx_batched: NULL pointer");
  ND4_CHECK_ARG(!U2 == !V2, "nd4hip_dbdsvdx_batched: U2 and V2 go together");
  return ND4_ARGS_GO;
}
inline int nd4_args_gesvdx(int64_t batch, int64_t M, int64_t N, int64_t i0, int64_t i1, const void* A, const void* U, const void* sv,
                           const void* V) {
  ND4_CHECK_ARG(batch >= 0 && M >= 0 && N >= 0, "nd4hip_dgesvdx_batched: negative extent");
  ND4_CHECK_ARG(0 <= i0 && i0 <= i1 && i1 <= (M < N ? M : N), "nd4hip_dgesvdx_batched: subset must satisfy 0 <= i0 <= i1 <= min(M, N)");
  ND4_CHECK_ARG((M < N ? M : N) <= 2048, "nd4hip_dgesvdx_batched: min(M, N) <= 2048");
  if (batch == 0 || M == 0 || N == 0 || i0 == i1) return ND4_ARGS_EMPTY;
  ND4_CHECK_ARG(A && sv, "nd4hip_dgesvdx_batched: NULL pointer");
  ND4_CHECK_ARG(!U == !V, "nd4hip_dgesvdx_batched: U and V go together");
  return ND4_ARGS_GO;
}
// the workspace and grid arithmetic of a dbdsvdx call (bdsvdx.hip; tools/bdsvdx_host_check.hip walks every K and J): the order of
// the Golub-Kahan matrix, its off-diagonals (what stx_bisect's LDS array must hold: at most 4096), the doubles of the vector stage
inline int64_t nd4_bdx_order(int64_t K, int64_t J) { return K + J; }
inline int64_t nd4_bdx_offdiagonals(int64_t K, int64_t J) { return K + J - 1; }
inline size_t nd4_bdx_lds_bytes(int64_t K, int64_t J) { return sizeof(double) * (size_t)nd4_bdx_offdiagonals(K, J); }
inline size_t nd4_bdx_vector_doubles(int64_t batch, int64_t K, int64_t J, int64_t k) { return (size_t)batch * (size_t)k * (size_t)nd4_bdx_order(K, J) * 5; }
// ---- symmetric eigenproblems: the divide & conquer solver takes N <= 2048, the Jacobi route (`jacobi`) N <= 128; V, X and the
// sweep counts are optional
inline int nd4_args_syev(const char* op, bool jacobi, int64_t batch, int64_t N, const void* S, const void* lambda) {
  ND4_CHECK_ARG(batch >= 0 && N >= 0, "nd4hip_%s: negative extent", op);
  ND4_CHECK_ARG(jacobi || N <= 2048, "nd4hip_%s: the divide & conquer solver takes N <= 2048", op);
  ND4_CHECK_ARG(!jacobi || N <= 128, "nd4hip_%s: the Jacobi route takes N <= 128", op);
  if (batch == 0 || N == 0) return ND4_ARGS_EMPTY;
  ND4_CHECK_ARG(S && lambda, "nd4hip_%s: NULL pointer", op);
  return ND4_ARGS_GO;
}
// ---- selected eigenpairs by bisection and inverse iteration (syevx.hip): the vectors (Z, V) are optional, e is not read for N = 1
inline int nd4_args_stcnt(int64_t batch, int64_t N, int64_t M, const void* d, const void* e, const void* x, const void* count) {
  ND4_CHECK_ARG(batch >= 0 && N >= 0 && M >= 0, "nd4hip_dstcnt_batched: negative extent");
  ND4_CHECK_ARG(N <= 2048, "nd4hip_dstcnt_batched: N <= 2048");
  if (batch == 0 || N == 0 || M == 0) return ND4_ARGS_EMPTY;
  ND4_CHECK_ARG(d && (e || N < 2) && x && count, "nd4hip_dstcnt_batched: NULL pointer");
  return ND4_ARGS_GO;
}
inline int nd4_args_subset(const char* op, int64_t batch, int64_t N, int64_t i0, int64_t i1, Nd4Ptrs ptrs) {
  ND4_CHECK_ARG(batch >= 0 && N >= 0, "nd4hip_%s: negative extent", op);
  ND4_CHECK_ARG(0 <= i0 && i0 <= i1 && i1 <= N, "nd4hip_%s: subset must satisfy 0 <= i0 <= i1 <= N", op);
  ND4_CHECK_ARG(N <= 2048, "nd4hip_%s: N <= 2048", op);
  if (batch == 0 || N == 0 || i0 == i1) return ND4_ARGS_EMPTY;
  ND4_CHECK_ARG(nd4_none_null(ptrs), "nd4hip_%s: NULL pointer", op);
  return ND4_ARGS_GO;
}
inline int nd4_args_stevx(int64_t batch, int64_t N, int64_t i0, int64_t i1, const void* d, const void* e, const void* lambda) {
  return nd4_args_subset("dstevx_batched", batch, N, i0, i1, {d, e || N < 2 ? d : nullptr, lambda});
}
inline int nd4_args_syevx(int64_t batch, int64_t N, int64_t i0, int64_t i1, const void* S, const void* lambda) {
  return nd4_args_subset("dsyevx_batched", batch, N, i0, i1, {S, lambda});
}
// ---- eigenpairs in a value interval (syevx.hip): bounds [batch, 2] = (lo, hi), lambda [batch, kcap], range
// [batch, 2] and the host word kmax are needed; the vectors are optional. `op`: dstevxv_batched (`e`: its off-diagonal, not read for
// N = 1), dsyevxv_batched or dsyevxv_tr_batched (e = NULL). An empty call writes neither range nor kmax.
inline int nd4_args_interval(const char* op, int64_t batch, int64_t N, int64_t kcap, const void* bounds, const void* in, const void* e,
                             bool needs_e, const void* lambda, const void* range, const void* kmax) {
  ND4_CHECK_ARG(batch >= 0 && N >= 0 && kcap >= 0, "nd4hip_%s: negative extent", op);
  ND4_CHECK_ARG(N <= 2048, "nd4hip_%s: N <= 2048", op);
  if (batch == 0 || N == 0) return ND4_ARGS_EMPTY;
  ND4_CHECK_ARG(bounds && in && (e || !needs_e || N < 2) && range && kmax && (lambda || kcap == 0), "nd4hip_%s: NULL pointer", op);
  return ND4_ARGS_GO;
}
inline int nd4_args_stevxv(int64_t batch, int64_t N, int64_t kcap, const void* bounds, const void* d, const void* e, const void* lambda,
                           const void* range, const void* kmax) {
  return nd4_args_interval("dstevxv_batched", batch, N, kcap, bounds, d, e, true, lambda, range, kmax);
}
inline int nd4_args_syevxv(bool tridiag, int64_t batch, int64_t N, int64_t kcap, const void* bounds, const void* S, const void* lambda,
                           const void* range, const void* kmax) {
  return nd4_args_interval(tridiag ? "dsyevxv_tr_batched" : "dsyevxv_batched", batch, N, kcap, bounds, S, nullptr, false, lambda, range, kmax);
}
// the bounds where they are host memory (the _host forms): NaN and lo > hi are refused; +-Infinity is a bound like any other
inline int nd4_args_bounds(const char* op, int64_t batch, const double* bounds) {
  for (int64_t b = 0; b < batch; ++b) {
    const double lo = bounds[2 * b], hi = bounds[2 * b + 1];
    ND4_CHECK_ARG(lo == lo && hi == hi, "nd4hip_%s: interval contains NaN", op);
    ND4_CHECK_ARG(lo <= hi, "nd4hip_%s: interval must satisfy lo <= hi", op);
  }
  return ND4_ARGS_GO;
}
// the ranges read back after the count, range [batch, 2] = (i0_b, i1_b) on the host: *kmax = max_b(i1_b - i0_b). lo > hi in device
// memory shows here as i1_b < i0_b
inline int nd4_interval_kmax(const char* op, int64_t batch, int64_t N, const int32_t* range, int64_t* kmax) {
  int64_t km = 0;
  for (int64_t b = 0; b < batch; ++b) {
    const int64_t i0 = range[2 * b], i1 = range[2 * b + 1];
    ND4_CHECK_ARG(0 <= i0 && i0 <= i1 && i1 <= N, "nd4hip_%s: interval must satisfy lo <= hi", op);
    km = i1 - i0 > km ? i1 - i0 : km;
  }
  *kmax = km;
  return ND4_ARGS_GO;
}
inline int nd4_args_kcap(const char* op, int64_t kcap, int64_t kmax) {
  ND4_CHECK_ARG(kcap >= kmax, "nd4hip_%s: kcap = %lld is less than the %lld eigenvalues a member has in its interval", op, (long long)kcap,
                (long long)kmax);
  return ND4_ARGS_GO;
}
// the grids of a call with k values per member (syevx.hip): workgroups of stx_bisect per member, of stx_factor_solve, and of
// stx_ragged over `rows` rows
inline int64_t nd4_stx_bisect_blocks(int64_t k) { return (k + 255) / 256; }
inline int64_t nd4_stx_solve_blocks(int64_t batch, int64_t k) { return (batch * k + 63) / 64; }
inline int64_t nd4_stx_ragged_blocks(int64_t batch, int64_t rows, int64_t k) { return (batch * rows * k + 255) / 256; }

// ---- symmetric tridiagonal reduction, its Q, and the eigen routes on it (sytrd.hip): tau and e have no entry for N = 1; V is optional
inline int nd4_args_sytrd(int64_t batch, int64_t N, const void* S, const void* F, const void* tau, const void* d, const void* e) {
  ND4_CHECK_ARG(batch >= 0 && N >= 0, "nd4hip_dsytrd_batched: negative extent");
  ND4_CHECK_ARG(N <= 2048, "nd4hip_dsytrd_batched: N <= 2048");
  if (batch == 0 || N == 0) return ND4_ARGS_EMPTY;
  ND4_CHECK_ARG(S && F && d && ((tau && e) || N < 2), "nd4hip_dsytrd_batched: NULL pointer");
  return ND4_ARGS_GO;
}
inline int nd4_args_ormtr(int64_t batch, int64_t N, int64_t K, int transpose, const void* F, const void* tau, const void* Z) {
  ND4_CHECK_ARG(batch >= 0 && N >= 0 && K >= 0, "nd4hip_dormtr_batched: negative extent");
  ND4_CHECK_ARG(N <= 2048, "nd4hip_dormtr_batched: N <= 2048");
  ND4_CHECK_ARG(transpose == 0 || transpose == 1, "nd4hip_dormtr_batched: transpose must be 0 or 1");
  if (batch == 0 || N == 0 || K == 0) return ND4_ARGS_EMPTY;
  ND4_CHECK_ARG(F && (tau || N < 2) && Z, "nd4hip_dormtr_batched: NULL pointer");
  return ND4_ARGS_GO;
}
inline int nd4_args_syevd_tr(int64_t batch, int64_t N, const void* S, const void* lambda) {
  ND4_CHECK_ARG(batch >= 0 && N >= 0, "nd4hip_dsyevd_tr_batched: negative extent");
  ND4_CHECK_ARG(N <= 2048, "nd4hip_dsyevd_tr_batched: N <= 2048");
  if (batch == 0 || N == 0) return ND4_ARGS_EMPTY;
  ND4_CHECK_ARG(S && lambda, "nd4hip_dsyevd_tr_batched: NULL pointer");
  return ND4_ARGS_GO;
}
inline int nd4_args_syevx_tr(int64_t batch, int64_t N, int64_t i0, int64_t i1, const void* S, const void* lambda) {
  return nd4_args_subset("dsyevx_tr_batched", batch, N, i0, i1, {S, lambda});
}
// ---- Hermitian tridiagonal reduction, its Q, and the eigen routes on it (hetrd.hip): the checks of the four above in the same order
inline int nd4_args_hetrd(int64_t batch, int64_t N, const void* H, const void* F, const void* tau, const void* d, const void* e) {
  ND4_CHECK_ARG(batch >= 0 && N >= 0, "nd4hip_zhetrd_batched: negative extent");
  ND4_CHECK_ARG(N <= 2048, "nd4hip_zhetrd_batched: N <= 2048");
  if (batch == 0 || N == 0) return ND4_ARGS_EMPTY;
  ND4_CHECK_ARG(H && F && d && ((tau && e) || N < 2), "nd4hip_zhetrd_batched: NULL pointer");
  return ND4_ARGS_GO;
}
inline int nd4_args_unmtr(int64_t batch, int64_t N, int64_t K, int adjoint, const void* F, const void* tau, const void* Z) {
  ND4_CHECK_ARG(batch >= 0 && N >= 0 && K >= 0, "nd4hip_zunmtr_batched: negative extent");
  ND4_CHECK_ARG(N <= 2048, "nd4hip_zunmtr_batched: N <= 2048");
  ND4_CHECK_ARG(adjoint == 0 || adjoint == 1, "nd4hip_zunmtr_batched: adjoint must be 0 or 1");
  if (batch == 0 || N == 0 || K == 0) return ND4_ARGS_EMPTY;
  ND4_CHECK_ARG(F && (tau || N < 2) && Z, "nd4hip_zunmtr_batched: NULL pointer");
  return ND4_ARGS_GO;
}
inline int nd4_args_heevd(int64_t batch, int64_t N, const void* H, const void* lambda) {
  ND4_CHECK_ARG(batch >= 0 && N >= 0, "nd4hip_zheevd_batched: negative extent");
  ND4_CHECK_ARG(N <= 2048, "nd4hip_zheevd_batched: N <= 2048");
  if (batch == 0 || N == 0) return ND4_ARGS_EMPTY;
  ND4_CHECK_ARG(H && lambda, "nd4hip_zheevd_batched: NULL pointer");
  return ND4_ARGS_GO;
}
inline int nd4_args_heevx(int64_t batch, int64_t N, int64_t i0, int64_t i1, const void* H, const void* lambda) {
  return nd4_args_subset("zheevx_batched", batch, N, i0, i1, {H, lambda});
}
// ---- Hermitian Cholesky, complex triangular solves and the generalised Hermitian-definite eigenproblem (hegv.hip): strides in complex
// elements, N*N or 0 (one L or B for every member)
inline int nd4_args_zpotrf(int64_t batch, int64_t N, const void* H, const void* L) {
  ND4_CHECK_ARG(batch >= 0 && N >= 0, "nd4hip_zpotrf_batched: negative extent");
  ND4_CHECK_ARG(N <= 2048, "nd4hip_zpotrf_batched: N <= 2048");
  if (batch == 0 || N == 0) return ND4_ARGS_EMPTY;
  ND4_CHECK_ARG(H && L, "nd4hip_zpotrf_batched: NULL pointer");
  return ND4_ARGS_GO;
}
// zpotrs and ztrsm: X [batch, N, K] in place
inline int nd4_args_ztrs(const char* op, int64_t batch, int64_t N, int64_t K, int adjoint, const void* L, int64_t strideL, const void* X) {
  ND4_CHECK_ARG(batch >= 0 && N >= 0 && K >= 0, "nd4hip_%s: negative extent", op);
  ND4_CHECK_ARG(N <= 2048, "nd4hip_%s: N <= 2048", op);
  ND4_CHECK_ARG(adjoint == 0 || adjoint == 1, "nd4hip_%s: adjoint must be 0 or 1", op);
  ND4_CHECK_ARG(strideL == 0 || strideL == N * N, "nd4hip_%s: strideL must be N*N or 0", op);
  if (batch == 0 || N == 0 || K == 0) return ND4_ARGS_EMPTY;
  ND4_CHECK_ARG(L && X, "nd4hip_%s: NULL pointer", op);
  return ND4_ARGS_GO;
}
inline int nd4_args_zpotrs(int64_t batch, int64_t N, int64_t K, const void* L, int64_t strideL, const void* Y, const void* X) {
  return nd4_args_ztrs("zpotrs_batched", batch, N, K, 0, L, strideL, Y ? X : nullptr);
}
inline int nd4_args_ztrsm(int64_t batch, int64_t N, int64_t K, int adjoint, const void* L, int64_t strideL, const void* X) {
  return nd4_args_ztrs("ztrsm_batched", batch, N, K, adjoint, L, strideL, X);
}
inline int nd4_args_zhegst(int64_t batch, int64_t N, const void* A, const void* L, int64_t strideL, const void* C) {
  ND4_CHECK_ARG(batch >= 0 && N >= 0, "nd4hip_zhegst_batched: negative extent");
  ND4_CHECK_ARG(N <= 2048, "nd4hip_zhegst_batched: N <= 2048");
  ND4_CHECK_ARG(strideL == 0 || strideL == N * N, "nd4hip_zhegst_batched: strideL must be N*N or 0");
  if (batch == 0 || N == 0) return ND4_ARGS_EMPTY;
  ND4_CHECK_ARG(A && L && C, "nd4hip_zhegst_batched: NULL pointer");
  return ND4_ARGS_GO;
}
inline int nd4_args_zhegvd(int64_t batch, int64_t N, const void* A, const void* B, int64_t strideB, const void* lambda) {
  ND4_CHECK_ARG(batch >= 0 && N >= 0, "nd4hip_zhegvd_batched: negative extent");
  ND4_CHECK_ARG(N <= 2048, "nd4hip_zhegvd_batched: N <= 2048");
  ND4_CHECK_ARG(strideB == 0 || strideB == N * N, "nd4hip_zhegvd_batched: strideB must be N*N or 0");
  if (batch == 0 || N == 0) return ND4_ARGS_EMPTY;
  ND4_CHECK_ARG(A && B && lambda, "nd4hip_zhegvd_batched: NULL pointer");
  return ND4_ARGS_GO;
}
inline int nd4_args_zhegvx(int64_t batch, int64_t N, int64_t i0, int64_t i1, const void* A, const void* B, int64_t strideB, const void* lambda) {
  ND4_CHECK_ARG(batch >= 0 && N >= 0, "nd4hip_zhegvx_batched: negative extent");
  ND4_CHECK_ARG(0 <= i0 && i0 <= i1 && i1 <= N, "nd4hip_zhegvx_batched: subset must satisfy 0 <= i0 <= i1 <= N");
  ND4_CHECK_ARG(N <= 2048, "nd4hip_zhegvx_batched: N <= 2048");
  ND4_CHECK_ARG(strideB == 0 || strideB == N * N, "nd4hip_zhegvx_batched: strideB must be N*N or 0");
  if (batch == 0 || N == 0 || i0 == i1) return ND4_ARGS_EMPTY;
  ND4_CHECK_ARG(A && B && lambda, "nd4hip_zhegvx_batched: NULL pointer");
  return ND4_ARGS_GO;
}
inline int nd4_args_sygvd(int algo, int64_t batch, int64_t N, const void* A, const void* B, int64_t strideB, const void* lambda) {
  ND4_CHECK_ARG(algo == 0 || algo == 1, "nd4hip_dsygvd_batched: algo must be 0 (dc) or 1 (jacobi)");
  ND4_CHECK_ARG(batch >= 0 && N >= 0, "nd4hip_dsygvd_batched: negative extent");
  ND4_CHECK_ARG(algo == 1 || N <= 2048, "nd4hip_dsygvd_batched: the divide & conquer solver takes N <= 2048");
  ND4_CHECK_ARG(algo == 0 || N <= 128, "nd4hip_dsygvd_batched: the Jacobi route takes N <= 128");
  ND4_CHECK_ARG(strideB == 0 || strideB == N * N, "nd4hip_dsygvd_batched: strideB must be N*N or 0");
  if (batch == 0 || N == 0) return ND4_ARGS_EMPTY;
  ND4_CHECK_ARG(A && B && lambda, "nd4hip_dsygvd_batched: NULL pointer");
  return ND4_ARGS_GO;
}
// eigen_sym_gen with a selector (divide & conquer side only): reduction 0 / 1, select 0 (all), 1 (subset (i0, i1)) or 2 (interval:
// bounds, kcap, range and kmax as the interval forms above); what a select does not use is not looked at
inline int nd4_args_sygvx(int reduction, int select, int64_t batch, int64_t N, int64_t i0, int64_t i1, int64_t kcap, const void* bounds,
                          const void* A, const void* B, int64_t strideB, const void* lambda, const void* range, const void* kmax) {
  ND4_CHECK_ARG(reduction == 0 || reduction == 1, "nd4hip_dsygvx_batched: reduction must be 0 (hessenberg) or 1 (tridiag)");
  ND4_CHECK_ARG(select >= 0 && select <= 2, "nd4hip_dsygvx_batched: select must be 0 (all), 1 (subset) or 2 (interval)");
  ND4_CHECK_ARG(batch >= 0 && N >= 0 && (select != 2 || kcap >= 0), "nd4hip_dsygvx_batched: negative extent");
  ND4_CHECK_ARG(select != 1 || (0 <= i0 && i0 <= i1 && i1 <= N), "nd4hip_dsygvx_batched: subset must satisfy 0 <= i0 <= i1 <= N");
  ND4_CHECK_ARG(N <= 2048, "nd4hip_dsygvx_batched: N <= 2048");
  ND4_CHECK_ARG(strideB == 0 || strideB == N * N, "nd4hip_dsygvx_batched: strideB must be N*N or 0");
  if (batch == 0 || N == 0 || (select == 1 && i0 == i1)) return ND4_ARGS_EMPTY;
  ND4_CHECK_ARG(A && B && (lambda || (select == 2 && kcap == 0)) && (select != 2 || (bounds && range && kmax)),
                "nd4hip_dsygvx_batched: NULL pointer");
  return ND4_ARGS_GO;
}
inline int nd4_args_sygst(int64_t batch, int64_t N, const void* A, const void* L, int64_t strideL, const void* C) {
  ND4_CHECK_ARG(batch >= 0 && N >= 0, "nd4hip_dsygst_batched: negative extent");
  ND4_CHECK_ARG(N <= 2048, "nd4hip_dsygst_batched: N <= 2048");
  ND4_CHECK_ARG(strideL == 0 || strideL == N * N, "nd4hip_dsygst_batched: strideL must be N*N or 0");
  if (batch == 0 || N == 0) return ND4_ARGS_EMPTY;
  ND4_CHECK_ARG(A && L && C, "nd4hip_dsygst_batched: NULL pointer");
  return ND4_ARGS_GO;
}
