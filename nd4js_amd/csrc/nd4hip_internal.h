// Internal declarations shared by the libnd4hip.so translation units (not part of the C ABI).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <cstdarg>
#include <vector>
#include "../../include/nd4hip.h"

struct Nd4WsBlock { char* p; size_t size, used; };

struct Nd4Stage { void* p; size_t bytes; bool in_use; };   // cached device staging block of the host-pointer entry points

struct nd4hip_handle {
  int device = 0;
  hipStream_t own_stream = nullptr;   // created by nd4hip_create
  hipStream_t stream = nullptr;       // the stream work is enqueued on (own or caller's)
  std::vector<Nd4WsBlock> ws;         // device workspace arena (bump allocation, LIFO release)
  std::vector<Nd4Stage> stage;        // staging blocks kept between host-pointer calls (hipMalloc/hipFree cost ~100 us each)
  size_t stage_bytes = 0;
  void* pinned = nullptr;             // small pinned host buffer for scalar read-backs
  size_t pinned_bytes = 0;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  hipEvent_t ev_order = nullptr;      // orders the workspace arena across a change of stream (nd4hip_set_stream)
  hipStream_t copy_stream = nullptr;  // H2D / D2H of the host-pointer entry points (overlaps the kernels on `stream`)
  hipStream_t aux_stream = nullptr;   // second chain of the block-Jacobi sweeps (svd_block.hip), beside the first on `stream`
  hipEvent_t ev_aux_a = nullptr, ev_aux_b = nullptr;
  hipEvent_t ev_in[2] = {nullptr, nullptr}, ev_chunk[2] = {nullptr, nullptr};   // per staging set: inputs landed / kernels done
  std::vector<nd4hip_handle*> peers;  // further devices of a multi-device handle (nd4hip_create_multi); owned
  int* xstat = nullptr;               // host-coherent status word the kernels raise when an in-kernel exchange times out (ND4HIP_ERR_XCHG)
  int num_cu = 256;
  unsigned ws_generation = 0;         // bumped whenever the idle arena is dropped and rebuilt (Nd4WsScope)
  int svd_sweeps = 0; unsigned long long svd_rotations = 0; double svd_offnorm = 0.0;   // audit of the last SVD call
  bool prof_on = false, prof_valid = false; int prof_depth = 0;                          // nd4hip_profile_enable / _last
  hipEvent_t ev_p0 = nullptr, ev_p1 = nullptr; double prof_flops = 0.0, prof_bytes = 0.0; char prof_op[32] = "";
  double dc_stage_ms[ND4HIP_DC_STAGES] = {0};   // per-stage times of the last divide & conquer SVD run with the profile enabled
  double syev_stage_ms[ND4HIP_SYEV_STAGES] = {0};   // the same for the last symmetric eigenproblem (syev.hip)
  double syevx_stage_ms[ND4HIP_SYEVX_STAGES] = {0}; // and for the last one by bisection and inverse iteration (syevx.hip)
  double svdx_stage_ms[ND4HIP_SVDX_STAGES] = {0};   // and for the last selected-triplet SVD (bdsvdx.hip)
};

// Makes h->device the calling thread's current HIP device for the duration of an entry point and restores the previous
// one: workspace hipMalloc, kernel launches and event records all act on the current device, and a caller such as torch may
// have another device current (tensor on cuda:1 while cuda:0 is current).
struct Nd4DeviceGuard {
  int prev = -1; bool switched = false;
  explicit Nd4DeviceGuard(const nd4hip_handle* h) {
    if (hipGetDevice(&prev) == hipSuccess && prev != h->device) switched = hipSetDevice(h->device) == hipSuccess;
  }
  ~Nd4DeviceGuard() { if (switched) (void)hipSetDevice(prev); }
  Nd4DeviceGuard(const Nd4DeviceGuard&) = delete;
  Nd4DeviceGuard& operator=(const Nd4DeviceGuard&) = delete;
};

// brackets the kernels of one entry point with the handle's profile events (outermost entry point only: QR inside SVD does not count)
struct Nd4Prof {
  nd4hip_handle* h; bool active;
  Nd4Prof(nd4hip_handle* hh, const char* op, double flops, double bytes);
  ~Nd4Prof();
  Nd4Prof(const Nd4Prof&) = delete;
  Nd4Prof& operator=(const Nd4Prof&) = delete;
};

void nd4_set_error(const char* fmt, ...);
// after a synchronisation: ND4HIP_ERR_XCHG (and the word cleared) if a kernel raised the handle's exchange status word
int  nd4_xchg_check(nd4hip_handle* h, const char* where);
// tests only: ND4HIP_TEST_DROP_PUBLISH=<panel> (read per call) makes one workgroup of that panel skip one publication
int  nd4_test_drop_panel();
int  nd4_hip_fail(hipError_t e, const char* what, const char* file, int line);

#define ND4_HIP(expr)                                                           \
  do { hipError_t _e = (expr);                                                  \
       if (_e != hipSuccess) return nd4_hip_fail(_e, #expr, __FILE__, __LINE__); } while (0)
#define ND4_CHECK_ARG(cond, ...)                                                \
  do { if (!(cond)) { nd4_set_error(__VA_ARGS__); return ND4HIP_ERR_ARG; } } while (0)
#define ND4_TRY(expr) do { int _rc = (expr); if (_rc != 0) return _rc; } while (0)

// Workspace arena. Kernels are stream-ordered, so a region released at the end of one call can be
// handed out to the next call on the same stream. Nested users (SVD -> QR -> GEMM) each open a
// Nd4WsScope; allocations never move or free blocks that are in use.
int nd4_ws_alloc(nd4hip_handle* h, size_t bytes, void** out);      // 256-byte aligned
struct Nd4WsScope {
  nd4hip_handle* h; size_t nblocks; size_t used_last; unsigned generation;
  explicit Nd4WsScope(nd4hip_handle* hh);
  ~Nd4WsScope();
};
int nd4_pinned(nd4hip_handle* h, size_t bytes, void** out);

// ---- internal launchers (device pointers, enqueue on h->stream) --------------------------------
// C = alpha*op(A)*op(B) + beta*C, batched over gridDim.y with element strides sA/sB/sC
int nd4_gemm(nd4hip_handle* h, bool transA, bool transB, int64_t M, int64_t N, int64_t K,
             double alpha, const double* A, int64_t lda, int64_t sA,
             const double* B, int64_t ldb, int64_t sB,
             double beta, double* C, int64_t ldc, int64_t sC, int64_t batch);
// complex: C[b] = A[b] * B[b] on interleaved (re, im) doubles, A complex I x K, B complex (b_complex) or real K x J,
// C dense complex [batch, I, J]; strides in elements of each operand, batch <= 65535 (zgemm.hip)
int nd4_zgemm(nd4hip_handle* h, bool b_complex, int64_t batch, int64_t I, int64_t K, int64_t J,
              const double* A, int64_t sA, const double* B, int64_t sB, double* C);

int nd4_getrf(nd4hip_handle* h, int64_t batch, int64_t N, const double* A, double* LU, int32_t* P);
int nd4_getrf_nopivot(nd4hip_handle* h, int64_t batch, int64_t N, const double* A, double* LU, int32_t* P);
int nd4_trsm(nd4hip_handle* h, bool upper, bool unit, int64_t batch, int64_t M, int64_t J, const double* T, int64_t sT, double* X);
int nd4_syrk_lower(nd4hip_handle* h, int64_t N, int64_t K, double alpha, const double* A, int64_t lda, int64_t sA,
                   double beta, double* C, int64_t ldc, int64_t sC, int64_t batch);
int nd4_gemm_nt_lower(nd4hip_handle* h, int64_t N, int64_t K, double alpha, const double* A, int64_t lda, int64_t sA,
                      const double* B, int64_t ldb, int64_t sB, double beta, double* C, int64_t ldc, int64_t sC, int64_t batch);
int nd4_trsm_ld(nd4hip_handle* h, bool upper, bool unit, int64_t batch, int64_t M, int64_t J, const double* T, int64_t ldT, int64_t sT,
                double* X, int64_t sX);
int nd4_trsm_t(nd4hip_handle* h, int64_t batch, int64_t M, int64_t J, const double* T, int64_t ldT, int64_t sT, double* X, int64_t sX);
int nd4_trsm_t_ex(nd4hip_handle* h, bool unit, int64_t batch, int64_t M, int64_t J, const double* T, int64_t ldT, int64_t sT, double* X, int64_t sX);
int nd4_ldltrf(nd4hip_handle* h, int64_t batch, int64_t N, const double* S, double* LD);
int nd4_ldltrs(nd4hip_handle* h, int64_t batch, int64_t N, int64_t J, const double* LD, int64_t sLD, const double* Y, int64_t sY, double* X);
// pivoted LDL^T (pldlp.hip); flags [batch] zero on entry, tier: what nd4_sytrf_bk_tier returned (0: N does not fit)
void nd4_sytrf_bk_limits(int* lds_max_n, int* global_max_n, int* grid_tile);
int nd4_sytrf_bk_tier(const nd4hip_handle* h, int64_t batch, int64_t N, int tier);
int nd4_sytrf_bk(nd4hip_handle* h, int64_t batch, int64_t N, const double* S, double* LD, int32_t* P, int* flags, int tier);
int nd4_sytrs_bk(nd4hip_handle* h, int64_t batch, int64_t N, int64_t J, const double* LD, int64_t sLD, const int32_t* P, int64_t sP,
                 const double* Y, int64_t sY, double* X, int* flag);
// the _dev entry point with the index of its first member in the caller's batch (for the error text of the host-pointer form);
// *first_bad (may be NULL) receives the lowest singular member, counted in the caller's batch, when ND4HIP_ERR_SINGULAR is returned
int nd4_sytrf_bk_run(nd4hip_handle* h, int64_t batch, int64_t N, const double* S, double* LD, int32_t* P, int tier, int64_t member0,
                     int64_t* first_bad);
int nd4_gebrd(nd4hip_handle* h, int64_t batch, int64_t M, int64_t N, const double* A, double* U, double* B, double* V);
int nd4_gehrd(nd4hip_handle* h, int64_t batch, int64_t N, const double* A, double* U, double* H);
int nd4_potrf(nd4hip_handle* h, int64_t batch, int64_t N, const double* S, double* L, int* flags);
int nd4_potrs(nd4hip_handle* h, int64_t batch, int64_t N, int64_t J, const double* L, int64_t sL, const double* Y, int64_t sY, double* X);
int nd4_qrls(nd4hip_handle* h, int64_t batch, int64_t N, int64_t M, int64_t I, int64_t J, const double* Q, int64_t sQ,
             const double* R, int64_t sR, const double* Y, int64_t sY, double* X);
int nd4_svdls(nd4hip_handle* h, int64_t batch, int64_t N, int64_t M, int64_t I, int64_t J, const double* U, int64_t sU,
              const double* sv, int64_t sSv, const double* V, int64_t sV, const double* Y, int64_t sY, double* X);
int nd4_getrs(nd4hip_handle* h, int64_t batch, int64_t N, int64_t J, const double* LU, int64_t sLU, const int32_t* P, int64_t sP,
              const double* Y, int64_t sY, double* X);
int nd4_geqrf_q(nd4hip_handle* h, int64_t batch, int64_t M, int64_t N, const double* A, double* Q, double* R);
int nd4_geqr2_panel(nd4hip_handle* h, int batch, int M, double* A, double* V, double* T);
int nd4_givens_signs(nd4hip_handle* h, int batch, int M, int L, int ncols, bool lu_rule, double* Q, long ldq, long sQ,
                     double* R, long ldr, long sR, const double* taus, long sTau, int* flips);
int nd4_wy_form(nd4hip_handle* h, int M, int n, const double* V, const double* Tdiag, int bs, double* Q, int Lq);
int nd4_geqrf_q_ex(nd4hip_handle* h, int64_t batch, int64_t M, int64_t N, const double* A, double* Q, double* R, bool full);
// column-pivoted QR, its rank estimate and least squares (rrqr.hip)
int nd4_geqp3(nd4hip_handle* h, int64_t batch, int64_t M, int64_t N, const double* A, double* Q, double* R, int32_t* P, bool full);
int nd4_qp3rank(nd4hip_handle* h, int64_t batch, int64_t M, int64_t N, const double* R, int64_t sR, int* rank);
int nd4_qp3ls(nd4hip_handle* h, int64_t batch, int64_t N, int64_t M, int64_t I, int64_t J, const double* Q, int64_t sQ,
              const double* R, int64_t sR, const int32_t* P, int64_t sP, const double* Y, int64_t sY, double* X, int* rank_out);
// strong rank-revealing QR (srrqr.hip)
int nd4_srrqr(nd4hip_handle* h, int64_t batch, int64_t M, int64_t N, const double* A, double dtol, double ztol, double* Q, double* R,
              int32_t* P, int32_t* rank);
int nd4_urv(nd4hip_handle* h, int64_t batch, int64_t M, int64_t N, const double* A, double* U, double* R, double* V, int32_t* rank);
int nd4_urvls(nd4hip_handle* h, int64_t batch, int64_t I, int64_t J, int64_t K, int64_t Lv, int64_t Jc, const double* U, int64_t sU,
              const double* R, int64_t sR, const double* V, int64_t sV, const int32_t* rank, int64_t sRank, const double* Y, int64_t sY,
              double* X);
// determinants and the Frobenius norm (det.hip)
int nd4_dettri(nd4hip_handle* h, bool log_form, int64_t batch, int64_t N, const double* A, int64_t sA, double* D, double* L);
int nd4_det(nd4hip_handle* h, bool log_form, int64_t batch, int64_t M, int64_t N, const double* A, double* D, double* L, bool force_qr);
int nd4_nrmfro(nd4hip_handle* h, int64_t n, const double* A, double* out);
// eigenpairs of a real Schur form and balancing (eigvec.hip); flags [batch]: ND4HIP_EV_FLAG_* per matrix
int nd4_trevals(nd4hip_handle* h, int64_t batch, int64_t N, const double* T, double* Lam, int* blk, int* flags);
int nd4_trevc(nd4hip_handle* h, int64_t batch, int64_t N, const double* Q, const double* T, double* Lam, double* V, int* flags);
int nd4_gebal(nd4hip_handle* h, int64_t batch, int64_t N, double p, const double* A, double* D, double* B, int* flags);
int nd4_gebak(nd4hip_handle* h, int64_t batch, int64_t N, const double* D, const double* V, double* W);
// the Francis iteration of schur_decomp (schur.hip); flags [batch] zero on entry, sweeps [batch]; tier: ND4HIP_SCHUR_TIER_*
int nd4_hseqr(nd4hip_handle* h, int64_t batch, int64_t N, const double* U, const double* H, double* Q, double* T, int* flags, int* sweeps,
              int tier);
int64_t nd4_hseqr_chunk(int64_t N);
// structure functions (struct.hip): the reference's name of a dpermute mode, and whether an input of in_elems doubles overlaps an
// output of out_elems doubles
const char* nd4_permute_name(int cols, int inverse);
bool nd4_struct_overlap(const void* in, int64_t in_elems, const void* out, int64_t out_elems);
int nd4_gesvdj(nd4hip_handle* h, int64_t batch, int64_t M, int64_t N, const double* A,
               double* U, double* sv, double* V, int* sweeps_out, double* offnorm_out);
// the exact power-of-two scaling of the SVD entries (svd.hip): max|a| per member, dst = 2^-e src, sv *= 2^e
int nd4_svd_scale_begin(nd4hip_handle* h, int64_t batch, int64_t n, const double* A, unsigned long long* mx);
int nd4_svd_scale_apply(nd4hip_handle* h, int64_t batch, int64_t n, const double* src, double* dst, const unsigned long long* mx);
int nd4_svd_scale_undo(nd4hip_handle* h, int64_t batch, int64_t L, double* sv, const unsigned long long* mx);
// divide & conquer SVD (svd_dc.hip): the level list of n columns as (level, off, n) triples; the bidiagonal solver with V2 as
// rows; svd_decomp through bidiagonalisation. The last two synchronise once to read the assertion flag.
int nd4_bdsdc_plan(int64_t n, int32_t* out, int64_t capacity);
int nd4_bdsdc_rows(nd4hip_handle* h, int64_t batch, int64_t K, int64_t J, const double* d, const double* e, double* U2, double* sv, double* V2);
int nd4_gesdd(nd4hip_handle* h, int64_t batch, int64_t M, int64_t N, const double* A, double* U, double* sv, double* V);
// selected singular triplets (bdsvdx.hip): arguments already checked, batch in 1 .. 32768, 1 <= K <= 2048, 0 <= i0 < i1 <= K (min(M, N)),
// k = i1 - i0. U2 [batch, K, k] and V2 [batch, k, J] (U [batch, M, k] and V [batch, k, N]) both or neither; fallback [batch] may be NULL.
// Both synchronise.
int nd4_bdsvdx(nd4hip_handle* h, int64_t batch, int64_t K, int64_t J, int64_t i0, int64_t i1, const double* d, const double* e, double* U2,
               double* sv, double* V2, int32_t* fallback);
int nd4_gesvdx(nd4hip_handle* h, int64_t batch, int64_t M, int64_t N, int64_t i0, int64_t i1, const double* A, double* U, double* sv, double* V,
               int32_t* fallback);
// symmetric eigenproblem (syev.hip): lower triangle of S -> lambda descending, V columns (V may be NULL); synchronises
int nd4_syevd(nd4hip_handle* h, int64_t batch, int64_t N, const double* S, double* lambda, double* V);
// the same by two-sided Jacobi in one launch (syevj.hip): 1 <= N <= 128; sweeps [batch] may be NULL; synchronises
int nd4_syevj(nd4hip_handle* h, int64_t batch, int64_t N, const double* S, double* lambda, double* V, int32_t* sweeps);
// selected eigenpairs by bisection and inverse iteration (syevx.hip): arguments already checked, batch in 1 .. 32768, 1 <= N <= 2048,
// 0 <= i0 < i1 <= N, k = i1 - i0. count [batch, M]; lambda [batch, k]; Z [batch, k, N] rows = vectors, V [batch, N, k] columns =
// vectors, either may be NULL. nd4_stevx and nd4_syevx synchronise, nd4_stcnt enqueues only
int nd4_stcnt(nd4hip_handle* h, int64_t batch, int64_t N, int64_t M, const double* d, const double* e, const double* x, int32_t* count);
int nd4_stevx(nd4hip_handle* h, int64_t batch, int64_t N, int64_t i0, int64_t i1, const double* d, const double* e, double* lambda, double* Z);
int nd4_syevx(nd4hip_handle* h, int64_t batch, int64_t N, int64_t i0, int64_t i1, const double* S, double* lambda, double* V);
// the eigenpairs in a value interval (syevx.hip): bounds [batch, 2] = (lo, hi) and range [batch, 2] on the device,
// *kmax on the host; lambda [batch, kcap], Z [batch, kcap, N] rows = vectors, V [batch, N, kcap] columns = vectors, either may be
// NULL. Both synchronise. nd4_stxv_pad: NaN / zeros in the columns k_b .. kmax - 1 of every member (any batch); enqueues only
int nd4_stevxv(nd4hip_handle* h, int64_t batch, int64_t N, int64_t kcap, const double* bounds, const double* d, const double* e, double* lambda,
               double* Z, int32_t* range, int64_t* kmax);
int nd4_syevxv(nd4hip_handle* h, bool tridiag, int64_t batch, int64_t N, int64_t kcap, const double* bounds, const double* S, double* lambda,
               double* V, int32_t* range, int64_t* kmax);
int nd4_stxv_pad(nd4hip_handle* h, int64_t batch, int64_t N, int64_t kcap, int64_t kmax, const int32_t* range, double* lambda, double* vectors,
                 bool by_rows);
// symmetric tridiagonal reduction and its Q (sytrd.hip): arguments already checked, batch in 1 .. 32768, 1 <= N <= 2048, K >= 1.
// nd4_sytrd_run synchronises (one flag word), nd4_ormtr (Z [batch, N, K] in place) enqueues only. The four functions after them are
// the host-side arithmetic of the tiers: 0 = one workgroup per member in LDS, 1 = one launch per column.
int nd4_sytrd_run(nd4hip_handle* h, int64_t batch, int64_t N, const double* S, double* F, double* tau, double* d, double* e);
int nd4_ormtr(nd4hip_handle* h, int64_t batch, int64_t N, int64_t K, bool transpose, const double* F, const double* tau, double* Z);
int nd4_sytrd_tier(int64_t N);
size_t nd4_sytrd_lds(int64_t N);
int64_t nd4_sytrd_blocks(int64_t N);
size_t nd4_sytrd_ws_doubles(int64_t N);
// eigen_sym(S, reduction='tridiag'): nd4_syevd / nd4_syevx with that reduction in place of nd4_gehrd, the vectors by nd4_ormtr
int nd4_syevd_tr(nd4hip_handle* h, int64_t batch, int64_t N, const double* S, double* lambda, double* V);
int nd4_syevx_tr(nd4hip_handle* h, int64_t batch, int64_t N, int64_t i0, int64_t i1, const double* S, double* lambda, double* V);
// Hermitian tridiagonal reduction, its Q and the eigen routes on them (hetrd.hip): complex128 operands (H, F, tau, Z,
// V) as interleaved doubles, d, e and lambda real. Arguments already checked, batch in 1 .. 32768, 1 <= N <= 2048, K >= 1. nd4_hetrd is
// nd4_sytrd's counterpart (mx ZERO on entry, *flag zero on entry; enqueues only), nd4_hetrd_run synchronises (one flag word), nd4_zunmtr
// (Z [batch, N, K] in place) enqueues only. The five functions after them are the host-side arithmetic of the tiers: 0 = one
// workgroup per member in LDS, 1 = one launch per column; bytes of dynamic LDS, row blocks, bytes of workspace per member.
int nd4_hetrd(nd4hip_handle* h, int64_t batch, int64_t N, const double* H, double* F, double* tau, double* d, double* e, unsigned long long* mx,
              bool unscale, int* flag);
int nd4_hetrd_run(nd4hip_handle* h, int64_t batch, int64_t N, const double* H, double* F, double* tau, double* d, double* e);
int nd4_zunmtr(nd4hip_handle* h, int64_t batch, int64_t N, int64_t K, bool adjoint, const double* F, const double* tau, double* Z);
int nd4_hetrd_tier(int64_t N);
size_t nd4_hetrd_lds(int64_t N);
size_t nd4_zunmtr_lds(int64_t N);
int64_t nd4_hetrd_blocks(int64_t N);
size_t nd4_hetrd_ws_bytes(int64_t N);
// the small kernels the routes share: d, e of F onto the diagonals of the real Tr [batch, N, N]; V [batch, N, k] complex = the transposed
// rows of the real R [batch, k, N] (both enqueue only); the eigen routes at N = 1 (lambda = Re h_00, V = 1 or NULL; synchronises: NaN or
// Inf is refused with eigen_herm's text)
int nd4_hetrd_diagonals(nd4hip_handle* h, int64_t batch, int N, const double* F, double* Tr);
int nd4_hetrd_rows_to_columns(nd4hip_handle* h, int64_t batch, int N, int k, const double* R, double* V);
int nd4_hetrd_order_one(nd4hip_handle* h, int64_t batch, const double* H, double* lambda, double* V);
// eigen_herm: every eigenpair by divide & conquer (syev.hip), the subset (i0, i1) by bisection and inverse iteration (hetrd.hip);
// V = NULL: the values alone. Both synchronise
int nd4_zheevd(nd4hip_handle* h, int64_t batch, int64_t N, const double* H, double* lambda, double* V);
int nd4_zheevx(nd4hip_handle* h, int64_t batch, int64_t N, int64_t i0, int64_t i1, const double* H, double* lambda, double* V);
// Hermitian Cholesky, complex lower triangular solves and the generalised Hermitian-definite eigenproblem (hegv.hip):
// complex128 operands as interleaved doubles, strides in complex elements (0 = one for all). Arguments already checked, batch >= 1,
// 1 <= N <= 2048, K >= 1; member0: index of the first member in the caller's batch (error text). nd4_zpotrf and nd4_zhegvx synchronise,
// nd4_ztrsm (mode 0 L X = Y, 1 L^H X = Y, 2 L L^H X = Y, X in place) and nd4_zhegst enqueue only. all: every eigenpair, else the subset
// i0 <= i < i1; X = NULL: the values alone. The three functions after them are the host-side arithmetic: tier (0: a member in LDS,
// 1: blocks of 64), the largest dynamic LDS request in bytes, members per pass.
int nd4_zpotrf(nd4hip_handle* h, int64_t batch, int64_t N, const double* H, double* L, int64_t member0);
int nd4_ztrsm(nd4hip_handle* h, int mode, int64_t batch, int64_t N, int64_t K, const double* L, int64_t sL, double* X);
int nd4_zhegst(nd4hip_handle* h, int64_t batch, int64_t N, const double* A, const double* L, int64_t sL, double* C);
int nd4_zhegvx(nd4hip_handle* h, bool all, int64_t i0, int64_t i1, int64_t batch, int64_t N, const double* A, const double* B, int64_t sB,
               double* lambda, double* X, int64_t member0);
int nd4_hegv_tier(int64_t N);
size_t nd4_hegv_lds(int64_t N);
int64_t nd4_hegv_chunk(int64_t batch, int64_t N);
// the entry points with member0, shared by the _dev and _host forms (nd4hip_api.hip)
int nd4_zpotrf_run(nd4hip_handle* h, int64_t batch, int64_t N, const double* H, double* L, int64_t member0);
int nd4_zhegvd_run(nd4hip_handle* h, int64_t batch, int64_t N, const double* A, const double* B, int64_t strideB, double* lambda, double* X,
                   int64_t member0);
int nd4_zhegvx_run(nd4hip_handle* h, int64_t batch, int64_t N, int64_t i0, int64_t i1, const double* A, const double* B, int64_t strideB,
                   double* lambda, double* X, int64_t member0);
// generalised symmetric-definite eigenproblem (sygv.hip): arguments already checked, batch >= 1, 1 <= N; sB / sL 0 = one for all;
// member0: index of the first member in the caller's batch (error text); nd4_sygvd synchronises
int nd4_sygvd(nd4hip_handle* h, int algo, int64_t batch, int64_t N, const double* A, const double* B, int64_t sB, double* lambda,
              double* X, int32_t* sweeps, int64_t member0);
int nd4_sygst(nd4hip_handle* h, int64_t batch, int64_t N, const double* A, const double* L, int64_t sL, double* C);
// eigen_sym_gen with subset, interval or reduction: what step 3 computes of C = L^-1 A L^-T. reduction 1: nd4_sytrd in
// place of the Hessenberg reduction. select 0: every eigenpair (lambda [batch, N], X [batch, N, N]); 1: the subset (i0, i1) (K = i1 - i0
// wide); 2: the interval bounds [batch, 2] of every member, kcap wide and ragged, with range [batch, 2] and *kmax as nd4_syevxv's.
// Fields that a select does not use are 0 / NULL.
struct Nd4SygvSel { int reduction, select; int64_t i0, i1, kcap; const double* bounds; int32_t* range; int64_t* kmax; };
int nd4_sygvx(nd4hip_handle* h, int algo, const Nd4SygvSel& sel, int64_t batch, int64_t N, const double* A, const double* B, int64_t sB,
              double* lambda, double* X, int32_t* sweeps, int64_t member0);
int nd4_sygvx_run(nd4hip_handle* h, int reduction, int select, int64_t batch, int64_t N, int64_t i0, int64_t i1, int64_t kcap,
                  const double* bounds, const double* A, const double* B, int64_t strideB, double* lambda, double* X, int32_t* range,
                  int64_t* kmax, int64_t member0);
// the _dev entry point of eigen_sym_gen with member0 (for the host-pointer form, as nd4_sytrf_bk_run)
int nd4_sygvd_run(nd4hip_handle* h, int algo, int64_t batch, int64_t N, const double* A, const double* B, int64_t strideB, double* lambda,
                  double* X, int32_t* sweeps, int64_t member0);

// small utility kernels (nd4hip_core.hip)
int nd4_copy_matrix(nd4hip_handle* h, int64_t rows, int64_t cols, const double* src, int64_t lds,
                    double* dst, int64_t ldd, int64_t batch, int64_t ssrc, int64_t sdst);
int nd4_transpose(nd4hip_handle* h, int64_t rows, int64_t cols, const double* src, int64_t lds,
                  double* dst, int64_t ldd, int64_t batch, int64_t ssrc, int64_t sdst);
int nd4_set_identity(nd4hip_handle* h, int64_t rows, int64_t cols, double* dst, int64_t ldd,
                     int64_t batch, int64_t sdst);
