/* nd4hip.h — C ABI of libnd4hip.so: the MI355X (gfx950) backend of nd4js's `nd.la` hot path.
 *
 * The reference (nd4js v1.3.0, pure JavaScript) has no FFI/plugin layer; its boundary for this path
 * is the JS call contract of src/la/{matmul,qr,lu,svd}.js on dense row-major Float64Array /
 * Int32Array buffers. This header is the C ABI a maintainer binds underneath those
 * functions (N-API shim: nd4js_amd/csrc/napi_shim.c; ctypes: nd4js_amd/_lib.py).
 *
 * Conventions
 *  - plain pointers and sizes only; every matrix is dense, row-major, contiguous, fp64; leading
 *    (batch) dimensions are flattened by the host into `batch`;
 *  - inputs are never modified; outputs are caller-allocated;
 *  - return 0 on success, negative on error; nd4hip_last_error() gives the message (thread-local);
 *  - `*_dev` entry points take DEVICE pointers and enqueue on the handle's stream without
 *    synchronising the host (except where a host-visible scalar is returned: noted per function);
 *    the un-suffixed entry points take HOST pointers (what the JS TypedArrays are) and do
 *    H2D -> kernels -> D2H -> stream sync internally;
 *  - one handle = one GPU + one stream + one growable device workspace; calls on one handle are
 *    serialised by the caller (the JS host is single-threaded, like the reference).
 */
#ifndef ND4HIP_H
#define ND4HIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct nd4hip_handle nd4hip_handle;

#define ND4HIP_OK            0
#define ND4HIP_ERR_ARG      -1   /* bad argument / shape */
#define ND4HIP_ERR_HIP      -2   /* HIP runtime error (message has the hipError string) */
#define ND4HIP_ERR_NOCONV   -3   /* Jacobi SVD hit the sweep limit; the divide & conquer SVD met one of the reference's assertions */
#define ND4HIP_ERR_NODEV    -4   /* no usable GPU */
#define ND4HIP_ERR_SINGULAR -5   /* Cholesky met a NaN pivot: 'Matrix contains NaNs or is (near) singular.'; dsytrf_bk a zero column or NaN */
#define ND4HIP_ERR_XCHG     -6   /* an exchange between co-resident workgroups INSIDE a kernel timed out (the row-split QR panels, the
                                    multi-workgroup LU panels, the one-launch Hessenberg reduction / bidiagonalisation of one matrix of
                                    128 .. 2048 rows and columns): the results of the call are invalid — Q / R hold NaN, the permutation
                                    vector of an LU holds -1, U / H / B / V are unspecified — and the handle stays usable. Reported by the next entry point that
                                    synchronises: every host-pointer form, nd4hip_synchronize, nd4hip_timer_stop. The _dev forms
                                    enqueue only and return 0; their callers see the NaN / -1 markers or the code at the next
                                    nd4hip_synchronize. (The reference never returns a half-valid factorisation: lu.js:24-81.) */

/* ---- lifecycle --------------------------------------------------------------------------- */
int  nd4hip_device_count(void);
/* device < 0: use the current HIP device. Creates a private non-blocking stream. */
int  nd4hip_create(nd4hip_handle** out, int device);
void nd4hip_destroy(nd4hip_handle* h);
/* One handle over SEVERAL devices of the node (SURVEY.md §8b `nd4hip_init(handle**, device_ids, n_dev)`, §8e): the HOST-pointer
 * batched entry points cut the leading batch axis — the reference's loops over independent matrices, src/la/qr.js:43-49,
 * lu.js:34-40, svd_dc.js:918-925, matmul.js:44-70 — into contiguous blocks, one per device (nd4hip_partition), each block
 * uploaded, computed and downloaded by its own host thread on its own device and streams; results land directly in the
 * caller's arrays, so there is no data-path collective. The *_dev entry points, nd4hip_malloc / nd4hip_set_stream and single
 * matrices (batch 1: "replicas only") use device_ids[0]. nd4hip_destroy releases all devices. */
int  nd4hip_create_multi(nd4hip_handle** out, const int* device_ids, int n_dev);
/* number of devices behind the handle; their ids are written to device_ids[0..capacity) when it is not NULL */
int  nd4hip_device_list(nd4hip_handle* h, int* device_ids, int capacity);
/* the block [lo, hi) of a batch that device number `index` (0-based position in the handle's list) of n_dev devices processes:
 * contiguous, sizes differ by at most one, remainder to the low devices; devices beyond the batch get an empty block */
int  nd4hip_partition(int64_t batch, int n_dev, int index, int64_t* lo, int64_t* hi);
/* run on a caller-owned hipStream_t (e.g. torch.cuda.current_stream().cuda_stream). NULL is a
 * valid value: HIP's default (null) stream. nd4hip_reset_stream goes back to the private stream. */
int  nd4hip_set_stream(nd4hip_handle* h, void* hip_stream);
int  nd4hip_reset_stream(nd4hip_handle* h);
int  nd4hip_synchronize(nd4hip_handle* h);
const char* nd4hip_last_error(void);
const char* nd4hip_version(void);

/* device memory for hosts without their own allocator (the N-API shim, C/C++ drivers) */
int  nd4hip_malloc(nd4hip_handle* h, size_t bytes, void** dev_ptr);
int  nd4hip_free(nd4hip_handle* h, void* dev_ptr);
int  nd4hip_memcpy_h2d(nd4hip_handle* h, void* dst_dev, const void* src_host, size_t bytes);
int  nd4hip_memcpy_d2h(nd4hip_handle* h, void* dst_host, const void* src_dev, size_t bytes);

/* hipEvent timing on the handle's stream (bench.py roofline leg): start, enqueue work, stop -> ms */
int  nd4hip_timer_start(nd4hip_handle* h);
int  nd4hip_timer_stop(nd4hip_handle* h, float* ms_out);   /* synchronises the stream */

/* synthetic inputs: out[i] = u(seed, offset+i) in [-1,1), bit-identical to nd4js_amd/rng.py */
int  nd4hip_fill_uniform_dev(nd4hip_handle* h, uint32_t seed, uint32_t offset, int64_t n, double* out_dev);

/* ---- matmul2: replaces the matmul2_RR hot loop, src/la/matmul.js:31-74 (:49-53) -------------
 * C[b] (I x J) = A[b] (I x K) * B[b] (K x J), b = 0..batch-1; element strides strideA/strideB
 * between consecutive batch members, 0 = the operand is broadcast (the reference's odometer,
 * matmul.js:44-70, is flattened into (batch, stride) groups by the host wrapper). C is dense
 * [batch, I, J]. */
int nd4hip_dgemm_batched_dev(nd4hip_handle* h, int64_t batch, int64_t I, int64_t K, int64_t J,
                             const double* A, int64_t strideA, const double* B, int64_t strideB, double* C);
int nd4hip_dgemm_batched    (nd4hip_handle* h, int64_t batch, int64_t I, int64_t K, int64_t J,
                             const double* A, int64_t strideA, const double* B, int64_t strideB, double* C);

/* ---- complex matmul2: replaces matmul2_CC, matmul2_CR and matmul2_RC, src/la/matmul.js:74-87 ------------------------
 * C[b] (I x J, complex) = A[b] (I x K) * B[b] (K x J). An operand whose flag (a_complex / b_complex) is set is complex128:
 * interleaved (re, im) doubles, the layout of the reference's ComplexArray._array, numpy and torch; otherwise it is float64.
 * At least one flag must be set; C is always complex and dense [batch, I, J]. Strides count elements of each operand (one
 * complex element = one element = 16 bytes), 0 = broadcast, as nd4hip_dgemm_batched. The reference's products are formed:
 * CC four (Re = Ar Br - Ai Bi, Im = Ar Bi + Ai Br, no 3M trick), CR and RC two, so NaN / Inf land where the reference puts
 * them. RC runs as the real product of A with the K x 2J real view of B. */
int nd4hip_zgemm_batched_dev(nd4hip_handle* h, int a_complex, int b_complex, int64_t batch, int64_t I, int64_t K, int64_t J,
                             const double* A, int64_t strideA, const double* B, int64_t strideB, double* C);
int nd4hip_zgemm_batched    (nd4hip_handle* h, int a_complex, int b_complex, int64_t batch, int64_t I, int64_t K, int64_t J,
                             const double* A, int64_t strideA, const double* B, int64_t strideB, double* C);

/* general strided form used by the decompositions and exposed for tests:
 * C = alpha * op(A) * op(B) + beta * C, row-major with leading dimensions; transA/transB != 0
 * means the stored matrix is the transpose of the operand (A stored K x M, B stored N x K). */
int nd4hip_dgemm_ex_dev(nd4hip_handle* h, int transA, int transB, int64_t M, int64_t N, int64_t K,
                        double alpha, const double* A, int64_t lda, const double* B, int64_t ldb,
                        double beta, double* C, int64_t ldc);

/* ---- lu_decomp: replaces src/la/lu.js:24-81 ---------------------------------------------------
 * A [batch,N,N] -> LU [batch,N,N] (unit-L below the diagonal, U on/above) and the PERMUTATION
 * VECTOR P [batch,N] int32 with A[P[i],:] = (L*U)[i,:] (not LAPACK ipiv); pivot = first maximum of
 * |x| down the column (lu.js:48-52). N > 2048 uses panels whose rows are spread over co-resident workgroups with one in-kernel
 * exchange per column: should such an exchange time out, every entry of P is -1 (never a half-valid permutation) and the next
 * synchronising entry point returns ND4HIP_ERR_XCHG; the host-pointer form returns it itself. */
int nd4hip_dgetrf_batched_dev(nd4hip_handle* h, int64_t batch, int64_t N, const double* A, double* LU, int32_t* P);
int nd4hip_dgetrf_batched    (nd4hip_handle* h, int64_t batch, int64_t N, const double* A, double* LU, int32_t* P);

/* ---- lu_solve: replaces src/la/lu.js:84-177 -------------------------------------
 * X [batch,N,J] = U^-1 L^-1 Y[P,:] for LU/P as returned by dgetrf. strides in ELEMENTS between consecutive
 * batch members, 0 = the operand is broadcast over the batch (lu.js:148-163 broadcasting, flattened by
 * the host wrapper). */
int nd4hip_dgetrs_batched_dev(nd4hip_handle* h, int64_t batch, int64_t N, int64_t J, const double* LU, int64_t strideLU,
                              const int32_t* P, int64_t strideP, const double* Y, int64_t strideY, double* X);
int nd4hip_dgetrs_batched    (nd4hip_handle* h, int64_t batch, int64_t N, int64_t J, const double* LU, int64_t strideLU,
                              const int32_t* P, int64_t strideP, const double* Y, int64_t strideY, double* X);

/* ---- tril_solve / triu_solve: replace src/la/tri.js:155-290 (kernels :45-95) ----------------------
 * X [batch,M,J] = T^-1 Y with T [batch,M,M] lower (upper = 0) or upper (upper != 0) triangular; only that
 * triangle of T is read; unit_diag != 0 treats the diagonal as ones: the stored diagonal is not read at all (it may hold
 * anything, NaN included, e.g. the D of a packed LDL^T or the U diagonal of a packed LU). strideT / strideY = 0 broadcast;
 * X is dense ([batch,M,J], no stride) and may be Y itself when strideY = M*J. T, Y and everything outside X are never written. */
int nd4hip_dtrsm_batched_dev(nd4hip_handle* h, int upper, int unit_diag, int64_t batch, int64_t M, int64_t J,
                             const double* T, int64_t strideT, const double* Y, int64_t strideY, double* X);
int nd4hip_dtrsm_batched    (nd4hip_handle* h, int upper, int unit_diag, int64_t batch, int64_t M, int64_t J,
                             const double* T, int64_t strideT, const double* Y, int64_t strideY, double* X);

/* ---- cholesky_decomp: replaces src/la/cholesky.js:51-71 (kernel :27-48)    -------------
 * S [batch,N,N] symmetric positive definite, only the lower triangle is read (:65-67) -> L [batch,N,N] lower
 * triangular with exact zeros above the diagonal, S = L L^T. A NaN pivot in any matrix returns ND4HIP_ERR_SINGULAR
 * with the reference's message (:43-44); L then holds NaNs from that pivot on. Both forms synchronise once
 * (a batch-sized flag read-back) to decide that. */
int nd4hip_dpotrf_batched_dev(nd4hip_handle* h, int64_t batch, int64_t N, const double* S, double* L);
int nd4hip_dpotrf_batched    (nd4hip_handle* h, int64_t batch, int64_t N, const double* S, double* L);

/* ---- cholesky_solve: replaces src/la/cholesky.js:74-150 ------------------------------------------------
 * X [batch,N,J] = L^-T L^-1 Y (forward substitution tri.js:45-71, then backward with the transpose :100-125).
 * strides in elements, 0 = broadcast. */
int nd4hip_dpotrs_batched_dev(nd4hip_handle* h, int64_t batch, int64_t N, int64_t J, const double* L, int64_t strideL,
                              const double* Y, int64_t strideY, double* X);
int nd4hip_dpotrs_batched    (nd4hip_handle* h, int64_t batch, int64_t N, int64_t J, const double* L, int64_t strideL,
                              const double* Y, int64_t strideY, double* X);

/* ---- ldl_decomp / ldl_solve: replace src/la/ldl.js:67-90 (kernel :47-64) and :133-201 (kernel :93-130) ----
 * S [batch,N,N] symmetric (lower triangle read), no pivoting -> packed LD [batch,N,N]: unit-lower L below the
 * diagonal, D on it, exact zeros above; S = L D L^T. A zero pivot propagates Inf/NaN exactly like the reference
 * (no check there either). dldltrs: X [batch,N,J] = L^-T D^-1 L^-1 Y; strides in elements, 0 = broadcast. */
int nd4hip_dldltrf_batched_dev(nd4hip_handle* h, int64_t batch, int64_t N, const double* S, double* LD);
int nd4hip_dldltrf_batched    (nd4hip_handle* h, int64_t batch, int64_t N, const double* S, double* LD);
int nd4hip_dldltrs_batched_dev(nd4hip_handle* h, int64_t batch, int64_t N, int64_t J, const double* LD, int64_t strideLD,
                               const double* Y, int64_t strideY, double* X);
int nd4hip_dldltrs_batched    (nd4hip_handle* h, int64_t batch, int64_t N, int64_t J, const double* LD, int64_t strideLD,
                               const double* Y, int64_t strideY, double* X);

/* ---- pldlp_decomp / pldlp_solve: replace src/la/pldlp.js:191-222 (kernel :35-188) and :519-604 (kernel :441-516) ----
 * Bunch-Kaufman partial pivoting after LAPACK's DSYTF2, 1x1 and 2x2 pivots. S [batch,N,N] symmetric (lower triangle read) ->
 * LD [batch,N,N] (unit-lower L below the diagonal blocks, the 1x1 and 2x2 blocks of D on them, exact zeros above the diagonal)
 * and P [batch,N] int32, the row order, with the SECOND row of every 2x2 block stored complemented (~p). LD and P are the
 * reference's bit for bit on every tier: the kernels restate its operation order and are compiled without FMA contraction
 * (csrc/pldlp.hip). S may be LD. A step before the last whose column is zero or holds a NaN where the searches look stops that
 * matrix: the call returns ND4HIP_ERR_SINGULAR and nd4hip_last_error is the reference's text followed by the lowest such
 * member, '_pldlp_decomp(M,N, LD,LD_off, P,P_off): Zero column or NaN encountered. (matrix <b>)'; the other members are
 * complete, in both forms (the host-pointer form brings every member back before it reports). The last step is not checked, like the reference's: [[0]] factorises.
 * The _ex forms take the tier. LDS: one workgroup per matrix, the triangle in LDS, N <= lds_max_n. GLOBAL: one workgroup per
 * matrix in global memory, N <= global_max_n. GRID: one matrix over the whole chip, a pivot launch and an update launch (tiles
 * of grid_tile^2) per step, a batch loops over its members. AUTO: LDS where N fits, else GLOBAL when the batch has at least as
 * many members as the device has CUs, else GRID. A tier that cannot hold N is ND4HIP_ERR_ARG. nd4hip_dsytrf_bk_limits reports
 * the three constants (any pointer may be NULL); nd4hip_dsytrf_bk_tier returns the tier a call would take (1..3) or
 * ND4HIP_ERR_ARG.
 * dsytrs_bk: X [batch,N,J] = P L^-T D^-1 L^-1 P^T Y; strides in elements, 0 = broadcast; X may be Y. Every index read from P
 * is range-checked on the device before it is used; an unusable P is ND4HIP_ERR_ARG 'pldlp_solve(LD,P,y): P contains
 * out-of-bounds indices.' and never reads or writes out of bounds. The host-pointer form checks P completely (range,
 * duplicates, block structure; the reference's pldlp_p messages) before any device work. */
#define ND4HIP_PLDLP_TIER_AUTO   0
#define ND4HIP_PLDLP_TIER_LDS    1
#define ND4HIP_PLDLP_TIER_GLOBAL 2
#define ND4HIP_PLDLP_TIER_GRID   3
int nd4hip_dsytrf_bk_batched_dev   (nd4hip_handle* h, int64_t batch, int64_t N, const double* S, double* LD, int32_t* P);
int nd4hip_dsytrf_bk_batched       (nd4hip_handle* h, int64_t batch, int64_t N, const double* S, double* LD, int32_t* P);
int nd4hip_dsytrf_bk_batched_ex_dev(nd4hip_handle* h, int64_t batch, int64_t N, const double* S, double* LD, int32_t* P, int tier);
int nd4hip_dsytrf_bk_batched_ex    (nd4hip_handle* h, int64_t batch, int64_t N, const double* S, double* LD, int32_t* P, int tier);
int nd4hip_dsytrs_bk_batched_dev   (nd4hip_handle* h, int64_t batch, int64_t N, int64_t J, const double* LD, int64_t strideLD,
                                    const int32_t* P, int64_t strideP, const double* Y, int64_t strideY, double* X);
int nd4hip_dsytrs_bk_batched       (nd4hip_handle* h, int64_t batch, int64_t N, int64_t J, const double* LD, int64_t strideLD,
                                    const int32_t* P, int64_t strideP, const double* Y, int64_t strideY, double* X);
int nd4hip_dsytrf_bk_tier          (nd4hip_handle* h, int64_t batch, int64_t N, int tier);
int nd4hip_dsytrf_bk_limits        (int* lds_max_n, int* global_max_n, int* grid_tile);

/* ---- bidiag_decomp: replaces src/la/bidiag.js:245-319 (kernels :32-242) -----------------------------------
 * A [batch,M,N] -> U [batch,M,K], B [batch,K,J] upper bidiagonal (exact zeros elsewhere), V [batch,J,N] with A = U B V,
 * K = min(M,N), J = K for M >= N and K+1 for M < N; U has orthonormal columns, V orthonormal rows. The signs follow
 * the reference's three branches (see csrc/bidiag.hip), so U, B, V agree with it to rounding. One matrix with 128 <= M, N <= 2048
 * is reduced by ONE launch whose 256 workgroups exchange inside the kernel (csrc/bidiag.hip: bdp): ND4HIP_ERR_XCHG applies. */
int nd4hip_dgebrd_batched_dev(nd4hip_handle* h, int64_t batch, int64_t M, int64_t N, const double* A, double* U, double* B, double* V);
int nd4hip_dgebrd_batched    (nd4hip_handle* h, int64_t batch, int64_t M, int64_t N, const double* A, double* U, double* B, double* V);

/* ---- hessenberg_decomp: replaces src/la/hessenberg.js:89-115 (kernel :27-86) -------------------------------
 * A [batch,N,N] -> U, H [batch,N,N] with A = U H U^T, U orthogonal (last row and column = unit vector), H upper
 * Hessenberg with exact zeros below the sub-diagonal. Same reflectors as the reference (rows finished from the bottom
 * up, sign chosen against cancellation), so U and H agree with it to rounding. H may alias A in the _dev form. One matrix with
 * 128 <= N <= 2048 is reduced by ONE launch whose 256 workgroups exchange inside the kernel (csrc/hess.hip: hessp): ND4HIP_ERR_XCHG
 * applies. */
int nd4hip_dgehrd_batched_dev(nd4hip_handle* h, int64_t batch, int64_t N, const double* A, double* U, double* H);
int nd4hip_dgehrd_batched    (nd4hip_handle* h, int64_t batch, int64_t N, const double* A, double* U, double* H);

/* ---- qr_lstsq: replaces src/la/qr.js:186-273 -------------------------------------
 * X [batch,I,J] = R[0:L,0:L]^-1 (Q^T Y)[0:L,:], L = min(M,I), rows L..I-1 zero; Q [batch,N,M], R [batch,M,I]
 * (as returned by dgeqrf_q for an N x I system: M = min(N,I)), Y [batch,N,J]. I > N is refused like qr.js:209.
 * strides in elements, 0 = broadcast. One TN GEMM + one blocked triangular solve on the device. */
int nd4hip_dqrls_batched_dev(nd4hip_handle* h, int64_t batch, int64_t N, int64_t M, int64_t I, int64_t J,
                             const double* Q, int64_t strideQ, const double* R, int64_t strideR,
                             const double* Y, int64_t strideY, double* X);
int nd4hip_dqrls_batched    (nd4hip_handle* h, int64_t batch, int64_t N, int64_t M, int64_t I, int64_t J,
                             const double* Q, int64_t strideQ, const double* R, int64_t strideR,
                             const double* Y, int64_t strideY, double* X);

/* ---- svd_lstsq / svd_solve: replace src/la/svd.js:66-228 ---------------------------------------------
 * X [batch,I,J] = V[0:r,:]^T diag(1/sv[0:r]) U[:,0:r]^T Y with r = first index with |sv_r| <= sqrt(eps)|sv_0|
 * (svd_rank, svd.js:31-63), U [batch,N,M], sv [batch,M], V [batch,M,I], Y [batch,N,J]. The host form
 * refuses non-finite singular values (svd.js:171-172, ND4HIP_ERR_ARG); the _dev form does not look. */
int nd4hip_dsvdls_batched_dev(nd4hip_handle* h, int64_t batch, int64_t N, int64_t M, int64_t I, int64_t J,
                              const double* U, int64_t strideU, const double* sv, int64_t strideSv,
                              const double* V, int64_t strideV, const double* Y, int64_t strideY, double* X);
int nd4hip_dsvdls_batched    (nd4hip_handle* h, int64_t batch, int64_t N, int64_t M, int64_t I, int64_t J,
                              const double* U, int64_t strideU, const double* sv, int64_t strideSv,
                              const double* V, int64_t strideV, const double* Y, int64_t strideY, double* X);

/* ---- qr_decomp: replaces src/la/qr.js:80-145 / qr_decomp_full :27-77 ----------------------------
 * A [batch,M,N] -> Q [batch,M,L], R [batch,L,N], L = min(M,N); blocked Householder with the
 * reference's Givens sign convention restored (R_jj >= 0 wherever a column had something to
 * eliminate, det(Q)=+1 for M <= N: SURVEY.md §8 A4). */
int nd4hip_dgeqrf_q_batched_dev(nd4hip_handle* h, int64_t batch, int64_t M, int64_t N, const double* A, double* Q, double* R);
int nd4hip_dgeqrf_q_batched    (nd4hip_handle* h, int64_t batch, int64_t M, int64_t N, const double* A, double* Q, double* R);

/* ---- qr_decomp_full: replaces src/la/qr.js:27-77 for every shape -----------------
 * A [batch,M,N] -> Q [batch,M,M], R [batch,M,N]. For M <= N identical to dgeqrf_q. For M > N the Givens-full
 * convention applies (R_jj >= 0 wherever something was eliminated, rows N.. of R zero) and the trailing M-N
 * columns of Q are AN orthonormal completion: the reference's own depends on its rotation order, so only
 * Q[:, 0:N], R and the properties Q Q^T = I, Q R = A are comparable. */
int nd4hip_dgeqrf_full_batched_dev(nd4hip_handle* h, int64_t batch, int64_t M, int64_t N, const double* A, double* Q, double* R);
int nd4hip_dgeqrf_full_batched    (nd4hip_handle* h, int64_t batch, int64_t M, int64_t N, const double* A, double* Q, double* R);

/* ---- _qr_decomp_inplace: replaces src/la/qr.js:146-183 (used by opt/_trust_region_solver_tls.js:1126) ----
 * In place: A [batch,M,N] <- R (upper trapezoid, zeros below), Y [batch,M,L] <- Q^T Y with the full M x M Q of
 * dgeqrf_full. Rows N.. of the result Y (only when M > N) are expressed in this library's completion basis. */
int nd4hip_dgeqrf_qty_batched_dev(nd4hip_handle* h, int64_t batch, int64_t M, int64_t N, int64_t L, double* A, double* Y);
int nd4hip_dgeqrf_qty_batched    (nd4hip_handle* h, int64_t batch, int64_t M, int64_t N, int64_t L, double* A, double* Y);

/* ---- rrqr_decomp / rrqr_decomp_full: replace src/la/rrqr.js:278-395 / :88-184 (column-pivoted QR) -----------------------
 * A [batch,M,N] -> P [batch,N] int32 with A[:, P] = Q R. dgeqp3: Q [batch,M,L], R [batch,L,N], L = min(M,N) (the economic form of
 * rrqr_decomp; for M <= N it is the full form). dgeqp3_full: Q [batch,M,M], R [batch,M,N]. The pivot is chosen as the reference does
 * (rrqr.js:124-138): before step i every remaining column's norm below row i is recomputed from scratch (no downdating), the first
 * maximum wins (an earlier column on a tie, a NaN never), and the pass stops when that maximum is exactly zero, leaving the
 * remaining columns in their order. Q and R are those of dgeqrf_q / dgeqrf_full on A[:, P] (as the reference's are those of
 * its qr_decomp of A[:, P]), with their sign conventions and, for M > N in the full form, the same orthonormal completion.
 * Two limits of those conventions show on structured input: for M > N the c >= 0 rule is read off the leading minors of Q's
 * top block, which vanish for a permuted diagonal or zero-row matrix, and a column whose part below the diagonal is exactly
 * zero can still get R_jj >= 0 where the reference keeps the entry's sign. There single columns of Q (rows of R) differ
 * from the reference's in sign. Deterministic: no atomics; a second call gives
 * the same bits. Non-finite input returns normally with unspecified factors. */
int nd4hip_dgeqp3_batched_dev     (nd4hip_handle* h, int64_t batch, int64_t M, int64_t N, const double* A, double* Q, double* R, int32_t* P);
int nd4hip_dgeqp3_batched         (nd4hip_handle* h, int64_t batch, int64_t M, int64_t N, const double* A, double* Q, double* R, int32_t* P);
int nd4hip_dgeqp3_full_batched_dev(nd4hip_handle* h, int64_t batch, int64_t M, int64_t N, const double* A, double* Q, double* R, int32_t* P);
int nd4hip_dgeqp3_full_batched    (nd4hip_handle* h, int64_t batch, int64_t M, int64_t N, const double* A, double* Q, double* R, int32_t* P);

/* ---- rrqr_rank: replaces src/la/rrqr.js:398-414 (_rrqr_rank :57-85) -----------------------------------------------------
 * rank [batch] int32 of R [batch,M,N]: tmp[i] = ||R[i:L, j >= row]|| (the upper-triangle entries of rows i.. L-1), T = 2 eps
 * max(M,N) tmp[0], rank = the number of leading tmp[i] > T. A non-finite tmp[i] gives rank -1 in the _dev form; the host form
 * returns ND4HIP_ERR_ARG with 'Infinity or NaN encountered during rank estimation.' */
int nd4hip_dqp3rank_batched_dev(nd4hip_handle* h, int64_t batch, int64_t M, int64_t N, const double* R, int32_t* rank);
int nd4hip_dqp3rank_batched    (nd4hip_handle* h, int64_t batch, int64_t M, int64_t N, const double* R, int32_t* rank);

/* ---- rrqr_lstsq: replaces src/la/rrqr.js:447-580 -------------------------------------------------------------------------
 * X [batch,I,J] with z[0:r] = R[0:r,0:r]^-1 (Q^T Y)[0:r], z[r:] = 0, X[P[i],:] = z[i,:], r = the rank of R as dqp3rank (each
 * matrix's own, computed on the device); Q [batch,N,M], R [batch,M,I], P [batch,I], Y [batch,N,J]; strides in elements, 0 =
 * broadcast. rank [batch] receives r (-1: non-finite) and may be NULL. The _dev form makes no device-to-host copy; the host form
 * refuses a P that is not a permutation ('rrqr_lstsq(Q,R,P,y): Invalid indices in P.') and a non-finite rank estimate (the
 * rrqr_rank message), both ND4HIP_ERR_ARG. rrqr_solve (:417-444) is this plus the host's check rank == N. */
int nd4hip_dqp3ls_batched_dev(nd4hip_handle* h, int64_t batch, int64_t N, int64_t M, int64_t I, int64_t J,
                              const double* Q, int64_t strideQ, const double* R, int64_t strideR, const int32_t* P, int64_t strideP,
                              const double* Y, int64_t strideY, double* X, int32_t* rank);
int nd4hip_dqp3ls_batched    (nd4hip_handle* h, int64_t batch, int64_t N, int64_t M, int64_t I, int64_t J,
                              const double* Q, int64_t strideQ, const double* R, int64_t strideR, const int32_t* P, int64_t strideP,
                              const double* Y, int64_t strideY, double* X, int32_t* rank);

/* ---- srrqr_decomp_full: replaces src/la/srrqr.js:58-802 (Gu-Eisenstat strong rank-revealing QR) ---------------------------
 * A [batch,M,N] -> Q [batch,M,M], R [batch,M,N], P [batch,N] int32 with A[:, P] = Q R, rank [batch] int32. P and the rank are
 * decided as the reference decides them: A is scaled by ||A||_F (a zero matrix by 1), the rank is found by a binary search over
 * k, and at each checkpoint the column swap with the first maximum F_ij = hypot((A_k^-1 B_k)_ij, ||row i of A_k^-1|| ||column
 * j of C_k||) (row-major order) is made while F > dtol, with the reference's cyclic shift, so P matches it position for
 * position. dtol >= 1 (the reference's default is 1.01); ztol < 0 selects the default sqrt(eps) ||A/||A||_F||_F max(M,N),
 * ztol >= 0 is used as given, in units of ||A||_F. Q and R are those of dgeqrf_full on A[:, P]: R[:r, :] and Q[:, :r] equal
 * the reference's up to the sign of each row of R (column of Q), R[r:, r:] is triangular (the reference leaves that block
 * untriangularised; its norm is <= ztol ||A||_F either way) and the columns r.. of Q are an orthonormal completion.
 * The _dev form leaves rank -1 / -3 for an ||A||_F that is Infinity / NaN and -2 for a matrix that hit the static swap cap; the
 * host form returns ND4HIP_ERR_ARG with the reference's 'Assertion failed: Infinity' / 'Assertion failed: NaN', resp.
 * ND4HIP_ERR_NOCONV. dtol < 1, NaN or Infinity and ztol NaN or Infinity are ND4HIP_ERR_ARG with the reference's messages.
 * One workgroup per matrix decides (csrc/srrqr.hip); nothing waits on another workgroup. Deterministic: a second call gives
 * the same bits. */
int nd4hip_dsrrqr_batched_dev(nd4hip_handle* h, int64_t batch, int64_t M, int64_t N, const double* A, double dtol, double ztol,
                              double* Q, double* R, int32_t* P, int32_t* rank);
int nd4hip_dsrrqr_batched    (nd4hip_handle* h, int64_t batch, int64_t M, int64_t N, const double* A, double dtol, double ztol,
                              double* Q, double* R, int32_t* P, int32_t* rank);

/* ---- urv_decomp_full / urv_lstsq: replace src/la/urv.js:100-135 / :138-323 (complete orthogonal decomposition) ------------
 * durv: A [batch,M,N] -> U [batch,M,M] (srrqr's Q), R [batch,M,N] = [[T,0],[0,0]] with T [r,r] upper triangular and exact zeros
 * elsewhere, V [batch,N,N] orthogonal, rank [batch] (srrqr's r, default tolerances), A = U R V. T and V[:r] equal the reference's
 * up to signs (a sign per row of T's rows / V's rows and per column of T); V[r:] is an orthonormal completion; r == N gives the
 * reference's permutation V[i, P[i]] = 1 exactly. The r x N trapezoid is reduced from the right by the full QR of its reversed
 * transpose (csrc/srrqr.hip: urv_pack / urv_unpack). Error markers and codes as dsrrqr (the host form: 'Assertion failed: Infinity' / 'NaN').
 * durvls: U [I,J], R [J,K], V [K,L], rank, Y [I,Jc] -> X [batch,L,Jc] = V[:r]^T T^-1 (U^T Y)[:r] with T = R[:r,:r] and r each
 * matrix's own rank (clamped to [0, min(J,K)]): the minimum-norm least-squares solution. Strides in elements, 0 = broadcast
 * (strideRank 0 or 1). J <= I and K <= L are required ('Assertion failed.', urv.js:263-264). The _dev form makes no
 * device-to-host copy. */
int nd4hip_durv_batched_dev(nd4hip_handle* h, int64_t batch, int64_t M, int64_t N, const double* A, double* U, double* R, double* V,
                            int32_t* rank);
int nd4hip_durv_batched    (nd4hip_handle* h, int64_t batch, int64_t M, int64_t N, const double* A, double* U, double* R, double* V,
                            int32_t* rank);
int nd4hip_durvls_batched_dev(nd4hip_handle* h, int64_t batch, int64_t I, int64_t J, int64_t K, int64_t L, int64_t Jc,
                              const double* U, int64_t strideU, const double* R, int64_t strideR, const double* V, int64_t strideV,
                              const int32_t* rank, int64_t strideRank, const double* Y, int64_t strideY, double* X);
int nd4hip_durvls_batched    (nd4hip_handle* h, int64_t batch, int64_t I, int64_t J, int64_t K, int64_t L, int64_t Jc,
                              const double* U, int64_t strideU, const double* R, int64_t strideR, const double* V, int64_t strideV,
                              const int32_t* rank, int64_t strideRank, const double* Y, int64_t strideY, double* X);

/* ---- det / slogdet / det_tri / slogdet_tri / norm: replace src/la/det.js:24-106 and src/la/norm.js:22-85 ---------------------
 * ddet: A [batch,M,N] -> det [batch]; dslogdet: -> sign [batch], logdet [batch]. The reference's det is det_tri(qr_decomp(A)[1]):
 * square N <= 64 runs qr_decomp_full's Givens elimination in its own operation order (blocked J, I, i, j with B = 8, its skips,
 * no contraction), so the result is the reference's bit for bit; N > 64 and every tall input (M > N) run qr_decomp's R without Q
 * (nd4_geqrf_q_ex's R-only mode; a tall input gives prod(diag(R)) of its N x N R with the c >= 0 signs, as the reference does).
 * M < N is ND4HIP_ERR_ARG with the reference's 'det_tri(a): a must be square matrices.' ('det_tri(A): A must be square
 * matrices.' for slogdet), raised before any device work. Where the reference's Givens rotation asserts (a NaN or Infinity
 * reached a rotation: 'Assertion failed: NaN'), the _dev form writes a NaN with the bits ND4HIP_DET_ASSERT_NAN_BITS into det
 * (sign and logdet) and the host form returns ND4HIP_ERR_ARG with that message. The environment variable ND4HIP_DET_FORCE_QR=1
 * (read per call) sends square N <= 64 through the R-only QR path too, to compare the two paths. The R-only path factors with
 * the row-split panels: an in-kernel exchange that times out is ND4HIP_ERR_XCHG (the host form returns it; after the _dev form
 * the next synchronising entry point does), never a determinant.
 * ddettri / dslogdettri: A [batch,N,N] -> the product of the diagonal in index order (bit for bit det_tri) / sign = the product of
 * Math.sign(a_ii) (signed zeros and NaN kept) and logdet = the sum of log|a_ii| in index order. Only the diagonal is read.
 * dnrmfro: the Frobenius norm of n elements (norm(A), ord 'fro', no axis), one double into *out (a host pointer for the host form,
 * a device pointer for _dev); n = 0 gives 0; any Infinity gives +Infinity, otherwise any NaN gives NaN; deterministic bits. */
#define ND4HIP_DET_ASSERT_NAN_BITS 0x7ff80000de7a5e27ull
int nd4hip_ddet_batched_dev(nd4hip_handle* h, int64_t batch, int64_t M, int64_t N, const double* A, double* det);
int nd4hip_ddet_batched    (nd4hip_handle* h, int64_t batch, int64_t M, int64_t N, const double* A, double* det);
int nd4hip_dslogdet_batched_dev(nd4hip_handle* h, int64_t batch, int64_t M, int64_t N, const double* A, double* sign, double* logdet);
int nd4hip_dslogdet_batched    (nd4hip_handle* h, int64_t batch, int64_t M, int64_t N, const double* A, double* sign, double* logdet);
int nd4hip_ddettri_batched_dev(nd4hip_handle* h, int64_t batch, int64_t N, const double* A, double* det);
int nd4hip_ddettri_batched    (nd4hip_handle* h, int64_t batch, int64_t N, const double* A, double* det);
int nd4hip_dslogdettri_batched_dev(nd4hip_handle* h, int64_t batch, int64_t N, const double* A, double* sign, double* logdet);
int nd4hip_dslogdettri_batched    (nd4hip_handle* h, int64_t batch, int64_t N, const double* A, double* sign, double* logdet);
int nd4hip_dnrmfro_dev(nd4hip_handle* h, int64_t n, const double* A, double* out);
int nd4hip_dnrmfro    (nd4hip_handle* h, int64_t n, const double* A, double* out);

/* ---- schur_eigenvals / schur_eigen / eigen_balance_pre / eigen_balance_post: replace src/la/schur.js:31-370 and
 * src/la/eigen.js:91-270 (the direct parts of the nonsymmetric eigenproblem; schur_decomp's Francis iteration follows below: dhseqr)
 * Complex values are interleaved (re, im) doubles, as in zgemm.
 * dtreval: T [batch,N,N] quasi-triangular -> Lam [batch,N] complex, the reference's block detection and 2x2 formula, bit for bit.
 * dtrevc: Q, T [batch,N,N] -> Lam [batch,N] complex and V = Q X [batch,N,N] complex, X the eigenvectors of T by the reference's
 * back-substitution (N <= 64: one lane per column in its operation order, no contraction; X has its bits) with unit columns, Q X as the
 * real GEMM on the N x 2N view of X.
 * dgebal: A [batch,N,N], p >= 1 or +Infinity -> D [batch,N] (powers of two), B = D^-1 A D [batch,N,N], the reference's
 * Gauss-Seidel sweeps with block-reduced norms. zgebak: D [batch,N], V [batch,N,N] complex -> W = diag(D) V with unit columns.
 * Where the reference throws, a per-matrix flag word is raised on the device; both forms read it back (one small copy, the call
 * synchronises) and return ND4HIP_ERR_ARG with the reference's text for the first such matrix: ND4HIP_EV_FLAG_REAL2X2
 * 'schur_eigenvals(T): T must not contain real eigenvalued 2x2 blocks.' (from dtrevc too, schur.js:308), ND4HIP_EV_FLAG_ASSERT
 * 'Assertion failed.' (a NaN tolerance or a zero 2x2 determinant), ND4HIP_EV_FLAG_NAN 'NaN encountered.' (dgebal). One deviation: the reference's balancing sweeps have no bound; dgebal stops
 * after 1024 sweeps (every accepted step shrinks a norm by at least 5 %, so finite input ends long before) and then returns
 * ND4HIP_ERR_ARG 'nd4hip_dgebal_batched: no fixed point after 1024 sweeps.' (ND4HIP_EV_FLAG_SWEEPS), so that no input can hold
 * a device. dtrevc at N > 64 is the blocked tier (row blocks of 64, one GEMM per block; within rounding of the reference, not its
 * bits) and reads the block structure back once per call (it synchronises the stream). */
#define ND4HIP_EV_FLAG_REAL2X2 1
#define ND4HIP_EV_FLAG_ASSERT  2
#define ND4HIP_EV_FLAG_NAN     4
#define ND4HIP_EV_FLAG_SWEEPS  8
int nd4hip_dtreval_batched_dev(nd4hip_handle* h, int64_t batch, int64_t N, const double* T, double* Lam);
int nd4hip_dtreval_batched    (nd4hip_handle* h, int64_t batch, int64_t N, const double* T, double* Lam);
int nd4hip_dtrevc_batched_dev(nd4hip_handle* h, int64_t batch, int64_t N, const double* Q, const double* T, double* Lam, double* V);
int nd4hip_dtrevc_batched    (nd4hip_handle* h, int64_t batch, int64_t N, const double* Q, const double* T, double* Lam, double* V);
int nd4hip_dgebal_batched_dev(nd4hip_handle* h, int64_t batch, int64_t N, double p, const double* A, double* D, double* B);
int nd4hip_dgebal_batched    (nd4hip_handle* h, int64_t batch, int64_t N, double p, const double* A, double* D, double* B);
int nd4hip_zgebak_batched_dev(nd4hip_handle* h, int64_t batch, int64_t N, const double* D, const double* V, double* W);
int nd4hip_zgebak_batched    (nd4hip_handle* h, int64_t batch, int64_t N, const double* D, const double* V, double* W);

/* ---- schur_decomp / eigen / eigenvals: replace src/la/schur.js:372-683 and src/la/eigen.js:33-88 --------------------------
 * dhseqr: a Hessenberg decomposition (U, H) [batch,N,N] -> the real Schur decomposition (Q, T) of U H U^T by the reference's
 * Francis iteration schur_qrfrancis_inplace (implicit double shift, nested calls on deflated windows, the exceptional shift
 * drawn from AleaRNG('nd.la.schur_qrfrancis_inplace'), the final pass over real-eigenvalued 2x2 blocks), bit for bit: every
 * decision and every element is computed in the reference's operation order (csrc/schur.hip). One workgroup per matrix, no
 * exchange between workgroups; N <= 2048. Q may be U and T may be H. The _ex forms take the tier: ND4HIP_SCHUR_TIER_AUTO,
 * _LDS (H, Q^T and the nested q in LDS: N <= 65) or _GLOBAL (in global memory, any N); both give the same bits.
 * dgees: A -> (Q, T) = dhseqr(dgehrd(A)), schur_decomp. The device Hessenberg reduction is within rounding of the reference's,
 * not its bits, so neither is T.
 * dgeev: A -> Lam [batch,N] complex and, unless V is NULL, V [batch,N,N] complex: eigen(A) / eigenvals(A) = dgebal with p = 2,
 * dgees, dtrevc (dtreval if V is NULL), zgebak, all on the device. zgebak scales by the complex (D_i, 0) where eigen.js:59
 * scales by the real D_i: the same values up to the sign of a zero.
 * sweeps_out is a HOST pointer (may be NULL): the most sweeps any one francis_qr call took, over the batch. All forms
 * synchronise the stream (the flag words are read back). One deviation: the reference gives up after 1e9 stuck iterations per
 * eigenvalue, which is no bound on a shared device; here a francis_qr call on a window of size n stops after 30 max(10, n)
 * sweeps (LAPACK's dlahqr budget; the fixtures stay below a tenth of it), raises ND4HIP_EV_FLAG_NOCONV and the call returns
 * ND4HIP_ERR_NOCONV 'nd4hip_dhseqr_batched: no convergence after 30 max(10, n) sweeps of one francis_qr call.' */
#define ND4HIP_EV_FLAG_NOCONV 16
#define ND4HIP_SCHUR_TIER_AUTO   0
#define ND4HIP_SCHUR_TIER_LDS    1
#define ND4HIP_SCHUR_TIER_GLOBAL 2
int nd4hip_dhseqr_batched_dev(nd4hip_handle* h, int64_t batch, int64_t N, const double* U, const double* H, double* Q, double* T, int* sweeps_out);
int nd4hip_dhseqr_batched    (nd4hip_handle* h, int64_t batch, int64_t N, const double* U, const double* H, double* Q, double* T, int* sweeps_out);
int nd4hip_dhseqr_batched_ex_dev(nd4hip_handle* h, int64_t batch, int64_t N, const double* U, const double* H, double* Q, double* T, int* sweeps_out, int tier);
int nd4hip_dhseqr_batched_ex    (nd4hip_handle* h, int64_t batch, int64_t N, const double* U, const double* H, double* Q, double* T, int* sweeps_out, int tier);
int nd4hip_dgees_batched_dev(nd4hip_handle* h, int64_t batch, int64_t N, const double* A, double* Q, double* T, int* sweeps_out);
int nd4hip_dgees_batched    (nd4hip_handle* h, int64_t batch, int64_t N, const double* A, double* Q, double* T, int* sweeps_out);
int nd4hip_dgeev_batched_dev(nd4hip_handle* h, int64_t batch, int64_t N, const double* A, double* Lam, double* V);
int nd4hip_dgeev_batched    (nd4hip_handle* h, int64_t batch, int64_t N, const double* A, double* Lam, double* V);

/* ---- structure functions: transposition (NDArray.T on the last two axes), tril / triu (src/la/tri.js:23-42), diag / diag_mat
 * (src/la/diag.js:23-88), permute_rows / permute_cols / unpermute_rows / unpermute_cols (src/la/permute.js:23-306) ----------
 * Values are moved, never computed: every copied element keeps its 64 bits (NaN payloads, +-Infinity, -0, denormals), every
 * filled element is +0.0. No output may overlap an input (the reference always returns a fresh array): ND4HIP_ERR_ARG.
 * dtranspose: A [batch,M,N] -> B [batch,N,M], B[b,j,i] = A[b,i,j].
 * dtri: A [batch,M,N] -> B [batch,M,N]; upper == 0 is tril, B = (i < j-k) ? +0.0 : A; upper != 0 is triu, B = (i > j-k) ? +0.0 : A;
 * any int64 k.
 * ddiag: A [batch,M,N] -> d [batch,L], L = min(M, M+offset, N, N-offset), d[b,i] = A[b, i+max(0,-offset), i+max(0,offset)];
 * -M < offset < N, else ND4HIP_ERR_ARG.
 * ddiagmat: d [batch,N] -> D [batch,N,N], written completely (zeros included).
 * dpermute: A [batch,M,N], P [batch,L] int32 with L = M (cols == 0) or N (cols != 0) -> B [batch,M,N];
 *   cols == 0, inverse == 0  permute_rows    B[i,:] = A[P[i],:]        cols != 0, inverse == 0  permute_cols    B[:,j] = A[:,P[j]]
 *   cols == 0, inverse != 0  unpermute_rows  B[P[i],:] = A[i,:]        cols != 0, inverse != 0  unpermute_cols  B[:,P[j]] = A[:,j]
 * strideA / strideP in elements between consecutive batch members, 0 = the operand is broadcast over the batch. P need not be a
 * permutation: in the inverse forms the largest i with P[i] = k wins (the reference's later store) and rows / columns that no
 * i names are +0.0, deterministically (a gather through an inverse map built with integer atomicMax; no scattered stores). An
 * index outside [0, L) is never turned into an address: it raises a device flag, nothing is read or written for it, and the
 * call returns ND4HIP_ERR_ARG with the reference's text, e.g. 'permute_rows(A,P): P.contains invalid indices.'; B is then
 * unspecified and the handle stays usable. To decide that, BOTH forms of dpermute read the flag back: they synchronise the
 * stream. The other four _dev forms enqueue only. */
int nd4hip_dtranspose_batched_dev(nd4hip_handle* h, int64_t batch, int64_t M, int64_t N, const double* A, double* B);
int nd4hip_dtranspose_batched    (nd4hip_handle* h, int64_t batch, int64_t M, int64_t N, const double* A, double* B);
int nd4hip_dtri_batched_dev(nd4hip_handle* h, int upper, int64_t k, int64_t batch, int64_t M, int64_t N, const double* A, double* B);
int nd4hip_dtri_batched    (nd4hip_handle* h, int upper, int64_t k, int64_t batch, int64_t M, int64_t N, const double* A, double* B);
int nd4hip_ddiag_batched_dev(nd4hip_handle* h, int64_t batch, int64_t M, int64_t N, int64_t offset, const double* A, double* d);
int nd4hip_ddiag_batched    (nd4hip_handle* h, int64_t batch, int64_t M, int64_t N, int64_t offset, const double* A, double* d);
int nd4hip_ddiagmat_batched_dev(nd4hip_handle* h, int64_t batch, int64_t N, const double* d, double* D);
int nd4hip_ddiagmat_batched    (nd4hip_handle* h, int64_t batch, int64_t N, const double* d, double* D);
int nd4hip_dpermute_batched_dev(nd4hip_handle* h, int cols, int inverse, int64_t batch, int64_t M, int64_t N, const double* A,
                                int64_t strideA, const int32_t* P, int64_t strideP, double* B);
int nd4hip_dpermute_batched    (nd4hip_handle* h, int cols, int inverse, int64_t batch, int64_t M, int64_t N, const double* A,
                                int64_t strideA, const int32_t* P, int64_t strideP, double* B);

/* ---- strided N-d copy: NDArray.sliceElems / transpose(...axes) (src/nd_array.js:375-436, 531-642), concat (src/concat.js) and
 * stack (src/stack.js) on device arrays ----------
 * For every index vector i of the box shape[0..ndim):  dst[dst_off + sum_d i_d dst_strides[d]] = src[src_off + sum_d i_d src_strides[d]].
 * Elements are opaque words of elem_bytes = 4 or 8 bytes, moved as integers: every bit is kept. Offsets and strides are in
 * elements; strides are signed (a negative stride is a reversed slice) and may be 0 where the extent is 1. ndim = 0 copies one
 * element. complex128 is a box with one more innermost axis of two 8-byte words. src_len / dst_len are the element counts of
 * the two allocations: before any launch the lowest and the highest element that each side reaches are computed, and the call
 * returns ND4HIP_ERR_ARG if either leaves [0, len), if an extent is < 1, if ndim is not in 0..8, if elem_bytes is neither 4 nor 8, or
 * if the byte ranges reached on the two sides intersect (the reference always returns a fresh array, and the tiled path reads
 * what another workgroup may have written). Nothing is written then and the handle stays usable. The call enqueues on the
 * handle's stream and does not synchronise; there is no flag to read back. nd4hip_profile_last reports it as "gather_nd" with
 * 2 elem_bytes count bytes. The axes should come in the order of dst (dst_strides descending, innermost last) and reduced
 * (extent-1 axes dropped, mergeable neighbours merged): the kernels are chosen from the box as given.
 * There is no host-pointer form: a host array would cross PCIe twice only to be copied; slice it on the host. */
int nd4hip_gather_nd_dev(nd4hip_handle* h, int elem_bytes, int ndim, const int64_t* shape,
                         const void* src, int64_t src_len, int64_t src_off, const int64_t* src_strides,
                         void* dst, int64_t dst_len, int64_t dst_off, const int64_t* dst_strides);

/* ---- elementwise arithmetic and ordered axis reductions on float64 device arrays: nd.zip_elems (src/zip_elems.js),
 * NDArray.mapElems and NDArray.reduceElems (src/nd_array.js:353-360, 464-529) with one of nd.math's add, sub, mul, div, min, max,
 * neg, abs as the closure ----------
 * Each operator is one IEEE operation on float64: every non-NaN result has the reference's 64 bits, denormals included. A NaN
 * result is a NaN; which payload survives is not specified. min and max are Math.min and Math.max: a NaN operand gives NaN,
 * min(+0, -0) = -0, max(-0, +0) = +0. neg and abs flip and clear the sign bit.
 *
 * dzip_nd: for every index vector i of the box shape[0..ndim):  C[i] = op(A[a_off + sum_d i_d a_strides[d]], B[b_off + sum_d i_d
 * b_strides[d]]), C dense row-major with c_len elements. Offsets and strides are in elements; strides are >= 0 and 0 broadcasts
 * along an axis of any extent. A unary op takes B == NULL (b_len, b_off, b_strides are ignored then). ndim = 0 is one element.
 * The kernels are chosen from the box as given, so pass it reduced (extent-1 axes dropped, mergeable neighbours merged).
 *
 * dreduce_nd: A is a dense row-major array of `shape`; axis d is folded away where reduced[d] != 0. Per output element the first
 * element met is copied and the others are folded in as acc = op(x, acc), in row-major order of the reduced axes: the reference's
 * order, so sums and products have its bits. op is ADD, MUL, MIN or MAX (the operators for which op(x, acc) and op(acc, x) agree).
 * No reduced axis: a copy. C has one element per index of the kept axes (one element when every axis is reduced).
 *
 * Both enqueue on the handle's stream, do not synchronise and have no flag to read back. Both return ND4HIP_ERR_ARG, with nothing
 * written and the handle still usable, for: an unknown op or one of the wrong arity (B given with a unary op, B missing with a
 * binary one, a reducer outside the four), ndim outside 0..8, an extent < 1, a negative stride, an operand reaching outside
 * [0, len), c_len different from the result's element count, C overlapping in bytes what is read of A or B.
 * nd4hip_profile_last reports "zip_nd" / "reduce_nd" with 0 flops and the bytes read plus written: 8 (count + the distinct
 * elements read of A and of B: the product of the extents whose stride is not 0), and 8 (elements of A + elements of C).
 * There is no host-pointer form: a host array would cross PCIe twice for work the host does at memory speed. */
#define ND4HIP_EW_ADD 0
#define ND4HIP_EW_SUB 1
#define ND4HIP_EW_MUL 2
#define ND4HIP_EW_DIV 3
#define ND4HIP_EW_MIN 4
#define ND4HIP_EW_MAX 5
#define ND4HIP_EW_NEG 16
#define ND4HIP_EW_ABS 17
int nd4hip_dzip_nd_dev(nd4hip_handle* h, int op, int ndim, const int64_t* shape,
                       const double* A, int64_t a_len, int64_t a_off, const int64_t* a_strides,
                       const double* B, int64_t b_len, int64_t b_off, const int64_t* b_strides,
                       double* C, int64_t c_len);
int nd4hip_dreduce_nd_dev(nd4hip_handle* h, int op, int ndim, const int64_t* shape, const int32_t* reduced,
                          const double* A, int64_t a_len, double* C, int64_t c_len);

/* ---- svd_decomp: replaces the output contract of src/la/svd.js:25 (= svd_dc.js:883-932) ----------
 * A [batch,M,N] -> U [batch,M,L], sv [batch,L] (>= 0, descending), V [batch,L,N] (rows = right
 * singular vectors), L = min(M,N); one-sided Jacobi with the reference's Jacobi post-processing
 * contract (_svd_jac_utils.js:123-188). sweeps_out / offnorm_out are HOST pointers (may be NULL):
 * max sweeps over the batch and the largest remaining |a_p.a_q| / (|a_p||a_q|). Both forms
 * synchronise the stream (the sweep loop is host-driven). Each member is scaled by the exact power
 * of two 2^-e, e = frexp exponent of its max|a|, before the QR / Jacobi and sv by 2^e afterwards:
 * any finite scale works (no overflow or underflow of the sums of squares), and svd_decomp(2^k A)
 * gives bit for bit the U and V of svd_decomp(A) and sv times 2^k while the entries stay normal. */
int nd4hip_dgesvdj_batched_dev(nd4hip_handle* h, int64_t batch, int64_t M, int64_t N, const double* A,
                               double* U, double* sv, double* V, int* sweeps_out, double* offnorm_out);
int nd4hip_dgesvdj_batched    (nd4hip_handle* h, int64_t batch, int64_t M, int64_t N, const double* A,
                               double* U, double* sv, double* V, int* sweeps_out, double* offnorm_out);

/* ---- svd_decomp by divide & conquer: the reference's own algorithm, src/la/svd_dc.js:37-932 (csrc/svd_dc.hip) ------------
 * dgesdd: the contract of dgesvdj above, A [batch,M,N] -> U [batch,M,L], sv [batch,L] (>= 0, descending), V [batch,L,N], by the
 * reference's route: bidiagonalise (dgebrd), solve the bidiagonal problem by divide & conquer (dbdsdc), U = U_b U2,
 * V = V2[:K] V_b; M > N goes through the transpose (svd_dc.js:893-897). The same power-of-two scaling as dgesvdj makes any finite
 * scale work. An opt-in second algorithm: nothing routes to it by default. min(M, N) <= 2048.
 * dbdsdc: the solver alone, for an upper bidiagonal K x J matrix, J = K or K + 1 (the shapes dgebrd produces): d [batch,K] the
 * diagonal, e [batch,J-1] the super-diagonal -> U2 [batch,K,K], sv [batch,K] (>= 0, descending), V2 [batch,J,J] (rows = right
 * vectors), B = U2 diag(sv) V2[:K]. The reference's tree (split at n >> 1, closed-form leaves of 2 and 3 columns) and its stages
 * per merge (deflation, secular roots by bisection in the shifted variable, the Gu-Eisenstat z, the two W matrices), one launch
 * per stage and level; the merges' products run on the fp64 MFMA GEMM. Sums and products across lanes are ordered differently
 * from the reference's loops: results agree with it to rounding, not bit for bit. Members are independent: a member's result
 * does not depend on the rest of the batch. K <= 2048.
 * Where the reference throws 'Assertion failed.' (svd_dc.js:393 sLo > sHi, :405 / :429 a non-finite secular sum, :507 / :583 a W
 * row of norm 0, ...; non-finite input ends here or in NaN outputs) the device raises a per-call flag word with that line. All
 * four forms read it back once at the end (they synchronise) and return ND4HIP_ERR_NOCONV with nd4hip_last_error
 * 'svd_dc: Assertion failed. (svd_dc.js:<line>)'; the outputs are unspecified then and the handle stays usable. Every loop on the
 * device has a fixed bound (the bisection: 1200 steps, csrc/svd_dc.hip), so no input can hold the device.
 * dbdsdc_levels needs no device: the level list that replaces the recursion for a problem of n = K + 1 columns, as (level, off,
 * n) triples in launch order (level 0: the leaves; then the merges of each depth, the deepest first). Returns the number of
 * nodes; at most `capacity` triples are written. */
int nd4hip_dbdsdc_batched_dev(nd4hip_handle* h, int64_t batch, int64_t K, int64_t J, const double* d, const double* e,
                              double* U2, double* sv, double* V2);
int nd4hip_dbdsdc_batched    (nd4hip_handle* h, int64_t batch, int64_t K, int64_t J, const double* d, const double* e,
                              double* U2, double* sv, double* V2);
int nd4hip_dgesdd_batched_dev(nd4hip_handle* h, int64_t batch, int64_t M, int64_t N, const double* A, double* U, double* sv, double* V);
int nd4hip_dgesdd_batched    (nd4hip_handle* h, int64_t batch, int64_t M, int64_t N, const double* A, double* U, double* sv, double* V);
int nd4hip_dbdsdc_levels(int64_t n, int32_t* nodes, int64_t capacity);
/* HIP-event time per stage of the LAST dgesdd / dbdsdc call made on this handle while nd4hip_profile_enable was on (all zero
 * otherwise), in ms, summed over the levels: bidiagonalisation (with the scaling and the transposes), leaves, preparation and
 * deflation, secular roots, z recomputation and inner order, the two W matrices, the merges' products, the final two products.
 * Writes min(capacity, ND4HIP_DC_STAGES) values; returns ND4HIP_DC_STAGES. */
#define ND4HIP_DC_STAGES 8
int nd4hip_dgesdd_last_stages(nd4hip_handle* h, double* ms, int capacity);

/* ---- selected singular triplets: svd_decomp(A, subset), svd_vals(A), bidiag_svd(d, e, subset), bidiag_svdvals (csrc/bdsvdx.hip,
 * DESIGN.md 4.23). As with the selected eigenpairs below, the host-pointer forms end in _host, not in the bare name.
 * B is the upper bidiagonal K x J matrix of dbdsdc (d [batch,K], e [batch,J-1], J = K or K + 1), 1 <= K <= 2048. The subset
 * (i0, i1), 0 <= i0 <= i1 <= K, selects sv[i0:i1] of the DESCENDING singular values, k = i1 - i0. K = 0, an empty batch and an empty
 * subset have nothing to do and write nothing.
 *   dbdsvdx: sv [batch,k] by bisection on the Sturm count of the Golub-Kahan matrix of B, the symmetric tridiagonal of order K + J
 *            with a zero diagonal and the off-diagonals d0, e0, d1, e1, ...: the arithmetic of dstevx below with d = 0 (the same
 *            scale, interval, stopping rule and 128-step cap), then max(value, +0). U2 [batch,K,k] (columns = left vectors) and
 *            V2 [batch,k,J] (rows = right vectors), both or neither (NULL, NULL: the values alone, the same bits): three rounds of
 *            dstevx's inverse iteration and Gram-Schmidt on the eigenvector (v0, u0, v1, u1, ...), then u and v are normalised
 *            each on its own. A member goes to the full solver instead (dbdsdc on that member alone, columns i0 .. i1 - 1 of its
 *            U2 and rows i0 .. i1 - 1 of its V2, bit for bit; sv stays the bisection's) when B = 0, when two or more of its
 *            selected scaled values lie below 1e-3 g / 2 (g the Gershgorin bound of the scaled member), or when
 *            min(|u|^2, |v|^2) < 1/8 for one of its vectors. fallback [batch] (int32, may be NULL) receives those flags.
 *            NaN or Inf in d or e: ND4HIP_ERR_NOCONV, 'bidiag_svd(d,e): d or e contains NaN or Infinity.'; dbdsdc's errors pass through.
 *   dgesvdx: A [batch,M,N] -> U [batch,M,k], sv [batch,k], V [batch,k,N] (U = V = NULL: the values alone, the same bits, no product):
 *            the scaling and dgebrd of dgesdd (M > N through the transpose), dbdsvdx, U = U_b U2 and V = V2 V_b on the k selected
 *            columns and rows. min(M, N) <= 2048. NaN or Inf in A: ND4HIP_ERR_NOCONV, 'svd_decomp(A): A contains NaN or Infinity.'
 * Bounds: 1e-12 norm-wise (values, both residuals, orthogonality of U and V). A member's results do not depend on the batch or on
 * the run. All forms synchronise (the flags are read back once per chunk). Profile ops "dbdsvdx_batched", "dgesvdx_batched". */
int nd4hip_dbdsvdx_batched_dev (nd4hip_handle* h, int64_t batch, int64_t K, int64_t J, int64_t i0, int64_t i1, const double* d, const double* e,
                                double* U2, double* sv, double* V2, int32_t* fallback);
int nd4hip_dbdsvdx_batched_host(nd4hip_handle* h, int64_t batch, int64_t K, int64_t J, int64_t i0, int64_t i1, const double* d, const double* e,
                                double* U2, double* sv, double* V2, int32_t* fallback);
int nd4hip_dgesvdx_batched_dev (nd4hip_handle* h, int64_t batch, int64_t M, int64_t N, int64_t i0, int64_t i1, const double* A, double* U,
                                double* sv, double* V, int32_t* fallback);
int nd4hip_dgesvdx_batched_host(nd4hip_handle* h, int64_t batch, int64_t M, int64_t N, int64_t i0, int64_t i1, const double* A, double* U,
                                double* sv, double* V, int32_t* fallback);
/* HIP-event time per stage of the LAST dgesvdx / dbdsvdx call (one chunk) made on this handle while nd4hip_profile_enable was on,
 * in ms: bidiagonalisation with the scaling and the transposes (0 for dbdsvdx), bisection, inverse iteration and split, the full
 * solver on the flagged members (the read-back included), the two products (0 for dbdsvdx). */
#define ND4HIP_SVDX_STAGES 5
int nd4hip_dgesvdx_last_stages(nd4hip_handle* h, double* ms, int capacity);

/* ---- eigen_sym / eigenvals_sym: the symmetric eigenproblem (planned by the reference, src/la/eigen.js:28-30; csrc/syev.hip) ----
 * S [batch,N,N] symmetric, read ONLY in its lower triangle (j <= i; the upper triangle may hold anything, NaN included) and never
 * written -> lambda [batch,N] descending and V [batch,N,N] with the eigenvectors as columns: S V = V diag(lambda), V^T V = I.
 * V = NULL: the values alone (the same bits as with V). Route: the mirrored lower triangle, scaled by an exact power of two, is
 * tridiagonalised by dgehrd; T is shifted by c = g (1 + 2^-20), g its Gershgorin bound, into a positive definite matrix whose
 * bidiagonal Cholesky factor B goes to dbdsdc; lambda = sv^2 - c, V = U V2^T. The error of every eigenvalue is a few
 * eps ||S||_F in absolute terms: small eigenvalues of a graded matrix are accurate relative to ||S||, not to themselves
 * (for N <= 128 nd4hip_dsyevj_batched below delivers them to their own relative accuracy).
 * N = 0 and N = 1 need no solver; N > 2048 (the solver's limit) is ND4HIP_ERR_ARG before anything is written. NaN or Inf in
 * the lower triangle: ND4HIP_ERR_NOCONV with 'eigen_sym(S): S contains NaN or Infinity in its lower triangle.' (one flag word
 * per call, read back at the end; the outputs are unspecified then, the solver ran on finite stand-in data, the handle stays
 * usable). Members are independent of the rest of the batch. Both forms synchronise. */
int nd4hip_dsyevd_batched_dev(nd4hip_handle* h, int64_t batch, int64_t N, const double* S, double* lambda, double* V);
int nd4hip_dsyevd_batched    (nd4hip_handle* h, int64_t batch, int64_t N, const double* S, double* lambda, double* V);
/* HIP-event time per stage of the LAST dsyevd call (one chunk of <= 32768 members) made on this handle while
 * nd4hip_profile_enable was on (all zero otherwise), in ms: symmetrise and scale, tridiagonal reduction, shift and Cholesky,
 * bidiagonal solver, values and the vectors' GEMM. Writes min(capacity, ND4HIP_SYEV_STAGES) values; returns ND4HIP_SYEV_STAGES. */
#define ND4HIP_SYEV_STAGES 5
int nd4hip_dsyevd_last_stages(nd4hip_handle* h, double* ms, int capacity);

/* ---- eigen_sym / eigenvals_sym, algo = 'jacobi': cyclic two-sided Jacobi for stacks of small matrices (csrc/syevj.hip) ----
 * The same contract as dsyevd (lower triangle read only, S never written, lambda descending, eigenvectors as the columns of V,
 * V = NULL: the values alone with the same bits and no V accumulated), for 1 <= N <= 128 (N = 0: nothing to do; N > 128 is
 * ND4HIP_ERR_ARG before anything is written). Every member is solved inside one launch: N <= 32 one wave per member, N <= 64 one
 * workgroup with S and V^T in LDS, N <= 128 one workgroup with S in LDS and V^T in global memory. A sweep is the round-robin
 * tournament over all pairs; pair (p, q) is rotated iff s_pq != 0 and |s_pq| > eps sqrt|s_pp| sqrt|s_qq|, eps = 2^-52; a member
 * is finished after a sweep that rotates nothing. sweeps [batch] (may be NULL) receives the sweeps of each member, that last
 * one included; a member that needs more than 60: ND4HIP_ERR_NOCONV, 'eigen_sym(S, algo='jacobi'): no convergence after 60
 * sweeps.' NaN or Inf in a lower triangle: ND4HIP_ERR_NOCONV with dsyevd's message; that member's outputs are not written.
 * Accuracy: the bounds of dsyevd, and, for symmetric positive definite S with A = D^-1 S D^-1, D = diag(sqrt s_ii):
 *   |lambda^ - lambda| <= N eps kappa_2(A) lambda   for EVERY eigenvalue,
 * however small it is against ||S|| (the default route's errors are relative to ||S||). Members are scaled by an exact power
 * of two: 2^k S gives bit-identical V and lambda 2^k while entries stay normal. A member's results do not depend on the batch.
 * All arithmetic is rounded operation by operation (no FMA contraction, no reductions). Both forms synchronise. */
int nd4hip_dsyevj_batched_dev(nd4hip_handle* h, int64_t batch, int64_t N, const double* S, double* lambda, double* V, int32_t* sweeps);
int nd4hip_dsyevj_batched    (nd4hip_handle* h, int64_t batch, int64_t N, const double* S, double* lambda, double* V, int32_t* sweeps);

/* ---- selected eigenpairs: eigen_sym(S, subset), tridiag_eigen(d, e, subset), tridiag_count(d, e, x) (csrc/syevx.hip) ----
 * The host-pointer forms of these three end in _host (not the bare name of every other pair): on purpose, see DESIGN.md 4.20.
 * T = tridiag(d [batch,N], e [batch,N-1]) symmetric tridiagonal; the subset (i0, i1), 0 <= i0 <= i1 <= N, selects lambda[i0:i1] of
 * the DESCENDING spectrum, k = i1 - i0 values. 1 <= N <= 2048 (d and e^2 of a member are staged in LDS); N = 0, an empty batch
 * and an empty subset have nothing to do and write nothing. Each member is scaled by the exact power of two that puts
 * max(|d|, |e|) in [0.5, 1): 2^m T gives 2^m lambda, the same counts and bit-identical vectors while entries stay normal.
 *   dstcnt: count [batch,M] (int32) = the number of eigenvalues of T greater than x [batch,M]: N minus the negative terms of the
 *           Sturm sequence q_0 = d_0 - x, q_i = (d_i - x) - e_i-1^2 / q_i-1, |q| < 2^-1022 replaced by -2^-1022. A probe exactly on
 *           an eigenvalue of a diagonal T does not count that eigenvalue. Enqueues only (the _dev form); members with NaN or Inf in
 *           d or e are counted as the identity. NaN in x is the caller's to refuse.
 *   dstevx: lambda [batch,k] by bisection on that count from the Gershgorin interval until hi - lo <= 2 eps max(|lo|,|hi|) + eps g
 *           (g the Gershgorin bound), at most 128 halvings: absolute error a few eps g per value. Z [batch,k,N] (may be NULL: the
 *           values alone, the same bits): row j is the unit eigenvector of lambda[j], by three rounds of inverse iteration with
 *           the start vector u(seed, (i0 + j) N + i) and Gram-Schmidt applied twice inside clusters (gaps <= 1e-3 g); its first
 *           component of largest magnitude is positive. A diagonal member: its d by descending rank, ties by index, and the unit
 *           vectors. NaN or Inf in d or e: ND4HIP_ERR_NOCONV, 'tridiag_eigen(d,e): d or e contains NaN or Infinity.'
 *   dsyevx: the same for the lower triangle of S [batch,N,N] (the contract of dsyevd: upper triangle never read, S never written):
 *           steps 1-2 of dsyevd, dstevx on diag(H), subdiag(H), V [batch,N,k] = U Z^T with the eigenvectors as columns (V = NULL:
 *           values alone, the same bits, no inverse iteration). NaN or Inf in the lower triangle: ND4HIP_ERR_NOCONV with dsyevd's
 *           message. A diagonal S returns lambda[i0:i1] and V[:, i0:i1] of dsyevd bit for bit.
 * Bounds as dsyevd's (1e-12 norm-wise); vectors whose eigenvalues are just more than 1e-3 g apart are orthogonal to about
 * eps / 1e-3 only. A member's results do not depend on the batch or on the run. dstevx and dsyevx synchronise (one flag word is
 * read back). Profile ops "dstcnt_batched", "dstevx_batched", "dsyevx_batched" (10/3 N^3 + 2 N^2 k flops with V). */
int nd4hip_dstcnt_batched_dev (nd4hip_handle* h, int64_t batch, int64_t N, int64_t M, const double* d, const double* e, const double* x,
                               int32_t* count);
int nd4hip_dstcnt_batched_host(nd4hip_handle* h, int64_t batch, int64_t N, int64_t M, const double* d, const double* e, const double* x,
                               int32_t* count);
int nd4hip_dstevx_batched_dev (nd4hip_handle* h, int64_t batch, int64_t N, int64_t i0, int64_t i1, const double* d, const double* e,
                               double* lambda, double* Z);
int nd4hip_dstevx_batched_host(nd4hip_handle* h, int64_t batch, int64_t N, int64_t i0, int64_t i1, const double* d, const double* e,
                               double* lambda, double* Z);
int nd4hip_dsyevx_batched_dev (nd4hip_handle* h, int64_t batch, int64_t N, int64_t i0, int64_t i1, const double* S, double* lambda, double* V);
int nd4hip_dsyevx_batched_host(nd4hip_handle* h, int64_t batch, int64_t N, int64_t i0, int64_t i1, const double* S, double* lambda, double* V);
/* HIP-event time per stage of the LAST dsyevx / dstevx call (one chunk) made on this handle while nd4hip_profile_enable was on, in
 * ms: symmetrise and scale, tridiagonal reduction (both 0 for dstevx), bisection, inverse iteration, the vectors' GEMM. */
#define ND4HIP_SYEVX_STAGES 5
int nd4hip_dsyevx_last_stages(nd4hip_handle* h, double* ms, int capacity);

/* ---- tridiag_factor / tridiag_apply_q / tridiag_decomp and eigen_sym(S, reduction='tridiag') (csrc/sytrd.hip) ----
 * As with the selected eigenpairs above, the host-pointer forms of these four end in _host, not in the bare name.
 * S [batch,N,N] symmetric, read only in its lower triangle and never written; 1 <= N <= 2048; N = 0 and an empty batch have nothing
 * to do and write nothing.
 *   dsytrd: S = Q tridiag(d, e) Q^T, Q = H_0 H_1 ... H_{N-3}, H_k = I - tau_k v_k v_k^T with v_k zero in rows 0..k, 1 in row k+1 and its
 *           tail in F[k+2:, k] (LAPACK's dsytrd, lower, on row-major members). F [batch,N,N] carries d on its diagonal, e on its first
 *           subdiagonal and zeros above the diagonal; tau [batch,N-1] with tau[N-2] = 0; d [batch,N]; e [batch,N-1] (tau and e may be
 *           NULL for N = 1). e_k = -sign(alpha) |x| for the column x = [alpha; tail] (sign(0) = +1); a column whose tail is zero gets
 *           tau_k = 0, e_k = alpha. Each member is scaled by the exact power of two that puts max|s_ij| in [0.5, 1): 2^m S gives the
 *           same tails, tau and Q bit for bit and 2^m d, 2^m e. NaN or Inf in a lower triangle: ND4HIP_ERR_NOCONV,
 *           'tridiag_decomp(S): S contains NaN or Infinity in its lower triangle.'; the outputs are then unspecified.
 *   dormtr: Z [batch,N,K] <- Q Z (transpose = 1: Q^T Z) in place; Q is never formed. Enqueues only (the _dev form).
 *   dsyevd_tr, dsyevx_tr: dsyevd and dsyevx (their argument lists, contracts, bounds and error text) with dsytrd in place of the
 *           symmetrised copy and the Hessenberg reduction and dormtr in place of the product with U; V = NULL runs neither Q nor dormtr.
 * No sum depends on the run, the batch or a member's position, up to the GEMM's choice of a split inner dimension for N > 512 in
 * dormtr. dsytrd and the two eigen routes synchronise (one flag word). Profile ops "dsytrd_batched" (4/3 N^3), "dormtr_batched"
 * (2 N^2 K), "dsyevd_tr_batched", "dsyevx_tr_batched"; the stage times of the last two are read with nd4hip_dsyevd_last_stages and
 * nd4hip_dsyevx_last_stages (the symmetrise stage is 0). */
int nd4hip_dsytrd_batched_dev (nd4hip_handle* h, int64_t batch, int64_t N, const double* S, double* F, double* tau, double* d, double* e);
int nd4hip_dsytrd_batched_host(nd4hip_handle* h, int64_t batch, int64_t N, const double* S, double* F, double* tau, double* d, double* e);
int nd4hip_dormtr_batched_dev (nd4hip_handle* h, int64_t batch, int64_t N, int64_t K, int transpose, const double* F, const double* tau,
                               double* Z);
int nd4hip_dormtr_batched_host(nd4hip_handle* h, int64_t batch, int64_t N, int64_t K, int transpose, const double* F, const double* tau,
                               double* Z);
int nd4hip_dsyevd_tr_batched_dev (nd4hip_handle* h, int64_t batch, int64_t N, const double* S, double* lambda, double* V);
int nd4hip_dsyevd_tr_batched_host(nd4hip_handle* h, int64_t batch, int64_t N, const double* S, double* lambda, double* V);
int nd4hip_dsyevx_tr_batched_dev (nd4hip_handle* h, int64_t batch, int64_t N, int64_t i0, int64_t i1, const double* S, double* lambda, double* V);
int nd4hip_dsyevx_tr_batched_host(nd4hip_handle* h, int64_t batch, int64_t N, int64_t i0, int64_t i1, const double* S, double* lambda, double* V);

/* ---- herm_tridiag_factor / herm_tridiag_apply_q / herm_tridiag_decomp, eigen_herm and eigenvals_herm (csrc/hetrd.hip) ----
 * The Hermitian counterparts of the four above; the host-pointer forms end in _host. H, F, tau, Z and V are complex128 as interleaved
 * (re, im) doubles; d, e and lambda are real. H [batch,N,N] Hermitian, read only where i >= j, the imaginary part of its diagonal
 * ignored, never written; 1 <= N <= 2048; N = 0 and an empty batch have nothing to do and write nothing.
 *   zhetrd: H = Q tridiag(d, e) Q^H with d and e REAL, Q = H_0 H_1 ... H_{N-2}, H_k = I - tau_k v_k v_k^H with v_k zero in rows 0..k, 1
 *           in row k+1 and its tail in F[k+2:, k] (LAPACK's zhetrd, lower, on row-major members): N - 1 reflectors, the last with an
 *           empty tail. F [batch,N,N] carries d on its diagonal and e on its first subdiagonal, both with zero imaginary part, and zeros
 *           above the diagonal; tau [batch,N-1] complex; d [batch,N]; e [batch,N-1] (tau and e may be NULL for N = 1). For the column
 *           x = [alpha; tail]: tail = 0 and Im alpha = 0 give tau_k = 0, e_k = Re alpha; else e_k = beta = -sign(Re alpha) |x|
 *           (sign(0) = +1), tau_k = ((beta - Re alpha) / beta, -Im alpha / beta), tail / (alpha - beta). Each member is scaled by the
 *           exact power of two that puts max(|Re h_ij|, |Im h_ij|) in [0.5, 1): 2^m H gives the same tails, tau and Q bit for bit and
 *           2^m d, 2^m e. NaN or Inf in what is read: ND4HIP_ERR_NOCONV, 'herm_tridiag_decomp(H): H contains NaN or Infinity in its
 *           lower triangle.'; the outputs are then unspecified, the handle stays usable.
 *   zunmtr: Z [batch,N,K] complex <- Q Z (adjoint = 1: Q^H Z) in place; Q is never formed. Enqueues only (the _dev form).
 *   zheevd: lambda [batch,N] real, descending; V [batch,N,N] complex, the eigenvectors as columns, H V = V diag(lambda), V^H V = I, or
 *           V = NULL for the values alone (neither Q nor zunmtr runs): zhetrd, then dsyevd_tr's real solver on (d, e), then zunmtr. The
 *           phase of a vector is what the route produces: deterministic, not normalised. N = 1: lambda = Re h_00, V = 1 (NaN or Inf in h_00 is refused there too).
 *   zheevx: the same for the subset i0 <= i < i1 of the descending spectrum (dstevx on (d, e)): lambda [batch,k], V [batch,N,k].
 *           NaN or Inf: 'eigen_herm(H): H contains NaN or Infinity in its lower triangle.'.
 * No sum depends on the run, the batch or a member's position. zhetrd and the two eigen routes synchronise. Profile ops
 * "zhetrd_batched" (16/3 N^3 real flops), "zunmtr_batched" (8 N^2 K), "zheevd_batched", "zheevx_batched"; the stage times of the last
 * two are read with nd4hip_dsyevd_last_stages and nd4hip_dsyevx_last_stages (the symmetrise stage is 0; zheevx reports the reduction
 * and the solver's stages, not its zunmtr). */
int nd4hip_zhetrd_batched_dev (nd4hip_handle* h, int64_t batch, int64_t N, const double* H, double* F, double* tau, double* d, double* e);
int nd4hip_zhetrd_batched_host(nd4hip_handle* h, int64_t batch, int64_t N, const double* H, double* F, double* tau, double* d, double* e);
int nd4hip_zunmtr_batched_dev (nd4hip_handle* h, int64_t batch, int64_t N, int64_t K, int adjoint, const double* F, const double* tau,
                               double* Z);
int nd4hip_zunmtr_batched_host(nd4hip_handle* h, int64_t batch, int64_t N, int64_t K, int adjoint, const double* F, const double* tau,
                               double* Z);
int nd4hip_zheevd_batched_dev (nd4hip_handle* h, int64_t batch, int64_t N, const double* H, double* lambda, double* V);
int nd4hip_zheevd_batched_host(nd4hip_handle* h, int64_t batch, int64_t N, const double* H, double* lambda, double* V);
int nd4hip_zheevx_batched_dev (nd4hip_handle* h, int64_t batch, int64_t N, int64_t i0, int64_t i1, const double* H, double* lambda, double* V);
int nd4hip_zheevx_batched_host(nd4hip_handle* h, int64_t batch, int64_t N, int64_t i0, int64_t i1, const double* H, double* lambda, double* V);

/* ---- herm_cholesky_decomp / herm_cholesky_solve / ztril_solve / herm_gen_reduce / eigen_herm_gen / eigenvals_herm_gen (csrc/hegv.hip,
 * DESIGN.md 4.25) ---- The Hermitian counterparts of dpotrf, dpotrs, dtrsm (lower), dsygst, dsygvd and dsygvx; the host-pointer forms
 * end in _host. H, L, A, B, C and X are complex128 as interleaved (re, im) doubles, lambda is real. H, A and B are read only where
 * i >= j, the imaginary part of their diagonals is ignored, and they are never written. 1 <= N <= 2048; an empty batch, N = 0 and
 * K = 0 have nothing to do and write nothing. strideL and strideB are in complex elements: N*N, or 0 for one L or B for all members.
 *   zpotrf: L [batch,N,N] with H = L L^H: exact zeros above the diagonal, a real diagonal > 0 with imaginary part +0. Column j:
 *           l_jj = sqrt(Re h_jj - sum_k |l_jk|^2), l_ij = (h_ij - sum_k l_ik conj(l_jk)) / l_jj. A radicand that is not a finite number
 *           > 0 (the exact zero in the last pivot included): ND4HIP_ERR_SINGULAR, 'herm_cholesky_decomp(H): H is not positive
 *           definite. (matrix <b>)' with the lowest such member.
 *   zpotrs: X [batch,N,K] with L L^H X = Y; X may be Y.       ztrsm: L X = X (adjoint = 1: L^H X = X) in place; L is complex
 *           lower triangular, read only where i >= j, its diagonal may be complex. Both only enqueue (the _dev forms).
 *   zhegst: C [batch,N,N] = L^-1 A L^-H (LAPACK's zhegst, itype 1, lower): the lower triangle, zeros above, a real diagonal. Enqueues.
 *   zhegvd: lambda [batch,N] descending and X [batch,N,N] (columns) with A X = B X diag(lambda), X^H B X = I, or X = NULL for the
 *           values alone: zpotrf(B), zhegst, zheevd on C, X = L^-H Y. zhegvx: the same for the subset i0 <= i < i1 (zheevx):
 *           lambda [batch,k], X [batch,N,k]. N = 1: lambda = Re a / Re b, X = 1 / sqrt(Re b). B not positive definite:
 *           ND4HIP_ERR_SINGULAR, 'eigen_herm_gen(A,B): B is not positive definite. (matrix <b>)'; a non-finite C: ND4HIP_ERR_NOCONV,
 *           'eigen_herm_gen(A,B): L^-1 A L^-H is not finite (NaN or Infinity in the lower triangle of A, or overflow).'. Outputs are
 *           unspecified after an error; the handle stays usable.
 * No sum depends on the run, the batch or a member's position. zpotrf, zhegvd and zhegvx synchronise. Profile ops "zpotrf_batched"
 * (4/3 N^3 real flops), "zpotrs_batched", "ztrsm_batched", "zhegst_batched" (8 N^3), "zhegvd_batched" and "zhegvx_batched" (zheevd's or
 * zheevx's count, + 4/3 N^3 + 8 N^3, + 4 N^2 k with vectors). */
int nd4hip_zpotrf_batched_dev (nd4hip_handle* h, int64_t batch, int64_t N, const double* H, double* L);
int nd4hip_zpotrf_batched_host(nd4hip_handle* h, int64_t batch, int64_t N, const double* H, double* L);
int nd4hip_zpotrs_batched_dev (nd4hip_handle* h, int64_t batch, int64_t N, int64_t K, const double* L, int64_t strideL, const double* Y,
                               double* X);
int nd4hip_zpotrs_batched_host(nd4hip_handle* h, int64_t batch, int64_t N, int64_t K, const double* L, int64_t strideL, const double* Y,
                               double* X);
int nd4hip_ztrsm_batched_dev (nd4hip_handle* h, int64_t batch, int64_t N, int64_t K, int adjoint, const double* L, int64_t strideL, double* X);
int nd4hip_ztrsm_batched_host(nd4hip_handle* h, int64_t batch, int64_t N, int64_t K, int adjoint, const double* L, int64_t strideL, double* X);
int nd4hip_zhegst_batched_dev (nd4hip_handle* h, int64_t batch, int64_t N, const double* A, const double* L, int64_t strideL, double* C);
int nd4hip_zhegst_batched_host(nd4hip_handle* h, int64_t batch, int64_t N, const double* A, const double* L, int64_t strideL, double* C);
int nd4hip_zhegvd_batched_dev (nd4hip_handle* h, int64_t batch, int64_t N, const double* A, const double* B, int64_t strideB, double* lambda,
                               double* X);
int nd4hip_zhegvd_batched_host(nd4hip_handle* h, int64_t batch, int64_t N, const double* A, const double* B, int64_t strideB, double* lambda,
                               double* X);
int nd4hip_zhegvx_batched_dev (nd4hip_handle* h, int64_t batch, int64_t N, int64_t i0, int64_t i1, const double* A, const double* B,
                               int64_t strideB, double* lambda, double* X);
int nd4hip_zhegvx_batched_host(nd4hip_handle* h, int64_t batch, int64_t N, int64_t i0, int64_t i1, const double* A, const double* B,
                               int64_t strideB, double* lambda, double* X);

/* ---- eigenpairs in a value interval: eigen_sym(S, interval=(lo, hi)), tridiag_eigen(d, e, interval) (csrc/syevx.hip) ----
 * dstevxv, dsyevxv and dsyevxv_tr are dstevx, dsyevx and dsyevx_tr with the subset of each member chosen by value: bounds [batch,2]
 * holds (lo, hi) per member and selects the eigenvalues lo < lambda <= hi, which is exactly the subset (i0_b, i1_b) =
 * (count(hi), count(lo)) with dstcnt's count on the member's scaled tridiagonal form. lo <= hi; +-Infinity is a bound like any other
 * (count(+inf) = 0, count(-inf) = N); NaN, or lo > hi, is ND4HIP_ERR_ARG (the _host forms look at bounds before anything moves; the
 * _dev forms see lo > hi as i1_b < i0_b after the count, and a NaN bound there selects nothing).
 * Results are ragged: range [batch,2] (int32) receives (i0_b, i1_b), *kmax (a host word in BOTH forms) the largest k_b = i1_b - i0_b.
 * lambda [batch,kcap], Z [batch,kcap,N] (dstevxv; rows = vectors) and V [batch,N,kcap] (columns = vectors) have room for kcap values
 * per member: member b's k_b results stand first, bit for bit those of the subset form with (i0_b, i1_b); its entries k_b .. kmax-1
 * are NaN in lambda and zero in Z / V; nothing from kmax on is written. kcap < kmax: ND4HIP_ERR_ARG, reported after the count and
 * before anything else is launched (kcap = N always fits). Z / V = NULL: the values alone. Device work, and the device-to-host copy
 * of the _host forms, grow with kmax, not with kcap; kmax = 0 launches nothing after the count. The ranges are read back once (the
 * host needs kmax to size the grids) and the calls synchronise. N = 0 and an empty batch have nothing to do and write nothing, kmax
 * included. Errors as the subset forms'. Profile ops "dstevxv_batched", "dsyevxv_batched", "dsyevxv_tr_batched"; stage times through
 * nd4hip_dsyevx_last_stages, the count inside the bisection stage. */
int nd4hip_dstevxv_batched_dev (nd4hip_handle* h, int64_t batch, int64_t N, int64_t kcap, const double* bounds, const double* d, const double* e,
                                double* lambda, double* Z, int32_t* range, int64_t* kmax);
int nd4hip_dstevxv_batched_host(nd4hip_handle* h, int64_t batch, int64_t N, int64_t kcap, const double* bounds, const double* d, const double* e,
                                double* lambda, double* Z, int32_t* range, int64_t* kmax);
int nd4hip_dsyevxv_batched_dev (nd4hip_handle* h, int64_t batch, int64_t N, int64_t kcap, const double* bounds, const double* S, double* lambda,
                                double* V, int32_t* range, int64_t* kmax);
int nd4hip_dsyevxv_batched_host(nd4hip_handle* h, int64_t batch, int64_t N, int64_t kcap, const double* bounds, const double* S, double* lambda,
                                double* V, int32_t* range, int64_t* kmax);
int nd4hip_dsyevxv_tr_batched_dev (nd4hip_handle* h, int64_t batch, int64_t N, int64_t kcap, const double* bounds, const double* S, double* lambda,
                                   double* V, int32_t* range, int64_t* kmax);
int nd4hip_dsyevxv_tr_batched_host(nd4hip_handle* h, int64_t batch, int64_t N, int64_t kcap, const double* bounds, const double* S, double* lambda,
                                   double* V, int32_t* range, int64_t* kmax);

/* ---- eigen_sym_gen / eigenvals_sym_gen with subset, interval or reduction (csrc/sygv.hip) ----
 * dsygvd below (divide & conquer side, algo 0) with step 3, the eigenproblem of C = L^-1 A L^-T, chosen by two selectors:
 *   reduction 0: the Hessenberg reduction (dsygvd's), 1: dsytrd;
 *   select 0: every eigenpair, lambda [batch,N], X [batch,N,N] (with reduction 1: dsyevd_tr);
 *          1: the subset (i0, i1) of the descending spectrum, lambda [batch,k], X [batch,N,k], k = i1 - i0 (dsyevx / dsyevx_tr);
 *          2: the eigenvalues lo < lambda <= hi of every member, bounds [batch,2] = (lo, hi): lambda [batch,kcap], X [batch,N,kcap],
 *             range [batch,2] (int32) and *kmax (a host word in both forms), ragged exactly as dsyevxv's (dsyevxv / dsyevxv_tr).
 * i0, i1 are looked at for select 1 only; kcap, bounds, range and kmax for select 2 only (pass 0 / NULL otherwise). Steps 1 and 2, the
 * errors (B not positive definite with its member: ND4HIP_ERR_SINGULAR; C not finite: ND4HIP_ERR_NOCONV) and the passes over a large
 * batch are dsygvd's. Step 4, X = L^-T Y, runs on the k (or kmax) columns that step 3 computed; for N <= 64 every column has the bits
 * it has in dsygvd's X. X = NULL: the values alone. The host-pointer form ends in _host, as those of the selected eigenpairs do. Profile op "dsygvx_batched". */
int nd4hip_dsygvx_batched_dev (nd4hip_handle* h, int reduction, int select, int64_t batch, int64_t N, int64_t i0, int64_t i1, int64_t kcap,
                               const double* bounds, const double* A, const double* B, int64_t strideB, double* lambda, double* X,
                               int32_t* range, int64_t* kmax);
int nd4hip_dsygvx_batched_host(nd4hip_handle* h, int reduction, int select, int64_t batch, int64_t N, int64_t i0, int64_t i1, int64_t kcap,
                              const double* bounds, const double* A, const double* B, int64_t strideB, double* lambda, double* X,
                              int32_t* range, int64_t* kmax);

/* ---- eigen_sym_gen / eigenvals_sym_gen: A x = lambda B x, A symmetric, B symmetric positive definite (csrc/sygv.hip) ----
 * A [batch,N,N]; B [batch,N,N] (strideB = N*N) or ONE B [N,N] for every member (strideB = 0; it is factorised once per call of the
 * _dev form, once per staged chunk of the host form, never once per member). Only the lower triangles of A and B are read and
 * neither is written: NaN or garbage above the diagonals changes no bit of the result. lambda [batch,N] descending; X [batch,N,N]
 * with the eigenvectors as columns, A X = B X diag(lambda), X^T B X = I; X = NULL: the values alone, the same bits, no
 * back-transformation. algo 0: the default route of dsyevd (N <= 2048); algo 1: dsyevj (N <= 128), sweeps [batch] (may be NULL; it
 * is not written for algo 0) then receives each member's sweep count. A larger N or another algo is ND4HIP_ERR_ARG before anything
 * is written. N = 0 and empty batches: nothing to do.
 * Route (LAPACK's dsygvd): L = chol(B); C = L^-1 A L^-T, lower triangle; (lambda, Y) of C by dsyevd / dsyevj, unchanged;
 * X = L^-T Y. Tiers: N <= 64 two fused kernels with one workgroup per member, A, B and L in LDS, all arithmetic rounded
 * operation by operation in the order of the numpy model in tests/sygv_common.py, whose bits they return; 64 < N <= 2048 dpotrf,
 * two dtrsm around a transposition, and the transposed solve for X.
 * Errors. B not positive definite (some Cholesky radicand is not a finite number > 0, an exact zero in the last pivot included):
 * ND4HIP_ERR_SINGULAR with 'eigen_sym_gen(A,B): B is not positive definite. (matrix <b>)', b the lowest such member. C not finite:
 * ND4HIP_ERR_NOCONV with 'eigen_sym_gen(A,B): L^-1 A L^-T is not finite (NaN or Infinity in the lower triangle of A, or
 * overflow).' The outputs are unspecified then; the handle stays usable.
 * Accuracy, per member, sigma the singular values of B and kappa = sigma_max / sigma_min, within 1e-12 of:
 *   |lambda^_i - lambda_i| <= ||A||_F / sigma_min + kappa |lambda_i|;   ||A X - B X diag(lambda)||_F <= (||A||_F + ||B||_F max|lambda|) ||X||_F;
 *   ||X^T B X - I||_F <= kappa sqrt(N);   and for step 2 (dsygst below, both tiers):   ||L C L^T - A||_F <= ||L||_F^2 ||C||_F.
 * 2^k A gives 2^k lambda and the same X, 4^j B gives 4^-j lambda and 2^-j X, exactly, while nothing leaves the normal range.
 * A member's results do not depend on the batch. Both forms synchronise. Profile op "dsygvd_batched": dsyevd's (dsyevj's) flops
 * plus (1/3 + 2) N^3 for L and C, plus N^3 with X. */
int nd4hip_dsygvd_batched_dev(nd4hip_handle* h, int algo, int64_t batch, int64_t N, const double* A, const double* B, int64_t strideB,
                              double* lambda, double* X, int32_t* sweeps);
int nd4hip_dsygvd_batched    (nd4hip_handle* h, int algo, int64_t batch, int64_t N, const double* A, const double* B, int64_t strideB,
                              double* lambda, double* X, int32_t* sweeps);
/* step 2 on its own (LAPACK's dsygst): C [batch,N,N] = L^-1 A L^-T from a given lower triangular L [batch,N,N] (strideL = N*N, or
 * 0: one L); the lower triangle of C is written and exact zeros above it. The same two tiers, N <= 2048. No verdict is read.
 * Accuracy: ||L C L^T - A||_F <= 1e-12 ||L||_F^2 ||C||_F with C mirrored from its lower triangle; for N <= 64 the bits of
 * sygst_model in tests/sygv_common.py. */
int nd4hip_dsygst_batched_dev(nd4hip_handle* h, int64_t batch, int64_t N, const double* A, const double* L, int64_t strideL, double* C);
int nd4hip_dsygst_batched    (nd4hip_handle* h, int64_t batch, int64_t N, const double* A, const double* L, int64_t strideL, double* C);

/* ---- one Householder panel on its own: geqr2 + larft of a 16-column panel (the inner step of qr_decomp, src/la/qr.js:54-68
 * eliminates the same entries column by column with Givens rotations) ---------------------------------------------
 * A [batch,M,16] (1 <= M <= 2048) is overwritten with R in its top 16 x 16 (entries below the diagonal are left as the kernel
 * leaves them); V [batch,M,16] receives the panel's reflector block, T [batch,16,16] its factor: Q_panel = I - V T V^T is
 * orthogonal and Q_panel^T A = [R; 0]. Panels of fewer than 64 rows take the thread-per-row Householder kernel: V explicit unit
 * lower trapezoidal, T upper triangular (compact WY). Everything else is CholeskyQR2 + a compact orthogonal completion:
 * V = Q - [S; 0] with a full top block, T a full 16 x 16 matrix — up to 8 panels as the row-split launch (the rows of a panel over
 * co-resident workgroups), more than 8 as ONE workgroup per panel on the matrix cores (round 4, qr_batched_panel.hip), which reads
 * every element of A once and writes V once and nothing else: the rows of A below the top 16 are left untouched. A panel the Gram
 * route must not take (nearly dependent columns, a column that is zero below the top block, non-finite data) is factorised by
 * the thread-per-row kernel in the same launch (compact WY form, rows below R zeroed).
 * Device pointers. Exposed for the panel roofline of bench.py (16 M b bytes per panel). */
int nd4hip_dgeqr2_panel_batched_dev(nd4hip_handle* h, int64_t batch, int64_t M, int64_t b, double* A, double* V, double* T);

/* Executed-work audit of the LAST nd4hip_dgesvdj_batched[_dev] call on this handle ("must print sweeps and
 * rotations actually applied"; the reference's loop is svd_jac_2sided.js:95-134): sweeps = max over the batch, rotations =
 * plane rotations applied over all matrices and sweeps, offnorm = largest |a_p.a_q| / (|a_p||a_q|) over the row pairs as they
 * were found during the last sweep (<= N*eps at convergence). Any pointer may be NULL. */
int nd4hip_dgesvdj_last_info(nd4hip_handle* h, int* sweeps, unsigned long long* rotations, double* offnorm);

/* ---- per-call profile (SURVEY.md 8b `nd4hip_profile_last`; the reference times calls with performance.now(),
 * benchmarks/bench_la_decomps.html:218-224) ---------------------------------------------------------------------
 * nd4hip_profile_enable(h, 1): from now on every device-side entry point (the *_dev forms; the host-pointer forms run them per
 * chunk and per device) brackets its kernels with two HIP events on the handle's stream and records the ALGORITHMIC work of the
 * call (SURVEY.md 8d conventions: matmul 2 I K J, LU 2/3 N^3, QR with explicit Q 4 (M N^2 - N^3 / 3) for M >= N, SVD nominal
 * 4 M^2 N + 8 M N^2 + 9 N^3, ...; bytes = every operand read once and every result written once). Off by default (two event
 * records per call). nd4hip_profile_last fills one record per device of the handle (capacity entries at most; a multi-device
 * handle's devices each report the last block they ran), waits for those kernels to finish, and returns the number of devices.
 * For a host-pointer call that was cut into chunks a record describes the LAST chunk of that device. */
typedef struct nd4hip_prof {
  double kernel_ms;   /* HIP-event time between the first and the last kernel of the call on this device */
  double flops;       /* algorithmic flops of the call (0 for pure data movement) */
  double bytes;       /* algorithmic HBM bytes of the call */
  int    device;      /* HIP device id */
  int    valid;       /* 0: nothing recorded on this device yet */
  char   op[32];      /* entry point without the nd4hip_ prefix, e.g. "dgetrf_batched" */
} nd4hip_prof;
int nd4hip_profile_enable(nd4hip_handle* h, int on);
int nd4hip_profile_last(nd4hip_handle* h, nd4hip_prof* out, int capacity);

#ifdef __cplusplus
}
#endif
#endif /* ND4HIP_H */
