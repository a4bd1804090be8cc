// The reference's Givens sign convention restored on a Householder-built (Q, R) pair: nd4_givens_signs, called by the QR drivers
// (qr.hip) and by bidiagonalisation. For M <= N the reference's plane rotations give R_jj = +norm for every column that had something
// eliminated below it and det(Q) = +1: column j of Q / row j of R is flipped where tau_j != 0 and R_jj < 0, and then, if the parity
// of (#reflectors + #flips) is odd, the last column of Q / last row of R.
#include "qr_internal.h"

namespace {
// ------------------------------------------------------------------------------------ sign fix
// One thread per matrix: decides the flips (reference convention, see file header).
// Tall input (M > N) follows the reference's other branch (qr.js:97-139): every rotation is normalised to
// c >= 0, which PRESERVES the sign of the pivot R_jj, so sign(R_jj) is whatever it was when row j finished its
// own eliminations = sign(det A[0:j+1,0:j+1] / det A[0:j,0:j]). With A[0:k,0:k] = Q[0:k,0:k] R[0:k,0:k] the
// flip of column j is the sign of the j-th pivot of Gaussian elimination WITHOUT pivoting on Q[0:N,0:N].
__global__ void qr_flips_tall(const double* __restrict__ LUq, int N, int* __restrict__ flips, int batch) {
  const long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
  if (i >= (long)batch * N) return;
  const long b = i / N, j = i % N;
  flips[i] = LUq[b * N * N + j * N + j] < 0.0 ? 1 : 0;
}
__global__ __launch_bounds__(256) void qr_flips(const double* __restrict__ Rm, long ldr, long strideR, const double* __restrict__ taus, long strideTau,
                                                 int M, int N, int L, int* __restrict__ flips, int batch) {
  // one workgroup per matrix: flags in parallel, parity by a block-wide XOR
  const int b = blockIdx.x;
  const double* R = Rm + b * strideR; const double* tau = taus + b * strideTau; int* f = flips + (long)b * L;
  __shared__ int s_par[4];
  int parity = 0;
  for (int j = threadIdx.x; j < L; j += 256) {
    int fl = 0;
    if (tau[j] != 0.0) { parity ^= 1; if (R[(long)j * ldr + j] < 0.0) { fl = 1; parity ^= 1; } }
    f[j] = fl;
  }
  parity = __popcll(__ballot(parity)) & 1;
  if ((threadIdx.x & 63) == 0) s_par[threadIdx.x >> 6] = parity;
  __syncthreads();
  // plane rotations never change the determinant: det(Q) = +1 whenever Q is square (M <= N)
  if (threadIdx.x == 0 && M <= N && ((s_par[0] ^ s_par[1] ^ s_par[2] ^ s_par[3]) & 1)) f[L - 1] ^= 1;
}
// scale rows of R (rows x cols, ld) by -1 where flips[row]
__global__ void qr_flip_rows(double* __restrict__ X, long ld, long strideX, int rows, int cols, const int* __restrict__ flips, int L) {
  X += blockIdx.z * strideX; flips += (long)blockIdx.z * L;
  const int col = blockIdx.x * blockDim.x + threadIdx.x;
  if (col >= cols) return;
  for (int r = blockIdx.y; r < rows; r += gridDim.y)
    if (flips[r]) X[(long)r * ld + col] = -X[(long)r * ld + col];
}
// scale columns of Q (rows x cols, ld) by -1 where flips[col]
__global__ void qr_flip_cols(double* __restrict__ X, long ld, long strideX, int rows, int cols, const int* __restrict__ flips, int L) {
  X += blockIdx.z * strideX; flips += (long)blockIdx.z * L;
  const int col = blockIdx.x * blockDim.x + threadIdx.x;
  if (col >= cols || !flips[col]) return;
  for (int r = blockIdx.y; r < rows; r += gridDim.y) X[(long)r * ld + col] = -X[(long)r * ld + col];
}

}  // namespace

// Sign convention of the reference's Givens-built factors, applied to a Householder-built pair (Q [M, >= L] with leading
// dimension ldq, R [L, ncols] with leading dimension ldr; column j of Q and row j of R are flipped together):
//   lu_rule = false (qr_decomp_full, the square / wide branches): R_jj >= 0 wherever a reflector was needed (tau_j != 0),
//             and det Q = +1 (plane rotations) decides the last one when Q is square (M == L);
//   lu_rule = true  (the c >= 0 branches for tall input, qr.js:97-139 / bidiag.js:49-61): every leading principal minor of
//             Q's top L x L block is positive = positive pivots in its LU factorisation WITHOUT pivoting.
// flips: L ints per matrix of scratch. Q == nullptr (lu_rule = false only): R's rows are flipped and there is no Q to follow them.
int nd4_givens_signs(nd4hip_handle* h, int batch, int M, int L, int ncols, bool lu_rule, double* Q, long ldq, long sQ,
                     double* R, long ldr, long sR, const double* taus, long sTau, int* flips) {
  ND4_CHECK_ARG(Q != nullptr || !lu_rule, "nd4_givens_signs: the c >= 0 rule needs Q");
  if (lu_rule) {
    Nd4WsScope scope2(h);
    void* q = nullptr;
    ND4_TRY(nd4_ws_alloc(h, sizeof(double) * (size_t)batch * L * L + sizeof(int32_t) * (size_t)batch * L, &q));
    double* LUq = static_cast<double*>(q);
    int32_t* Pq = reinterpret_cast<int32_t*>(LUq + (size_t)batch * L * L);
    ND4_TRY(nd4_copy_matrix(h, L, L, Q, ldq, LUq, L, batch, sQ, (long)L * L));
    ND4_TRY(nd4_getrf_nopivot(h, batch, L, LUq, LUq, Pq));
    hipLaunchKernelGGL(qr_flips_tall, dim3((unsigned)(((long)batch * L + 255) / 256)), dim3(256), 0, h->stream, LUq, L, flips, batch);
  } else {
    // qr_flips decides the parity flip by "M <= N": pass N = M when Q is square, N = M - 1 otherwise
    hipLaunchKernelGGL(qr_flips, dim3((unsigned)batch), dim3(256), 0, h->stream,
                       R, ldr, sR, taus, sTau, M, (M == L ? M : M - 1), L, flips, batch);
  }
  {
    const unsigned gy = (unsigned)(L < 512 ? L : 512);
    hipLaunchKernelGGL(qr_flip_rows, dim3((unsigned)((ncols + 255) / 256), gy, (unsigned)batch), dim3(256), 0, h->stream,
                       R, ldr, sR, L, ncols, flips, L);
    const unsigned gq = (unsigned)(M < 512 ? M : 512);
    if (Q) hipLaunchKernelGGL(qr_flip_cols, dim3((unsigned)((L + 255) / 256), gq, (unsigned)batch), dim3(256), 0, h->stream,
                       Q, ldq, sQ, M, L, flips, L);
  }
  ND4_HIP(hipGetLastError());
  return 0;
}
