// Block reflectors and compact-WY factors, shared by the QR drivers (qr.hip), Hessenberg and bidiagonalisation (nd4_wy_form):
//   qr_vtc, qr_tw     Wp = V^T C on fp64 MFMA per 256-row chunk, W2 = op(T) * sum_chunks(Wp); with nd4_gemm's C -= V W2 they apply one
//                     16-column block reflector (nd4_qr_apply_block_reflector)
//   nd4_qr_block_update   C <- (I - V op(T) V^T) C for wider blocks, as three GEMMs
//   wy_t_diag, wy_t_small, nd4_qr_wy_build_T, nd4_wy_form   the n x n compact-WY factor from the panels' factors, and Q formed from it
#include "qr_internal.h"

namespace {

constexpr int VTC_COLS = 64;      // columns per workgroup of qr_vtc
// ------------------------------------------------------------------------------------ V^T C
// Wp[chunk][i][j] = sum_{r in chunk} V[r][i] * C[r][j]; V: m x 16 (ldv), C: m x n (ldc).
// grid (ceil(n/64), ceil(m/256), batch), 256 threads: wave w takes rows chunk*256 + w*64 .. +64 and
// all 4 column strips of 16; the 4 waves' tiles are summed through LDS.
__global__ __launch_bounds__(256) void qr_vtc(const double* __restrict__ V, long ldv, long strideV,
                                               const double* __restrict__ C, long ldc, long strideC,
                                               int m, int n, double* __restrict__ Wp, long ldw, long strideChunk, long strideWb) {
  __shared__ double s_acc[4][4][4][64];      // [wave][strip][reg][lane]
  V += blockIdx.z * strideV; C += blockIdx.z * strideC; Wp += blockIdx.z * strideWb + blockIdx.y * strideChunk;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int fx = lane & 15, fk = lane >> 4;
  const int col0 = blockIdx.x * VTC_COLS;
  const int row0 = blockIdx.y * VTC_ROWS + wave * 64;
  d4 acc[4];
#pragma unroll
  for (int s = 0; s < 4; s++) acc[s] = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll 4
  for (int kk = 0; kk < 16; kk++) {
    const int r = row0 + kk * 4 + fk;
    const bool rok = r < m;
    const double a = rok ? V[(long)r * ldv + fx] : 0.0;
    double b[4];
#pragma unroll
    for (int s = 0; s < 4; s++) {
      const int col = col0 + s * 16 + fx;
      b[s] = (rok && col < n) ? C[(long)r * ldc + col] : 0.0;
    }
#pragma unroll
    for (int s = 0; s < 4; s++) acc[s] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b[s], acc[s], 0, 0, 0);
  }
#pragma unroll
  for (int s = 0; s < 4; s++)
#pragma unroll
    for (int r = 0; r < 4; r++) s_acc[wave][s][r][lane] = acc[s][r];
  __syncthreads();
  // thread t -> (strip s = wave, lane): sums the four waves' copies, fixed order
#pragma unroll
  for (int r = 0; r < 4; r++) {
    const double v = ((s_acc[0][wave][r][lane] + s_acc[1][wave][r][lane]) + s_acc[2][wave][r][lane]) + s_acc[3][wave][r][lane];
    const int i = fk + 4 * r, col = col0 + wave * 16 + fx;
    if (col < n) Wp[(long)i * ldw + col] = v;
  }
}

// W2[:, j] = op(T) * sum_chunks Wp[chunk][:, j]; T upper triangular 16x16; trans -> T^T
__global__ __launch_bounds__(256) void qr_tw(const double* __restrict__ Tall, long strideT, int panel, int trans,
                                              const double* __restrict__ Wp, long ldw, long strideChunk, long strideWb, int nchunks,
                                              int n, double* __restrict__ W2, long strideW2) {
  __shared__ double s_T[NB][NB + 1];
  const double* T = Tall + blockIdx.y * strideT + (long)panel * NB * NB;
  Wp += blockIdx.y * strideWb; W2 += blockIdx.y * strideW2;
  const int t = threadIdx.x;
  s_T[t / NB][t % NB] = T[t];
  __syncthreads();
  const int col = blockIdx.x * 256 + t;
  if (col >= n) return;
  double w[NB];
#pragma unroll
  for (int i = 0; i < NB; i++) w[i] = 0.0;
  for (int ch = 0; ch < nchunks; ch++)
#pragma unroll
    for (int i = 0; i < NB; i++) w[i] += Wp[ch * strideChunk + (long)i * ldw + col];
#pragma unroll
  for (int i = 0; i < NB; i++) {
    double s = 0.0;
    if (trans) {
#pragma unroll
      for (int j = 0; j < NB; j++) s += s_T[j][i] * w[j];
    } else {
#pragma unroll
      for (int j = 0; j < NB; j++) s += s_T[i][j] * w[j];
    }
    W2[(long)i * ldw + col] = s;
  }
}

// diagonal bs x bs blocks of the n x n compact-WY factor <- the given blocks (everything else zero); bs = 1: the taus
__global__ void wy_t_diag(const double* __restrict__ Tp, double* __restrict__ Tall, int n, int bs) {
  const int blk = blockIdx.x, t = threadIdx.x;                      // bs * bs threads
  Tall[(long)(blk * bs + t / bs) * n + blk * bs + t % bs] = Tp[(long)blk * bs * bs + t];
}

// Compact-WY factor of up to 64 reflector columns = up to four panels of a batch member: T (n x n) from the panels' 16 x 16 factors
// on its diagonal and G = V^T V, T12 = -T1 (V1^T V2) T2 level by level (16, then 32 columns; valid for the FULL factors of the
// matrix-core panels as well as for triangular ones). One workgroup per matrix, everything in LDS: each G12 block is used once, so
// G12 T2 overwrites it. Batches beyond the look-ahead form (qr_batch: the rank-16 updates were 56 % of the run).
__global__ __launch_bounds__(256) void wy_t_small(const double* __restrict__ Tdiag, long sTd, const double* __restrict__ G, int ldg, long sG,
                                                   double* __restrict__ Tout, int ldt, long sTo, int n) {
  static_assert(NB == 16, "the 64 x 64 LDS tiles below hold four 16-column panels; the index arithmetic is written for NB = 16");
  __shared__ double s_t[64 * 64], s_g[64 * 64];
  const long m = blockIdx.x;
  const int t = threadIdx.x;
  for (int e = t; e < 4096; e += 256) {
    const int i = e >> 6, j = e & 63;
    const bool in = i < n && j < n;
    s_g[e] = in ? G[m * sG + (long)i * ldg + j] : 0.0;
    s_t[e] = (in && (i >> 4) == (j >> 4)) ? Tdiag[m * sTd + (long)(i >> 4) * 256 + (i & 15) * 16 + (j & 15)] : 0.0;
  }
  __syncthreads();
  for (int b = 16; b < n; b <<= 1) {
    double v[16];
#pragma unroll
    for (int k = 0; k < 16; k++) {                                    // X = G12 T2 on the 12-blocks of this level
      const int e = t + 256 * k, i = e >> 6, j = e & 63, p0 = i & ~(2 * b - 1);
      const int qe = (p0 + 2 * b < n) ? p0 + 2 * b : n;
      double x = 0.0;
      if (i - p0 < b && j >= p0 + b && j < qe) for (int q = p0 + b; q < qe; q++) x += s_g[i * 64 + q] * s_t[q * 64 + j];
      v[k] = x;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 16; k++) {
      const int e = t + 256 * k, i = e >> 6, j = e & 63, p0 = i & ~(2 * b - 1);
      const int qe = (p0 + 2 * b < n) ? p0 + 2 * b : n;
      if (i - p0 < b && j >= p0 + b && j < qe) s_g[e] = v[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 16; k++) {                                    // T12 = -T1 X
      const int e = t + 256 * k, i = e >> 6, j = e & 63, p0 = i & ~(2 * b - 1);
      const int qe = (p0 + 2 * b < n) ? p0 + 2 * b : n;
      double y = 0.0;
      if (i - p0 < b && j >= p0 + b && j < qe) for (int q = p0; q < p0 + b; q++) y += s_t[i * 64 + q] * s_g[q * 64 + j];
      v[k] = y;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 16; k++) {
      const int e = t + 256 * k, i = e >> 6, j = e & 63, p0 = i & ~(2 * b - 1);
      const int qe = (p0 + 2 * b < n) ? p0 + 2 * b : n;
      if (i - p0 < b && j >= p0 + b && j < qe) s_t[e] = -v[k];
    }
    __syncthreads();
  }
  for (int e = t; e < 4096; e += 256) {
    const int i = e >> 6, j = e & 63;
    if (i < n && j < n) Tout[m * sTo + (long)i * ldt + j] = s_t[e];
  }
}

}  // namespace

// C (rows [j0,M) x n columns starting at C0) <- (I - V op(T) V^T) C, V = Vall[j0:, j0:j0+nb]
int nd4_qr_apply_block_reflector(nd4hip_handle* h, const QrWs& ws, int batch, int M, int j0, int panel, int trans,
                                 double* C0, long ldc, long strideC, int n) {
  if (n <= 0) return 0;
  const int m = M - j0;
  const int nchunks = (m + VTC_ROWS - 1) / VTC_ROWS;
  const double* Vp = ws.V + (long)j0 * ws.ldv + j0;
  hipLaunchKernelGGL(qr_vtc, dim3((unsigned)((n + VTC_COLS - 1) / VTC_COLS), (unsigned)nchunks, (unsigned)batch), dim3(256), 0, h->stream,
                     Vp, ws.ldv, ws.sV, C0, ldc, strideC, m, n, ws.Wp, ws.ldw, ws.sChunk, ws.sWb);
  hipLaunchKernelGGL(qr_tw, dim3((unsigned)((n + 255) / 256), (unsigned)batch), dim3(256), 0, h->stream,
                     ws.T, ws.sT, panel, trans, ws.Wp, ws.ldw, ws.sChunk, ws.sWb, nchunks, n, ws.W2, ws.sW2);
  ND4_HIP(hipGetLastError());
  return nd4_gemm(h, false, false, m, n, NB, -1.0, Vp, ws.ldv, ws.sV, ws.W2, ws.ldw, ws.sW2, 1.0, C0, ldc, strideC, batch);
}

// C <- (I - V op(T) V^T) C for nblk reflector columns V [m, nblk] and their nblk x nblk factor T: X = V^T C, W = op(T) X, C -= V W
// (X, W: nblk x n, leading dimension n); strides per matrix of the batch (0 for one matrix)
int nd4_qr_block_update(nd4hip_handle* h, bool transT, int m, int n, int nblk, const double* V, long ldv, long sV, const double* T, long sT,
                        double* C, long ldc, long sC, double* X, double* W, long sX, int batch) {
  ND4_TRY(nd4_gemm(h, true, false, nblk, n, m, 1.0, V, ldv, sV, C, ldc, sC, 0.0, X, n, sX, batch));
  ND4_TRY(nd4_gemm(h, transT, false, nblk, n, nblk, 1.0, T, nblk, sT, X, n, sX, 0.0, W, n, sX, batch));
  return nd4_gemm(h, false, false, m, n, nblk, -1.0, V, ldv, sV, W, n, sX, 1.0, C, ldc, sC, batch);
}

void nd4_qr_wy_t_small(nd4hip_handle* h, int batch, const double* Tdiag, long sTd, const double* G, int ldg, long sG,
                       double* Tout, int ldt, long sTo, int n) {
  hipLaunchKernelGGL(wy_t_small, dim3((unsigned)batch), dim3(256), 0, h->stream, Tdiag, sTd, G, ldg, sG, Tout, ldt, sTo, n);
}

// The n x n compact-WY factor T of n reflector columns V [M, n] (leading dimension ldv) from its bs x bs diagonal blocks Tdiag
// ([n / bs][bs][bs]; bs = 1: the taus) and the Gram matrix V^T V: T[1,2] = -T1 (V1^T V2) T2 for two adjacent groups, level by level
// (groups of bs, 2 bs, 4 bs, ... columns). G, tmp: workspaces of n * n and n * n / 2 + 16 doubles. n must be a multiple of bs.
int nd4_qr_wy_build_T(nd4hip_handle* h, int M, int n, const double* V, long ldv, const double* Tdiag, int bs, double* Tall, double* G, double* tmp) {
  ND4_TRY(nd4_gemm(h, true, false, n, n, M, 1.0, V, ldv, 0, V, ldv, 0, 0.0, G, n, 0, 1));
  ND4_HIP(hipMemsetAsync(Tall, 0, sizeof(double) * (size_t)n * n, h->stream));
  hipLaunchKernelGGL(wy_t_diag, dim3((unsigned)(n / bs)), dim3((unsigned)(bs * bs)), 0, h->stream, Tdiag, Tall, n, bs);
  ND4_HIP(hipGetLastError());
  for (int b = bs; b < n; b *= 2) {
    const long step = 2l * b * (n + 1);                             // from one pair of groups to the next, along the diagonal
    const int full = n / (2 * b);
    for (int f0 = 0; f0 < full; f0 += 32768) {                      // gridDim.y limit of the batched launch
      const int nf = full - f0 < 32768 ? full - f0 : 32768;
      const long o = f0 * step;
      ND4_TRY(nd4_gemm(h, false, false, b, b, b, 1.0, G + b + o, n, step, Tall + (long)b * (n + 1) + o, n, step, 0.0, tmp, b, (long)b * b, nf));
      ND4_TRY(nd4_gemm(h, false, false, b, b, b, -1.0, Tall + o, n, step, tmp, b, (long)b * b, 0.0, Tall + b + o, n, step, nf));
    }
    const int i0 = full * 2 * b, n2 = n - i0 - b;                    // ragged last pair: second group narrower
    if (n2 > 0) {
      ND4_TRY(nd4_gemm(h, false, false, b, n2, n2, 1.0, G + (long)i0 * n + i0 + b, n, 0, Tall + (long)(i0 + b) * (n + 1), n, 0, 0.0, tmp, n2, 0, 1));
      ND4_TRY(nd4_gemm(h, false, false, b, n2, b, -1.0, Tall + (long)i0 * (n + 1), n, 0, tmp, n2, 0, 0.0, Tall + (long)i0 * n + i0 + b, n, 0, 1));
    }
  }
  return 0;
}

// Q [M, Lq] (row-major, ld Lq) = (H_0 H_1 ... H_{n-1}) [I; 0] for reflectors H_j = I - tau_j v_j v_j^T given as the columns of
// V [M, n] (ld n), formed at once from their compact-WY representation H_0 ... H_{n-1} = I - V T V^T: T is upper triangular
// with the given bs x bs factors on its diagonal (bs = 1: the taus themselves) and T[1,2] = -T1 (V1^T V2) T2 for two adjacent
// groups, applied level by level (groups of bs, 2 bs, 4 bs, ... columns). One Gram matrix V^T V (TN GEMM), two
// strided-batched small GEMMs per level, W = T V[0:Lq,:]^T and Q = E - V W: ~20-30 launches and 6 M n^2 flop on the MFMA
// kernels instead of a backward loop of rank-bs updates. n must be a multiple of bs; zero columns of V are harmless.
int nd4_wy_form(nd4hip_handle* h, int M, int n, const double* V, const double* Tdiag, int bs, double* Q, int Lq) {
  Nd4WsScope scope(h);
  void* p = nullptr;
  ND4_TRY(nd4_ws_alloc(h, sizeof(double) * ((size_t)n * n * 2 + (size_t)n * n / 2 + (size_t)n * Lq + 64), &p));
  double* G = static_cast<double*>(p);
  double* Tall = G + (size_t)n * n;
  double* tmp = Tall + (size_t)n * n;
  double* W = tmp + (size_t)n * n / 2 + 16;
  ND4_TRY(nd4_qr_wy_build_T(h, M, n, V, n, Tdiag, bs, Tall, G, tmp));
  ND4_TRY(nd4_gemm(h, false, true, n, Lq, n, 1.0, Tall, n, 0, V, n, 0, 0.0, W, Lq, 0, 1));                   // W = T V[0:Lq,:]^T
  ND4_TRY(nd4_set_identity(h, M, Lq, Q, Lq, 1, (long)M * Lq));
  return nd4_gemm(h, false, false, M, Lq, n, -1.0, V, n, 0, W, Lq, 0, 1.0, Q, Lq, 0, 1);                     // Q = E - V W
}
