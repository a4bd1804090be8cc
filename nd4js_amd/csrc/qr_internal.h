// Declarations shared by the QR units: the constants more than one of them needs, the workspace slices of a factorisation, and the
// host launchers each unit offers the others (a kernel is launched only from the unit that defines it).
//   qr.hip                drivers                         qr_house.hip          Householder panels (global-memory, thread-per-row, split)
//   qr_rowsplit.hip       row-split panels (qrh_*)        qr_batched_panel.hip  one-workgroup matrix-core panels (qrb_*)
//   qr_wy.hip             block reflectors, compact WY    qr_signs.hip          the reference's sign convention
#pragma once
#include "nd4hip_internal.h"

typedef double d4 __attribute__((ext_vector_type(4)));

constexpr int NB = 16;            // panel width
// A reflector is formed only when the column below the diagonal has sum of squares sigma >= QR_SIGMA_MIN (or is not finite). The work
// copy is normalised to max|a| in [1, 2), but a column can still shrink far below that: with bitwise identical columns (a matrix of
// ones) every reflector leaves the next column at eps times the previous one, and after ~10 columns the squares are subnormal. sigma
// and alpha^2 then carry only a few bits, beta and tau stop matching v, and H = I - tau v v^T is no longer orthogonal (Q of
// ones(96, 80) was off by 1e-3). Below 2^-960 the column (norm < 2^-480 against a max of 1) is left as it is (tau = 0, like an
// exactly zero column): a backward error far below eps. At or above it the subnormal terms change sigma by < 2^-90 relatively.
constexpr double QR_SIGMA_MIN = 0x1p-960;
constexpr int VTC_ROWS = 256;     // rows per workgroup of qr_vtc (the drivers size its chunk partials)

// The Gram-route panels (qr_rowsplit.hip, qr_batched_panel.hip) and who takes them.
// (HR_*, QR_ROWSPLIT_MAX_BATCH and QR_SMALL_WG_BATCH are restated in tests/qr_common.py, which models these decisions: keep the two in step)
constexpr double HR_PIVOT_THR = 1e-5;
constexpr double HR_SERIES_MAX = 1e-5;
// max |Q1^T Q1 - I| after the first pass beyond which the panel is flagged after all. With max |E| <= 1e-2, ||E||_2 <= 0.16 and
// cond(Q1)^2 <= 1.16 / 0.84 = 1.4: the second pass leaves Q orthonormal to 1.4 times what it leaves for a well-conditioned panel. Beyond
// (cond(panel) from about 1e7: max |E| ~ eps cond^2) CholeskyQR2 loses orthogonality: 1e4 ... 1e5 eps at cond = 3e11, measured.
constexpr double HR_PASS1_MAX = 1e-2;
constexpr int HR_MIN_ROWS = 64;
constexpr int QR_ROWSPLIT_MAX_BATCH = 8;   // row-split panels (qrh_bc) up to this many matrices; more: one workgroup per panel
constexpr int QR_SMALL_WG_BATCH = 64;      // from this many panels on, a panel of <= 1024 rows takes few waves with four rows per thread

struct QrWs {
  double *V, *T, *Tside, *taus, *Wp, *W2, *work; int* flips;
  long ldv, sV, sT, sTau, ldw, sChunk, sWb, sW2;
  int nchunks_max;
};

// ---- qr_house.hip ----
struct QrPanelShape { int R, NWV; };       // rows per thread, waves per workgroup
// <R, NWV> of a one-workgroup panel of m <= 2048 rows in a batch (qr_panel_row and qrb_panel share the rule)
QrPanelShape nd4_qr_panel_shape(int batch, int m);
void nd4_qr_panel_global(nd4hip_handle* h, int batch, double* W, int M, long ld, long sW, double* V, long ldv, long sV,
                         double* T, long sT, double* taus, long sTau, int j0, int nb);
void nd4_qr_panel_flagged(nd4hip_handle* h, int batch, double* W, int M, long ld, long sW, double* V, long ldv, long sV,
                          double* T, long sT, double* taus, long sTau, int j0, int nb, const int* flag);
void nd4_qr_panel_rows(nd4hip_handle* h, int batch, double* W, int M, int m, long ld, long sW, double* V, long ldv, long sV,
                       double* T, long sT, double* taus, long sTau, int j0, int nb);
// nwg workgroups per matrix: the panel, nwide column blocks of W, then blocks of Q^T
void nd4_qr_panel_row_la(nd4hip_handle* h, int batch, int nwg, double* W, int M, int N, long ld, long sW, double* V, long ldv, long sV,
                         double* T, long sT, double* taus, long sTau, int j0, int nb, int pj0, int wc0, int nwide, double* QT, long sQT);
void nd4_qr_narrow_x(nd4hip_handle* h, int batch, const double* W, int M, int N, long ld, long sW, const double* V, long ldv, long sV,
                     int pj0, int c0, double* Xp, long sXp);
void nd4_qr_narrow_apply(nd4hip_handle* h, int batch, double* W, int M, int N, long ld, long sW, const double* V, long ldv, long sV,
                         const double* T, long sT, int pj0, int c0, const double* Xp, long sXp, int nparts);
void nd4_qr_update_blocks(nd4hip_handle* h, int batch, int nblocks, double* C, int M, int ncols, long ld, long sC,
                          const double* V, long ldv, long sV, const double* T, long sT, int pj0, int wc0);
// one part of w = 8 (m <= 4096) or 4 (m <= 8192) columns of a 16-column slot
void nd4_qr_panel_part(nd4hip_handle* h, int batch, int w, double* W, int M, long ld, long sW, double* V, long ldv, long sV,
                       double* T, double* Tside, long sT, double* taus, long sTau, int c0, int nb);
void nd4_qr_t_assemble(nd4hip_handle* h, int batch, double* T, const double* Tside, long sT, int panel, const double* G, long sG, int bs);

// ---- qr_batched_panel.hip ----
// in-matrix panels of a batch (the rows below the top block are zeroed in W) / the panel entry point's, with its debug switches
void nd4_qr_panel_mfma(nd4hip_handle* h, int batch, double* W, int M, int m, long ld, long sW, double* V, long ldv, long sV,
                       double* T, long sT, double* taus, long sTau, int j0);
int nd4_qr_panel_mfma_alone(nd4hip_handle* h, int batch, int M, double* A, double* V, double* T, double* taus);

// ---- qr_wy.hip ----
int nd4_qr_apply_block_reflector(nd4hip_handle* h, const QrWs& ws, int batch, int M, int j0, int panel, int trans,
                                 double* C0, long ldc, long strideC, int n);
int nd4_qr_block_update(nd4hip_handle* h, bool transT, int m, int n, int nblk, const double* V, long ldv, long sV, const double* T, long sT,
                        double* C, long ldc, long sC, double* X, double* W, long sX, int batch);
void nd4_qr_wy_t_small(nd4hip_handle* h, int batch, const double* Tdiag, long sTd, const double* G, int ldg, long sG,
                       double* Tout, int ldt, long sTo, int n);
int nd4_qr_wy_build_T(nd4hip_handle* h, int M, int n, const double* V, long ldv, const double* Tdiag, int bs, double* Tall, double* G, double* tmp);
