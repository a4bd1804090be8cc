// Row-split (multi-workgroup) QR panels, host side: the launch parameters QrhP of the qrh_* kernels and the object QrhHost that
// sequences them (qr_rowsplit.hip). In a header because a QR job (qr.hip: QrJob) holds one.
#pragma once
#include "qr_internal.h"
enum { SEG_NX = 0, SEG_NA, SEG_F };   // SEG_F: partial X, exchange, apply in one go
struct QrhSeg { int kind, first, count; };

struct QrhP {
  double* Wm; int M, N; long ld, strideW;
  double* Vall; long ldv, strideV;
  double* Tall; long strideT;
  double* taus; long strideTau;
  double* Xp; long strideXp;        // partials of X = V^T C on the next panel's columns: [part][256]
  int* flag;                        // per matrix: fall-back flag
  double* QT; long strideQT;
  double* Xs; long strideXs;        // side work: partials of X per (column block, row chunk): [cb][rc][256]
  int j0;                           // first row / column of the panel
  int pj0;                          // previous panel (-1: none): its reflector is what the side blocks and phase A apply
  int nxp;                          // partials of X to sum in phase A
  int nrow;                         // row workgroups of this launch
  int wide0, nnw, nqb, nrc;         // side work (reflector pj0): nnw column blocks of W from wide0 on, then nqb blocks of Q^T; nrc row chunks each;
                                    // a side workgroup takes TWO adjacent blocks (pairs of W blocks first, then pairs of Q^T blocks)
  int nseg; QrhSeg seg[2];          // the side work of this launch: workgroups nrow.. walk these segments
  int skip_x;                       // phase C: no partial X for the next panel (last panel of an outer block: the block update covers it)
  int na_shift;                     // the side pairs start at this block of W (1: the panel launch's row workgroups take the next panel's columns themselves)
  unsigned long long* Xch; long strideXch;   // the panel launch: the row workgroups' exchange slots (QX_ROW_SLOT tagged words each)
  unsigned long long* Xsx; long strideXsx;   // fused side work: [column block][row chunk] slots of 512 tagged words (rcs_max chunks per block)
  int rcs_max;
  long long* stamps; int stamp_slot; // debug (ND4HIP_QR_STAMPS): 100 MHz wall-clock stamps of workgroup 0, 8 per launch
  int* status;                      // the handle's exchange status word (host-coherent): raised when a spin limit is hit
  int drop_tag;                     // tests only (ND4HIP_TEST_DROP_PUBLISH): the last row workgroup of the panel with this tag skips its first publication
};

// words per row workgroup of the panel launch's exchange (qrh_bc): values [0,256) G, [256,512) X of the next block, [512,768) top-tile
// Gram, 768 "stores are out", [1024,1280) Gram of Q1
constexpr long QX_ROW_SLOT = 2560;

// host side of the multi-workgroup panels: one launch per panel (+ a conditional one for panels taller than the register kernel),
// the previous reflector's side work riding along on the column blocks of W up to near_end (then, optionally, Q^T)
struct QrhHost {
  nd4hip_handle* h; QrhP P; int batch; int nq;          // nq: column blocks of Q^T (0: no Q^T accumulation)
  double *V, *T; long ldv, sV, sT;                        // for qr_narrow_apply
  int pj0 = -1;                                           // the reflector whose narrow / side work is pending (-1: none)
  int init(nd4hip_handle* hh, int nmat, double* W, int M, int N, long ld, long sW, double* Vm, long ldv_, long sV_, double* Tm, long sT_,
           double* taus, long sTau, int* flag, unsigned long long* Xch, long sXch, double* Xp, long sXp, double* QT, long sQT,
           double* Xs, long sXs, unsigned long long* Xsx, long sXsx, int rcs_max);
  void add_seg(int kind, int first, int count);
  int seg_total() const;
  void side_launch();
  int side_of(int pj, int near_end, bool with_qt);
  int panel(int j0, int near_end, bool with_qt, bool skip_x);
  int finish(int near_end, bool with_qt, bool narrow);
  int dump_stamps();
};
