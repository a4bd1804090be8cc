// What the two symmetric eigen-solvers that start from the lower triangle of S share (syev.hip: the default route; syevx.hip:
// selected eigenpairs by bisection and inverse iteration): the entrance step W = 2^-e1 sym(lower(S)) and the reading of its
// per-member word mx. And what the bisection and inverse-iteration kernels of syevx.hip share with the bidiagonal solver built on them
// (bdsvdx.hip: the same kernels on the Golub-Kahan form of a bidiagonal matrix): the constants, the bisection loop, the vector
// stage, the stage stamps and the flag read-back.
#pragma once
#include "nd4hip_internal.h"
#include <cfloat>
#include <cmath>

typedef unsigned long long u64;

constexpr u64 SYEV_MAX_BITS = 0x7FEFFFFFFFFFFFFFull;   // the bits of DBL_MAX: those of Inf and of every |NaN| lie above

// e1 of a member from the bits of max|s_ij| (0 for a zero or non-finite member: those are left alone)
__device__ __forceinline__ int syev_exp(u64 bits) {
  const double m = __longlong_as_double((long long)bits);
  int e = 0;
  if (m > 0.0 && m <= DBL_MAX) (void)frexp(m, &e);
  return e;
}

// steps 1 of syev.hip's route: mx [batch] (zero on entry) receives the bits of max|s_ij| over each lower triangle, W [batch, N, N]
// the mirrored lower triangle times 2^-e1. Two launches on h->stream; S is not written.
int nd4_syev_symm(nd4hip_handle* h, int64_t batch, int N, const double* S, double* W, u64* mx);

// the symmetric tridiagonal reduction (sytrd.hip), for the reduction='tridiag' routes of both solvers: S [batch, N, N] -> F with the
// reflector tails below its subdiagonal, tau [batch, N-1]; d [batch, N], e [batch, N-1] may be NULL. mx [batch] ZERO on entry, as
// above; *flag (zero on entry) is raised for NaN or Inf in a lower triangle. unscale = false leaves d and e, on F's diagonal and
// subdiagonal, scaled by 2^-e1: what syev_shift_chol and stx_prepare take together with mx. Allocates from the caller's workspace
// scope; enqueues only.
int nd4_sytrd(nd4hip_handle* h, int64_t batch, int64_t N, const double* S, double* F, double* tau, double* d, double* e, u64* mx, bool unscale,
              int* flag);

// ---- shared by syevx.hip and bdsvdx.hip ---------------------------------------------------------------------------------------------
constexpr int STX_MAXIT = 128;
constexpr double STX_EPS = 0x1p-52;
constexpr double STX_PIVMIN = 0x1p-1022;

// The bisection of one value: index j of the descending spectrum of a symmetric tridiagonal of order N whose scaled Gershgorin bound
// is gg. negatives(x) = #{i: q_i < 0} of the Sturm sequence at x. From [-g', g'], g' = g (1 + 2^-20), until
// hi - lo <= 2 eps max(|lo|, |hi|) + eps g or the midpoint meets an end, at most STX_MAXIT halvings. Returns the scaled midpoint.
template <class Negatives> __device__ __forceinline__ double stx_bisect_value(double gg, int j, int N, Negatives negatives) {
  const double floor_ = STX_EPS * gg;
  double hi = gg * (1.0 + 0x1p-20), lo = -hi;
  for (int it = 0; it < STX_MAXIT; ++it) {
    const double mid = 0.5 * (lo + hi);
    if (hi - lo <= (2.0 * STX_EPS) * fmax(fabs(lo), fabs(hi)) + floor_ || mid == lo || mid == hi) break;
    if (N - negatives(mid) > j) lo = mid; else hi = mid;
  }
  return 0.5 * (lo + hi);
}

template <class T> int stx_alloc(nd4hip_handle* h, size_t count, T** out) {
  void* p = nullptr;
  ND4_TRY(nd4_ws_alloc(h, sizeof(T) * (count ? count : 1), &p));
  *out = static_cast<T*>(p);
  return 0;
}

// HIP-event time per stage while the profile is enabled: NS stages between NS + 1 marks, written to out [NS] by collect()
template <int NS> struct Nd4StageStamps {
  nd4hip_handle* h; double* out; bool on; int n = 0;
  hipEvent_t ev[NS + 1] = {};
  Nd4StageStamps(nd4hip_handle* hh, double* o) : h(hh), out(o), on(hh->prof_on) {}
  void mark() {
    if (!on || n > NS) return;
    if (hipEventCreate(&ev[n]) != hipSuccess) { on = false; return; }
    (void)hipEventRecord(ev[n++], h->stream);
  }
  void collect() {                                            // after the call's synchronisation
    for (int i = 0; i < NS; ++i) {
      float ms = 0.f;
      out[i] = on && i + 1 < n && hipEventElapsedTime(&ms, ev[i], ev[i + 1]) == hipSuccess ? ms : 0.0;
    }
  }
  ~Nd4StageStamps() { for (int i = 0; i < n; ++i) (void)hipEventDestroy(ev[i]); }
};

// Steps 4-6 of syevx.hip on prepared members (ds, es [batch, N] scaled, g, diag [batch]) whose scaled values lams [batch, k] are
// known: stx_clusters, then three rounds of stx_factor_solve and stx_orth into Z [batch, k, N] (rows = vectors). rng as stx_solve's.
// Allocates from the caller's workspace scope; enqueues only.
int nd4_stx_vectors(nd4hip_handle* h, int64_t batch, int N, int i0, int k, const int* rng, const double* ds, const double* es, const double* g,
                    const int* diag, const double* lams, double* Z);
// `count` ints from the device into the handle's pinned buffer, synchronised; *host stays valid until the next nd4_pinned of the handle
int nd4_stx_read_flags(nd4hip_handle* h, const int* flags, size_t count, const int** host);
