// What the two symmetric eigen-solvers that start from the lower triangle of S share (syev.hip: the default route; syevx.hip:
// selected eigenpairs by bisection and inverse iteration): the entrance step W = 2^-e1 sym(lower(S)) and the reading of its
// per-member word mx.
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
