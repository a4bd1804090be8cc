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
