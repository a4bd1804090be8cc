// The Francis iteration of schur_decomp (src/la/schur.js:388-683: schur_qrfrancis_inplace) for gfx950, with the reference's bits.
//
// Everything in the reference's iteration is one of three kinds of work, and each keeps its bits here (the unit is compiled
// without contraction):
//   scalar decisions (is_zero, the double shift, the exceptional shift with its AleaRNG draw, the first column a1 a2 a3,
//       _giv_rot_qr, the pass that resolves real-eigenvalued 2x2 blocks): EVERY lane takes them, from the same values, so all
//       branches are uniform and nothing is broadcast; fp64 '/' and sqrt are correctly rounded on the device.
//   plane rotations giv(i, j, c, s) (:428-451): a row pair of H, a column pair of H and a row pair of Q^T, element by element, so
//       any distribution over lanes has the reference's bits: the lanes take the row pair's columns, the column pair's rows
//       and Q^T's columns of one rotation at once; the lane at column i of the row pair takes the 2x2 intersection, rows first
//       and then columns. The '*= 0.0' that follows a rotation (:586, :674) is folded into the lane that owns that element.
//   recurse(s, e) (:458-496): a nested iteration on the window with its own q, then three products with one lane per output
//       element and a plain sum over ascending j (never the MFMA GEMM, whose order differs).
//
// One workgroup per matrix; nothing waits on another workgroup. The call stack of francis_qr / recurse is an explicit array of
// levels in LDS (s, e, start, end, the stuck counter, the sweep count, the Alea state, the windows); a nested window is at most half
// its parent, so the depth is at most log2 N and the q workspaces take sum_k (N >> k)^2 < N^2 / 3 doubles. H (N x ld), Q^T
// (N x ld) and the q workspace form one arena per matrix, ld = N | 1 (an odd row length keeps a column pair off one LDS bank):
//   LDS tier     the arena is in LDS while it fits: 31 KiB (N <= 41, one wave per matrix, five workgroups per CU) or 79 KiB
//                (N <= 65, four waves, two workgroups per CU: 2 x (79 KiB + the stack) fills the CU's 160 KiB).
//   global tier  any larger N <= 2048: the arena is in global memory (L2-resident up to N of about 500), the same code, four
//                waves. Rotations are applied as they are produced in this tier too: two barriers and a memory round trip per
//                rotation, so one large matrix is correct but slow.
// Every loop is bounded: a francis_qr call at size n stops after 30 max(10, n) sweeps (LAPACK's dlahqr budget; the reference
// allows 1e9 stuck iterations per eigenvalue), raising ND4HIP_EV_FLAG_NOCONV in the matrix's flag word.
#include "nd4hip_internal.h"
#include <cmath>

namespace {

#pragma clang fp contract(off)

constexpr int SCHUR_MAXL = 12;             // levels of francis_qr / recurse: a nested window is at most half its parent and at least 3
constexpr int SCHUR_MAX_N = 2048;
constexpr int SCHUR_LDS_SMALL = 3968;      // doubles: 31 KiB, with the level stack under 32 KiB
constexpr int SCHUR_LDS_BIG = 10112;       // doubles: 79 KiB, with the level stack under 80 KiB
constexpr int SCHUR_THREADS = 256;

struct Alea { double s0, s1, s2, c; };     // alea_rng.js:85-90
struct Level { int s, e, kind, start, end, stuck, sweeps, n, hoff, qoff, ldq; Alea rng; };

__device__ __forceinline__ double alea_next(Alea& r) {
  const double t = 2091639.0 * r.s0 + r.c * 0x1p-32;
  r.s0 = r.s1; r.s1 = r.s2;
  r.c = (double)(int)t;
  r.s2 = t - r.c;
  return r.s2;
}
__device__ __forceinline__ double alea_uniform(Alea& r, double lo, double hi) {   // alea_rng.js:135-142
  const double x = alea_next(r);
  const double s = x + (double)(int)(alea_next(r) * 2097152.0) * 0x1p-53;
  return lo * (1.0 - s) + s * hi;
}

// _giv_rot.js:22-37 (Math.max hands a NaN on)
__device__ __forceinline__ void giv_rot_qr(double a, double b, double& c, double& s, double& norm) {
  const double x = fabs(a), y = fabs(b);
  const double mx = (x != x || y != y) ? NAN : (x > y ? x : y);
  if (mx == 0.0) { c = 1.0; s = 0.0; norm = 0.0; return; }
  a /= mx; b /= mx;
  const double nrm = sqrt(a * a + b * b);
  c = a / nrm; s = b / nrm; norm = nrm * mx;
}

// node 12's Math.hypot of two numbers: an infinity wins, then NaN, else max * sqrt(sum (x / max)^2)
__device__ __forceinline__ double hypot_node12(double a, double b) {
  a = fabs(a); b = fabs(b);
  if (a == INFINITY || b == INFINITY) return INFINITY;
  if (a != a || b != b) return NAN;
  const double mx = a > b ? a : b;
  if (mx == 0.0) return 0.0;
  const double x = a / mx, y = b / mx;
  return sqrt(x * x + y * y) * mx;
}

__device__ __forceinline__ void rot_pair(double* pi, double* pj, double c, double s, bool zero_j) {
  const double Hi = *pi, Hj = *pj;
  *pi = s * Hj + c * Hi;
  const double v = c * Hj - s * Hi;
  *pj = zero_j ? v * 0.0 : v;
}

// the two-sided rotation of rows / columns i < j of the n x n window of H at hoff and of rows i, j of the n x ldq matrix at qoff:
// row pair over columns k0..n-1, column pair over rows 0..m-1. zmode 1: H[j, k0] *= 0.0 afterwards (:586); 2: H[j, i] *= 0.0 (:674)
__device__ __forceinline__ void rotate(double* a, int hoff, int ld, int n, int qoff, int ldq, int i, int j, double c, double s,
                                       int k0, int m, int zmode, int tid, int nt) {
  __syncthreads();                                        // every lane has read what it decided on
  const int nr = n - k0, W = nr + m + n;
  for (int t = tid; t < W; t += nt) {
    if (t < nr) {
      const int k = k0 + t;
      if (k == j) continue;
      if (k != i) { rot_pair(a + hoff + i * ld + k, a + hoff + j * ld + k, c, s, zmode == 1 && t == 0); continue; }
      double* p = a + hoff;                               // the 2x2 intersection: rows first, then columns
      const double hii = p[i * ld + i], hij = p[i * ld + j], hji = p[j * ld + i], hjj = p[j * ld + j];
      const double rii = s * hji + c * hii, rji = c * hji - s * hii;
      const double rij = s * hjj + c * hij, rjj = c * hjj - s * hij;
      p[i * ld + i] = s * rij + c * rii; p[i * ld + j] = c * rij - s * rii;
      const double vji = s * rjj + c * rji;
      p[j * ld + i] = zmode == 2 ? vji * 0.0 : vji; p[j * ld + j] = c * rjj - s * rji;
    } else if (t < nr + m) {
      const int r = t - nr;
      if (r != i && r != j) rot_pair(a + hoff + r * ld + i, a + hoff + r * ld + j, c, s, false);
    } else {
      const int k = t - nr - m;
      rot_pair(a + qoff + i * ldq + k, a + qoff + j * ldq + k, c, s, false);
    }
  }
  __syncthreads();
}

// in place, for each of nvec vectors x (element j at xoff + v * vs + j * es): x[k] = sum over ascending j of q[k, j] x[j], q the
// m x m matrix at qoff (rows of the nested call's q: the reference transposes it first and reads q[j, k], schur.js:468-495)
__device__ __forceinline__ void apply_q(double* a, int qoff, int ldq, int m, int xoff, int es, int vs, int nvec, int tid, int nt) {
  if (m <= nt) {
    const int G = nt / m;                                 // whole vectors per pass, one lane per output element
    for (int v0 = 0; v0 < nvec; v0 += G) {
      const int v = v0 + tid / m, k = tid % m;
      const bool on = tid < G * m && v < nvec;
      double acc = 0.0;
      if (on) for (int j = 0; j < m; j++) acc += a[qoff + k * ldq + j] * a[xoff + v * vs + j * es];
      __syncthreads();
      if (on) a[xoff + v * vs + k * es] = acc;
      __syncthreads();
    }
  } else {                                                // m <= SCHUR_MAX_N / 2 = 4 nt: one vector per pass, up to four elements per lane
    for (int v = 0; v < nvec; v++) {
      double acc[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const int k = tid + r * nt;
        if (k < m) for (int j = 0; j < m; j++) acc[r] += a[qoff + k * ldq + j] * a[xoff + v * vs + j * es];
      }
      __syncthreads();
#pragma unroll
      for (int r = 0; r < 4; r++) { const int k = tid + r * nt; if (k < m) a[xoff + v * vs + k * es] = acc[r]; }
      __syncthreads();
    }
  }
}

// LDSD > 0: the arena of LDSD doubles is in LDS; LDSD == 0: in ws, `arena` doubles per matrix
template <int LDSD>
__global__ __launch_bounds__(SCHUR_THREADS) void schur_francis(int N, int arena, const double* U, const double* H, double* Q, double* T,
                                                               double* ws, Alea seed, int* __restrict__ flags, int* __restrict__ sweeps_out) {
  __shared__ Level stack[SCHUR_MAXL];
  __shared__ double sh[LDSD > 0 ? LDSD : 1];
  const int64_t b = blockIdx.x;
  const int tid = threadIdx.x, nt = blockDim.x;
  const int ld = N | 1, qt0 = N * ld;
  double* a = LDSD > 0 ? sh : ws + b * (int64_t)arena;
  const double TOL = 0x1p-52;

  {   // H and Q^T = U^T into the arena
    const double *u = U + b * N * N, *hh = H + b * N * N;
    for (int e = tid; e < N * N; e += nt) { const int r = e / N, c = e % N; a[r * ld + c] = hh[e]; a[qt0 + c * ld + r] = u[e]; }
  }
  __syncthreads();

  // the current level of francis_qr (uniform over the lanes)
  int L = 0, n = N, hoff = 0, qoff = qt0, ldq = ld, wsoff = 2 * qt0;
  int start = 0, end = N, stuck = 0, sweeps = 0, maxsw = 0, fail = 0;
  Alea rng = seed;
  bool returning = false;

  auto h = [&](int i, int j) -> double { return a[hoff + i * ld + j]; };
  auto is_zero = [&](int i) -> bool {                                         // :418-425
    const double x = h(i, i - 1);
    if (fabs(x) > TOL * (fabs(h(i - 1, i - 1)) + fabs(h(i, i)))) return false;   // a NaN goes on to the zeroing
    __syncthreads();
    if (tid == 0) a[hoff + i * ld + i - 1] = x * 0.0;
    __syncthreads();
    return true;
  };

  for (;;) {
    if (returning) {                                                          // the level's francis_qr has returned
      if (L == 0) break;
      L--;
      const Level p = stack[L];
      __syncthreads();
      const int cq = qoff, cld = ldq, m = n;                                  // the nested call's q
      n = p.n; hoff = p.hoff; qoff = p.qoff; ldq = p.ldq; start = p.start; end = p.end; stuck = p.stuck; sweeps = p.sweeps; rng = p.rng;
      wsoff = cq;
      apply_q(a, cq, cld, m, qoff + p.s * ldq, ldq, 1, n, tid, nt);           // Q' = q^T Q          (:473-479)
      apply_q(a, cq, cld, m, hoff + p.s * ld + p.e, ld, 1, n - p.e, tid, nt); // H' = q^T H, columns e..  (:481-487)
      apply_q(a, cq, cld, m, hoff + p.s, 1, ld, p.s, tid, nt);                // H" = H' q, rows 0..s-1   (:489-495)
      returning = p.kind == 1;                                                // 'return recurse(start, end)' (:507)
      continue;
    }

    // DETECT ZEROS ON THE SUB-DIAGONAL AND SHRINK WORK SIZE ACCORDINGLY (:504-524)
    bool call = false;
    int cs = 0, ce = 0, kind = 0;
    for (bool done = false; !done;) {
      if (end - start < 3) { returning = true; break; }
      if (end - start < (n >> 4)) { call = true; cs = start; ce = end; kind = 1; break; }
      done = false;
      if (is_zero(start + 1)) start += 1; else if (is_zero(end - 1)) end -= 1;
      else if (is_zero(start + 2)) start += 2; else if (is_zero(end - 2)) end -= 2;
      else done = true;
      const int mid = (start + end) >> 1;
      for (int i = start + 2; done && ++i < end - 2;)
        if (is_zero(i)) {
          done = false; call = true; kind = 0;
          if (i > mid) { cs = i; ce = end; end = i; }
          else         { cs = start; ce = i; start = i; }
        }
      if (!done) stuck = 0;
      if (call) break;
    }
    if (returning) continue;
    if (call) {                                                               // recurse(cs, ce) (:458-466)
      const int m = ce - cs, mld = m | 1;
      if (L + 1 >= SCHUR_MAXL || wsoff + m * mld > arena || m > (n >> 1) || m < 3) { fail |= ND4HIP_EV_FLAG_ASSERT; break; }
      if (tid == 0) stack[L] = Level{cs, ce, kind, start, end, stuck, sweeps, n, hoff, qoff, ldq, rng};
      L++;
      hoff += cs * ld + cs; qoff = wsoff; ldq = mld; wsoff += m * mld; n = m;
      for (int e = tid; e < m * m; e += nt) { const int r = e / m, c = e % m; a[qoff + r * ldq + c] = r == c ? 1.0 : 0.0; }
      __syncthreads();
      start = 0; end = n; stuck = 0; sweeps = 0; rng = seed;
      continue;
    }

    if (sweeps >= 30 * (n > 10 ? n : 10)) { fail |= ND4HIP_EV_FLAG_NOCONV; break; }
    stuck += 1; sweeps += 1;
    if (sweeps > maxsw) maxsw = sweeps;

    double tr, det;
    {   // DETERMINE (DOUBLE) SHIFT FROM LOWER RIGHT 2x2 BLOCK (:528-557)
      const int i = end - 2, j = end - 1;
      const double hii = h(i, i), hij = h(i, j), hji = h(j, i), hjj = h(j, j);
      tr = hii + hjj;
      det = hii * hjj - hij * hji;
      if (tr * tr > 4.0 * det) {
        const double sign = tr >= 0.0 ? 1.0 : -1.0;
        const double den = tr + sign * sqrt(tr * tr - 4.0 * det);
        double ev1 = 0.5 * den;
        const double ev2 = det * 2.0 / den;
        if (fabs(hjj - ev1) > fabs(hjj - ev2)) ev1 = ev2;
        tr = ev1 * 2.0;
        det = ev1 * ev1;
      }
      if (stuck % 16 == 0) {
        tr = fabs(hji) + fabs(h(i, end - 3));
        det = tr * tr;
        tr *= alea_uniform(rng, 1.25, 1.75);
      }
    }
    {   // FIRST COLUMN OF THE DOUBLE SHIFTED MATRIX AND ITS TWO ROTATIONS (:560-574)
      const int i = start, j = start + 1, k = start + 2;
      const double hii = h(i, i), hij = h(i, j), hji = h(j, i), hjj = h(j, j), hkj = h(k, j);
      double a1 = hii * hii + hij * hji - tr * hii + det;
      double a2 = hji * (hii + hjj - tr);
      const double a3 = hji * hkj;
      int jj = j;
      for (int row = 0; row < 2; row++) {
        if (a2 != 0.0) {
          double c, s, norm;
          giv_rot_qr(a1, a2, c, s, norm);
          rotate(a, hoff, ld, n, qoff, ldq, i, jj, c, s, i > 0 ? i - 1 : 0, jj + 2 < n ? jj + 2 : n, 0, tid, nt);
          a1 = norm;
        }
        jj = k; a2 = a3;
      }
    }
    // REINSTATE HESSENBERG PROPERTY (:577-589)
    for (int col = start; col < end - 2; col++) {
      const int i = col + 1, J = end < col + 4 ? end : col + 4;
      for (int j = col + 2; j < J; j++) {
        const double Hi = h(i, col), Hj = h(j, col);
        if (Hj == 0.0) continue;
        double c, s, norm;
        giv_rot_qr(Hi, Hj, c, s, norm);
        rotate(a, hoff, ld, n, qoff, ldq, i, j, c, s, col, j + 2 < n ? j + 2 : n, 1, tid, nt);
      }
    }
  }

  // RESOLVE REAL-VALUED 2x2 BLOCKS (:603-676)
  __syncthreads();
  if (!fail)
    for (int j = 1; j < N; j++) {
      const int i = j - 1;
      const double Hji = a[j * ld + i];
      if (Hji == 0.0) continue;
      const double Hii = a[i * ld + i], Hij = a[i * ld + j], Hjj = a[j * ld + j];
      const double A = Hjj - Hii, ABC = A * A + 4.0 * Hij * Hji;
      if (ABC < 0.0) continue;
      double c = 0.0, s = 1.0;
      if (Hij != 0.0) {
        const double Tt = A + (A < 0.0 ? -1.0 : 1.0) * sqrt(ABC), R = Hij * 2.0, TR = hypot_node12(Tt, R);
        s = (R < 0.0 ? -Tt : Tt) / TR;
        c = fabs(R) / TR;
      }
      rotate(a, 0, ld, N, qt0, ld, i, j, c, s, i, j + 1, 2, tid, nt);
    }
  __syncthreads();

  {
    double *q = Q + b * N * N, *t = T + b * N * N;
    for (int e = tid; e < N * N; e += nt) { const int r = e / N, c = e % N; t[e] = a[r * ld + c]; q[e] = a[qt0 + c * ld + r]; }
  }
  if (tid == 0) { if (fail) flags[b] |= fail; sweeps_out[b] = maxsw; }
}

// (s0, s1, s2, c) of a fresh AleaRNG('nd.la.schur_qrfrancis_inplace') (alea_rng.js:37-82), in double arithmetic on the host
double mash(const char* str, double seed) {
  for (; *str; str++) {
    seed += (double)(unsigned char)*str;
    double temp = 0.02519603282416938 * seed;
    seed = (double)(uint32_t)(uint64_t)temp;
    temp -= seed;
    temp *= seed;
    seed = (double)(uint32_t)(uint64_t)temp;
    temp -= seed;
    seed += temp * 4294967296.0;
  }
  return seed;
}
Alea alea_seed() {
  const char* text = "nd.la.schur_qrfrancis_inplace";
  double s[3], t[3];
  s[0] = mash(" ", (double)0xefc8249du); s[1] = mash(" ", s[0]); s[2] = mash(" ", s[1]);
  t[0] = mash(text, s[2]); t[1] = mash(text, t[0]); t[2] = mash(text, t[1]);
  for (int i = 0; i < 3; i++) {
    double x = (double)(uint32_t)(uint64_t)s[i];
    x -= (double)(uint32_t)(uint64_t)t[i];
    x *= 0x1p-32;
    if (x < 0) x += 1.0;
    s[i] = x;
  }
  return Alea{s[0], s[1], s[2], 1.0};
}

int64_t arena_doubles(int64_t N) {
  int64_t a = 2 * N * (N | 1);
  for (int64_t m = N >> 1; m >= 3; m >>= 1) a += m * (m | 1);
  return a;
}

}  // namespace

// the tier nd4_hseqr takes for N under `tier` (0: by size): 1 LDS (31 KiB), 2 LDS (79 KiB), 3 global; 0 if the request cannot be met
static int schur_tier(int64_t N, int tier) {
  const int64_t a = arena_doubles(N);
  const int fit = a <= SCHUR_LDS_SMALL ? 1 : a <= SCHUR_LDS_BIG ? 2 : 3;
  if (tier == 0) return fit;
  if (tier == ND4HIP_SCHUR_TIER_LDS) return fit < 3 ? fit : 0;
  return tier == ND4HIP_SCHUR_TIER_GLOBAL ? 3 : 0;
}

// schur_qrfrancis_inplace on [batch] Hessenberg decompositions (U, H) -> (Q, T) (in place allowed); flags [batch] must be zero on
// entry, sweeps [batch] receives the most sweeps of one francis_qr call per matrix. batch <= 65535 * 32768 (grid x), N <= 2048.
int nd4_hseqr(nd4hip_handle* h, int64_t batch, int64_t N, const double* U, const double* H, double* Q, double* T, int* flags, int* sweeps,
              int tier) {
  if (batch == 0 || N == 0) return 0;
  ND4_CHECK_ARG(N <= SCHUR_MAX_N, "nd4hip_dhseqr_batched: N <= %d (one workgroup per matrix)", SCHUR_MAX_N);
  const int t = schur_tier(N, tier);
  ND4_CHECK_ARG(t != 0, "nd4hip_dhseqr_batched: tier %d is not available at N = %lld", tier, (long long)N);
  static const Alea seed = alea_seed();
  const int arena = (int)arena_doubles(N);
  const dim3 grid((unsigned)batch);
  if (t == 1) {
    hipLaunchKernelGGL(schur_francis<SCHUR_LDS_SMALL>, grid, dim3(64), 0, h->stream, (int)N, SCHUR_LDS_SMALL, U, H, Q, T, (double*)nullptr, seed, flags, sweeps);
  } else if (t == 2) {
    hipLaunchKernelGGL(schur_francis<SCHUR_LDS_BIG>, grid, dim3(SCHUR_THREADS), 0, h->stream, (int)N, SCHUR_LDS_BIG, U, H, Q, T, (double*)nullptr, seed, flags, sweeps);
  } else {
    Nd4WsScope scope(h);
    void* p = nullptr;
    ND4_TRY(nd4_ws_alloc(h, sizeof(double) * (size_t)batch * (size_t)arena, &p));
    hipLaunchKernelGGL(schur_francis<0>, grid, dim3(SCHUR_THREADS), 0, h->stream, (int)N, arena, U, H, Q, T, static_cast<double*>(p), seed, flags, sweeps);
  }
  ND4_HIP(hipGetLastError());
  return 0;
}

// how many matrices of size N one nd4_hseqr call may take so that the global tier's arenas stay within 1 GiB
int64_t nd4_hseqr_chunk(int64_t N) {
  const int64_t per = 8 * arena_doubles(N), cap = (int64_t(1) << 30) / (per > 0 ? per : 1);
  return cap < 1 ? 1 : cap > 32768 ? 32768 : cap;
}
