// relpose.hip -- relative pose from matches (src/Tracker.py:356-360 estimatePose, :458-548
// track_reference_frame, :571-610 compute_pusdo_depth_np; src/utils/utils_geom.py:140-207).  All float64.
//
//   k_fivept            S minimal samples -> up to 10 essential matrices each (Nister's five-point solver).
//                       One 16-lane group per sample, four samples per wave, 16 per workgroup.  Each lane owns
//                       one matrix row, pivot rows travel by __shfl inside the group:
//                         5 x 9 epipolar system, Gauss-Jordan with complete pivoting (lanes 0-4) -> a null-space
//                         basis X, Y, Z, W, orthonormalised, parked in LDS;
//                         lanes 0-8 expand one entry each of 2 E E^T E - tr(E E^T) E, lane 9 det E, over
//                         E = x X + y Y + z Z + W: 20 monomial coefficients a lane (the 10 x 20 matrix is 40
//                         VGPRs a lane);
//                         Gauss-Jordan with row pivoting on the leading 10 x 10 block; rows e..j give the 3 x 3
//                         polynomial matrix B(z), det B a degree-10 polynomial;
//                         real roots through the derivative chain: the roots of p^(k+1) cut the line into
//                         intervals on which p^(k) is monotone, lane r bisects interval r, so every level is
//                         one parallel step and the roots come out in ascending order, one per lane; two
//                         guarded Newton steps polish the last level;
//                         lane r evaluates B(z_r), takes (x, y, 1) from the best-conditioned pair of rows,
//                         polishes (x, y, z) by three Gauss-Newton steps on the ten constraints and writes
//                         E / |E|_F to hypothesis 10 s + r.
//   k_score             Sampson inlier counts of all hypotheses on v_mfma_f64_16x16x4_f64: a wave holds 16
//                       hypotheses as B operands (columns), walks the matches 16 at a time as A operands
//                       (rows): a = E x1 is three products of (x1, y1, 1, 0), b0, b1 of E^T x2 two products of
//                       (x2, y2, 1, 0).  D register r of lane l is match 4 r + l / 16, hypothesis l % 16.  The
//                       matches pass through LDS once per workgroup.  Counts stay in registers, are summed over
//                       the four lane groups by __shfl_xor and published as count << 32 | (0xFFFFFFFF - h) by a
//                       64-bit atomicMax: highest count, then lowest index, whatever the schedule.
//   k_relpose_finalize  one workgroup: mask and count of the best E, E = U diag(s, s, 0) V^T by one-sided
//                       Jacobi, the four (R, t) candidates, the cheirality vote over the inliers, R, t, Trc.
//   k_triangulate       one thread per match: the 4 x 4 DLT system, its smallest right singular vector by
//                       one-sided (Hestenes) Jacobi on A itself, and the two projections K (Rcw p + tcw).
//   k_paint_*           the pseudo-depth map: clear owners, atomicMax of i + 1 over each point's pixels, resolve.
// Integer atomics only, vector stores only.
#include "jacobi.h"
#include "pnr_internal.h"

namespace pnr {

namespace {

typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int64_t kMaxMatches = 1 << 20;
constexpr int64_t kMaxSamples = 1 << 16;
constexpr double kMaxDepth = 50.0;  // cv2.recoverPose's distanceThresh

// ---- small dense helpers --------------------------------------------------------------------------------
template <typename T, int N>
__device__ __forceinline__ T sel(const T (&a)[N], int i) {
  T v = a[0];
#pragma unroll
  for (int c = 1; c < N; ++c) v = c == i ? a[c] : v;
  return v;
}

// DLT of utils_geom.py:140-147: rows x P[2] - P[0], y P[2] - P[1] of both views; X = the right singular vector
// of the smallest singular value.  P1, P2: 3 x 4 row-major.
__device__ __forceinline__ void dlt_point(const double* P1, const double* P2, double x1, double y1, double x2,
                                          double y2, double (&X)[4]) {
  double A[4][4], V[4][4];
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    A[0][c] = x1 * P1[8 + c] - P1[c];
    A[1][c] = y1 * P1[8 + c] - P1[4 + c];
    A[2][c] = x2 * P2[8 + c] - P2[c];
    A[3][c] = y2 * P2[8 + c] - P2[4 + c];
  }
  jacobi<4>(A, V);
  double best = 0.0;
  int at = 0;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const double n = A[0][c] * A[0][c] + A[1][c] * A[1][c] + A[2][c] * A[2][c] + A[3][c] * A[3][c];
    if (c == 0 || n < best) {
      best = n;
      at = c;
    }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) X[i] = sel(V[i], at);
}

__device__ __forceinline__ double sampson(const double* E, double x1, double y1, double x2, double y2) {
  const double a0 = E[0] * x1 + E[1] * y1 + E[2], a1 = E[3] * x1 + E[4] * y1 + E[5], a2 = E[6] * x1 + E[7] * y1 + E[8];
  const double b0 = E[0] * x2 + E[3] * y2 + E[6], b1 = E[1] * x2 + E[4] * y2 + E[7];
  const double num = x2 * a0 + y2 * a1 + a2;
  return num * num / (a0 * a0 + a1 * a1 + b0 * b0 + b1 * b1);
}

// ---- the sample draw (include/pnr.h states the rule) ------------------------------------------------------
__host__ __device__ __forceinline__ uint32_t draw_hash(uint32_t seed, uint32_t s, uint32_t d, uint32_t retry) {
  unsigned long long z = ((unsigned long long)seed << 32 | s) * 0x9E3779B97F4A7C15ull +
                         ((unsigned long long)d << 32 | retry) * 0xD1B54A32D192ED03ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z ^= z >> 31;
  return (uint32_t)(z >> 32);
}

__device__ __forceinline__ void draw_sample(uint32_t seed, uint32_t s, uint32_t L, int (&idx)[5]) {
#pragma unroll
  for (int d = 0; d < 5; ++d) {
    uint32_t pick = 0;
    for (uint32_t retry = 0;; ++retry) {
      // after 64 refused draws: the next index up, cyclically (L >= 5 ends it)
      pick = retry < 64 ? (uint32_t)(((unsigned long long)draw_hash(seed, s, d, retry) * L) >> 32) : (pick + 1) % L;
      bool fresh = true;
#pragma unroll
      for (int e = 0; e < 5; ++e) fresh = fresh && (e >= d || idx[e] != (int)pick);
      if (fresh) break;
    }
    idx[d] = (int)pick;
  }
}

// ---- polynomials in (x, y, z, 1) = variables 0..3 ---------------------------------------------------------
// quadratic coefficient of variables u <= v
__host__ __device__ constexpr int quad_at(int u, int v) {
  return u <= v ? u * 4 - u * (u - 1) / 2 + (v - u) : v * 4 - v * (v - 1) / 2 + (u - v);
}
// column of the cubic monomial u v w in Nister's order:
//   x3 y3 x2y xy2 x2z x2 y2z y2 xyz xy | xz2 xz x yz2 yz y z3 z2 z 1
__host__ __device__ constexpr int cubic_at(int u, int v, int w) {
  const int lo = u < v ? (u < w ? u : w) : (v < w ? v : w);
  const int hi = u > v ? (u > w ? u : w) : (v > w ? v : w);
  const int mid = u + v + w - lo - hi;
  switch (lo * 16 + mid * 4 + hi) {
    case 0: return 0;    // x x x
    case 21: return 1;   // y y y
    case 1: return 2;    // x x y
    case 5: return 3;    // x y y
    case 2: return 4;    // x x z
    case 3: return 5;    // x x 1
    case 22: return 6;   // y y z
    case 23: return 7;   // y y 1
    case 6: return 8;    // x y z
    case 7: return 9;    // x y 1
    case 10: return 10;  // x z z
    case 11: return 11;  // x z 1
    case 15: return 12;  // x 1 1
    case 26: return 13;  // y z z
    case 27: return 14;  // y z 1
    case 31: return 15;  // y 1 1
    case 42: return 16;  // z z z
    case 43: return 17;  // z z 1
    case 47: return 18;  // z 1 1
    default: return 19;  // 1 1 1
  }
}

__device__ __forceinline__ void mul_ll(const double (&a)[4], const double (&b)[4], double (&q)[10]) {
#pragma unroll
  for (int u = 0; u < 4; ++u)
#pragma unroll
    for (int v = 0; v < 4; ++v) q[quad_at(u, v)] += a[u] * b[v];
}
__device__ __forceinline__ void mul_ql(const double (&q)[10], const double (&l)[4], double sgn, double (&c)[20]) {
#pragma unroll
  for (int u = 0; u < 4; ++u)
#pragma unroll
    for (int v = u; v < 4; ++v)
#pragma unroll
      for (int w = 0; w < 4; ++w) c[cubic_at(u, v, w)] += sgn * q[quad_at(u, v)] * l[w];
}
// out += sgn a b for univariate polynomials (ascending powers)
template <int NA, int NB>
__device__ __forceinline__ void pmul(const double (&a)[NA], const double (&b)[NB], double sgn,
                                     double (&out)[NA + NB - 1]) {
#pragma unroll
  for (int i = 0; i < NA; ++i)
#pragma unroll
    for (int j = 0; j < NB; ++j) out[i + j] += sgn * a[i] * b[j];
}
template <int N>
__device__ __forceinline__ double horner(const double (&a)[N], double z) {
  double v = a[N - 1];
#pragma unroll
  for (int i = N - 2; i >= 0; --i) v = fma(v, z, a[i]);
  return v;
}

// (10 - D)-th derivative of p, degree D
template <int D>
__device__ __forceinline__ double deriv_at(const double (&p)[11], double z) {
  constexpr int k = 10 - D;
  double v = 0.0;
#pragma unroll
  for (int i = D; i >= 0; --i) {
    double ff = 1.0;  // (i + k)! / i!
#pragma unroll
    for (int m = 1; m <= k; ++m) ff *= (double)(i + m);
    v = fma(v, z, p[i + k] * ff);
  }
  return v;
}

__device__ __forceinline__ int nth_set(uint32_t mask, int n) {
  int at = 0;
#pragma unroll
  for (int b = 0; b < 16; ++b) {
    const bool set = (mask >> b) & 1u;
    at = (set && n == 0) ? b : at;
    n -= set ? 1 : 0;
  }
  return at;
}

// One level of the derivative chain.  In: lanes 0..m-1 of the group hold the m real roots of the degree D - 1
// derivative, ascending (crit).  Out: lanes 0..m'-1 hold the m' real roots of the degree D one.
template <int D>
__device__ __forceinline__ void chain_level(const double (&p)[11], double bound, int gl, int gshift, double& crit,
                                            int& m) {
  const double prev = __shfl(crit, (gl + 15) & 15, 16);
  double lo = gl == 0 ? -bound : prev;
  double hi = gl >= m ? bound : crit;
  const double flo = deriv_at<D>(p, lo), fhi = deriv_at<D>(p, hi);
  const bool has = gl <= m && ((flo < 0.0 && fhi > 0.0) || (flo > 0.0 && fhi < 0.0));
  if (has) {
    for (int it = 0; it < 200; ++it) {
      const double mid = 0.5 * (lo + hi);
      if (!(mid > lo && mid < hi)) break;
      const double fm = deriv_at<D>(p, mid);
      if ((fm < 0.0) == (flo < 0.0)) lo = mid; else hi = mid;
    }
  }
  double root = 0.5 * (lo + hi);
  if (D == 10 && has) {  // polish: Newton steps that stay inside the bracket
#pragma unroll
    for (int it = 0; it < 2; ++it) {
      const double f = deriv_at<10>(p, root);
      double df = 0.0;
#pragma unroll
      for (int i = 10; i >= 1; --i) df = fma(df, root, p[i] * (double)i);
      const double nr = root - f / df;
      if (nr >= lo && nr <= hi) root = nr;
    }
  }
  const uint32_t mask = (uint32_t)(__ballot(has) >> gshift) & 0xFFFFu;
  m = __popc(mask);
  crit = __shfl(root, nth_set(mask, gl), 16);
}

template <int D>
struct Chain {
  static __device__ __forceinline__ void run(const double (&p)[11], double bound, int gl, int gshift, double& crit,
                                             int& m) {
    Chain<D - 1>::run(p, bound, gl, gshift, crit, m);
    chain_level<D>(p, bound, gl, gshift, crit, m);
  }
};
template <>
struct Chain<0> {
  static __device__ __forceinline__ void run(const double (&)[11], double, int, int, double&, int& m) { m = 0; }
};

// highest |value| of the group, ties to the lowest lane; every lane of the group gets (value, lane, tag)
__device__ __forceinline__ void group_argmax(double& best, int& lane, int& tag) {
#pragma unroll
  for (int s = 1; s < 16; s <<= 1) {
    const double ob = __shfl_xor(best, s, 16);
    const int ol = __shfl_xor(lane, s, 16), ot = __shfl_xor(tag, s, 16);
    if (ob > best || (ob == best && ol < lane)) {
      best = ob;
      lane = ol;
      tag = ot;
    }
  }
}

// C = A B, A B^T or A^T B for 3 x 3 row-major
__device__ __forceinline__ void mm3(const double* A, const double* B, bool ta, bool tb, double* C) {
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      double v = 0.0;
#pragma unroll
      for (int k = 0; k < 3; ++k) v += (ta ? A[3 * k + i] : A[3 * i + k]) * (tb ? B[3 * j + k] : B[3 * k + j]);
      C[3 * i + j] = v;
    }
}

// Gauss-Newton on the ten constraints over (x, y, z), E = x X + y Y + z Z + W: the root of the degree-10
// polynomial carries the rounding of two eliminations, the constraints themselves do not
__device__ __forceinline__ void polish(const double (&N)[4][9], double (&v)[3]) {
  for (int it = 0; it < 3; ++it) {
    double E[9], G[9], EG[9], r[10], J[3][10];
#pragma unroll
    for (int c = 0; c < 9; ++c) E[c] = v[0] * N[0][c] + v[1] * N[1][c] + v[2] * N[2][c] + N[3][c];
    mm3(E, E, false, true, G);  // E E^T
    mm3(G, E, false, false, EG);
    const double tr = G[0] + G[4] + G[8];
    double cof[9];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const int i1 = (i + 1) % 3, i2 = (i + 2) % 3, j1 = (j + 1) % 3, j2 = (j + 2) % 3;
        cof[3 * i + j] = E[3 * i1 + j1] * E[3 * i2 + j2] - E[3 * i1 + j2] * E[3 * i2 + j1];
      }
#pragma unroll
    for (int c = 0; c < 9; ++c) r[c] = 2.0 * EG[c] - tr * E[c];
    r[9] = E[0] * cof[0] + E[1] * cof[1] + E[2] * cof[2];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      double BE[9], T1[9], T2[9], T3[9];
      mm3(N[a], E, false, true, BE);   // B E^T
      mm3(BE, E, false, false, T1);    // B E^T E
      mm3(E, N[a], false, true, T2);   // E B^T
      mm3(T2, E, false, false, T3);    // E B^T E
      mm3(G, N[a], false, false, T2);  // E E^T B
      const double trb = BE[0] + BE[4] + BE[8];
      double dd = 0.0;
#pragma unroll
      for (int c = 0; c < 9; ++c) {
        J[a][c] = 2.0 * (T1[c] + T3[c] + T2[c]) - 2.0 * trb * E[c] - tr * N[a][c];
        dd += cof[c] * N[a][c];
      }
      J[a][9] = dd;
    }
    double M[3][3], g[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
#pragma unroll
      for (int b = 0; b < 3; ++b) {
        double m = 0.0;
#pragma unroll
        for (int c = 0; c < 10; ++c) m += J[a][c] * J[b][c];
        M[a][b] = m;
      }
      double q = 0.0;
#pragma unroll
      for (int c = 0; c < 10; ++c) q += J[a][c] * r[c];
      g[a] = q;
    }
    const double c00 = M[1][1] * M[2][2] - M[1][2] * M[2][1], c01 = M[1][2] * M[2][0] - M[1][0] * M[2][2],
                 c02 = M[1][0] * M[2][1] - M[1][1] * M[2][0];
    const double det = M[0][0] * c00 + M[0][1] * c01 + M[0][2] * c02;
    const double d0 = (g[0] * c00 + g[1] * (M[0][2] * M[2][1] - M[0][1] * M[2][2]) + g[2] * (M[0][1] * M[1][2] - M[0][2] * M[1][1])) / det;
    const double d1 = (g[0] * c01 + g[1] * (M[0][0] * M[2][2] - M[0][2] * M[2][0]) + g[2] * (M[0][2] * M[1][0] - M[0][0] * M[1][2])) / det;
    const double d2 = (g[0] * c02 + g[1] * (M[0][1] * M[2][0] - M[0][0] * M[2][1]) + g[2] * (M[0][0] * M[1][1] - M[0][1] * M[1][0])) / det;
    const double step = fabs(d0) + fabs(d1) + fabs(d2), size = 1.0 + fabs(v[0]) + fabs(v[1]) + fabs(v[2]);
    if (!(step < 1e-2 * size)) break;  // only a small correction is a polish (also ends on NaN)
    v[0] -= d0;
    v[1] -= d1;
    v[2] -= d2;
  }
}

struct FiveArgs {
  const double* x1;  // (n,2) points of the first view
  const double* x2;  // (n,2) points of the second view
  int32_t L;         // > 0: draw 5 of L matches per sample; 0: sample s is points 5 s .. 5 s + 4
  int32_t S;
  uint32_t seed;
  int32_t* samples;  // (S,5), L > 0
  double* cand;      // (10 S, 9)
  uint8_t* valid;    // (10 S)
  unsigned long long* best;  // cleared for k_score (may be null)
};

__global__ __launch_bounds__(256) void k_fivept(FiveArgs a) {
  __shared__ double s_basis[16][36];
  const int t = threadIdx.x, gl = t & 15, g = t >> 4, gshift = t & 48;
  const int s_raw = blockIdx.x * 16 + g;
  const bool live = s_raw < a.S;
  const int s = live ? s_raw : a.S - 1;  // an idle group repeats the last sample and writes nothing
  if (a.best && blockIdx.x == 0 && t == 0) *a.best = 0ull;

  int idx[5] = {-1, -1, -1, -1, -1};
  if (a.L > 0) {
    draw_sample(a.seed, (uint32_t)s, (uint32_t)a.L, idx);
    if (live && gl < 5) a.samples[5 * s + gl] = sel(idx, gl);
  } else {
#pragma unroll
    for (int d = 0; d < 5; ++d) idx[d] = 5 * s + d;
  }

  // ---- 5 x 9 epipolar rows: x2^T E x1 = 0 over e = E row-major
  double row9[9];
  {
    const int n = sel(idx, gl < 5 ? gl : 0);
    const double x1 = a.x1[2 * (int64_t)n], y1 = a.x1[2 * (int64_t)n + 1];
    const double x2 = a.x2[2 * (int64_t)n], y2 = a.x2[2 * (int64_t)n + 1];
    const double r[9] = {x2 * x1, x2 * y1, x2, y2 * x1, y2 * y1, y2, x1, y1, 1.0};
#pragma unroll
    for (int c = 0; c < 9; ++c) row9[c] = gl < 5 ? r[c] : 0.0;
  }
  bool ok = true;
  int prow[5], pcol[5];
  uint32_t colmask = 0;
  bool used = false;
  double scale = 0.0;
#pragma unroll
  for (int k = 0; k < 5; ++k) {
    double best = -1.0;
    int bc = 0, bl = gl;
#pragma unroll
    for (int c = 0; c < 9; ++c) {
      const double v = fabs(row9[c]);
      if (!((colmask >> c) & 1u) && v > best) {
        best = v;
        bc = c;
      }
    }
    if (gl >= 5 || used) best = -1.0;
    group_argmax(best, bl, bc);
    if (k == 0) scale = best;
    if (!(best > 1e-10 * scale)) ok = false;  // rank-deficient (or NaN)
    double pr[9];
#pragma unroll
    for (int c = 0; c < 9; ++c) pr[c] = __shfl(row9[c], bl, 16);
    const double inv = ok ? 1.0 / sel(pr, bc) : 0.0;
    const double f = sel(row9, bc);
#pragma unroll
    for (int c = 0; c < 9; ++c) {
      const double pn = pr[c] * inv;
      double v = gl == bl ? pn : row9[c] - f * pn;
      if (c == bc) v = gl == bl ? 1.0 : 0.0;
      row9[c] = v;
    }
    used = used || gl == bl;
    colmask |= 1u << bc;
    prow[k] = bl;
    pcol[k] = bc;
  }
  // null space: free column f_j -> 1, pivot column pcol[k] -> -row_k[f_j]
  {
    double* nb = s_basis[g];
    for (int i = gl; i < 36; i += 16) nb[i] = 0.0;
    __syncthreads();
    const uint32_t free_mask = ~colmask & 0x1FFu;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int fj = nth_set(free_mask, j);
      const double mine = sel(row9, fj);
#pragma unroll
      for (int k = 0; k < 5; ++k) {
        const double v = __shfl(mine, prow[k], 16);
        if (gl == 0) nb[9 * j + pcol[k]] = -v;
      }
      if (gl == 0) nb[9 * j + fj] = 1.0;
    }
    __syncthreads();
  }
  double N[4][9];
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int c = 0; c < 9; ++c) N[j][c] = s_basis[g][9 * j + c];
  // modified Gram-Schmidt (every lane alike)
#pragma unroll
  for (int j = 0; j < 4; ++j) {
#pragma unroll
    for (int i = 0; i < j; ++i) {
      double d = 0.0;
#pragma unroll
      for (int c = 0; c < 9; ++c) d += N[i][c] * N[j][c];
#pragma unroll
      for (int c = 0; c < 9; ++c) N[j][c] -= d * N[i][c];
    }
    double n2 = 0.0;
#pragma unroll
    for (int c = 0; c < 9; ++c) n2 += N[j][c] * N[j][c];
    const double inv = 1.0 / sqrt(n2);
#pragma unroll
    for (int c = 0; c < 9; ++c) N[j][c] *= inv;
  }
  __syncthreads();
  if (gl == 0) {
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int c = 0; c < 9; ++c) s_basis[g][9 * j + c] = N[j][c];
  }
  __syncthreads();

  // ---- the ten cubic constraints, one per lane
  double row[20];
#pragma unroll
  for (int c = 0; c < 20; ++c) row[c] = 0.0;
  {
    const double* nb = s_basis[g];
    auto lin = [&](int i, int j, double (&l)[4]) {
#pragma unroll
      for (int b = 0; b < 4; ++b) l[b] = nb[9 * b + 3 * i + j];
    };
    if (gl < 9) {
      const int i = gl / 3, j = gl % 3;
      double tr[10];
#pragma unroll
      for (int c = 0; c < 10; ++c) tr[c] = 0.0;
#pragma unroll
      for (int l = 0; l < 3; ++l) {
        double q[10], lj[4];
#pragma unroll
        for (int c = 0; c < 10; ++c) q[c] = 0.0;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          double eik[4], elk[4];
          lin(i, k, eik);
          lin(l, k, elk);
          mul_ll(eik, elk, q);   // (E E^T)_il
          mul_ll(elk, elk, tr);  // tr(E E^T)
        }
        lin(l, j, lj);
        mul_ql(q, lj, 2.0, row);
      }
      double eij[4];
      lin(i, j, eij);
      mul_ql(tr, eij, -1.0, row);
    } else if (gl == 9) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {  // det E along the first row
        const int c1 = (c + 1) % 3, c2 = (c + 2) % 3;
        double q[10], a1[4], a2[4], b1[4], b2[4], e0[4];
#pragma unroll
        for (int m = 0; m < 10; ++m) q[m] = 0.0;
        lin(1, c1, a1);
        lin(2, c2, a2);
        lin(1, c2, b1);
        lin(2, c1, b2);
#pragma unroll
        for (int m = 0; m < 4; ++m) b1[m] = -b1[m];
        mul_ll(a1, a2, q);
        mul_ll(b1, b2, q);
        lin(0, c, e0);
        mul_ql(q, e0, 1.0, row);
      }
    }
  }
  {
    double mx = 0.0;
#pragma unroll
    for (int c = 0; c < 20; ++c) mx = fmax(mx, fabs(row[c]));
    const double inv = mx > 0.0 ? 1.0 / mx : 0.0;
#pragma unroll
    for (int c = 0; c < 20; ++c) row[c] *= inv;
  }
  // ---- Gauss-Jordan on the leading 10 x 10 block, row pivoting
  int owner[10];
  int mypiv = -1;
#pragma unroll
  for (int k = 0; k < 10; ++k) {
    double best = (gl < 10 && mypiv < 0) ? fabs(row[k]) : -1.0;
    int bl = gl, tag = 0;
    group_argmax(best, bl, tag);
    if (!(best > 1e-14)) ok = false;
    const double inv = ok ? 1.0 / __shfl(row[k], bl, 16) : 0.0;
    const double f = row[k];
#pragma unroll
    for (int c = k; c < 20; ++c) {
      const double pn = __shfl(row[c], bl, 16) * inv;
      row[c] = gl == bl ? pn : row[c] - f * pn;
    }
    row[k] = gl == bl ? 1.0 : 0.0;
    if (gl == bl) mypiv = k;
    owner[k] = bl;
  }
  // ---- B(z): rows e - z f, g - z h, i - z j over the columns (x, y, 1)
  double Bx[3][4], By[3][4], B1[3][5];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    double hi[10], lo[10];  // the pair's right halves: [xz2 xz x yz2 yz y z3 z2 z 1]
#pragma unroll
    for (int c = 0; c < 10; ++c) {
      hi[c] = __shfl(row[10 + c], owner[4 + 2 * r], 16);
      lo[c] = __shfl(row[10 + c], owner[5 + 2 * r], 16);
    }
    Bx[r][0] = hi[2];
    Bx[r][1] = hi[1] - lo[2];
    Bx[r][2] = hi[0] - lo[1];
    Bx[r][3] = -lo[0];
    By[r][0] = hi[5];
    By[r][1] = hi[4] - lo[5];
    By[r][2] = hi[3] - lo[4];
    By[r][3] = -lo[3];
    B1[r][0] = hi[9];
    B1[r][1] = hi[8] - lo[9];
    B1[r][2] = hi[7] - lo[8];
    B1[r][3] = hi[6] - lo[7];
    B1[r][4] = -lo[6];
  }
  // det B = Bx0 (By1 B12 - B11 By2) - By0 (Bx1 B12 - B11 Bx2) + B10 (Bx1 By2 - By1 Bx2)
  double p[11];
#pragma unroll
  for (int c = 0; c < 11; ++c) p[c] = 0.0;
  {
    double m7[8], m6[7];
#pragma unroll
    for (int c = 0; c < 8; ++c) m7[c] = 0.0;
    pmul<4, 5>(By[1], B1[2], 1.0, m7);
    pmul<5, 4>(B1[1], By[2], -1.0, m7);
    pmul<4, 8>(Bx[0], m7, 1.0, p);
#pragma unroll
    for (int c = 0; c < 8; ++c) m7[c] = 0.0;
    pmul<4, 5>(Bx[1], B1[2], 1.0, m7);
    pmul<5, 4>(B1[1], Bx[2], -1.0, m7);
    pmul<4, 8>(By[0], m7, -1.0, p);
#pragma unroll
    for (int c = 0; c < 7; ++c) m6[c] = 0.0;
    pmul<4, 4>(Bx[1], By[2], 1.0, m6);
    pmul<4, 4>(By[1], Bx[2], -1.0, m6);
    pmul<5, 7>(B1[0], m6, 1.0, p);
  }
  double bound = 0.0;
  {
    double mx = 0.0;
#pragma unroll
    for (int c = 0; c < 11; ++c) mx = fmax(mx, fabs(p[c]));
    if (!(mx > 0.0) || !(mx < 1e300)) ok = false;
    const double inv = ok ? 1.0 / mx : 0.0;
#pragma unroll
    for (int c = 0; c < 11; ++c) p[c] = ok ? p[c] * inv : (c == 0 ? 1.0 : 0.0);
    // Cauchy: every root (of p and, by Gauss-Lucas, of its derivatives) lies within 1 + max |p_i / p_10|
    bound = fabs(p[10]) > 1e-10 ? 1.0 + 1.0 / fabs(p[10]) : 1e10;
  }
  double z = 0.0;
  int nroots = 0;
  Chain<10>::run(p, bound, gl, gshift, z, nroots);

  // ---- lane r: back-substitute root r
  double E[9];
  bool good = ok && gl < nroots;
  {
    double M[3][3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      M[r][0] = horner(Bx[r], z);
      M[r][1] = horner(By[r], z);
      M[r][2] = horner(B1[r], z);
    }
    double n[3] = {0.0, 0.0, 0.0}, best = -1.0;
#pragma unroll
    for (int r = 0; r < 3; ++r) {  // the null vector of B(z) from the best-conditioned pair of rows
      const int r1 = (r + 1) % 3, r2 = (r + 2) % 3;
      const double c0 = M[r1][1] * M[r2][2] - M[r1][2] * M[r2][1];
      const double c1 = M[r1][2] * M[r2][0] - M[r1][0] * M[r2][2];
      const double c2 = M[r1][0] * M[r2][1] - M[r1][1] * M[r2][0];
      const double nn = c0 * c0 + c1 * c1 + c2 * c2;
      if (nn > best) {
        best = nn;
        n[0] = c0;
        n[1] = c1;
        n[2] = c2;
      }
    }
    if (fabs(n[2]) > 1e-8 * (fabs(n[0]) + fabs(n[1]))) {  // a finite (x, y): polish it
      double v[3] = {n[0] / n[2], n[1] / n[2], z};
      polish(N, v);
      n[0] = v[0];
      n[1] = v[1];
      n[2] = 1.0;
      z = v[2];
    }
    double fro = 0.0;
#pragma unroll
    for (int c = 0; c < 9; ++c) {
      E[c] = n[0] * N[0][c] + n[1] * N[1][c] + n[2] * (z * N[2][c] + N[3][c]);
      fro += E[c] * E[c];
    }
    const double inv = 1.0 / sqrt(fro);
    good = good && fro > 0.0 && inv > 0.0 && inv < 1e300;  // false for NaN and infinity
#pragma unroll
    for (int c = 0; c < 9; ++c) E[c] = good ? E[c] * inv : 0.0;
  }
  if (live && gl < 10) {
    const int64_t h = 10 * (int64_t)s + gl;
#pragma unroll
    for (int c = 0; c < 9; ++c) a.cand[9 * h + c] = E[c];
    a.valid[h] = good ? 1 : 0;
  }
}

// ---- scoring ------------------------------------------------------------------------------------------------
constexpr int kStage = 256;  // matches per LDS stage

__global__ __launch_bounds__(256) void k_score(const double* __restrict__ x1, const double* __restrict__ x2, int32_t L,
                                               const double* __restrict__ cand, const uint8_t* __restrict__ valid,
                                               int32_t Hn, double thr2, unsigned long long* best) {
  __shared__ double sm[kStage][4];  // x1, y1, x2, y2
  const int t = threadIdx.x, lane = t & 63, j = lane & 15, kq = lane >> 4;
  const int w = __builtin_amdgcn_readfirstlane(t >> 6);
  const int h = (blockIdx.x * 4 + w) * 16 + j;
  const bool hv = h < Hn && valid[h];
  double e[9];
#pragma unroll
  for (int c = 0; c < 9; ++c) e[c] = hv ? cand[9 * (int64_t)h + c] : 0.0;
  // B operands (k = kq, column = hypothesis j): row r of E for a_r, column c of E for b_c
  double ba[3], bb[2];
#pragma unroll
  for (int r = 0; r < 3; ++r) ba[r] = kq == 0 ? e[3 * r] : kq == 1 ? e[3 * r + 1] : kq == 2 ? e[3 * r + 2] : 0.0;
#pragma unroll
  for (int c = 0; c < 2; ++c) bb[c] = kq == 0 ? e[c] : kq == 1 ? e[3 + c] : kq == 2 ? e[6 + c] : 0.0;
  const f64x4 zero = {0.0, 0.0, 0.0, 0.0};
  int count = 0;
  for (int base = 0; base < L; base += kStage) {
    __syncthreads();
    {
      const int n = base + t;
      const bool in = n < L;
      sm[t][0] = in ? x1[2 * (int64_t)n] : 0.0;
      sm[t][1] = in ? x1[2 * (int64_t)n + 1] : 0.0;
      sm[t][2] = in ? x2[2 * (int64_t)n] : 0.0;
      sm[t][3] = in ? x2[2 * (int64_t)n + 1] : 0.0;
    }
    __syncthreads();
    const int here = L - base < kStage ? L - base : kStage;
    for (int m0 = 0; m0 < here; m0 += 16) {
      // A operands (row = match m0 + j, k = kq)
      const double a1 = kq == 0 ? sm[m0 + j][0] : kq == 1 ? sm[m0 + j][1] : kq == 2 ? 1.0 : 0.0;
      const double a2 = kq == 0 ? sm[m0 + j][2] : kq == 1 ? sm[m0 + j][3] : kq == 2 ? 1.0 : 0.0;
      const f64x4 va0 = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, ba[0], zero, 0, 0, 0);
      const f64x4 va1 = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, ba[1], zero, 0, 0, 0);
      const f64x4 va2 = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, ba[2], zero, 0, 0, 0);
      const f64x4 vb0 = __builtin_amdgcn_mfma_f64_16x16x4f64(a2, bb[0], zero, 0, 0, 0);
      const f64x4 vb1 = __builtin_amdgcn_mfma_f64_16x16x4f64(a2, bb[1], zero, 0, 0, 0);
#pragma unroll
      for (int r = 0; r < 4; ++r) {  // register r: match m0 + 4 r + kq, hypothesis j
        const int m = m0 + 4 * r + kq;
        const double num = sm[m][2] * va0[r] + sm[m][3] * va1[r] + va2[r];
        const double den = va0[r] * va0[r] + va1[r] * va1[r] + vb0[r] * vb0[r] + vb1[r] * vb1[r];
        count += (m < here && num * num / den <= thr2) ? 1 : 0;
      }
    }
  }
  count += __shfl_xor(count, 16);
  count += __shfl_xor(count, 32);
  unsigned long long key = hv ? ((unsigned long long)(uint32_t)count << 32) | (0xFFFFFFFFu - (uint32_t)h) : 0ull;
#pragma unroll
  for (int s = 1; s < 16; s <<= 1) {
    const unsigned long long o = __shfl_xor(key, s);
    key = o > key ? o : key;
  }
  if (lane == 0 && key) atomicMax(best, key);
}

// ---- best hypothesis -> mask, pose ----------------------------------------------------------------------
__device__ __forceinline__ void cross3(const double* a, const double* b, double* c) {
  c[0] = a[1] * b[2] - a[2] * b[1];
  c[1] = a[2] * b[0] - a[0] * b[2];
  c[2] = a[0] * b[1] - a[1] * b[0];
}

__global__ __launch_bounds__(256) void k_relpose_finalize(const double* __restrict__ x1, const double* __restrict__ x2,
                                                          int32_t L, const double* __restrict__ cand,
                                                          const unsigned long long* __restrict__ best, double thr2,
                                                          double* __restrict__ pose, uint8_t* __restrict__ mask,
                                                          int32_t* __restrict__ count) {
  __shared__ int s_cnt, s_good[4];
  __shared__ double s_R[2][9], s_t[3];
  const int t = threadIdx.x;
  const unsigned long long key = *best;
  const bool have = key != 0ull;
  const int64_t h = (int64_t)(0xFFFFFFFFu - (uint32_t)key);
  double E[9];
#pragma unroll
  for (int c = 0; c < 9; ++c) E[c] = have ? cand[9 * h + c] : 0.0;
  if (t < 4) s_good[t] = 0;
  if (t == 0) s_cnt = 0;
  __syncthreads();
  int mine = 0;
  for (int n = t; n < L; n += 256) {
    const bool in = have && sampson(E, x1[2 * (int64_t)n], x1[2 * (int64_t)n + 1], x2[2 * (int64_t)n],
                                    x2[2 * (int64_t)n + 1]) <= thr2;
    mask[n] = in ? 1 : 0;
    mine += in ? 1 : 0;
  }
  if (mine) atomicAdd(&s_cnt, mine);
  if (t == 0 && have) {
    // E V = U S by one-sided Jacobi; the two leading columns give u1, u2, v1, v2, and u3 = u1 x u2,
    // v3 = v1 x v2 make det U = det V = +1.  R1 = U W V^T, R2 = U W^T V^T, W = [0 1 0; -1 0 0; 0 0 1]
    double A[3][3], V[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int c = 0; c < 3; ++c) A[i][c] = E[3 * i + c];
    jacobi<3>(A, V);
    double nrm[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) nrm[c] = sqrt(A[0][c] * A[0][c] + A[1][c] * A[1][c] + A[2][c] * A[2][c]);
    int lowest = 0;
#pragma unroll
    for (int c = 1; c < 3; ++c) lowest = nrm[c] < nrm[lowest] ? c : lowest;
    const int ca = lowest == 0 ? 1 : 0, cb = lowest == 2 ? 1 : 2;
    double U[3][3], W3[3][3];  // columns as rows: U[k] = u_k, W3[k] = v_k
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      U[0][i] = sel(A[i], ca) / sel(nrm, ca);
      U[1][i] = sel(A[i], cb) / sel(nrm, cb);
      W3[0][i] = sel(V[i], ca);
      W3[1][i] = sel(V[i], cb);
    }
    cross3(U[0], U[1], U[2]);
    cross3(W3[0], W3[1], W3[2]);
    // U W = [-u2 u1 u3], U W^T = [u2 -u1 u3]
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const double z3 = U[2][i] * W3[2][c];
        const double r = U[0][i] * W3[1][c] - U[1][i] * W3[0][c];
        s_R[0][3 * i + c] = r + z3;
        s_R[1][3 * i + c] = -r + z3;
      }
#pragma unroll
    for (int i = 0; i < 3; ++i) s_t[i] = U[2][i];
  }
  __syncthreads();
  if (have) {
    const double P1[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
    for (int n = t; n < L; n += 256) {
      if (!mask[n]) continue;  // this thread's own store
      const double u1 = x1[2 * (int64_t)n], v1 = x1[2 * (int64_t)n + 1];
      const double u2 = x2[2 * (int64_t)n], v2 = x2[2 * (int64_t)n + 1];
      for (int c = 0; c < 4; ++c) {  // cv2.recoverPose's order: (R1,t) (R2,t) (R1,-t) (R2,-t)
        const double* R = s_R[c & 1];
        const double sg = (c & 2) ? -1.0 : 1.0;
        double P2[12], X[4];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
          P2[4 * i] = R[3 * i];
          P2[4 * i + 1] = R[3 * i + 1];
          P2[4 * i + 2] = R[3 * i + 2];
          P2[4 * i + 3] = sg * s_t[i];
        }
        dlt_point(P1, P2, u1, v1, u2, v2, X);
        const double px = X[0] / X[3], py = X[1] / X[3], pz = X[2] / X[3];
        const double z2 = P2[8] * px + P2[9] * py + P2[10] * pz + P2[11];
        if (pz > 0.0 && pz < kMaxDepth && z2 > 0.0 && z2 < kMaxDepth) atomicAdd(&s_good[c], 1);
      }
    }
  }
  __syncthreads();
  if (t == 0) {
    int pick = 0;
    for (int c = 1; c < 4; ++c) pick = s_good[c] > s_good[pick] ? c : pick;  // the first maximum
    const double sg = (pick & 2) ? -1.0 : 1.0;
    double* oE = pose;
    double* oR = pose + 9;
    double* ot = pose + 18;
    double* oT = pose + 21;
    for (int c = 0; c < 9; ++c) {
      oE[c] = E[c];
      oR[c] = have ? s_R[pick & 1][c] : (c % 4 == 0 ? 1.0 : 0.0);
    }
    for (int i = 0; i < 3; ++i) ot[i] = have ? sg * s_t[i] : 0.0;
    for (int i = 0; i < 3; ++i) {
      for (int c = 0; c < 3; ++c) oT[4 * i + c] = oR[3 * i + c];
      oT[4 * i + 3] = ot[i];
    }
    oT[12] = oT[13] = oT[14] = 0.0;
    oT[15] = 1.0;
    *count = s_cnt;
  }
}

// ---- triangulation ----------------------------------------------------------------------------------------
struct TriArgs {
  const double* T1;  // (4,4) world -> camera of view 1
  const double* T2;
  const double* k1;  // (L,2) normalised keypoints
  const double* k2;
  const double* K;   // (3,3) or null
  int64_t L;
  double* pts;       // (L,3)
  uint8_t* good;     // (L)
  double* uv1;       // (L,2), z1 (L): with K
  double* z1;
  double* uv2;
  double* z2;
};

__global__ __launch_bounds__(256) void k_triangulate(TriArgs a) {
  const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (n >= a.L) return;
  double P1[12], P2[12], X[4];
#pragma unroll
  for (int c = 0; c < 12; ++c) {
    P1[c] = a.T1[c];
    P2[c] = a.T2[c];
  }
  dlt_point(P1, P2, a.k1[2 * n], a.k1[2 * n + 1], a.k2[2 * n], a.k2[2 * n + 1], X);
  const double p[3] = {X[0] / X[3], X[1] / X[3], X[2] / X[3]};
  a.pts[3 * n] = p[0];
  a.pts[3 * n + 1] = p[1];
  a.pts[3 * n + 2] = p[2];
  a.good[n] = X[3] != 0.0 ? 1 : 0;
  if (!a.K) return;
  double K[9];
#pragma unroll
  for (int c = 0; c < 9; ++c) K[c] = a.K[c];
#pragma unroll
  for (int v = 0; v < 2; ++v) {  // src/camera.py:62-68 over Rcw p + tcw
    const double* P = v ? P2 : P1;
    double pc[3], q[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) pc[i] = (P[4 * i] * p[0] + P[4 * i + 1] * p[1] + P[4 * i + 2] * p[2]) + P[4 * i + 3];
#pragma unroll
    for (int i = 0; i < 3; ++i) q[i] = K[3 * i] * pc[0] + K[3 * i + 1] * pc[1] + K[3 * i + 2] * pc[2];
    double* uv = v ? a.uv2 : a.uv1;
    double* z = v ? a.z2 : a.z1;
    uv[2 * n] = q[0] / q[2];
    uv[2 * n + 1] = q[1] / q[2];
    z[n] = q[2];
  }
}

// ---- pseudo-depth map ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_paint_clear(int32_t* __restrict__ owner, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) owner[i] = 0;
}

// one workgroup per point: owner[pixel] = max(i + 1) over the points that paint it
__global__ __launch_bounds__(256) void k_paint_claim(const double* __restrict__ uv, int32_t H, int32_t W, int32_t patch,
                                                     int32_t* __restrict__ owner) {
  const int i = blockIdx.x;
  const double u = uv[2 * (int64_t)i], v = uv[2 * (int64_t)i + 1];  // u: column, v: row
  const double pd = (double)patch;
  if (pd < v && v < (double)H - pd && pd < u && u < (double)W - pd) {
    const int r0 = (int)(v - pd), r1 = (int)(v + pd), c0 = (int)(u - pd), c1 = (int)(u + pd);
    const int wdt = c1 - c0, cells = (r1 - r0) * wdt;
    for (int q = threadIdx.x; q < cells; q += 256) {
      const int r = r0 + q / wdt, c = c0 + q % wdt;
      if (r >= 0 && r < H && c >= 0 && c < W) atomicMax(&owner[(int64_t)r * W + c], i + 1);
    }
  } else if (threadIdx.x == 0 && v > 0.0 && v < (double)H && u > 0.0 && u < (double)W) {
    atomicMax(&owner[(int64_t)(int)v * W + (int)u], i + 1);
  }
}

__global__ __launch_bounds__(256) void k_paint_resolve(const int32_t* __restrict__ owner, const double* __restrict__ depth,
                                                       int64_t n, float* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int32_t o = owner[i];
  out[i] = o > 0 ? (float)depth[o - 1] : 0.f;
}

struct Workspace {
  unsigned long long* best;
  double* cand;
  int32_t* samples;
  uint8_t* valid;
  size_t bytes;
};
// best key (64 B) | cand (10 S, 9) float64 | samples (S, 5) int32 | valid (10 S) uint8
Workspace carve(void* ws, int64_t S) {
  char* p = static_cast<char*>(ws);
  Workspace w;
  size_t off = 64;
  w.best = reinterpret_cast<unsigned long long*>(p);
  w.cand = reinterpret_cast<double*>(p + off);
  off += (size_t)S * 720;
  w.samples = reinterpret_cast<int32_t*>(p + off);
  off += ((size_t)S * 20 + 7) / 8 * 8;
  w.valid = reinterpret_cast<uint8_t*>(p + off);
  off += ((size_t)S * 10 + 7) / 8 * 8;
  w.bytes = off;
  return w;
}

}  // namespace

size_t relpose_workspace_bytes(int64_t L, int64_t S) {
  if (L < 5 || L > kMaxMatches || S < 1 || S > kMaxSamples) return 0;
  return carve(nullptr, S).bytes;
}

int launch_fivept_solve(const double* x1, const double* x2, int64_t S, double* E, uint8_t* valid, hipStream_t st) {
  if (S < 0 || S > kMaxSamples) return PNR_E_ARG;
  if (S == 0) return PNR_OK;
  if (!x1 || !x2 || !E || !valid) return PNR_E_ARG;
  FiveArgs a{x1, x2, 0, (int32_t)S, 0u, nullptr, E, valid, nullptr};
  hipLaunchKernelGGL(k_fivept, dim3((unsigned)((S + 15) / 16)), dim3(256), 0, st, a);
  return hip_status(hipGetLastError());
}

int launch_relpose_estimate(const double* x1, const double* x2, int64_t L, int64_t S, uint32_t seed, double threshold,
                            double* pose, uint8_t* mask, int32_t* count, void* ws, size_t ws_bytes, hipStream_t st) {
  if (L < 5 || L > kMaxMatches || S < 1 || S > kMaxSamples || !(threshold >= 0.0)) return PNR_E_ARG;
  if (!x1 || !x2 || !pose || !mask || !count || !ws || (reinterpret_cast<uintptr_t>(ws) & 7)) return PNR_E_ARG;
  const Workspace w = carve(ws, S);
  if (ws_bytes < w.bytes) return PNR_E_WORKSPACE;
  const int32_t Hn = (int32_t)(10 * S);
  const double thr2 = threshold * threshold;
  FiveArgs a{x1, x2, (int32_t)L, (int32_t)S, seed, w.samples, w.cand, w.valid, w.best};
  hipLaunchKernelGGL(k_fivept, dim3((unsigned)((S + 15) / 16)), dim3(256), 0, st, a);
  hipLaunchKernelGGL(k_score, dim3((unsigned)((Hn + 63) / 64)), dim3(256), 0, st, x1, x2, (int32_t)L, w.cand, w.valid,
                     Hn, thr2, w.best);
  hipLaunchKernelGGL(k_relpose_finalize, dim3(1), dim3(256), 0, st, x1, x2, (int32_t)L, w.cand, w.best, thr2, pose,
                     mask, count);
  return hip_status(hipGetLastError());
}

int launch_triangulate(const double* T1, const double* T2, const double* k1, const double* k2, int64_t L,
                       const double* K, double* pts, uint8_t* good, double* uv1, double* z1, double* uv2, double* z2,
                       hipStream_t st) {
  if (L < 0 || L > (int64_t(1) << 30)) return PNR_E_ARG;
  if (L == 0) return PNR_OK;
  if (!T1 || !T2 || !k1 || !k2 || !pts || !good || (K && (!uv1 || !z1 || !uv2 || !z2))) return PNR_E_ARG;
  TriArgs a{T1, T2, k1, k2, K, L, pts, good, uv1, z1, uv2, z2};
  hipLaunchKernelGGL(k_triangulate, dim3((unsigned)((L + 255) / 256)), dim3(256), 0, st, a);
  return hip_status(hipGetLastError());
}

size_t paint_depth_workspace_bytes(int32_t H, int32_t W) {
  if (H < 1 || W < 1 || (int64_t)H * W >= (int64_t(1) << 30)) return 0;
  return (size_t)H * W * 4;
}

int launch_paint_depth(const double* uv, const double* depth, int64_t n, int32_t H, int32_t W, int32_t patch,
                       float* out, void* ws, size_t ws_bytes, hipStream_t st) {
  const size_t need = paint_depth_workspace_bytes(H, W);
  if (!need || n < 0 || n >= (int64_t(1) << 30) || patch < 0 || patch > 4096) return PNR_E_ARG;
  if (!out || !ws || (reinterpret_cast<uintptr_t>(ws) & 3) || (n > 0 && (!uv || !depth))) return PNR_E_ARG;
  if (ws_bytes < need) return PNR_E_WORKSPACE;
  int32_t* owner = static_cast<int32_t*>(ws);
  const int64_t px = (int64_t)H * W;
  const unsigned blocks = (unsigned)((px + 255) / 256);
  hipLaunchKernelGGL(k_paint_clear, dim3(blocks), dim3(256), 0, st, owner, px);
  if (n > 0) hipLaunchKernelGGL(k_paint_claim, dim3((unsigned)n), dim3(256), 0, st, uv, H, W, patch, owner);
  hipLaunchKernelGGL(k_paint_resolve, dim3(blocks), dim3(256), 0, st, owner, depth, px, out);
  return hip_status(hipGetLastError());
}

}  // namespace pnr
