// recon.hip -- scoring a reconstruction on the device (src/tools/eval_recon.py: calc_3d_metric and what it
// calls in open3d, trimesh and scipy).  Everything is float64.
//
// Exact nearest neighbour, brute force over all pairs on v_mfma_f64_16x16x4_f64.  With both clouds centred,
// d^2 = |a|^2 + (|b|^2 - 2 a.b) is one MFMA of inner dimension 4: A row (x, y, z, 1), B column
// (-2x, -2y, -2z, |b|^2), C = the row's |a|^2.
//   k_nn_centre    one block: the query's bounding-box centre (min and max are exact, so any order will do).
//   k_nn_pack      centred query rows (x, y, z, |a|^2) and ref columns (-2x, -2y, -2z, |b|^2), 32 bytes each,
//                  padded to whole blocks / LDS chunks: zero rows, and columns of |b|^2 = 2^1000 that never win.
//   k_nn_scan      a workgroup of 4 waves owns 256 query rows (4 row tiles of 16 per wave: A and C stay in
//                  registers for the whole scan) and one slice of the ref columns, streamed through LDS in
//                  double-buffered 512-column chunks.  One ds_read_b64 per lane is a column tile's B fragment and
//                  feeds 4 MFMAs.  A lane sees column lane & 15 of every tile and rows 4 r + (lane >> 4), so it
//                  keeps one running minimum per (row tile, r) and the lanes are reduced once, at the end.
//                  The minimum is one v_min_f64 over keys: max(d^2, 0) with its low 24 mantissa bits replaced
//                  by the slice's column-tile counter, so the key carries its argument and equal d^2 prefixes
//                  resolve to the lower column.  Each (slice, row) writes its winner; no atomics.
//   k_nn_finalize  per query: the least (key prefix, index) over the slices -- the pair order of a single-slice
//                  scan, so the answer does not depend on the slice count -- then the winner's distance again
//                  from coordinate differences, and the max_dist test.
// Surface sampling (trimesh.sample.sample_surface's rule): k_face_area, then k_sample_surface: one thread per
// sample, three uniforms (given, or a counter-based hash of seed and sample number), a binary search of the
// cumulative areas, a point in the triangle.
// Metrics: k_dist_partial / k_dist_final: sum of distances and count below a threshold, fixed order.
// ICP (open3d registration_icp, point to point): k_transform, the search above, k_icp_accum (fixed-order sums
// of the correspondences about the search's centre), k_icp_solve (Kabsch on the one-sided Jacobi SVD of jacobi.h, the
// composed transform, fitness and RMSE).
// Vector stores only, no atomics.
#include "jacobi.h"
#include "pnr_internal.h"
#include "window_sample.h"

namespace pnr {

namespace {

typedef double f64x4 __attribute__((ext_vector_type(4)));
typedef double f64x2 __attribute__((ext_vector_type(2)));

constexpr int64_t kMaxPts = int64_t(1) << 28;  // a slice's column-tile counter has 24 bits
constexpr int kRowTiles = 4;                    // 16-row tiles a wave holds
constexpr int kBlockRows = 4 * kRowTiles * 16;  // 256 query rows per workgroup
constexpr int kChunk = 512;                     // ref columns per LDS stage (16 KiB; two stages)
constexpr int kMaxSlices = 32;
constexpr int kMinSliceCap = 4;  // the workspace always has room for this many slices (fewer chunks: for those)
constexpr int kFillBlocks = 1024;  // workgroups the automatic slice count aims at (4 per CU)
constexpr uint32_t kCntMask = 0xFFFFFFu;
constexpr double kPadNorm = 0x1p+1000;
constexpr int kPartBlocks = 256;  // per-block partials of the reductions
constexpr int kIcpSums = 17;      // n | sum a (3) | sum b (3) | sum a b^T (9) | sum d^2

// Sum over the 256 threads of a block in a fixed order: xor-shuffles inside a wave, then waves 0..3.
__device__ __forceinline__ double block_sum_256(double v, double* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}

// ---- nearest neighbour --------------------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void k_nn_centre(const double* __restrict__ q, int64_t Q, double* __restrict__ centre) {
  __shared__ double lo[16][3], hi[16][3];
  double mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (int64_t i = threadIdx.x; i < Q; i += 1024)
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const double v = q[3 * i + c];
      mn[c] = fmin(mn[c], v);
      mx[c] = fmax(mx[c], v);
    }
#pragma unroll
  for (int c = 0; c < 3; ++c)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      mn[c] = fmin(mn[c], __shfl_xor(mn[c], o));
      mx[c] = fmax(mx[c], __shfl_xor(mx[c], o));
    }
  if ((threadIdx.x & 63) == 0)
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      lo[threadIdx.x >> 6][c] = mn[c];
      hi[threadIdx.x >> 6][c] = mx[c];
    }
  __syncthreads();
  if (threadIdx.x < 3) {
    const int c = threadIdx.x;
    double a = lo[0][c], b = hi[0][c];
    for (int w = 1; w < 16; ++w) {
      a = fmin(a, lo[w][c]);
      b = fmax(b, hi[w][c]);
    }
    centre[c] = 0.5 * a + 0.5 * b;
  }
}

__global__ __launch_bounds__(256) void k_nn_pack(const double* __restrict__ q, int64_t Q, int64_t Qpad,
                                                 const double* __restrict__ ref, int64_t R, int64_t Rpad,
                                                 const double* __restrict__ centre, f64x2* __restrict__ qpack,
                                                 f64x2* __restrict__ bpack) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const double cx = centre[0], cy = centre[1], cz = centre[2];
  if (i < Qpad) {
    f64x2 u = {0.0, 0.0}, v = {0.0, 0.0};
    if (i < Q) {
      const double x = q[3 * i] - cx, y = q[3 * i + 1] - cy, z = q[3 * i + 2] - cz;
      u = f64x2{x, y};
      v = f64x2{z, x * x + y * y + z * z};
    }
    qpack[2 * i] = u;
    qpack[2 * i + 1] = v;
  }
  if (i < Rpad) {
    f64x2 u = {0.0, 0.0}, v = {0.0, kPadNorm};
    if (i < R) {
      const double x = ref[3 * i] - cx, y = ref[3 * i + 1] - cy, z = ref[3 * i + 2] - cz;
      u = f64x2{-2.0 * x, -2.0 * y};
      v = f64x2{-2.0 * z, x * x + y * y + z * z};
    }
    bpack[2 * i] = u;
    bpack[2 * i + 1] = v;
  }
}

// max(d^2, 0) with the low 24 mantissa bits replaced by the column-tile counter: positive doubles order as
// their bit patterns, so the minimum over keys is the minimum over (d^2 prefix, tile)
__device__ __forceinline__ double nn_key(double v, uint32_t cnt) {
  asm("v_max_f64 %0, %1, 0" : "=v"(v) : "v"(v));  // the bare instruction, as min_key below
  const uint32_t lo = ((uint32_t)__double2loint(v) & ~kCntMask) | cnt;
  return __hiloint2double(__double2hiint(v), (int)lo);
}
// the instruction itself: the builtin canonicalises both operands first (two more v_max_f64 per value), and a
// key is never NaN (float64 denormals are kept: a key of d^2 = 0 is one)
__device__ __forceinline__ double min_key(double a, double b) {
  double r;
  asm("v_min_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}

// grid (Qpad / 256, slices); slice y scans chunks [y cps, min((y + 1) cps, nchunks)), never an empty range
__global__ __launch_bounds__(256) void k_nn_scan(const double* __restrict__ qpack, const f64x2* __restrict__ bpack,
                                                 int32_t nchunks, int32_t cps, int64_t Qpad,
                                                 double* __restrict__ win_key, int32_t* __restrict__ win_idx) {
  __shared__ f64x2 sb[2][kChunk * 2];
  const int t = threadIdx.x, lane = t & 63, j = lane & 15, kq = lane >> 4;
  const int w = __builtin_amdgcn_readfirstlane(t >> 6);
  const int64_t row0 = (int64_t)blockIdx.x * kBlockRows + w * (kRowTiles * 16);
  // A operand (row j, k = kq) = (x, y, z, 1); C (register r: row 4 r + kq) = |a|^2
  double a[kRowTiles];
  f64x4 c0[kRowTiles], best[kRowTiles];
#pragma unroll
  for (int tt = 0; tt < kRowTiles; ++tt) {
    a[tt] = kq < 3 ? qpack[(row0 + tt * 16 + j) * 4 + kq] : 1.0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      c0[tt][r] = qpack[(row0 + tt * 16 + 4 * r + kq) * 4 + 3];
      best[tt][r] = INFINITY;
    }
  }
  const int c_begin = blockIdx.y * cps, c_end = min(c_begin + cps, nchunks);
  // a chunk is 1024 x 16 bytes: 4 per thread, held in registers while the chunk before it is scanned
  const f64x2* src = bpack + (int64_t)c_begin * (kChunk * 2);
  f64x2 pre[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) pre[i] = src[i * 256 + t];
#pragma unroll
  for (int i = 0; i < 4; ++i) sb[0][i * 256 + t] = pre[i];
  __syncthreads();
  uint32_t cnt = 0;
  for (int c = c_begin; c < c_end; ++c) {
    const int buf = (c - c_begin) & 1;
    const bool more = c + 1 < c_end;
    if (more) {
      src += kChunk * 2;
#pragma unroll
      for (int i = 0; i < 4; ++i) pre[i] = src[i * 256 + t];
    }
    // B operand (k = kq, column j) of tile m: double (16 m + j) 4 + kq; the 64 lanes read 512 contiguous bytes
    const double* b = reinterpret_cast<const double*>(sb[buf]) + j * 4 + kq;
#pragma unroll 4
    for (int m = 0; m < kChunk / 16; ++m, ++cnt) {
      const double bv = b[m * 64];
#pragma unroll
      for (int tt = 0; tt < kRowTiles; ++tt) {
        const f64x4 d = __builtin_amdgcn_mfma_f64_16x16x4f64(a[tt], bv, c0[tt], 0, 0, 0);
#pragma unroll
        for (int r = 0; r < 4; ++r) best[tt][r] = min_key(best[tt][r], nn_key(d[r], cnt));
      }
    }
    if (more) {
#pragma unroll
      for (int i = 0; i < 4; ++i) sb[buf ^ 1][i * 256 + t] = pre[i];
    }
    __syncthreads();
  }
  // the 16 lanes of a row: least (key, column).  Equal keys share the tile, so the lower lane is the lower index
  const int64_t slot0 = (int64_t)blockIdx.y * Qpad + row0;
#pragma unroll
  for (int tt = 0; tt < kRowTiles; ++tt)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      double k = best[tt][r];
      int jj = j;
#pragma unroll
      for (int s = 1; s < 16; s <<= 1) {
        const double ok = __shfl_xor(k, s);
        const int oj = __shfl_xor(jj, s);
        const bool take = ok < k || (ok == k && oj < jj);
        k = take ? ok : k;
        jj = take ? oj : jj;
      }
      if (j == 0) {
        const uint32_t lo = (uint32_t)__double2loint(k);
        const int64_t col = (int64_t)c_begin * kChunk + (int64_t)(lo & kCntMask) * 16 + jj;
        const int64_t slot = slot0 + tt * 16 + 4 * r + kq;
        win_key[slot] = __hiloint2double(__double2hiint(k), (int)(lo & ~kCntMask));
        win_idx[slot] = (int32_t)col;
      }
    }
}

__device__ __forceinline__ double dist2(const double* __restrict__ p, const double* __restrict__ q) {
#pragma clang fp contract(off)
  const double dx = p[0] - q[0], dy = p[1] - q[1], dz = p[2] - q[2];
  return (dx * dx + dy * dy) + dz * dz;
}

__global__ __launch_bounds__(256) void k_nn_finalize(const double* __restrict__ q, int64_t Q, int64_t Qpad,
                                                     const double* __restrict__ ref, int64_t R, int32_t slices,
                                                     const double* __restrict__ win_key,
                                                     const int32_t* __restrict__ win_idx, double max_dist,
                                                     double* __restrict__ dist, int64_t* __restrict__ idx) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= Q) return;
  double bk = INFINITY;
  int64_t bi = -1;
  for (int s = 0; s < slices; ++s) {  // ascending slices are ascending indices: a strict test keeps the lower
    const double k = win_key[(int64_t)s * Qpad + i];
    const int64_t id = win_idx[(int64_t)s * Qpad + i];
    if (id < R && (bi < 0 || k < bk)) {
      bk = k;
      bi = id;
    }
  }
  double d = INFINITY;
  if (bi >= 0) {
    d = sqrt(dist2(q + 3 * i, ref + 3 * bi));
    if (!(d <= max_dist)) {
      d = INFINITY;
      bi = -1;
    }
  }
  dist[i] = d;
  idx[i] = bi;
}

struct NnPlan {
  int64_t Qpad, Rpad;
  int32_t nchunks, slices, cps, cap;
  double* centre;
  double* qpack;
  f64x2* bpack;
  double* win_key;
  int32_t* win_idx;
  size_t bytes;
};
// centre (64 B) | query rows (Qpad, 4) | ref columns (Rpad, 4) | winner keys (cap, Qpad) | winner indices
NnPlan nn_plan(void* ws, int64_t Q, int64_t R, int32_t want) {
  NnPlan p;
  p.Qpad = (Q + kBlockRows - 1) / kBlockRows * kBlockRows;
  p.Rpad = (R + kChunk - 1) / kChunk * kChunk;
  p.nchunks = (int32_t)(p.Rpad / kChunk);
  const int64_t bx = p.Qpad / kBlockRows;
  int64_t au = (kFillBlocks + bx - 1) / bx;
  au = au > kMaxSlices ? kMaxSlices : au;
  au = au > p.nchunks ? p.nchunks : au;
  int64_t cap = au > kMinSliceCap ? au : kMinSliceCap;
  cap = cap > p.nchunks ? p.nchunks : cap;
  p.cap = (int32_t)cap;
  const int32_t s = want > 0 ? want : (int32_t)au;
  p.cps = (p.nchunks + s - 1) / s;
  p.slices = (p.nchunks + p.cps - 1) / p.cps;
  char* b = static_cast<char*>(ws);
  size_t off = 64;
  p.centre = reinterpret_cast<double*>(b);
  p.qpack = reinterpret_cast<double*>(b + off);
  off += (size_t)p.Qpad * 32;
  p.bpack = reinterpret_cast<f64x2*>(b + off);
  off += (size_t)p.Rpad * 32;
  p.win_key = reinterpret_cast<double*>(b + off);
  off += (size_t)cap * p.Qpad * 8;
  p.win_idx = reinterpret_cast<int32_t*>(b + off);
  off += (size_t)cap * p.Qpad * 4;
  p.bytes = (off + 15) / 16 * 16;
  return p;
}

void nn_launch(const NnPlan& p, const double* q, int64_t Q, const double* ref, int64_t R, double max_dist, double* dist,
               int64_t* idx, hipStream_t st) {
  hipLaunchKernelGGL(k_nn_centre, dim3(1), dim3(1024), 0, st, q, Q, p.centre);
  const int64_t n = p.Qpad > p.Rpad ? p.Qpad : p.Rpad;
  hipLaunchKernelGGL(k_nn_pack, dim3((unsigned)(n / 256)), dim3(256), 0, st, q, Q, p.Qpad, ref, R, p.Rpad, p.centre,
                     reinterpret_cast<f64x2*>(p.qpack), p.bpack);
  hipLaunchKernelGGL(k_nn_scan, dim3((unsigned)(p.Qpad / kBlockRows), (unsigned)p.slices), dim3(256), 0, st, p.qpack,
                     p.bpack, p.nchunks, p.cps, p.Qpad, p.win_key, p.win_idx);
  hipLaunchKernelGGL(k_nn_finalize, dim3((unsigned)((Q + 255) / 256)), dim3(256), 0, st, q, Q, p.Qpad, ref, R, p.slices,
                     p.win_key, p.win_idx, max_dist, dist, idx);
}

// ---- surface sampling -----------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_face_area(const double* __restrict__ verts, int64_t V,
                                                   const int64_t* __restrict__ faces, int64_t F,
                                                   double* __restrict__ area) {
#pragma clang fp contract(off)
  const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (f >= F) return;
  const int64_t i0 = faces[3 * f], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
  double s = 0.0;
  if (i0 >= 0 && i0 < V && i1 >= 0 && i1 < V && i2 >= 0 && i2 < V) {
    const double* a = verts + 3 * i0;
    const double* b = verts + 3 * i1;
    const double* c = verts + 3 * i2;
    const double ux = b[0] - a[0], uy = b[1] - a[1], uz = b[2] - a[2];
    const double vx = c[0] - a[0], vy = c[1] - a[1], vz = c[2] - a[2];
    const double nx = uy * vz - uz * vy, ny = uz * vx - ux * vz, nz = ux * vy - uy * vx;
    s = 0.5 * sqrt((nx * nx + ny * ny) + nz * nz);
  }
  area[f] = s;
}

// uniform k of sample i in [0, 1): 53 bits of the splitmix64 finaliser of (seed, 3 i + k)
__device__ __forceinline__ double sample_uniform(uint64_t base, int64_t i, int k) {
  const uint64_t z = mix64(base + (uint64_t)(3 * i + k) * 0xD1B54A32D192ED03ull);
  return (double)(z >> 11) * 0x1p-53;
}

__global__ __launch_bounds__(256) void k_sample_surface(const double* __restrict__ verts,
                                                        const int64_t* __restrict__ faces,
                                                        const double* __restrict__ cum, int64_t F, int64_t count,
                                                        uint64_t seed, const double* __restrict__ uniforms,
                                                        double* __restrict__ points, int64_t* __restrict__ face_idx) {
#pragma clang fp contract(off)
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= count) return;
  double u0, u1, u2;
  if (uniforms) {
    u0 = uniforms[3 * i];
    u1 = uniforms[3 * i + 1];
    u2 = uniforms[3 * i + 2];
  } else {
    const uint64_t base = mix64(seed * 0x9E3779B97F4A7C15ull);
    u0 = sample_uniform(base, i, 0);
    u1 = sample_uniform(base, i, 1);
    u2 = sample_uniform(base, i, 2);
  }
  const double total = cum[F - 1];
  if (!(total > 0.0) || !(total < INFINITY)) {  // no area to sample (or a face out of range of float64)
    points[3 * i] = points[3 * i + 1] = points[3 * i + 2] = NAN;
    face_idx[i] = -1;
    return;
  }
  // the first face whose cumulative area reaches u0 total and is positive: never a zero-area face
  const double target = u0 * total;
  int64_t lo = 0, hi = F - 1;
  while (lo < hi) {
    const int64_t mid = lo + (hi - lo) / 2;
    const double c = cum[mid];
    if (c >= target && c > 0.0)
      hi = mid;
    else
      lo = mid + 1;
  }
  if (u1 + u2 > 1.0) {
    u1 = 1.0 - u1;
    u2 = 1.0 - u2;
  }
  const double* a = verts + 3 * faces[3 * lo];
  const double* b = verts + 3 * faces[3 * lo + 1];
  const double* c = verts + 3 * faces[3 * lo + 2];
#pragma unroll
  for (int k = 0; k < 3; ++k) points[3 * i + k] = ((b[k] - a[k]) * u1 + (c[k] - a[k]) * u2) + a[k];
  face_idx[i] = lo;
}

// ---- metrics ----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_dist_partial(const double* __restrict__ dist, int64_t n, double th,
                                                      double* __restrict__ part) {
  __shared__ double red[4];
  double s = 0.0, c = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const double d = dist[i];
    s += d;
    c += d < th ? 1.0 : 0.0;
  }
  s = block_sum_256(s, red);
  c = block_sum_256(c, red);
  if (threadIdx.x == 0) {
    part[2 * blockIdx.x] = s;
    part[2 * blockIdx.x + 1] = c;
  }
}

__global__ __launch_bounds__(256) void k_dist_final(const double* __restrict__ part, int32_t nb, double* __restrict__ out) {
  __shared__ double red[4];
  const int t = threadIdx.x;
  const double s = block_sum_256(t < nb ? part[2 * t] : 0.0, red);
  const double c = block_sum_256(t < nb ? part[2 * t + 1] : 0.0, red);
  if (t == 0) {
    out[0] = s;
    out[1] = c;
  }
}

// ---- ICP ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_transform(const double* __restrict__ p, int64_t n, const double* __restrict__ T,
                                                   double* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const double x = p[3 * i], y = p[3 * i + 1], z = p[3 * i + 2];
#pragma unroll
  for (int r = 0; r < 3; ++r) out[3 * i + r] = fma(T[4 * r], x, fma(T[4 * r + 1], y, fma(T[4 * r + 2], z, T[4 * r + 3])));
}

// Correspondence sums about a pivot (the moved cloud's bounding-box centre, which the search left behind):
// a = p_i - pivot, b = q_idx(i) - pivot over the rows with a match.  The covariance does not depend on the pivot;
// near the data it keeps the sums as small as centred ones
__global__ __launch_bounds__(256) void k_icp_accum(const double* __restrict__ p, int64_t n, const double* __restrict__ q,
                                                   const int64_t* __restrict__ idx, const double* __restrict__ dist,
                                                   const double* __restrict__ pivot, double* __restrict__ part) {
  __shared__ double red[4];
  const double px = pivot[0], py = pivot[1], pz = pivot[2];
  double s[kIcpSums];
#pragma unroll
  for (int c = 0; c < kIcpSums; ++c) s[c] = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const int64_t m = idx[i];
    if (m < 0) continue;
    const double a[3] = {p[3 * i] - px, p[3 * i + 1] - py, p[3 * i + 2] - pz};
    const double b[3] = {q[3 * m] - px, q[3 * m + 1] - py, q[3 * m + 2] - pz};
    const double d = dist[i];
    s[0] += 1.0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      s[1 + c] += a[c];
      s[4 + c] += b[c];
#pragma unroll
      for (int e = 0; e < 3; ++e) s[7 + 3 * c + e] += a[c] * b[e];
    }
    s[16] += d * d;
  }
#pragma unroll
  for (int c = 0; c < kIcpSums; ++c) {
    const double v = block_sum_256(s[c], red);
    if (threadIdx.x == 0) part[kIcpSums * blockIdx.x + c] = v;
  }
}

template <typename T, int N>
__device__ __forceinline__ T sel(const T (&a)[N], int i) {
  T v = a[0];
#pragma unroll
  for (int c = 1; c < N; ++c) v = c == i ? a[c] : v;
  return v;
}

__device__ __forceinline__ void cross3(const double* a, const double* b, double* c) {
  c[0] = a[1] * b[2] - a[2] * b[1];
  c[1] = a[2] * b[0] - a[0] * b[2];
  c[2] = a[0] * b[1] - a[1] * b[0];
}

// One block: the partials in block order, then Kabsch.  H = sum (a - mean a)(b - mean b)^T = U S V^T by
// one-sided Jacobi on H (H <- U S); the two leading pairs (u, v) and u3 = u1 x u2, v3 = v1 x v2, which makes
// R = V U^T proper: the reflection fix of Kabsch / Umeyama.  T_out = [R t] T_in, t = mean b - R mean a.
__global__ __launch_bounds__(64) void k_icp_solve(const double* __restrict__ part, int32_t nb, const double* __restrict__ p,
                                                  int64_t n, const double* __restrict__ T_in, double* __restrict__ T_out,
                                                  double* __restrict__ stats) {
  __shared__ double sum[kIcpSums];
  const int t = threadIdx.x;
  if (t < kIcpSums) {
    double v = 0.0;
    for (int b = 0; b < nb; ++b) v += part[kIcpSums * b + t];
    sum[t] = v;
  }
  __syncthreads();
  if (t != 0) return;
  const double m = sum[0];
  double R[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}}, tr[3] = {0, 0, 0};
  if (m > 0.0) {
    double ma[3], mb[3], A[3][3], V[3][3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      ma[c] = sum[1 + c] / m;
      mb[c] = sum[4 + c] / m;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
      for (int e = 0; e < 3; ++e) A[c][e] = sum[7 + 3 * c + e] - m * ma[c] * mb[e];
    jacobi<3>(A, V);
    double nrm[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) nrm[c] = sqrt(A[0][c] * A[0][c] + A[1][c] * A[1][c] + A[2][c] * A[2][c]);
    int lowest = 0;
#pragma unroll
    for (int c = 1; c < 3; ++c) lowest = nrm[c] < nrm[lowest] ? c : lowest;
    const int ca = lowest == 0 ? 1 : 0, cb = lowest == 2 ? 1 : 2;
    const double na = sel(nrm, ca), nc = sel(nrm, cb);
    if (na > 0.0 && nc > 0.0) {  // else fewer than two directions: the translation alone
      double U[3][3], W[3][3];   // columns as rows: U[k] = u_k, W[k] = v_k
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        U[0][i] = sel(A[i], ca) / na;
        U[1][i] = sel(A[i], cb) / nc;
        W[0][i] = sel(V[i], ca);
        W[1][i] = sel(V[i], cb);
      }
      cross3(U[0], U[1], U[2]);
      cross3(W[0], W[1], W[2]);
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int c = 0; c < 3; ++c) R[i][c] = (W[0][i] * U[0][c] + W[1][i] * U[1][c]) + W[2][i] * U[2][c];
    }
    // means about the pivot: t = (mb + pivot) - R (ma + pivot)
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      double v = mb[i] + p[i];
#pragma unroll
      for (int c = 0; c < 3; ++c) v -= R[i][c] * (ma[c] + p[c]);
      tr[i] = v;
    }
  }
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      double v = c == 3 ? tr[i] : 0.0;
#pragma unroll
      for (int e = 0; e < 3; ++e) v += R[i][e] * T_in[4 * e + c];
      T_out[4 * i + c] = v;
    }
#pragma unroll
  for (int c = 0; c < 4; ++c) T_out[12 + c] = c == 3 ? 1.0 : 0.0;
  stats[0] = m / (double)n;
  stats[1] = m > 0.0 ? sqrt(sum[16] / m) : 0.0;
  stats[2] = m;
}

int part_blocks(int64_t n) { return (int)(n < (int64_t)kPartBlocks * 256 ? (n + 255) / 256 : kPartBlocks); }

bool misaligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) != 0; }

struct IcpPlan {
  double* moved;
  double* dist;
  int64_t* idx;
  double* part;
  void* nn;
  size_t nn_bytes, bytes;
};
// moved (N,3) | dist (N) | idx (N) | partials (256, 17) | the search's workspace
IcpPlan icp_plan(void* ws, int64_t N, int64_t M) {
  IcpPlan p;
  char* b = static_cast<char*>(ws);
  size_t off = 0;
  p.moved = reinterpret_cast<double*>(b);
  off += ((size_t)N * 24 + 15) / 16 * 16;
  p.dist = reinterpret_cast<double*>(b + off);
  off += ((size_t)N * 8 + 15) / 16 * 16;
  p.idx = reinterpret_cast<int64_t*>(b + off);
  off += ((size_t)N * 8 + 15) / 16 * 16;
  p.part = reinterpret_cast<double*>(b + off);
  off += (size_t)kPartBlocks * kIcpSums * 8;
  p.nn = b + off;
  p.nn_bytes = nn_plan(nullptr, N, M, 0).bytes;
  p.bytes = off + p.nn_bytes;
  return p;
}

}  // namespace

size_t nn_workspace_bytes(int64_t Q, int64_t R) {
  if (Q < 1 || R < 1 || Q > kMaxPts || R > kMaxPts) return 0;
  return nn_plan(nullptr, Q, R, 0).bytes;
}

int launch_nn_search(const double* query, int64_t Q, const double* ref, int64_t R, double max_dist, int32_t slices,
                     double* dist, int64_t* idx, void* ws, size_t ws_bytes, hipStream_t st) {
  if (Q < 0 || R < 0 || Q > kMaxPts || R > kMaxPts || !(max_dist >= 0.0) || slices < 0) return PNR_E_ARG;
  if (Q == 0 || R == 0) return PNR_OK;
  if (!query || !ref || !dist || !idx || !ws || misaligned(ws, 16)) return PNR_E_ARG;
  if (slices > nn_plan(nullptr, Q, R, 0).cap) return PNR_E_ARG;
  const NnPlan p = nn_plan(ws, Q, R, slices);
  if (ws_bytes < p.bytes) return PNR_E_WORKSPACE;
  nn_launch(p, query, Q, ref, R, max_dist, dist, idx, st);
  return hip_status(hipGetLastError());
}

int launch_face_areas(const double* verts, int64_t V, const int64_t* faces, int64_t F, double* area, hipStream_t st) {
  if (V < 0 || F < 0 || V > kMaxPts || F > kMaxPts) return PNR_E_ARG;
  if (F == 0) return PNR_OK;
  if (!faces || !area || (V > 0 && !verts)) return PNR_E_ARG;
  hipLaunchKernelGGL(k_face_area, dim3((unsigned)((F + 255) / 256)), dim3(256), 0, st, verts, V, faces, F, area);
  return hip_status(hipGetLastError());
}

int launch_sample_surface(const double* verts, const int64_t* faces, const double* cum, int64_t F, int64_t count,
                          uint64_t seed, const double* uniforms, double* points, int64_t* face_idx, hipStream_t st) {
  if (F < 1 || F > kMaxPts || count < 0 || count > kMaxPts) return PNR_E_ARG;
  if (count == 0) return PNR_OK;
  if (!verts || !faces || !cum || !points || !face_idx) return PNR_E_ARG;
  hipLaunchKernelGGL(k_sample_surface, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, st, verts, faces, cum, F,
                     count, seed, uniforms, points, face_idx);
  return hip_status(hipGetLastError());
}

size_t dist_stats_workspace_bytes() { return (size_t)kPartBlocks * 2 * 8; }

int launch_dist_stats(const double* dist, int64_t n, double dist_th, double* out, void* ws, size_t ws_bytes,
                      hipStream_t st) {
  if (n < 1 || n > kMaxPts || !dist || !out || !ws || misaligned(ws, 8)) return PNR_E_ARG;
  if (ws_bytes < dist_stats_workspace_bytes()) return PNR_E_WORKSPACE;
  const int nb = part_blocks(n);
  double* part = static_cast<double*>(ws);
  hipLaunchKernelGGL(k_dist_partial, dim3(nb), dim3(256), 0, st, dist, n, dist_th, part);
  hipLaunchKernelGGL(k_dist_final, dim3(1), dim3(256), 0, st, part, nb, out);
  return hip_status(hipGetLastError());
}

int launch_transform_points(const double* pts, int64_t n, const double* T, double* out, hipStream_t st) {
  if (n < 0 || n > kMaxPts) return PNR_E_ARG;
  if (n == 0) return PNR_OK;
  if (!pts || !T || !out) return PNR_E_ARG;
  hipLaunchKernelGGL(k_transform, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, pts, n, T, out);
  return hip_status(hipGetLastError());
}

size_t icp_workspace_bytes(int64_t N, int64_t M) {
  if (N < 1 || M < 1 || N > kMaxPts || M > kMaxPts) return 0;
  return icp_plan(nullptr, N, M).bytes;
}

int launch_icp_step(const double* src, int64_t N, const double* dst, int64_t M, const double* T_in, double threshold,
                    double* T_out, double* stats, void* ws, size_t ws_bytes, hipStream_t st) {
  if (N < 1 || M < 1 || N > kMaxPts || M > kMaxPts || !(threshold >= 0.0)) return PNR_E_ARG;
  if (!src || !dst || !T_in || !T_out || !stats || T_in == T_out || !ws || misaligned(ws, 16)) return PNR_E_ARG;
  const IcpPlan p = icp_plan(ws, N, M);
  if (ws_bytes < p.bytes) return PNR_E_WORKSPACE;
  const NnPlan nn = nn_plan(p.nn, N, M, 0);
  hipLaunchKernelGGL(k_transform, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, src, N, T_in, p.moved);
  nn_launch(nn, p.moved, N, dst, M, threshold, p.dist, p.idx, st);
  const int nb = part_blocks(N);
  hipLaunchKernelGGL(k_icp_accum, dim3(nb), dim3(256), 0, st, p.moved, N, dst, p.idx, p.dist, nn.centre, p.part);
  hipLaunchKernelGGL(k_icp_solve, dim3(1), dim3(64), 0, st, p.part, nb, nn.centre, N, T_in, T_out, stats);
  return hip_status(hipGetLastError());
}

}  // namespace pnr
