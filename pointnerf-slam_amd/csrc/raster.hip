// raster.hip -- depth images of a triangle mesh on the device (src/tools/eval_recon.py: calc_2d_metric and
// check_proj; src/tools/cull_mesh.py).  Everything is float64; the image is rounded once to float32.
//
// The rendering rule is the one include/pnr.h states under "mesh depth rasteriser": homogeneous edge functions
// (Olano-Greer, no near-plane clipping for coverage), depth = det / (E0 + E1 + E2), the least kept depth wins.
//   face_setup     the one statement of a (view, face) pair: camera transform, q vectors, z rejection, the
//                  conservative pixel box (from the polygon clipped at z_near when the face crosses it), the edge
//                  normals (cross products formed lower vertex index first) and det, signs folded so that
//                  "covered" is E_k >= 0.  Unfused arithmetic: count, fill and tile inline the same roundings,
//                  so they cannot disagree about a face's tiles.
//   k_rast_bin<0>  the count pass.  One thread per face, looping over the views of the batch (the vertices are
//                  read once): an integer atomicAdd on every 32 x 32-pixel tile counter the box overlaps.
//   (scan)         the caller's inclusive scan of the counters (torch.cumsum) gives the list ends.
//   k_rast_bin<1>  the fill pass: the same traversal; int32 face ids into the tile lists through atomic cursors.
//                  The bins hold ids, not 96-byte setup records: three 24-byte vertices recompute cheaper than a
//                  record reloads.
//   k_rast_tile    one 256-thread workgroup per (view, tile).  The tile's 1,024 depths are float64 bit patterns
//                  in LDS (8 KiB, +inf at the start): positive doubles order as unsigned integers, so a 64-bit
//                  LDS unsigned-min atomic is the depth test.  A chunk of 256 list entries is set up one face per
//                  thread.  A face with at most 16 pixel centres in its clipped box (the marching-cubes case) is
//                  walked by its own thread; a larger one is appended, as its setup record, to an LDS queue
//                  (22 KiB), which whole waves then drain with their lanes striding over the box (a wall's
//                  triangle fills the tile: 16 centres per lane, not 1,024 per thread).  The tile leaves
//                  coalesced as float32, +inf as 0, partial tiles masked.  No global atomics touch the image.
//   k_depth_l1_*   per view the float64 sum of |a - b| in a fixed order: per-block partials, then one block.
//   k_frustum_seen check_proj's test for every (point, view), reduced with "any" along either axis by plain
//                  stores of 1 into flags a small kernel cleared.
// Vector stores and vector atomics only.
#include "pnr_internal.h"

namespace pnr {

namespace {

constexpr int kTile = 32;               // pixels per tile side
constexpr int kTilePix = kTile * kTile;
constexpr int kSmallPix = 16;           // a clipped box of at most this many centres is walked by one thread
constexpr int kMaxSide = 8192;          // image side
constexpr int kMaxViews = 4096;         // views per call (grid y)
constexpr int64_t kMaxCounters = int64_t(1) << 24;
constexpr int64_t kMaxPairs = int64_t(1) << 30;
constexpr int64_t kMaxFaces = int64_t(1) << 28;
constexpr double kBoxPad = 0x1p-8;      // pixels the box is widened by: far above the float64 error of a centre
                                        // that the edge functions can still decide
constexpr int kL1Blocks = 256;          // per-view partials of the depth L1 sum

struct RastArgs {
  const double* verts;
  const int64_t* faces;
  const double* c2w;
  int64_t V, F;
  int32_t n, H, W, tx, ty;
  double fx, fy, cx, cy, zn, zf;
};

// A face under a view, ready for pixels: E_k(j, i) = (n[k][0] j + n[k][1] i) + n[k][2] >= 0 for k = 0, 1, 2 is
// coverage (signs folded by sign(det)), det > 0, z = det / ((E0 + E1) + E2).  Box in pixels, inclusive.
struct FaceSetup {
  double n[3][3];
  double det;
  int x0, x1, y0, y1;
};

// camera-space point of a world point: R^T (x - t) for c2w = [R t], unfused
__device__ __forceinline__ void to_camera(const double* __restrict__ M, const double* __restrict__ p, double& x, double& y,
                                          double& z) {
#pragma clang fp contract(off)
  const double dx = p[0] - M[3], dy = p[1] - M[7], dz = p[2] - M[11];
  x = (M[0] * dx + M[4] * dy) + M[8] * dz;
  y = (M[1] * dx + M[5] * dy) + M[9] * dz;
  z = (M[2] * dx + M[6] * dy) + M[10] * dz;
}

__device__ __forceinline__ bool face_setup(const RastArgs& a, int view, int64_t f, FaceSetup& s) {
#pragma clang fp contract(off)
  const int64_t id[3] = {a.faces[3 * f], a.faces[3 * f + 1], a.faces[3 * f + 2]};
  if (id[0] < 0 || id[0] >= a.V || id[1] < 0 || id[1] >= a.V || id[2] < 0 || id[2] >= a.V) return false;
  const double* M = a.c2w + 16 * (int64_t)view;
  double q[3][3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    double x, y, z;
    to_camera(M, a.verts + 3 * id[k], x, y, z);
    q[k][0] = a.fx * x + a.cx * z;
    q[k][1] = a.fy * y + a.cy * z;
    q[k][2] = z;
  }
  const double zmin = fmin(fmin(q[0][2], q[1][2]), q[2][2]), zmax = fmax(fmax(q[0][2], q[1][2]), q[2][2]);
  if (!(zmax >= a.zn) || !(zmin <= a.zf)) return false;  // wholly nearer than z_near or beyond z_far
  // the box of what can be kept: the part of the triangle with z >= z_near, projected
  double ulo = INFINITY, uhi = -INFINITY, vlo = INFINITY, vhi = -INFINITY;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    if (q[k][2] >= a.zn) {
      const double u = q[k][0] / q[k][2], v = q[k][1] / q[k][2];
      ulo = fmin(ulo, u), uhi = fmax(uhi, u), vlo = fmin(vlo, v), vhi = fmax(vhi, v);
    }
    const int l = (k + 1) % 3;
    if ((q[k][2] >= a.zn) != (q[l][2] >= a.zn)) {  // the edge crosses z_near: its point there
      const double t = (a.zn - q[k][2]) / (q[l][2] - q[k][2]);
      const double u = (q[k][0] + t * (q[l][0] - q[k][0])) / a.zn, v = (q[k][1] + t * (q[l][1] - q[k][1])) / a.zn;
      ulo = fmin(ulo, u), uhi = fmax(uhi, u), vlo = fmin(vlo, v), vhi = fmax(vhi, v);
    }
  }
  // clamped as doubles before the conversion (fmin / fmax drop a NaN: every index stays inside the image)
  s.x0 = (int)fmin(fmax(ceil(ulo - kBoxPad), 0.0), (double)a.W);
  s.x1 = (int)fmax(fmin(floor(uhi + kBoxPad), (double)(a.W - 1)), -1.0);
  s.y0 = (int)fmin(fmax(ceil(vlo - kBoxPad), 0.0), (double)a.H);
  s.y1 = (int)fmax(fmin(floor(vhi + kBoxPad), (double)(a.H - 1)), -1.0);
  if (s.x0 > s.x1 || s.y0 > s.y1) return false;
  // edge k, opposite vertex k: q_i x q_j for (i, j) = (k + 1, k + 2), formed with the lower vertex index first
  // and negated if that swapped them, so the face across the edge sees exactly the negated values
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int i = (k + 1) % 3, j = (k + 2) % 3;
    const bool sw = id[i] > id[j];
    double u[3], w[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      u[c] = sw ? q[j][c] : q[i][c];
      w[c] = sw ? q[i][c] : q[j][c];
    }
    const double n0 = u[1] * w[2] - u[2] * w[1], n1 = u[2] * w[0] - u[0] * w[2], n2 = u[0] * w[1] - u[1] * w[0];
    s.n[k][0] = sw ? -n0 : n0;
    s.n[k][1] = sw ? -n1 : n1;
    s.n[k][2] = sw ? -n2 : n2;
  }
  const double det = (q[0][0] * s.n[0][0] + q[0][1] * s.n[0][1]) + q[0][2] * s.n[0][2];
  if (!(det != 0.0)) return false;
  if (det < 0.0) {  // negation is exact and the sums below are symmetric in sign: the rule's E_k sign(det)
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
      for (int c = 0; c < 3; ++c) s.n[k][c] = -s.n[k][c];
  }
  s.det = fabs(det);
  return true;
}

// the tiles a set-up face overlaps, inclusive
__device__ __forceinline__ void face_tiles(const FaceSetup& s, int& tx0, int& tx1, int& ty0, int& ty1) {
  tx0 = s.x0 / kTile, tx1 = s.x1 / kTile, ty0 = s.y0 / kTile, ty1 = s.y1 / kTile;
}

__global__ __launch_bounds__(256) void k_rast_zero(int32_t* __restrict__ p, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) p[i] = 0;
}

// FILL = false: counts[view][tile] += 1 per overlapped tile.  FILL = true: the face id into the tile's list at
// ends - counts + cursor++ (guarded: a count that does not match leaves entries out, never writes outside)
template <bool FILL>
__global__ __launch_bounds__(256) void k_rast_bin(RastArgs a, int32_t* __restrict__ counts,
                                                  const int64_t* __restrict__ ends, int32_t* __restrict__ cursor,
                                                  int32_t* __restrict__ pairs, int64_t n_pairs) {
  const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (f >= a.F) return;
  const int tiles = a.tx * a.ty;
  for (int v = 0; v < a.n; ++v) {
    FaceSetup s;
    if (!face_setup(a, v, f, s)) continue;
    int tx0, tx1, ty0, ty1;
    face_tiles(s, tx0, tx1, ty0, ty1);
    for (int y = ty0; y <= ty1; ++y)
      for (int x = tx0; x <= tx1; ++x) {
        const int64_t c = (int64_t)v * tiles + y * a.tx + x;
        if (!FILL) {
          atomicAdd(counts + c, 1);
        } else {
          const int32_t cnt = counts[c];
          const int32_t k = atomicAdd(cursor + c, 1);
          const int64_t pos = ends[c] - cnt + k;
          if (k < cnt && pos >= 0 && pos < n_pairs) pairs[pos] = (int32_t)f;
        }
      }
  }
}

// one pixel centre (column j, row i) against a set-up face: the depth test on the tile's LDS word
__device__ __forceinline__ void rast_pixel(const FaceSetup& s, int j, int i, double zn, double zf,
                                           unsigned long long* slot) {
#pragma clang fp contract(off)
  const double dj = (double)j, di = (double)i;
  const double e0 = (s.n[0][0] * dj + s.n[0][1] * di) + s.n[0][2];
  const double e1 = (s.n[1][0] * dj + s.n[1][1] * di) + s.n[1][2];
  const double e2 = (s.n[2][0] * dj + s.n[2][1] * di) + s.n[2][2];
  if (e0 >= 0.0 && e1 >= 0.0 && e2 >= 0.0) {
    const double z = s.det / ((e0 + e1) + e2);
    if (z >= zn && z <= zf) {
      const unsigned long long bits = (unsigned long long)__double_as_longlong(z);
      if (bits < *slot) atomicMin(slot, bits);  // the read only spares the atomic behind a nearer surface
    }
  }
}

constexpr int kRecDoubles = 10;  // a queued record: the nine edge coefficients and det

// grid (tiles, views)
__global__ __launch_bounds__(256) void k_rast_tile(RastArgs a, const int32_t* __restrict__ counts,
                                                   const int64_t* __restrict__ ends,
                                                   const int32_t* __restrict__ pairs, int64_t n_pairs,
                                                   float* __restrict__ out) {
  __shared__ unsigned long long depth[kTilePix];
  __shared__ double qrec[256][kRecDoubles + 1];  // + 1: rows 88 bytes apart
  __shared__ int qbox[256];                       // x0 | w - 1 | y0 | h - 1 inside the tile, 5 bits each
  __shared__ int qn[2];                           // by chunk parity: the idle one is cleared under the drain
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int view = blockIdx.y, tile = blockIdx.x;
  const int px0 = (tile % a.tx) * kTile, py0 = (tile / a.tx) * kTile;
  const unsigned long long inf_bits = (unsigned long long)__double_as_longlong(INFINITY);
#pragma unroll
  for (int p = t; p < kTilePix; p += 256) depth[p] = inf_bits;
  const int64_t c = (int64_t)view * gridDim.x + tile;
  int64_t end = ends[c];
  end = end < 0 ? 0 : (end > n_pairs ? n_pairs : end);
  int64_t begin = end - counts[c];
  begin = begin < 0 ? 0 : (begin > end ? end : begin);
  if (t == 0) qn[0] = 0;
  __syncthreads();
  int par = 0;
  for (int64_t base = begin; base < end; base += 256, par ^= 1) {
    const int64_t e = base + t;
    if (e < end) {
      const int64_t f = pairs[e];
      FaceSetup s;
      if (f >= 0 && f < a.F && face_setup(a, view, f, s)) {
        const int x0 = max(s.x0, px0), x1 = min(s.x1, px0 + kTile - 1);
        const int y0 = max(s.y0, py0), y1 = min(s.y1, py0 + kTile - 1);
        if (x0 <= x1 && y0 <= y1) {
          if ((x1 - x0 + 1) * (y1 - y0 + 1) <= kSmallPix) {
            for (int i = y0; i <= y1; ++i)
              for (int j = x0; j <= x1; ++j)
                rast_pixel(s, j, i, a.zn, a.zf, depth + (i - py0) * kTile + (j - px0));
          } else {
            const int slot = atomicAdd(&qn[par], 1);
#pragma unroll
            for (int k = 0; k < 3; ++k)
#pragma unroll
              for (int cc = 0; cc < 3; ++cc) qrec[slot][3 * k + cc] = s.n[k][cc];
            qrec[slot][9] = s.det;
            qbox[slot] = (x0 - px0) | (x1 - x0) << 5 | (y0 - py0) << 10 | (y1 - y0) << 15;
          }
        }
      }
    }
    __syncthreads();
    const int nq = qn[par];
    if (t == 0) qn[par ^ 1] = 0;  // last read before this barrier, next used after the one below
    for (int r = wave; r < nq; r += 4) {  // a wave per queued face, lanes over its box
      FaceSetup s;
#pragma unroll
      for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int cc = 0; cc < 3; ++cc) s.n[k][cc] = qrec[r][3 * k + cc];
      s.det = qrec[r][9];
      const int b = qbox[r];
      const int bx = b & 31, bw = (b >> 5 & 31) + 1, by = b >> 10 & 31, bh = (b >> 15 & 31) + 1;
      for (int p = lane; p < bw * bh; p += 64) {
        const int lx = bx + p % bw, ly = by + p / bw;
        rast_pixel(s, px0 + lx, py0 + ly, a.zn, a.zf, depth + ly * kTile + lx);
      }
    }
    __syncthreads();  // the queue is drained before the next chunk appends
  }
  float* img = out + (int64_t)view * a.H * a.W;
#pragma unroll
  for (int p = t; p < kTilePix; p += 256) {
    const int i = py0 + p / kTile, j = px0 + p % kTile;
    if (i < a.H && j < a.W) {
      const unsigned long long bits = depth[p];
      img[(int64_t)i * a.W + j] = bits == inf_bits ? 0.f : (float)__longlong_as_double((long long)bits);
    }
  }
}

// Sum over the 256 threads of a block in a fixed order: xor-shuffles inside a wave, then waves 0..3 (recon.hip's)
__device__ __forceinline__ double block_sum_256(double v, double* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}

// grid (blocks, views): part[view][block] = the block's share of sum |a - b|, elements strided by the grid
__global__ __launch_bounds__(256) void k_depth_l1_partial(const float* __restrict__ x, const float* __restrict__ y,
                                                          int64_t hw, double* __restrict__ part) {
  __shared__ double red[4];
  const float* xa = x + (int64_t)blockIdx.y * hw;
  const float* ya = y + (int64_t)blockIdx.y * hw;
  double s = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < hw; i += (int64_t)gridDim.x * 256)
    s += fabs((double)xa[i] - (double)ya[i]);
  s = block_sum_256(s, red);
  if (threadIdx.x == 0) part[(int64_t)blockIdx.y * kL1Blocks + blockIdx.x] = s;
}

__global__ __launch_bounds__(256) void k_depth_l1_final(const double* __restrict__ part, int32_t nb, int64_t hw,
                                                        double* __restrict__ out) {
  __shared__ double red[4];
  const int t = threadIdx.x;
  const double s = block_sum_256(t < nb ? part[(int64_t)blockIdx.x * kL1Blocks + t] : 0.0, red);
  if (t == 0) out[blockIdx.x] = s / (double)hw;
}

// one thread per point, looping over the views
__global__ __launch_bounds__(256) void k_frustum_seen(const double* __restrict__ pts, int64_t P,
                                                      const double* __restrict__ c2w, int32_t n, double W, double H,
                                                      double fx, double fy, double cx, double cy,
                                                      uint8_t* __restrict__ view_any, uint8_t* __restrict__ point_any) {
#pragma clang fp contract(off)
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= P) return;
  bool any = false;
  for (int v = 0; v < n; ++v) {
    double x, y, z;
    to_camera(c2w + 16 * (int64_t)v, pts + 3 * i, x, y, z);
    const double zz = z + 1e-5;
    const double uu = (fx * x + cx * z) / zz, vv = (fy * y + cy * z) / zz;
    if (zz > 0.0 && uu > 0.0 && uu < W && vv > 0.0 && vv < H) {
      any = true;
      if (view_any) view_any[v] = 1;
    }
  }
  if (any && point_any) point_any[i] = 1;
}

__global__ __launch_bounds__(256) void k_flags_zero(uint8_t* __restrict__ a, int64_t na, uint8_t* __restrict__ b,
                                                    int64_t nb) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (a && i < na) a[i] = 0;
  if (b && i < nb) b[i] = 0;
}

bool rast_args(const pnr_raster* r, RastArgs& a) {
  if (!r || r->V < 0 || r->F < 0 || r->V > kMaxFaces || r->F > kMaxFaces) return false;
  if (r->n_views < 1 || r->n_views > kMaxViews || r->H < 1 || r->W < 1 || r->H > kMaxSide || r->W > kMaxSide) return false;
  if (!(r->z_near > 0.0) || !(r->z_far >= r->z_near) || !(r->z_far < INFINITY)) return false;
  a.verts = r->verts;
  a.faces = r->faces;
  a.c2w = r->c2w;
  a.V = r->V;
  a.F = r->F;
  a.n = r->n_views;
  a.H = r->H;
  a.W = r->W;
  a.tx = (r->W + kTile - 1) / kTile;
  a.ty = (r->H + kTile - 1) / kTile;
  a.fx = r->fx, a.fy = r->fy, a.cx = r->cx, a.cy = r->cy, a.zn = r->z_near, a.zf = r->z_far;
  return (int64_t)a.n * a.tx * a.ty <= kMaxCounters;
}

bool rast_ptrs(const pnr_raster* r) { return r->c2w && (r->F == 0 || (r->faces && (r->V == 0 || r->verts))); }

size_t cursor_bytes(const RastArgs& a) { return ((size_t)a.n * a.tx * a.ty * 4 + 15) / 16 * 16; }

}  // namespace

int64_t raster_counters(const pnr_raster* r) {
  RastArgs a;
  return rast_args(r, a) ? (int64_t)a.n * a.tx * a.ty : 0;
}

size_t raster_workspace_bytes(const pnr_raster* r, int64_t pairs) {
  RastArgs a;
  if (!rast_args(r, a) || pairs < 0 || pairs > kMaxPairs) return 0;
  return cursor_bytes(a) + ((size_t)pairs * 4 + 15) / 16 * 16 + 16;
}

int launch_raster_count(const pnr_raster* r, int32_t* counts, hipStream_t st) {
  RastArgs a;
  if (!rast_args(r, a) || !rast_ptrs(r) || !counts) return PNR_E_ARG;
  const int64_t nc = (int64_t)a.n * a.tx * a.ty;
  hipLaunchKernelGGL(k_rast_zero, dim3((unsigned)((nc + 255) / 256)), dim3(256), 0, st, counts, nc);
  if (a.F > 0)
    hipLaunchKernelGGL(k_rast_bin<false>, dim3((unsigned)((a.F + 255) / 256)), dim3(256), 0, st, a, counts,
                       (const int64_t*)nullptr, (int32_t*)nullptr, (int32_t*)nullptr, (int64_t)0);
  return hip_status(hipGetLastError());
}

int launch_raster_fill(const pnr_raster* r, const int32_t* counts, const int64_t* ends, int64_t pairs, void* ws,
                       size_t ws_bytes, hipStream_t st) {
  RastArgs a;
  if (!rast_args(r, a) || !rast_ptrs(r) || !counts || !ends || pairs < 0 || pairs > kMaxPairs || !ws ||
      (reinterpret_cast<uintptr_t>(ws) & 15))
    return PNR_E_ARG;
  if (ws_bytes < raster_workspace_bytes(r, pairs)) return PNR_E_WORKSPACE;
  const int64_t nc = (int64_t)a.n * a.tx * a.ty;
  int32_t* cursor = static_cast<int32_t*>(ws);
  int32_t* list = reinterpret_cast<int32_t*>(static_cast<char*>(ws) + cursor_bytes(a));
  hipLaunchKernelGGL(k_rast_zero, dim3((unsigned)((nc + 255) / 256)), dim3(256), 0, st, cursor, nc);
  if (a.F > 0 && pairs > 0)
    hipLaunchKernelGGL(k_rast_bin<true>, dim3((unsigned)((a.F + 255) / 256)), dim3(256), 0, st, a,
                       const_cast<int32_t*>(counts), ends, cursor, list, pairs);
  return hip_status(hipGetLastError());
}

int launch_raster_tiles(const pnr_raster* r, const int32_t* counts, const int64_t* ends, int64_t pairs, float* depth,
                        const void* ws, size_t ws_bytes, hipStream_t st) {
  RastArgs a;
  if (!rast_args(r, a) || !rast_ptrs(r) || !counts || !ends || pairs < 0 || pairs > kMaxPairs || !depth || !ws ||
      (reinterpret_cast<uintptr_t>(ws) & 15))
    return PNR_E_ARG;
  if (ws_bytes < raster_workspace_bytes(r, pairs)) return PNR_E_WORKSPACE;
  const int32_t* list = reinterpret_cast<const int32_t*>(static_cast<const char*>(ws) + cursor_bytes(a));
  hipLaunchKernelGGL(k_rast_tile, dim3((unsigned)(a.tx * a.ty), (unsigned)a.n), dim3(256), 0, st, a, counts, ends, list,
                     pairs, depth);
  return hip_status(hipGetLastError());
}

size_t depth_l1_workspace_bytes(int64_t n) {
  return n < 1 || n > kMaxCounters ? 0 : (size_t)n * kL1Blocks * 8;
}

int launch_depth_l1(const float* x, const float* y, int64_t n, int64_t hw, double* out, void* ws, size_t ws_bytes,
                    hipStream_t st) {
  if (n < 1 || n > 65535 || hw < 1 || hw > (int64_t)kMaxSide * kMaxSide || !x || !y || !out || !ws ||
      (reinterpret_cast<uintptr_t>(ws) & 7))
    return PNR_E_ARG;
  if (ws_bytes < depth_l1_workspace_bytes(n)) return PNR_E_WORKSPACE;
  const int nb = (int)(hw < (int64_t)kL1Blocks * 256 ? (hw + 255) / 256 : kL1Blocks);
  double* part = static_cast<double*>(ws);
  hipLaunchKernelGGL(k_depth_l1_partial, dim3(nb, (unsigned)n), dim3(256), 0, st, x, y, hw, part);
  hipLaunchKernelGGL(k_depth_l1_final, dim3((unsigned)n), dim3(256), 0, st, part, nb, hw, out);
  return hip_status(hipGetLastError());
}

int launch_frustum_seen(const double* pts, int64_t P, const double* c2w, int32_t n, int32_t H, int32_t W, double fx,
                        double fy, double cx, double cy, uint8_t* view_any, uint8_t* point_any, hipStream_t st) {
  if (P < 0 || P > kMaxFaces || n < 0 || n > (1 << 24) || H < 1 || W < 1) return PNR_E_ARG;
  if ((P > 0 && !pts) || (n > 0 && !c2w) || (!view_any && !point_any)) return PNR_E_ARG;
  const int64_t nv = view_any ? n : 0, np = point_any ? P : 0, nz = nv > np ? nv : np;
  if (nz > 0)
    hipLaunchKernelGGL(k_flags_zero, dim3((unsigned)((nz + 255) / 256)), dim3(256), 0, st, view_any, (int64_t)n,
                       point_any, P);
  if (P > 0 && n > 0)
    hipLaunchKernelGGL(k_frustum_seen, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, st, pts, P, c2w, n, (double)W,
                       (double)H, fx, fy, cx, cy, view_any, point_any);
  return hip_status(hipGetLastError());
}

}  // namespace pnr
