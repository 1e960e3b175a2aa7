// mesh.hip -- the geometry between the Mesher's grid query and its vertex colouring
// (src/utils/Mesher.py:349-574): the seen / forecast point masks (Mesher.point_masks, :53-212) and
// marching cubes over the occupancy volume (the reference calls skimage.measure.marching_cubes).
//
// Point masks: one thread per point, a loop over the K keyframes, the reference's fp32 arithmetic
// restated per keyframe (cam = w2c [p;1], cam.x *= -1, uv = K cam, z = uv.z + 1e-8, uv.xy /= z).  The
// 4x4 matrices are read with wave-uniform addresses (scalar loads).  depth_test=True needs
// max_k(depth_sample) over all points of the call before any mask is decided: a partial-maximum
// pass per block and keyframe and a final pass per keyframe run first (fixed order, and max is exact,
// so the result does not depend on the schedule).
//
// Marching cubes: three launches, no atomics, so the output order is a function of the volume alone.
//   k_mc_count   one thread per grid point (ix, iy, iz), linear id (ix ny + iy) nz + iz.  A point owns
//                the three grid edges that leave it towards +x, +y, +z (0..3 vertices) and, when it is
//                the minimum corner of a cell, that cell's triangles (mc_table.h).  The block scans
//                both counts and stores one word per point: its edge mask, case and block-local
//                offsets; the block totals go to the workspace.
//   k_mc_scan    one block: exclusive scan of the block totals, grand totals to the caller.
//   k_mc_emit    writes the float64 vertices and the int32 faces at the scanned offsets; a face finds a
//                vertex through the word of the grid point that owns the edge.
#include <hip/hip_runtime.h>

#include "mc_table.h"
#include "pnr_internal.h"

namespace pnr {
namespace {

constexpr int kMeshBlock = 256;
constexpr int kScanBlock = 1024;

// ---- point masks -----------------------------------------------------------------------------
struct Proj {
  float u, v, z, proj;
};

__device__ inline Proj project(const float* __restrict__ m, float px, float py, float pz, float fx, float fy,
                               float cx, float cy) {
  const float x = -(m[0] * px + m[1] * py + m[2] * pz + m[3]);
  const float y = m[4] * px + m[5] * py + m[6] * pz + m[7];
  const float zc = m[8] * px + m[9] * py + m[10] * pz + m[11];
  Proj r;
  r.z = zc + 1e-8f;
  r.u = (fx * x + cx * zc) / r.z;
  r.v = (fy * y + cy * zc) / r.z;
  r.proj = -zc;
  return r;
}

// F.grid_sample(bilinear, padding_mode='zeros', align_corners=True) of one (H, W) image at the pixel
// (u, v), through the reference's normalisation (Mesher.py:161-162) and torch's inverse of it
__device__ inline float depth_sample(const float* __restrict__ img, int H, int W, float u, float v) {
  const float gx = u / (float)(W - 1) * 2.0f - 1.0f;
  const float gy = v / (float)(H - 1) * 2.0f - 1.0f;
  const float ix = ((gx + 1.0f) / 2.0f) * (float)(W - 1);
  const float iy = ((gy + 1.0f) / 2.0f) * (float)(H - 1);
  const float x0 = floorf(ix), y0 = floorf(iy);
  const float x1 = x0 + 1.0f, y1 = y0 + 1.0f;
  const float xmax = (float)(W - 1), ymax = (float)(H - 1);
  const bool bx0 = x0 >= 0.0f && x0 <= xmax, bx1 = x1 >= 0.0f && x1 <= xmax;
  const bool by0 = y0 >= 0.0f && y0 <= ymax, by1 = y1 >= 0.0f && y1 <= ymax;
  float out = 0.0f;
  if (bx0 && by0) out += img[(int64_t)y0 * W + (int64_t)x0] * ((x1 - ix) * (y1 - iy));
  if (bx1 && by0) out += img[(int64_t)y0 * W + (int64_t)x1] * ((ix - x0) * (y1 - iy));
  if (bx0 && by1) out += img[(int64_t)y1 * W + (int64_t)x0] * ((x1 - ix) * (iy - y0));
  if (bx1 && by1) out += img[(int64_t)y1 * W + (int64_t)x1] * ((ix - x0) * (iy - y0));
  return out;
}

// torch.max: a NaN wins
__device__ inline float max_nan(float a, float b) { return (a != a) ? a : ((b != b) ? b : fmaxf(a, b)); }

__device__ inline float block_max(float v, float* sh) {
  const int t = threadIdx.x;
  sh[t] = v;
  __syncthreads();
  for (int s = kMeshBlock / 2; s > 0; s >>= 1) {
    if (t < s) sh[t] = max_nan(sh[t], sh[t + s]);
    __syncthreads();
  }
  const float r = sh[0];
  __syncthreads();
  return r;
}

// part[k * gridDim.x + block] = max over the block's points of depth_sample_k
__global__ __launch_bounds__(kMeshBlock) void k_mask_depth_part(const float* __restrict__ pts, int64_t P,
                                                                 const float* __restrict__ w2c, int K, int H, int W,
                                                                 float fx, float fy, float cx, float cy,
                                                                 const float* __restrict__ depth,
                                                                 float* __restrict__ part) {
  __shared__ float sh[kMeshBlock];
  const int64_t i = (int64_t)blockIdx.x * kMeshBlock + threadIdx.x;
  const bool live = i < P;
  const float px = live ? pts[3 * i] : 0.0f, py = live ? pts[3 * i + 1] : 0.0f, pz = live ? pts[3 * i + 2] : 0.0f;
  for (int k = 0; k < K; ++k) {
    float ds = -INFINITY;
    if (live) {
      const Proj r = project(w2c + 16 * k, px, py, pz, fx, fy, cx, cy);
      ds = depth_sample(depth + (int64_t)k * H * W, H, W, r.u, r.v);
    }
    const float m = block_max(ds, sh);
    if (threadIdx.x == 0) part[(int64_t)k * gridDim.x + blockIdx.x] = m;
  }
}

// maxd[k] = max over the n_part partial maxima of keyframe k (one block per keyframe)
__global__ __launch_bounds__(kMeshBlock) void k_mask_depth_final(const float* __restrict__ part, int64_t n_part,
                                                                  float* __restrict__ maxd) {
  __shared__ float sh[kMeshBlock];
  const float* p = part + (int64_t)blockIdx.x * n_part;
  float m = -INFINITY;
  for (int64_t j = threadIdx.x; j < n_part; j += kMeshBlock) m = max_nan(m, p[j]);
  m = block_max(m, sh);
  if (threadIdx.x == 0) maxd[blockIdx.x] = m;
}

template <int MODE>
__global__ __launch_bounds__(kMeshBlock) void k_point_masks(const float* __restrict__ pts, int64_t P,
                                                             const float* __restrict__ w2c, int K, int H, int W,
                                                             float fx, float fy, float cx, float cy,
                                                             const float* __restrict__ depth,
                                                             const float* __restrict__ maxd,
                                                             uint8_t* __restrict__ seen_out,
                                                             uint8_t* __restrict__ fore_out) {
  const int64_t i = (int64_t)blockIdx.x * kMeshBlock + threadIdx.x;
  if (i >= P) return;
  const float px = pts[3 * i], py = pts[3 * i + 1], pz = pts[3 * i + 2];
  const float fw = (float)W, fh = (float)H;
  bool seen = false, fore = false;
  for (int k = 0; k < K; ++k) {
    const Proj r = project(w2c + 16 * k, px, py, pz, fx, fy, cx, cy);
    const bool front = r.z < 0.0f;
    bool cs = r.u < fw && r.u > 0.0f && r.v < fh && r.v > 0.0f && front;
    bool cf = r.u < fw + 1000.0f && r.u > -1000.0f && r.v < fh + 1000.0f && r.v > -1000.0f && front;
    if (MODE == PNR_MASK_MAX_DEPTH) {
      const float md = maxd[k];
      cs = cs && r.proj < md;
      cf = cf && r.proj < md;
    } else if (MODE == PNR_MASK_DEPTH_TEST) {
      const float md = maxd[k];
      cf = cf && r.proj < md;
      if (cs) {
        const float ds = depth_sample(depth + (int64_t)k * H * W, H, W, r.u, r.v);
        cs = (r.proj < ds + 2.4f) && (ds - 2.4f < r.proj);
      }
    }
    seen = seen || cs;
    fore = fore || cf;
  }
  seen_out[i] = seen ? 1 : 0;
  fore_out[i] = (fore && !seen) ? 1 : 0;
}

// ---- marching cubes --------------------------------------------------------------------------
// word of a grid point: bits 0-2 owned crossing edges (x, y, z), 3-12 block-local vertex offset
// (<= 255 * 3), 13-23 block-local triangle offset (<= 255 * MC_MAX_TRI), 24-31 the cell's case
static_assert((kMeshBlock - 1) * 3 < (1 << 10) && (kMeshBlock - 1) * MC_MAX_TRI < (1 << 11), "word fields");

struct McGrid {
  const float* vol;
  int64_t nx, ny, nz, sx, sy, sz, n;
  double level;
};

__device__ inline bool below(const McGrid& g, int64_t ix, int64_t iy, int64_t iz) {
  return (double)g.vol[ix * g.sx + iy * g.sy + iz * g.sz] < g.level;
}

__global__ __launch_bounds__(kMeshBlock) void k_mc_count(McGrid g, uint32_t* __restrict__ word,
                                                          int32_t* __restrict__ blk_v, int32_t* __restrict__ blk_t) {
  __shared__ int sv[kMeshBlock], st[kMeshBlock];
  const int t = threadIdx.x;
  const int64_t gid = (int64_t)blockIdx.x * kMeshBlock + t;
  int nv = 0, nt = 0;
  uint32_t mask = 0, cs = 0;
  if (gid < g.n) {
    const int64_t iz = gid % g.nz, iy = (gid / g.nz) % g.ny, ix = gid / (g.nz * g.ny);
    const bool hx = ix + 1 < g.nx, hy = iy + 1 < g.ny, hz = iz + 1 < g.nz;
    const bool b0 = below(g, ix, iy, iz);
    const bool bx = hx ? below(g, ix + 1, iy, iz) : b0;
    const bool by = hy ? below(g, ix, iy + 1, iz) : b0;
    const bool bz = hz ? below(g, ix, iy, iz + 1) : b0;
    mask = (uint32_t)(bx != b0) | ((uint32_t)(by != b0) << 1) | ((uint32_t)(bz != b0) << 2);
    nv = __popc(mask);
    if (hx && hy && hz) {
      cs = (uint32_t)b0 | ((uint32_t)bx << 1) | ((uint32_t)by << 2) | ((uint32_t)below(g, ix + 1, iy + 1, iz) << 3) |
           ((uint32_t)bz << 4) | ((uint32_t)below(g, ix + 1, iy, iz + 1) << 5) |
           ((uint32_t)below(g, ix, iy + 1, iz + 1) << 6) | ((uint32_t)below(g, ix + 1, iy + 1, iz + 1) << 7);
      nt = MC_NTRI[cs];
    }
  }
  sv[t] = nv;
  st[t] = nt;
  __syncthreads();
  for (int s = 1; s < kMeshBlock; s <<= 1) {   // inclusive scan of both counts
    const int av = t >= s ? sv[t - s] : 0, at = t >= s ? st[t - s] : 0;
    __syncthreads();
    sv[t] += av;
    st[t] += at;
    __syncthreads();
  }
  if (gid < g.n) word[gid] = mask | ((uint32_t)(sv[t] - nv) << 3) | ((uint32_t)(st[t] - nt) << 13) | (cs << 24);
  if (t == kMeshBlock - 1) {
    blk_v[blockIdx.x] = sv[t];
    blk_t[blockIdx.x] = st[t];
  }
}

// one block: blk_v / blk_t (n_blk totals) -> exclusive offsets in place, grand totals to n_v / n_t
__global__ __launch_bounds__(kScanBlock) void k_mc_scan(int32_t* __restrict__ blk_v, int32_t* __restrict__ blk_t,
                                                         int64_t n_blk, int64_t* __restrict__ n_v,
                                                         int64_t* __restrict__ n_t) {
  __shared__ long long sv[kScanBlock], st[kScanBlock];
  const int t = threadIdx.x;
  const int64_t per = (n_blk + kScanBlock - 1) / kScanBlock;
  const int64_t lo = (int64_t)t * per, hi = lo + per < n_blk ? lo + per : n_blk;
  long long av = 0, at = 0;
  for (int64_t j = lo; j < hi; ++j) {
    av += blk_v[j];
    at += blk_t[j];
  }
  sv[t] = av;
  st[t] = at;
  __syncthreads();
  for (int s = 1; s < kScanBlock; s <<= 1) {
    const long long bv = t >= s ? sv[t - s] : 0, bt = t >= s ? st[t - s] : 0;
    __syncthreads();
    sv[t] += bv;
    st[t] += bt;
    __syncthreads();
  }
  long long ov = sv[t] - av, ot = st[t] - at;
  for (int64_t j = lo; j < hi; ++j) {
    const int32_t cv = blk_v[j], ct = blk_t[j];
    blk_v[j] = (int32_t)ov;
    blk_t[j] = (int32_t)ot;
    ov += cv;
    ot += ct;
  }
  if (t == kScanBlock - 1) {
    *n_v = sv[t];
    *n_t = st[t];
  }
}

struct McFrame {
  double origin[3], spacing[3];
};

__global__ __launch_bounds__(kMeshBlock) void k_mc_emit(McGrid g, McFrame fr, const uint32_t* __restrict__ word,
                                                         const int32_t* __restrict__ blk_v,
                                                         const int32_t* __restrict__ blk_t,
                                                         double* __restrict__ verts, int32_t* __restrict__ faces) {
  const int64_t gid = (int64_t)blockIdx.x * kMeshBlock + threadIdx.x;
  if (gid >= g.n) return;
  const uint32_t w = word[gid];
  const uint32_t mask = w & 7u, cs = w >> 24;
  if (mask == 0 && cs == 0) return;
  const int64_t iz = gid % g.nz, iy = (gid / g.nz) % g.ny, ix = gid / (g.nz * g.ny);
  if (mask) {
    const int64_t at = ix * g.sx + iy * g.sy + iz * g.sz;
    const double a = (double)g.vol[at];
    int64_t v = (int64_t)blk_v[blockIdx.x] + ((w >> 3) & 1023u);
    const double pos[3] = {(double)ix, (double)iy, (double)iz};
    const int64_t step[3] = {g.sx, g.sy, g.sz};
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) {
      if (!(mask & (1u << ax))) continue;
      const double b = (double)g.vol[at + step[ax]];
      const double tt = (g.level - a) / (b - a);
#pragma unroll
      for (int c = 0; c < 3; ++c)
        verts[3 * v + c] = fr.origin[c] + (pos[c] + (c == ax ? tt : 0.0)) * fr.spacing[c];
      ++v;
    }
  }
  const int nt = MC_NTRI[cs];
  if (nt == 0) return;
  int64_t f = (int64_t)blk_t[blockIdx.x] + ((w >> 13) & 2047u);
  for (int k = 0; k < nt; ++k, ++f) {
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const int e = MC_TRI[cs][3 * k + j];
      const int ax = e >> 2, db = e & 1, dc = (e >> 1) & 1;
      // the two other axes in increasing order carry (db, dc)
      const int ox = ax == 0 ? 0 : db, oy = ax == 1 ? 0 : (ax == 0 ? db : dc), oz = ax == 2 ? 0 : dc;
      const int64_t n = ((ix + ox) * g.ny + (iy + oy)) * g.nz + (iz + oz);
      const uint32_t wn = word[n];
      faces[3 * f + j] =
          blk_v[n / kMeshBlock] + (int32_t)((wn >> 3) & 1023u) + __popc(wn & ((1u << ax) - 1u));
    }
  }
}

}  // namespace

int64_t point_masks_parts(int64_t P) { return (P + kMeshBlock - 1) / kMeshBlock; }

int launch_point_masks(const float* pts, int64_t P, const float* w2c, int K, int H, int W, float fx, float fy,
                       float cx, float cy, int mode, const float* depth, const float* max_depth, uint8_t* seen,
                       uint8_t* fore, float* ws, hipStream_t st) {
  if (P == 0) return 0;
  const int64_t nb = point_masks_parts(P);
  if (mode == PNR_MASK_DEPTH_TEST) {
    float* maxd = ws;            // K floats, then K * nb partial maxima
    float* part = ws + K;
    k_mask_depth_part<<<dim3((unsigned)nb), kMeshBlock, 0, st>>>(pts, P, w2c, K, H, W, fx, fy, cx, cy, depth, part);
    k_mask_depth_final<<<dim3((unsigned)K), kMeshBlock, 0, st>>>(part, nb, maxd);
    k_point_masks<PNR_MASK_DEPTH_TEST><<<dim3((unsigned)nb), kMeshBlock, 0, st>>>(pts, P, w2c, K, H, W, fx, fy, cx, cy,
                                                                               depth, maxd, seen, fore);
  } else if (mode == PNR_MASK_MAX_DEPTH) {
    k_point_masks<PNR_MASK_MAX_DEPTH><<<dim3((unsigned)nb), kMeshBlock, 0, st>>>(pts, P, w2c, K, H, W, fx, fy, cx, cy,
                                                                              nullptr, max_depth, seen, fore);
  } else {
    k_point_masks<PNR_MASK_POSES><<<dim3((unsigned)nb), kMeshBlock, 0, st>>>(pts, P, w2c, K, H, W, fx, fy, cx, cy,
                                                                          nullptr, nullptr, seen, fore);
  }
  return hip_status(hipGetLastError());
}

int64_t mc_blocks(int64_t n) { return (n + kMeshBlock - 1) / kMeshBlock; }
int mc_max_tri() { return MC_MAX_TRI; }

namespace {
struct McWs {
  int32_t *blk_v, *blk_t;
  uint32_t* word;
};
McWs mc_ws(void* ws, int64_t n) {
  const int64_t nb = (mc_blocks(n) + 63) / 64 * 64;
  McWs w;
  w.blk_v = static_cast<int32_t*>(ws);
  w.blk_t = w.blk_v + nb;
  w.word = reinterpret_cast<uint32_t*>(w.blk_t + nb);
  return w;
}
}  // namespace

int64_t mc_workspace_bytes(int64_t n) { return ((mc_blocks(n) + 63) / 64 * 64 * 2 + n) * 4; }

int launch_mc_count(const float* vol, int64_t nx, int64_t ny, int64_t nz, int64_t sx, int64_t sy, int64_t sz,
                    double level, void* ws, int64_t* n_v, int64_t* n_t, hipStream_t st) {
  const McGrid g{vol, nx, ny, nz, sx, sy, sz, nx * ny * nz, level};
  const McWs w = mc_ws(ws, g.n);
  const int64_t nb = mc_blocks(g.n);
  k_mc_count<<<dim3((unsigned)nb), kMeshBlock, 0, st>>>(g, w.word, w.blk_v, w.blk_t);
  k_mc_scan<<<1, kScanBlock, 0, st>>>(w.blk_v, w.blk_t, nb, n_v, n_t);
  return hip_status(hipGetLastError());
}

int launch_mc_emit(const float* vol, int64_t nx, int64_t ny, int64_t nz, int64_t sx, int64_t sy, int64_t sz,
                   double level, const double* origin, const double* spacing, const void* ws, double* verts,
                   int32_t* faces, hipStream_t st) {
  const McGrid g{vol, nx, ny, nz, sx, sy, sz, nx * ny * nz, level};
  const McWs w = mc_ws(const_cast<void*>(ws), g.n);
  McFrame fr;
  for (int a = 0; a < 3; ++a) {
    fr.origin[a] = origin[a];
    fr.spacing[a] = spacing[a];
  }
  k_mc_emit<<<dim3((unsigned)mc_blocks(g.n)), kMeshBlock, 0, st>>>(g, fr, w.word, w.blk_v, w.blk_t, verts, faces);
  return hip_status(hipGetLastError());
}

}  // namespace pnr
