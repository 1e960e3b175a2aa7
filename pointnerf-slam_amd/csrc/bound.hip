// bound.hip -- the device passes of the mesh bound (src/utils/Mesher.py:214-279, used at :426-433 and
// :475-485).
//
// The reference fuses the keyframes' depth into an open3d TSDF volume and takes the convex hull of the
// fused surface.  Here the hull is taken over the point set P itself -- every valid depth pixel of every
// keyframe, back-projected by the device function the map growth uses (window_sample.h backproject), plus
// the camera centres -- by a quickhull on the host (pnr/bound.py) that never holds P: each of its passes
// over P is one call of the support function below.
//   k_bound_support   persistent workgroups over tiles of 1,024 point slots.  A tile is back-projected
//                     once (4 slots per thread) into LDS as (x, y, z, index) rows, an invalid slot as a
//                     NaN row; then every thread runs its directions -- held in registers -- over the
//                     tile's rows (LDS broadcast reads): 5 unfused float32 operations, one compare and
//                     two selects per point and direction.  D <= 256 directions: a power-of-two number dg
//                     of direction slots, and the 256 / dg threads that share a slot take interleaved
//                     rows of the tile and are combined through LDS when the workgroup is done.
//                     256 < D <= 1,024: 2 or 4 directions per thread.  A strict `>` over rows in index
//                     order keeps the smallest index of a maximum; the combine and the reduce break
//                     ties by index, so the result is the same for every grid.  One (value, index) row
//                     per workgroup, plain stores.
//   k_bound_reduce    one thread per direction over the workgroups' rows in workgroup order.
//   k_bound_points    positions of given indices through the same slot function.
//   k_bound_contains  one thread per point, planes staged through LDS 256 at a time (wave-uniform
//                     reads), unfused float64; a wave leaves the facet loop once none of its lanes is
//                     still inside.
// No float atomics, no atomics at all.
#include <float.h>

#include "pnr_internal.h"
#include "points_hash.h"
#include "window_sample.h"

namespace pnr {

namespace {

constexpr int kTile = 1024;        // point slots per tile (4 per thread)
constexpr int kBoundMaxDirs = 1024;
constexpr int kBoundMaxWg = 1024;  // rows of the partial buffers
constexpr int kPlaneChunk = 256;   // planes per LDS stage (8 KiB)

static inline size_t a256(size_t x) { return (x + 255) / 256 * 256; }

struct BoundArgs {
  pnr_bound_frames f;
  int64_t hw;         // H W
  int64_t n0;         // K H W: index of the first extra point
  int64_t per_frame;  // lattice points per keyframe
  int64_t n_lat;      // K per_frame
  int64_t n_slots;    // n_lat + n_extra
  int64_t n_tiles;
  int32_t nW;         // lattice columns
  const float* dirs;
  int32_t D;
  int32_t dg_log2;    // log2 of the direction slots of a workgroup pass (D <= 256), 8 otherwise
  float* part_h;      // [workgroups][D]
  int32_t* part_i;
};

// Slot s of the point set: lattice point s of the keyframes in index order, then the extra points.
// Returns the point's index, or -1 (and a NaN position) when the slot holds no valid point.
__device__ __forceinline__ int64_t slot_point(const BoundArgs& a, int64_t s, float& x, float& y, float& z) {
  PNR_FP_STRICT
  x = y = z = __int_as_float(0x7FC00000);
  if (s < 0 || s >= a.n_slots) return -1;
  if (s < a.n_lat) {
    const int64_t k = s / a.per_frame;
    const int64_t r = s - k * a.per_frame;
    const int row = (int)(r / a.nW);
    const int v = row * a.f.stride;
    const int u = (int)(r - (int64_t)row * a.nW) * a.f.stride;
    const int64_t pix = (int64_t)v * a.f.W + u;
    const float d = a.f.depth[k * a.hw + pix];
    if (!(d > 0.f && d <= a.f.depth_trunc && d <= FLT_MAX)) return -1;
    backproject((float)u, (float)v, d, a.f.fx, a.f.fy, a.f.cx, a.f.cy, a.f.c2w + k * 16, x, y, z);
    return k * a.hw + pix;
  }
  const int64_t e = s - a.n_lat;
  const float ex = a.f.extra_xyz[e * 3 + 0], ey = a.f.extra_xyz[e * 3 + 1], ez = a.f.extra_xyz[e * 3 + 2];
  if (ex != ex || ey != ey || ez != ez) return -1;
  x = ex;
  y = ey;
  z = ez;
  return a.n0 + e;
}

// (value, index) b beats a: a larger value, or the same value at a smaller index
__device__ __forceinline__ bool beats(float bv, int bi, float av, int ai) { return bv > av || (bv == av && bi < ai); }

template <int DPL>
__global__ __launch_bounds__(256) void k_bound_support(BoundArgs a) {
  PNR_FP_STRICT
  __shared__ int4 s_pt[kTile];
  __shared__ float s_h[256];
  __shared__ int s_i[256];
  const int t = threadIdx.x;
  const int dg = 1 << a.dg_log2;
  const int dsl = t & (dg - 1);
  const int sub = t >> a.dg_log2;
  const int nsub = 256 >> a.dg_log2;
  float nx[DPL], ny[DPL], nz[DPL], best[DPL];
  int bi[DPL];
#pragma unroll
  for (int i = 0; i < DPL; ++i) {
    const int d = dsl + 256 * i;
    const bool ok = d < a.D;
    nx[i] = ok ? a.dirs[d * 3 + 0] : 0.f;
    ny[i] = ok ? a.dirs[d * 3 + 1] : 0.f;
    nz[i] = ok ? a.dirs[d * 3 + 2] : 0.f;
    best[i] = -INFINITY;
    bi[i] = -1;
  }
  for (int64_t tile = blockIdx.x; tile < a.n_tiles; tile += gridDim.x) {
    __syncthreads();  // the previous tile's rows are no longer read
#pragma unroll
    for (int q = 0; q < kTile / 256; ++q) {
      const int j = q * 256 + t;
      float x, y, z;
      const int64_t idx = slot_point(a, tile * kTile + j, x, y, z);
      s_pt[j] = make_int4(__float_as_int(x), __float_as_int(y), __float_as_int(z), (int)idx);
    }
    __syncthreads();
#pragma unroll 4
    for (int j = sub; j < kTile; j += nsub) {
      const int4 p = s_pt[j];
      const float px = __int_as_float(p.x), py = __int_as_float(p.y), pz = __int_as_float(p.z);
#pragma unroll
      for (int i = 0; i < DPL; ++i) {
        const float v = (px * nx[i] + py * ny[i]) + pz * nz[i];
        const bool up = v > best[i];  // a NaN row (an invalid slot) never wins
        best[i] = up ? v : best[i];
        bi[i] = up ? p.w : bi[i];
      }
    }
  }
  if (nsub > 1) {  // (DPL == 1) the threads that share a direction slot
    __syncthreads();
    s_h[t] = best[0];
    s_i[t] = bi[0];
    __syncthreads();
    if (t < dg) {
      for (int q = 1; q < nsub; ++q) {
        const float ov = s_h[q * dg + t];
        const int oi = s_i[q * dg + t];
        if (beats(ov, oi, best[0], bi[0])) {
          best[0] = ov;
          bi[0] = oi;
        }
      }
    }
  }
  if (sub == 0) {
#pragma unroll
    for (int i = 0; i < DPL; ++i) {
      const int d = dsl + 256 * i;
      if (d < a.D) {
        a.part_h[(int64_t)blockIdx.x * a.D + d] = best[i];
        a.part_i[(int64_t)blockIdx.x * a.D + d] = bi[i];
      }
    }
  }
}

__global__ __launch_bounds__(256) void k_bound_reduce(const float* __restrict__ part_h,
                                                      const int32_t* __restrict__ part_i, int nwg, int D,
                                                      float* __restrict__ h, int64_t* __restrict__ arg) {
  const int d = blockIdx.x * 256 + threadIdx.x;
  if (d >= D) return;
  float bv = -INFINITY;
  int bi = -1;
  for (int g = 0; g < nwg; ++g) {
    const float ov = part_h[(int64_t)g * D + d];
    const int oi = part_i[(int64_t)g * D + d];
    if (beats(ov, oi, bv, bi)) {
      bv = ov;
      bi = oi;
    }
  }
  h[d] = bv;
  arg[d] = (int64_t)bi;
}

__global__ __launch_bounds__(256) void k_bound_points(BoundArgs a, const int64_t* __restrict__ idx, int64_t n,
                                                      float* __restrict__ xyz) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int64_t g = idx[i];
  int64_t s = -1;
  if (g >= 0 && g < a.n0) {
    const int64_t k = g / a.hw;
    const int64_t pix = g - k * a.hw;
    const int v = (int)(pix / a.f.W);
    const int u = (int)(pix - (int64_t)v * a.f.W);
    if (v % a.f.stride == 0 && u % a.f.stride == 0) s = k * a.per_frame + (int64_t)(v / a.f.stride) * a.nW + u / a.f.stride;
  } else if (g >= a.n0 && g < a.n0 + a.f.n_extra) {
    s = a.n_lat + (g - a.n0);
  }
  float x, y, z;
  slot_point(a, s, x, y, z);
  xyz[i * 3 + 0] = x;
  xyz[i * 3 + 1] = y;
  xyz[i * 3 + 2] = z;
}

template <typename T>
__global__ __launch_bounds__(256) void k_bound_contains(const T* __restrict__ p, int64_t P,
                                                        const double* __restrict__ planes, int F,
                                                        uint8_t* __restrict__ inside) {
  PNR_FP_STRICT
  __shared__ double s_pl[kPlaneChunk * 4];
  const int t = threadIdx.x;
  const int64_t i = (int64_t)blockIdx.x * 256 + t;
  const bool in = i < P;
  double x = 0.0, y = 0.0, z = 0.0;
  if (in) {
    x = (double)p[i * 3 + 0];
    y = (double)p[i * 3 + 1];
    z = (double)p[i * 3 + 2];
  }
  bool ok = in;
  for (int f0 = 0; f0 < F; f0 += kPlaneChunk) {
    const int nf = F - f0 < kPlaneChunk ? F - f0 : kPlaneChunk;
    __syncthreads();
    for (int q = t; q < nf * 4; q += 256) s_pl[q] = planes[(int64_t)f0 * 4 + q];
    __syncthreads();
    if (__any(ok)) {
      for (int f = 0; f < nf; ++f) {
        const double a = s_pl[f * 4 + 0], b = s_pl[f * 4 + 1], c = s_pl[f * 4 + 2], d = s_pl[f * 4 + 3];
        ok = ok && ((x * a + y * b) + z * c <= d);
        if ((f & 7) == 7 && !__any(ok)) break;  // wave-uniform: no lane of the wave is still inside
      }
    }
  }
  if (in) inside[i] = ok ? 1 : 0;
}

// The geometry of a call; false = bad arguments.
static bool bound_geometry(const pnr_bound_frames& f, BoundArgs& a) {
  if (f.K < 0 || f.stride < 1 || f.n_extra < 0) return false;
  if (f.K > 0 && (f.H < 1 || f.W < 1 || !f.depth || !f.c2w)) return false;
  if (f.n_extra > 0 && !f.extra_xyz) return false;
  a = BoundArgs{};
  a.f = f;
  a.hw = f.K > 0 ? (int64_t)f.H * f.W : 1;
  a.n0 = f.K > 0 ? (int64_t)f.K * a.hw : 0;
  if (a.n0 >= (1LL << 31) || f.n_extra >= (1LL << 31) || a.n0 + f.n_extra >= (1LL << 31)) return false;
  a.nW = f.K > 0 ? (f.W + f.stride - 1) / f.stride : 1;
  a.per_frame = f.K > 0 ? (int64_t)((f.H + f.stride - 1) / f.stride) * a.nW : 1;
  a.n_lat = f.K > 0 ? (int64_t)f.K * a.per_frame : 0;
  a.n_slots = a.n_lat + f.n_extra;
  a.n_tiles = (a.n_slots + kTile - 1) / kTile;
  return true;
}

}  // namespace

int bound_support_max_dirs() { return kBoundMaxDirs; }

size_t bound_support_workspace_bytes(const pnr_bound_frames& f, int32_t D) {
  BoundArgs a;
  if (D < 0 || D > kBoundMaxDirs || !bound_geometry(f, a)) return 0;
  const int64_t rows = a.n_tiles < kBoundMaxWg ? (a.n_tiles > 0 ? a.n_tiles : 1) : kBoundMaxWg;
  return 2 * a256((size_t)rows * (size_t)(D > 0 ? D : 1) * 4);
}

int launch_bound_support(const pnr_bound_frames& f, const float* dirs, int32_t D, float* h, int64_t* arg, void* ws,
                         size_t ws_bytes, hipStream_t st) {
  BoundArgs a;
  if (D < 0 || D > kBoundMaxDirs || !bound_geometry(f, a)) return PNR_E_ARG;
  if (D == 0) return PNR_OK;
  if (!dirs || !h || !arg) return PNR_E_ARG;
  const size_t need = bound_support_workspace_bytes(f, D);
  if (!ws || ws_bytes < need) return PNR_E_WORKSPACE;
  a.dirs = dirs;
  a.D = D;
  a.part_h = static_cast<float*>(ws);
  a.part_i = reinterpret_cast<int32_t*>(static_cast<char*>(ws) + need / 2);
  int64_t nwg = 2 * (int64_t)device_cu_count();
  if (nwg > kBoundMaxWg) nwg = kBoundMaxWg;
  if (nwg > a.n_tiles) nwg = a.n_tiles;
  if (nwg > 0) {
    if (D <= 256) {
      a.dg_log2 = 0;
      while ((1 << a.dg_log2) < D) ++a.dg_log2;
      hipLaunchKernelGGL(k_bound_support<1>, dim3((unsigned)nwg), dim3(256), 0, st, a);
    } else {
      a.dg_log2 = 8;
      if (D <= 512)
        hipLaunchKernelGGL(k_bound_support<2>, dim3((unsigned)nwg), dim3(256), 0, st, a);
      else
        hipLaunchKernelGGL(k_bound_support<4>, dim3((unsigned)nwg), dim3(256), 0, st, a);
    }
  }
  hipLaunchKernelGGL(k_bound_reduce, dim3((unsigned)((D + 255) / 256)), dim3(256), 0, st, a.part_h, a.part_i, (int)nwg,
                     (int)D, h, arg);
  return hip_status(hipGetLastError());
}

int launch_bound_points(const pnr_bound_frames& f, const int64_t* idx, int64_t n, float* xyz, hipStream_t st) {
  BoundArgs a;
  if (n < 0 || !bound_geometry(f, a)) return PNR_E_ARG;
  if (n == 0) return PNR_OK;
  if (!idx || !xyz || (n + 255) / 256 >= (1LL << 31)) return PNR_E_ARG;
  hipLaunchKernelGGL(k_bound_points, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, a, idx, n, xyz);
  return hip_status(hipGetLastError());
}

template <typename T>
static int launch_contains(const T* p, int64_t P, const double* planes, int32_t F, uint8_t* inside, hipStream_t st) {
  if (P < 0 || F < 0 || (P + 255) / 256 >= (1LL << 31)) return PNR_E_ARG;
  if (P == 0) return PNR_OK;
  if (!p || !inside || (F > 0 && !planes)) return PNR_E_ARG;
  hipLaunchKernelGGL(k_bound_contains<T>, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, st, p, P, planes, (int)F,
                     inside);
  return hip_status(hipGetLastError());
}

int launch_bound_contains_f32(const float* p, int64_t P, const double* planes, int32_t F, uint8_t* inside,
                              hipStream_t st) {
  return launch_contains(p, P, planes, F, inside, st);
}
int launch_bound_contains_f64(const double* p, int64_t P, const double* planes, int32_t F, uint8_t* inside,
                              hipStream_t st) {
  return launch_contains(p, P, planes, F, inside, st);
}

}  // namespace pnr
