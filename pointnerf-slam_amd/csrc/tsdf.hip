// tsdf.hip -- the block-sparse TSDF volume the keyframes' depth is fused into (src/utils/Mesher.py:231-266,
// open3d's ScalableTSDFVolume; the rules are stated in include/pnr.h at `pnr_tsdf`).
//
// Blocks of 16^3 voxels behind a dense int32 directory over the caller's box; slots are structure of arrays
// (tsdf, weight, rgb planes of 4,096 floats), voxel index (k 16 + j) 16 + i, so thread t = j 16 + i of a
// 256-thread workgroup owns the column i, j of a block and each of its 16 loads / stores is one 1 KiB row.
//   k_tsdf_mark       a thread per depth pixel of the call: back-projects it (window_sample.h backproject)
//                     and raises every directory entry its [p - trunc, p + trunc] box meets to the mark
//                     -2 - k by atomicMax.  The encoding orders the states: INT32_MIN (empty) < marks (the
//                     earliest frame the largest) < -1 (dropped) < slots, so one integer atomic serves every
//                     state and the directory after the pass does not depend on the schedule.
//   k_tsdf_flags, scan_exclusive (points.hip), k_tsdf_assign
//                     the marked entries take the slots after the live ones in entry order; the birth frame
//                     of a new slot goes to the workspace; the counters are the directory's header.
//   k_tsdf_integrate  persistent workgroups over the live slots (the device counter).  The frame table
//                     (R, t of up to 64 frames) sits in LDS; per block, thread f < frames runs the frustum
//                     test of frame f into LDS, and every wave then reads the same flag (wave-uniform
//                     branch).  A column's 16 x (tsdf, weight, r, g, b) stay in 80 registers over all the
//                     frames: a block is read once (not at all when it is new) and written once.
//   k_tsdf_extract    count and emit in one template: a wave covers 64 consecutive voxel indices of a row,
//                     three ballots per row give the wave's count (count) or a lane's offset inside the
//                     wave (emit); the scan runs over (slot, row, wave) counts.
//   k_tsdf_mesh       marching cubes slot by slot, count and emit in one template (described at the kernel):
//                     an 18^3 halo tile per block in LDS, ballot prefix sums, and per slot 256 rank rows in the
//                     workspace through which a face finds a vertex that a neighbour block owns.
// Integer atomics only; vector stores only.
#include <float.h>
#include <limits.h>

#include "mc_table.h"
#include "pnr_internal.h"
#include "points_hash.h"
#include "window_sample.h"

namespace pnr {

namespace {

constexpr int kBlk = 16;              // voxels per block edge
constexpr int kVox = kBlk * kBlk * kBlk;
constexpr int kHdrInts = 64;          // directory header: n_blocks, dropped_blocks, n_old | padding
constexpr int kMaxFrames = 64;        // frames of one integrate launch (the LDS table)
constexpr int kRowsPerSlot = kBlk * 4;  // (row, wave) counters of a slot
constexpr int32_t kEmpty = INT_MIN;
constexpr int32_t kDropped = -1;
constexpr int64_t kMaxDir = 1ll << 27;
constexpr int32_t kMaxBlocks = 1 << 17;

static inline size_t a256(size_t x) { return (x + 255) / 256 * 256; }

struct TsdfArgs {
  float o0, o1, o2, vl, trunc, depth_trunc, bl;
  int32_t nx, ny, nz, max_blocks, H, W;
  int64_t n_dir;
  float fx, fy, cx, cy;
  int32_t* hdr;
  int32_t* dir;
  float* tsdf;
  float* weight;
  float* rgb;
  int32_t* block_index;
};

// The geometry of a volume; false = bad arguments.  The size queries come before the buffers exist, so the
// pointers are checked for the launches only.
static bool tsdf_args(const pnr_tsdf* v, TsdfArgs& a, bool need_buffers = true) {
  if (!v || (need_buffers && (!v->directory || !v->tsdf || !v->weight || !v->block_index))) return false;
  const float bl = 16.f * v->voxel_length;
  if (!(v->voxel_length > 0.f && v->voxel_length <= FLT_MAX) || !(v->sdf_trunc > 0.f && v->sdf_trunc < bl)) return false;
  if (!(v->fx > 0.f && v->fx <= FLT_MAX && v->fy > 0.f && v->fy <= FLT_MAX) || v->cx != v->cx || v->cy != v->cy) return false;
  if (v->depth_trunc != v->depth_trunc || v->H < 1 || v->W < 1 || (int64_t)v->H * v->W >= (1ll << 30)) return false;
  if (v->max_blocks < 1 || v->max_blocks > kMaxBlocks) return false;
  for (int k = 0; k < 3; ++k)
    if (v->dims[k] < 1 || v->dims[k] > kMaxDir || !(v->origin[k] >= -FLT_MAX && v->origin[k] <= FLT_MAX)) return false;
  const int64_t n = (int64_t)v->dims[0] * v->dims[1] * v->dims[2];
  if (n > kMaxDir) return false;
  a = TsdfArgs{v->origin[0], v->origin[1], v->origin[2], v->voxel_length, v->sdf_trunc, v->depth_trunc, bl,
               v->dims[0], v->dims[1], v->dims[2], v->max_blocks, v->H, v->W, n, v->fx, v->fy, v->cx, v->cy,
               v->directory, v->directory ? v->directory + kHdrInts : nullptr, v->tsdf, v->weight, v->rgb, v->block_index};
  return true;
}

// workspace of a call: integrate = flags[n_dir] | offs[n_dir + 1] | scan scratch | birth[max_blocks];
// extract = cnt[n_rows] | offs[n_rows + 1] | scan scratch, n_rows = max_blocks 64
struct TsdfWs {
  int32_t* flags;
  int32_t* offs;
  int32_t* scratch;
  int32_t* birth;
};
static size_t ws_layout(void* base, int64_t n, bool with_birth, int32_t max_blocks, TsdfWs* w) {
  char* b = static_cast<char*>(base);
  size_t off = 0;
  auto take = [&](size_t bytes) {
    char* p = b ? b + off : nullptr;
    off += a256(bytes);
    return reinterpret_cast<int32_t*>(p);
  };
  TsdfWs v;
  v.flags = take((size_t)n * 4);
  v.offs = take((size_t)(n + 1) * 4);
  v.scratch = take((size_t)scan_scratch_ints(n) * 4);
  v.birth = with_birth ? take((size_t)max_blocks * 4) : nullptr;
  if (w) *w = v;
  return off;
}

__device__ __forceinline__ bool depth_valid(float d, float depth_trunc) { return d > 0.f && d <= depth_trunc && d <= FLT_MAX; }

__device__ __forceinline__ float voxel_centre(float o, int g, float vl) {
  PNR_FP_STRICT
  return o + ((float)g + 0.5f) * vl;
}

__global__ __launch_bounds__(256) void k_tsdf_reset(int32_t* hdr, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < kHdrInts) hdr[i] = 0;
  if (i < n) hdr[kHdrInts + i] = kEmpty;
}

__global__ __launch_bounds__(256) void k_tsdf_mark(TsdfArgs a, const float* __restrict__ depth,
                                                  const float* __restrict__ c2w, int64_t n_pix) {
  PNR_FP_STRICT
  const int64_t hw = (int64_t)a.H * a.W;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n_pix; i += (int64_t)gridDim.x * 256) {
    const float d = depth[i];
    if (!depth_valid(d, a.depth_trunc)) continue;
    const int k = (int)(i / hw);
    const int64_t pix = i - (int64_t)k * hw;
    const int v = (int)(pix / a.W), u = (int)(pix - (int64_t)v * a.W);
    float p[3];
    backproject((float)u, (float)v, d, a.fx, a.fy, a.cx, a.cy, c2w + (int64_t)k * 16, p[0], p[1], p[2]);
    const float o[3] = {a.o0, a.o1, a.o2};
    const int nd[3] = {a.nx, a.ny, a.nz};
    float fl[3], fh[3];
    bool any = true;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      fl[c] = floorf(((p[c] - a.trunc) - o[c]) / a.bl);
      fh[c] = floorf(((p[c] + a.trunc) - o[c]) / a.bl);
      any = any && fh[c] >= 0.f && fl[c] <= (float)(nd[c] - 1);  // (a non-finite p fails one of the two)
    }
    if (!any) continue;
    int lo[3], hi[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      lo[c] = (int)fmaxf(fl[c], 0.f);
      hi[c] = (int)fminf(fh[c], (float)(nd[c] - 1));
    }
    const int32_t mark = -2 - k;
    for (int bz = lo[2]; bz <= hi[2]; ++bz)
      for (int by = lo[1]; by <= hi[1]; ++by)
        for (int bx = lo[0]; bx <= hi[0]; ++bx) {
          int32_t* e = a.dir + ((int64_t)bz * a.ny + by) * a.nx + bx;
          if (*e < mark) atomicMax(e, mark);
        }
  }
}

__device__ __forceinline__ bool is_mark(int32_t v) { return v <= -2 && v != kEmpty; }

__global__ __launch_bounds__(256) void k_tsdf_flags(TsdfArgs a, int32_t* __restrict__ flags) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i == 0) a.hdr[2] = a.hdr[0];
  if (i < a.n_dir) flags[i] = is_mark(a.dir[i]) ? 1 : 0;
}

__global__ __launch_bounds__(256) void k_tsdf_assign(TsdfArgs a, const int32_t* __restrict__ offs,
                                                    int32_t* __restrict__ birth) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int n_old = a.hdr[2];
  if (i == 0) {
    const int64_t want = (int64_t)n_old + offs[a.n_dir];
    a.hdr[0] = want < a.max_blocks ? (int32_t)want : a.max_blocks;
    if (want > a.max_blocks) a.hdr[1] += (int32_t)(want - a.max_blocks);
  }
  if (i >= a.n_dir) return;
  const int32_t v = a.dir[i];
  if (!is_mark(v)) return;
  const int64_t slot = (int64_t)n_old + offs[i];
  if (slot < a.max_blocks) {
    a.dir[i] = (int32_t)slot;
    a.block_index[slot] = (int32_t)i;
    birth[slot] = -2 - v;
  } else {
    a.dir[i] = kDropped;
  }
}

// The frustum test of one block and frame: true when no voxel of the block can be updated.  The corners are
// those of the box of the block's voxel centres grown by 1.5 voxels; zc and the four side functions below are
// linear in the position, so their extremes over the block are bounded by the corners', with a slack of at
// least voxel_length (zc) and fx voxel_length (sides), and a relative 2^-16 on top: orders of magnitude above
// the float32 rounding of either evaluation as long as the volume is fewer than 2^16 voxels from the origin.
__device__ __forceinline__ bool block_unreachable(const TsdfArgs& a, const float* __restrict__ fr, int bx, int by,
                                                  int bz) {
  PNR_FP_STRICT
  const float lo[3] = {a.o0 + (float)(bx * kBlk - 1) * a.vl, a.o1 + (float)(by * kBlk - 1) * a.vl,
                       a.o2 + (float)(bz * kBlk - 1) * a.vl};
  const float ext = (float)(kBlk + 2) * a.vl;
  const float cl = a.cx + 0.5f, cr = (float)a.W - a.cx - 0.5f, ct = a.cy + 0.5f, cb = (float)a.H - a.cy - 0.5f;
  const float rel = 0x1p-16f;
  bool behind = true, left = true, right = true, top = true, bottom = true;
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const float q0 = (lo[0] + ((c & 1) ? ext : 0.f)) - fr[9], q1 = (lo[1] + ((c & 2) ? ext : 0.f)) - fr[10],
                q2 = (lo[2] + ((c & 4) ? ext : 0.f)) - fr[11];
    const float px = (fr[0] * q0 + fr[3] * q1) + fr[6] * q2;
    const float py = (fr[1] * q0 + fr[4] * q1) + fr[7] * q2;
    const float zc = -((fr[2] * q0 + fr[5] * q1) + fr[8] * q2);
    const float mag = rel * (fabsf(q0) + fabsf(q1) + fabsf(q2));
    const float fxp = a.fx * px, fyp = -(a.fy * py);
    behind = behind && zc < -mag;
    left = left && fxp + cl * zc < -(a.fx + cl) * mag;     // u < 0 for every zc > 0
    right = right && fxp - cr * zc > (a.fx + cr) * mag;    // u >= W
    top = top && fyp + ct * zc < -(a.fy + ct) * mag;       // v < 0
    bottom = bottom && fyp - cb * zc > (a.fy + cb) * mag;  // v >= H
  }
  return behind || left || right || top || bottom;
}

struct IntegrateArgs {
  const float* depth;  // frames [f0, f0 + nf) of the call
  const float* color;
  const float* c2w;
  const int32_t* birth;
  int32_t f0, nf;
  int32_t first;  // the first launch of the call: a new slot starts from zero and is not read
};

template <bool COLOR>
__global__ __launch_bounds__(256) void k_tsdf_integrate(TsdfArgs a, IntegrateArgs g) {
  PNR_FP_STRICT
  __shared__ float s_fr[kMaxFrames][12];  // R row-major (9) | t (3)
  __shared__ int s_skip[kMaxFrames];
  const int t = threadIdx.x;
  const int ix = t & (kBlk - 1), iy = t >> 4;
  for (int q = t; q < g.nf * 12; q += 256) {
    const int f = q / 12, r = q - f * 12;
    const float* m = g.c2w + (int64_t)(g.f0 + f) * 16;
    s_fr[f][r] = r < 9 ? m[(r / 3) * 4 + r % 3] : m[(r - 9) * 4 + 3];
  }
  const int n_blocks = a.hdr[0], n_old = a.hdr[2];
  const int64_t hw = (int64_t)a.H * a.W;
  const float fw = (float)a.W, fh = (float)a.H;
  for (int slot = blockIdx.x; slot < n_blocks; slot += gridDim.x) {
    const int e = a.block_index[slot];
    const int bx = e % a.nx, by = (e / a.nx) % a.ny, bz = e / (a.nx * a.ny);
    const bool fresh = slot >= n_old;
    const int born = fresh ? g.birth[slot] : 0;
    __syncthreads();  // the table is written; the previous block's flags are no longer read
    if (t < g.nf) s_skip[t] = (g.f0 + t < born || block_unreachable(a, s_fr[t], bx, by, bz)) ? 1 : 0;
    __syncthreads();
    const int64_t base = (int64_t)slot * kVox + t, cbase = (int64_t)slot * 3 * kVox + t;  // + plane c 4096
    float ts[kBlk], w[kBlk], cr[kBlk], cg[kBlk], cb[kBlk];
    const bool read = !(fresh && g.first);
#pragma unroll
    for (int z = 0; z < kBlk; ++z) {
      ts[z] = read ? a.tsdf[base + z * 256] : 0.f;
      w[z] = read ? a.weight[base + z * 256] : 0.f;
      if (COLOR) {
        cr[z] = read ? a.rgb[cbase + z * 256] : 0.f;
        cg[z] = read ? a.rgb[cbase + kVox + z * 256] : 0.f;
        cb[z] = read ? a.rgb[cbase + 2 * kVox + z * 256] : 0.f;
      }
    }
    const float X = voxel_centre(a.o0, bx * kBlk + ix, a.vl), Y = voxel_centre(a.o1, by * kBlk + iy, a.vl);
    for (int f = 0; f < g.nf; ++f) {
      if (s_skip[f]) continue;  // the same word for every lane
      const float* fr = s_fr[f];
      const float r00 = fr[0], r01 = fr[1], r02 = fr[2], r10 = fr[3], r11 = fr[4], r12 = fr[5], r20 = fr[6],
                  r21 = fr[7], r22 = fr[8];
      const float q0 = X - fr[9], q1 = Y - fr[10], t2 = fr[11];
      const float h0 = r00 * q0 + r10 * q1, h1 = r01 * q0 + r11 * q1, h2 = r02 * q0 + r12 * q1;
      const float* dep = g.depth + (int64_t)(g.f0 + f) * hw;
      // (a call without colour on a volume that keeps one leaves the colour as it is; new blocks hold zeros)
      const float* col = COLOR && g.color ? g.color + (int64_t)(g.f0 + f) * hw * 3 : nullptr;
#pragma unroll
      for (int z = 0; z < kBlk; ++z) {
        const float q2 = voxel_centre(a.o2, bz * kBlk + z, a.vl) - t2;
        const float p0 = h0 + r20 * q2, p1 = h1 + r21 * q2;
        const float zc = -(h2 + r22 * q2);
        if (!(zc > 0.f)) continue;
        const float uf = ((a.fx * p0) / zc + a.cx) + 0.5f, vf = ((-(a.fy * p1)) / zc + a.cy) + 0.5f;
        if (!(uf >= 0.f && uf < fw && vf >= 0.f && vf < fh)) continue;
        const float fu = floorf(uf), fv = floorf(vf);
        const int64_t pix = (int64_t)(int)fv * a.W + (int)fu;
        const float d = dep[pix];
        if (!depth_valid(d, a.depth_trunc)) continue;
        const float ca = (fu - a.cx) / a.fx, cbv = (fv - a.cy) / a.fy;
        const float m = sqrtf((ca * ca + cbv * cbv) + 1.f);
        const float sdf = (d - zc) * m;
        if (sdf <= -a.trunc) continue;
        const float s = fminf(1.f, sdf / a.trunc);
        const float w0 = w[z], w1 = w0 + 1.f;
        ts[z] = (ts[z] * w0 + s) / w1;
        if (COLOR && col) {
          cr[z] = (cr[z] * w0 + col[pix * 3 + 0]) / w1;
          cg[z] = (cg[z] * w0 + col[pix * 3 + 1]) / w1;
          cb[z] = (cb[z] * w0 + col[pix * 3 + 2]) / w1;
        }
        w[z] = w1;
      }
    }
#pragma unroll
    for (int z = 0; z < kBlk; ++z) {
      a.tsdf[base + z * 256] = ts[z];
      a.weight[base + z * 256] = w[z];
      if (COLOR) {
        a.rgb[cbase + z * 256] = cr[z];
        a.rgb[cbase + kVox + z * 256] = cg[z];
        a.rgb[cbase + 2 * kVox + z * 256] = cb[z];
      }
    }
  }
}

// Voxel (x, y, z) of the block at (bx, by, bz) with one coordinate possibly 16: the first voxel of the next
// block along that axis, through the directory.  Returns its flat index slot 4096 + voxel index, or -1.
__device__ __forceinline__ int64_t neighbour_index(const TsdfArgs& a, int slot, int bx, int by, int bz, int x, int y,
                                                   int z) {
  if (x < kBlk && y < kBlk && z < kBlk) return (int64_t)slot * kVox + (z * kBlk + y) * kBlk + x;
  const int cx = bx + (x >> 4), cy = by + (y >> 4), cz = bz + (z >> 4);
  if (cx >= a.nx || cy >= a.ny || cz >= a.nz) return -1;
  const int s1 = a.dir[((int64_t)cz * a.ny + cy) * a.nx + cx];
  if (s1 < 0) return -1;
  return (int64_t)s1 * kVox + ((z & 15) * kBlk + (y & 15)) * kBlk + (x & 15);
}

template <bool EMIT>
__global__ __launch_bounds__(256) void k_tsdf_extract(TsdfArgs a, int32_t* __restrict__ cnt,
                                                     const int32_t* __restrict__ offs, float* __restrict__ xyz,
                                                     float* __restrict__ rgb) {
  PNR_FP_STRICT
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int ix = t & (kBlk - 1), iy = t >> 4;
  const int n_blocks = a.hdr[0];
  const int n_slots = EMIT ? n_blocks : a.max_blocks;  // the count zeroes the rows of the unused slots too
  for (int slot = blockIdx.x; slot < n_slots; slot += gridDim.x) {
    const bool live = slot < n_blocks;
    const int e = live ? a.block_index[slot] : 0;
    const int bx = e % a.nx, by = (e / a.nx) % a.ny, bz = e / (a.nx * a.ny);
    for (int z = 0; z < kBlk; ++z) {
      const int64_t i0 = (int64_t)slot * kVox + z * 256 + t;
      int64_t i1[3] = {-1, -1, -1};
      float t0 = 0.f;
      if (live && a.weight[i0] > 0.f) {
        t0 = a.tsdf[i0];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const int64_t j = neighbour_index(a, slot, bx, by, bz, ix + (c == 0), iy + (c == 1), z + (c == 2));
          if (j < 0 || !(a.weight[j] > 0.f)) continue;
          const float t1 = a.tsdf[j];
          if ((t0 < 0.f && t1 > 0.f) || (t0 > 0.f && t1 < 0.f)) i1[c] = j;
        }
      }
      const unsigned long long b0 = __ballot(i1[0] >= 0), b1 = __ballot(i1[1] >= 0), b2 = __ballot(i1[2] >= 0);
      const int row = slot * kRowsPerSlot + z * 4 + wave;
      if (!EMIT) {
        if (lane == 0) cnt[row] = __popcll(b0) + __popcll(b1) + __popcll(b2);
        continue;
      }
      const unsigned long long lt = (1ull << lane) - 1ull;
      int64_t pos = (int64_t)offs[row] + __popcll(b0 & lt) + __popcll(b1 & lt) + __popcll(b2 & lt);
      float X[3] = {voxel_centre(a.o0, bx * kBlk + ix, a.vl), voxel_centre(a.o1, by * kBlk + iy, a.vl),
                    voxel_centre(a.o2, bz * kBlk + z, a.vl)};
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        if (i1[c] < 0) continue;
        const float s = t0 / (t0 - a.tsdf[i1[c]]);
#pragma unroll
        for (int k = 0; k < 3; ++k) xyz[pos * 3 + k] = k == c ? X[k] + a.vl * s : X[k];
        if (rgb) {
#pragma unroll
          for (int k = 0; k < 3; ++k) {
            const float c0 = a.rgb[((int64_t)slot * 3 + k) * kVox + z * 256 + t];
            const int64_t s1 = i1[c] / kVox, v1 = i1[c] - s1 * kVox;
            const float c1 = a.rgb[(s1 * 3 + k) * kVox + v1];
            rgb[pos * 3 + k] = c0 + (c1 - c0) * s;
          }
        }
        ++pos;
      }
    }
  }
}

__global__ void k_tsdf_total(const int32_t* __restrict__ offs, int64_t n, int64_t* __restrict__ out) { out[0] = offs[n]; }

// ---- triangle mesh (pnr_tsdf_mesh_count / _emit) ---------------------------------------------------------
// One template for both calls, a workgroup per live slot.  The slot's 18^3 halo tile (voxels -1..16 per axis;
// tile index (z 18 + y) 18 + x of voxel (x - 1, y - 1, z - 1)) is staged through the 27 directory entries
// around the block: a flag byte per voxel (bit 0 valid, bit 1 below) and, for the emit, the tsdf value.  A
// second sweep marks the 17^3 cells of the tile whose eight corners are valid, so the voxel pass decides from
// LDS alone which owned edges carry a vertex (one of the four cells around the edge is valid) and the cell's
// case.  Thread t = j 16 + i walks its column in z as the other kernels here do; a wave covers 64 consecutive
// voxel indices, ballots of the edge bits and of the triangle count's three bits give the wave's totals and
// every lane's offset, and wave 0 scans the 64 (z, wave) totals of the block.  The count writes the block's
// totals and its rank rows; the emit rebuilds the same offsets, keeps its own rank rows in LDS and reads a
// neighbour's from the workspace.
constexpr int kTile = kBlk + 2;
constexpr int kTileN = kTile * kTile * kTile;
constexpr int kTy = kTile, kTz = kTile * kTile;  // tile strides
constexpr int kRankRows = kBlk * kBlk;           // rows (k, j) of a slot
constexpr int kUnits = kBlk * 4;                 // (z, wave) units of a slot

// workspace of the mesh calls: vcnt[max_blocks] | fcnt[max_blocks] | voff[max_blocks + 1] | foff[max_blocks + 1]
// | scan scratch | rank[max_blocks][256] uint64.  A rank row (k, j) of a slot: bits 0-15, 16-31, 32-47 the
// voxels i of the row whose x, y, z edge carries a vertex, bits 48-63 the slot's vertices before the row.
struct MeshWs {
  int32_t *vcnt, *fcnt, *voff, *foff, *scratch;
  unsigned long long* rank;
};
static size_t mesh_ws_layout(void* base, int32_t max_blocks, MeshWs* w) {
  char* b = static_cast<char*>(base);
  size_t off = 0;
  auto take = [&](size_t bytes) {
    char* p = b ? b + off : nullptr;
    off += a256(bytes);
    return p;
  };
  MeshWs v;
  v.vcnt = reinterpret_cast<int32_t*>(take((size_t)max_blocks * 4));
  v.fcnt = reinterpret_cast<int32_t*>(take((size_t)max_blocks * 4));
  v.voff = reinterpret_cast<int32_t*>(take((size_t)(max_blocks + 1) * 4));
  v.foff = reinterpret_cast<int32_t*>(take((size_t)(max_blocks + 1) * 4));
  v.scratch = reinterpret_cast<int32_t*>(take((size_t)scan_scratch_ints(max_blocks) * 4));
  v.rank = reinterpret_cast<unsigned long long*>(take((size_t)max_blocks * kRankRows * 8));
  if (w) *w = v;
  return off;
}

struct MeshOut {
  float* xyz;
  float* rgb;
  int32_t* faces;
};

// The vertices of a slot before the one on edge `ax` of voxel xi of a rank row (order: voxel, then axis).
__device__ __forceinline__ int rank_in_slot(unsigned long long row, int xi, int ax) {
  const unsigned long long lo = (1ull << xi) - 1ull, le = (2ull << xi) - 1ull;
  const unsigned long long sel = (ax > 0 ? le : lo) | ((ax > 1 ? le : lo) << 16) | (lo << 32);
  return (int)(row >> 48) + __popcll(row & sel);
}

template <bool EMIT>
__global__ __launch_bounds__(256) void k_tsdf_mesh(TsdfArgs a, MeshWs m, MeshOut o) {
  PNR_FP_STRICT
  __shared__ float s_t[EMIT ? kTileN : 1];
  // flags and cells; the emit writes the voxel words over them once the voxel pass has read them
  __shared__ __attribute__((aligned(16))) unsigned char s_buf[EMIT ? kVox * 4 : 2 * kTileN];
  static_assert(2 * kTileN <= kVox * 4, "the words cover the flags and the cells");
  unsigned char* const s_flag = s_buf;
  unsigned char* const s_cell = s_buf + kTileN;
  uint32_t* const s_word = reinterpret_cast<uint32_t*>(s_buf);
  __shared__ unsigned long long s_rank[EMIT ? kRankRows : 1];
  __shared__ int s_nb[27], s_uv[kUnits], s_uf[kUnits], s_tot[2];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int ix = t & (kBlk - 1), iy = t >> 4;
  const unsigned long long lt = (1ull << lane) - 1ull;
  const int n_blocks = a.hdr[0];
  const int n_slots = EMIT ? n_blocks : a.max_blocks;  // the count zeroes the totals of the unused slots too
  for (int slot = blockIdx.x; slot < n_slots; slot += gridDim.x) {
    if (slot >= n_blocks) {
      if (t == 0) m.vcnt[slot] = m.fcnt[slot] = 0;
      continue;
    }
    const int e = a.block_index[slot];
    const int bx = e % a.nx, by = (e / a.nx) % a.ny, bz = e / (a.nx * a.ny);
    __syncthreads();  // the previous slot's tile is no longer read
    if (t < 27) {
      const int cx = bx + t % 3 - 1, cy = by + (t / 3) % 3 - 1, cz = bz + t / 9 - 1;
      int s1 = -1;
      if (cx >= 0 && cx < a.nx && cy >= 0 && cy < a.ny && cz >= 0 && cz < a.nz)
        s1 = a.dir[((int64_t)cz * a.ny + cy) * a.nx + cx];
      s_nb[t] = s1 < 0 ? -1 : s1;
    }
    __syncthreads();
    for (int q = t; q < kTileN; q += 256) {
      const int x = q % kTile, y = (q / kTile) % kTile, z = q / kTz;
      // x = 0 lies in the block before, 1..16 in this one, 17 in the next: (x + 15) >> 4 = 0, 1, 2
      const int s1 = s_nb[(((z + 15) >> 4) * 3 + ((y + 15) >> 4)) * 3 + ((x + 15) >> 4)];
      unsigned char flag = 0;
      float tv = 0.f;
      if (s1 >= 0) {
        const int64_t at = (int64_t)s1 * kVox + ((((z + 15) & 15) * kBlk + ((y + 15) & 15)) * kBlk + ((x + 15) & 15));
        if (a.weight[at] > 0.f) {
          tv = a.tsdf[at];
          flag = tv < 0.f ? 3 : 1;
        }
      }
      s_flag[q] = flag;
      if (EMIT) s_t[q] = tv;
    }
    __syncthreads();
    for (int q = t; q < kTileN; q += 256) {
      const int x = q % kTile, y = (q / kTile) % kTile, z = q / kTz;
      unsigned char c = 0;
      if (x < kTile - 1 && y < kTile - 1 && z < kTile - 1)
        c = s_flag[q] & s_flag[q + 1] & s_flag[q + kTy] & s_flag[q + kTy + 1] & s_flag[q + kTz] &
            s_flag[q + kTz + 1] & s_flag[q + kTz + kTy] & s_flag[q + kTz + kTy + 1] & 1;
      s_cell[q] = c;
    }
    __syncthreads();
    // per voxel: bits 0-2 owned edges with a vertex, 3-10 the case of its cell (0 when the cell is not valid),
    // 11-18 the vertices and 19-27 the faces of the lanes before it in the wave (<= 63 3, <= 63 MC_MAX_TRI)
    static_assert(63 * 3 < (1 << 8) && 63 * MC_MAX_TRI < (1 << 9) && (kVox - 1) * 3 < (1 << 16), "packed fields");
    uint32_t word[kBlk];
#pragma unroll
    for (int z = 0; z < kBlk; ++z) {
      const int q0 = ((z + 1) * kTile + (iy + 1)) * kTile + (ix + 1);
      const uint32_t f0 = s_flag[q0], fx = s_flag[q0 + 1], fy = s_flag[q0 + kTy], fz = s_flag[q0 + kTz];
      const uint32_t c0 = s_cell[q0], cmx = s_cell[q0 - 1], cmy = s_cell[q0 - kTy], cmz = s_cell[q0 - kTz];
      const uint32_t around_x = c0 | cmy | cmz | s_cell[q0 - kTy - kTz];
      const uint32_t around_y = c0 | cmx | cmz | s_cell[q0 - 1 - kTz];
      const uint32_t around_z = c0 | cmx | cmy | s_cell[q0 - 1 - kTy];
      const uint32_t em = (((f0 ^ fx) >> 1) & around_x) | ((((f0 ^ fy) >> 1) & around_y) << 1) |
                          ((((f0 ^ fz) >> 1) & around_z) << 2);
      uint32_t cs = 0;
      if (c0)
        cs = (f0 >> 1) | ((fx >> 1) << 1) | ((fy >> 1) << 2) | ((uint32_t)(s_flag[q0 + kTy + 1] >> 1) << 3) |
             ((fz >> 1) << 4) | ((uint32_t)(s_flag[q0 + kTz + 1] >> 1) << 5) |
             ((uint32_t)(s_flag[q0 + kTz + kTy] >> 1) << 6) | ((uint32_t)(s_flag[q0 + kTz + kTy + 1] >> 1) << 7);
      const uint32_t nt = MC_NTRI[cs];
      const unsigned long long v0 = __ballot(em & 1), v1 = __ballot(em & 2), v2 = __ballot(em & 4);
      const unsigned long long t0 = __ballot(nt & 1), t1 = __ballot(nt & 2), t2 = __ballot(nt & 4);
      const uint32_t pv = __popcll(v0 & lt) + __popcll(v1 & lt) + __popcll(v2 & lt);
      const uint32_t pf = __popcll(t0 & lt) + 2 * __popcll(t1 & lt) + 4 * __popcll(t2 & lt);
      if (lane == 0) {
        s_uv[z * 4 + wave] = __popcll(v0) + __popcll(v1) + __popcll(v2);
        s_uf[z * 4 + wave] = __popcll(t0) + 2 * __popcll(t1) + 4 * __popcll(t2);
      }
      word[z] = em | (cs << 3) | (pv << 11) | (pf << 19);
    }
    __syncthreads();
    if (wave == 0) {  // exclusive scan of the 64 unit totals, in (z, wave) order
      const int cv = s_uv[lane], cf = s_uf[lane];
      int sv = cv, sf = cf;
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        const int uv = __shfl_up(sv, d), uf = __shfl_up(sf, d);
        if (lane >= d) {
          sv += uv;
          sf += uf;
        }
      }
      s_uv[lane] = sv - cv;
      s_uf[lane] = sf - cf;
      if (lane == 63) {
        s_tot[0] = sv;
        s_tot[1] = sf;
      }
    }
    __syncthreads();
    if (!EMIT && t == 0) {
      m.vcnt[slot] = s_tot[0];
      m.fcnt[slot] = s_tot[1];
    }
    unsigned long long* rows = EMIT ? s_rank : m.rank + (int64_t)slot * kRankRows;
#pragma unroll
    for (int z = 0; z < kBlk; ++z) {
      const uint32_t em = word[z] & 7u;
      const unsigned long long v0 = __ballot(em & 1), v1 = __ballot(em & 2), v2 = __ballot(em & 4);
      if (ix == 0) {  // the first lane of each of the wave's four rows
        const int sh = lane & 48;
        const unsigned long long before = (1ull << sh) - 1ull;
        const unsigned long long pre =
            (unsigned long long)(s_uv[z * 4 + wave] + __popcll(v0 & before) + __popcll(v1 & before) + __popcll(v2 & before));
        rows[z * kBlk + iy] = (pre << 48) | ((v0 >> sh) & 0xffffull) | (((v1 >> sh) & 0xffffull) << 16) |
                              (((v2 >> sh) & 0xffffull) << 32);
      }
    }
    if (!EMIT) continue;
#pragma unroll
    for (int z = 0; z < kBlk; ++z) s_word[z * 256 + t] = word[z];  // (every flag and cell was read two barriers ago)
    __syncthreads();  // the rank rows and the words of this slot are in LDS
    const int64_t vbase = m.voff[slot], fbase = m.foff[slot];
    const float X0 = voxel_centre(a.o0, bx * kBlk + ix, a.vl), X1 = voxel_centre(a.o1, by * kBlk + iy, a.vl);
    for (int z = 0; z < kBlk; ++z) {
      const uint32_t w = s_word[z * 256 + t], em = w & 7u, cs = (w >> 3) & 255u;
      const int unit = z * 4 + wave;
      if (em) {
        const int q0 = ((z + 1) * kTile + (iy + 1)) * kTile + (ix + 1);
        const float X[3] = {X0, X1, voxel_centre(a.o2, bz * kBlk + z, a.vl)};
        const float t0 = s_t[q0];
        int64_t pos = vbase + s_uv[unit] + (int)((w >> 11) & 255u);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          if (!(em & (1u << c))) continue;
          const float s = t0 / (t0 - s_t[q0 + (c == 0 ? 1 : (c == 1 ? kTy : kTz))]);
#pragma unroll
          for (int k = 0; k < 3; ++k) o.xyz[pos * 3 + k] = k == c ? X[k] + a.vl * s : X[k];
          if (o.rgb) {
            const int x1 = ix + (c == 0), y1 = iy + (c == 1), z1 = z + (c == 2);
            const int64_t s1 = s_nb[(((z1 >> 4) + 1) * 3 + ((y1 >> 4) + 1)) * 3 + ((x1 >> 4) + 1)];
            const int v1i = ((z1 & 15) * kBlk + (y1 & 15)) * kBlk + (x1 & 15);
#pragma unroll
            for (int k = 0; k < 3; ++k) {
              const float c0 = a.rgb[((int64_t)slot * 3 + k) * kVox + z * 256 + t];
              const float c1 = a.rgb[(s1 * 3 + k) * kVox + v1i];
              o.rgb[pos * 3 + k] = c0 + (c1 - c0) * s;
            }
          }
          ++pos;
        }
      }
      const int nt = MC_NTRI[cs];
      int64_t f = fbase + s_uf[unit] + (int)((w >> 19) & 511u);
      for (int k = 0; k < nt; ++k, ++f) {
#pragma unroll
        for (int j = 0; j < 3; ++j) {
          const int ed = MC_TRI[cs][3 * k + j];
          const int ax = ed >> 2, db = ed & 1, dc = (ed >> 1) & 1;
          // the two other axes in increasing order carry (db, dc), as in mesh.hip
          const int x1 = ix + (ax == 0 ? 0 : db), y1 = iy + (ax == 1 ? 0 : (ax == 0 ? db : dc)),
                    z1 = z + (ax == 2 ? 0 : dc);
          const int nb = (((z1 >> 4) + 1) * 3 + ((y1 >> 4) + 1)) * 3 + ((x1 >> 4) + 1);
          const int row = (z1 & 15) * kBlk + (y1 & 15);
          // a valid cell's corners are voxels of live blocks: s_nb[nb] >= 0
          const int s1 = s_nb[nb];
          const unsigned long long r = nb == 13 ? s_rank[row] : m.rank[(int64_t)s1 * kRankRows + row];
          const int32_t base = nb == 13 ? (int32_t)vbase : m.voff[s1];
          o.faces[f * 3 + j] = base + rank_in_slot(r, x1 & 15, ax);
        }
      }
    }
  }
}

__global__ void k_tsdf_mesh_total(const int32_t* __restrict__ voff, const int32_t* __restrict__ foff, int64_t n,
                                  int64_t* __restrict__ n_v, int64_t* __restrict__ n_f) {
  n_v[0] = voff[n];
  n_f[0] = foff[n];
}

}  // namespace

size_t tsdf_directory_bytes(const pnr_tsdf* v) {
  TsdfArgs a;
  if (!tsdf_args(v, a, false)) return 0;
  return ((size_t)kHdrInts + (size_t)a.n_dir) * 4;
}

size_t tsdf_workspace_bytes(const pnr_tsdf* v) {
  TsdfArgs a;
  if (!tsdf_args(v, a, false)) return 0;
  const size_t wi = ws_layout(nullptr, a.n_dir, true, a.max_blocks, nullptr);
  const size_t we = ws_layout(nullptr, (int64_t)a.max_blocks * kRowsPerSlot, false, a.max_blocks, nullptr);
  return wi > we ? wi : we;
}

int launch_tsdf_reset(const pnr_tsdf* v, hipStream_t st) {
  TsdfArgs a;
  if (!tsdf_args(v, a)) return PNR_E_ARG;
  const int64_t n = a.n_dir > kHdrInts ? a.n_dir : kHdrInts;
  hipLaunchKernelGGL(k_tsdf_reset, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, a.hdr, a.n_dir);
  return hip_status(hipGetLastError());
}

int launch_tsdf_integrate(const pnr_tsdf* v, const float* depth, const float* color, const float* c2w, int32_t K,
                          void* ws, size_t ws_bytes, hipStream_t st) {
  TsdfArgs a;
  if (!tsdf_args(v, a) || K < 0) return PNR_E_ARG;
  if (K == 0) return PNR_OK;
  if (!depth || !c2w || (color && !a.rgb) || K > (1 << 20)) return PNR_E_ARG;
  const int64_t n_pix = (int64_t)K * a.H * a.W;
  if (n_pix >= (1ll << 40)) return PNR_E_ARG;
  if (!ws || ws_bytes < tsdf_workspace_bytes(v)) return PNR_E_WORKSPACE;
  TsdfWs w;
  ws_layout(ws, a.n_dir, true, a.max_blocks, &w);
  const int cus = device_cu_count();
  int64_t nwg = (n_pix + 255) / 256;
  if (nwg > 8ll * cus) nwg = 8ll * cus;
  const unsigned dir_wg = (unsigned)((a.n_dir + 255) / 256);
  hipLaunchKernelGGL(k_tsdf_mark, dim3((unsigned)nwg), dim3(256), 0, st, a, depth, c2w, n_pix);
  hipLaunchKernelGGL(k_tsdf_flags, dim3(dir_wg), dim3(256), 0, st, a, w.flags);
  int rc = scan_exclusive(w.flags, w.offs, a.n_dir, w.scratch, st);
  if (rc) return rc;
  hipLaunchKernelGGL(k_tsdf_assign, dim3(dir_wg), dim3(256), 0, st, a, w.offs, w.birth);
  const int grid = a.max_blocks < 4 * cus ? a.max_blocks : 4 * cus;
  for (int32_t f0 = 0; f0 < K; f0 += kMaxFrames) {
    IntegrateArgs g{depth, color, c2w, w.birth, f0, K - f0 < kMaxFrames ? K - f0 : kMaxFrames, f0 == 0 ? 1 : 0};
    if (a.rgb)
      hipLaunchKernelGGL(k_tsdf_integrate<true>, dim3((unsigned)grid), dim3(256), 0, st, a, g);
    else
      hipLaunchKernelGGL(k_tsdf_integrate<false>, dim3((unsigned)grid), dim3(256), 0, st, a, g);
  }
  return hip_status(hipGetLastError());
}

int launch_tsdf_extract_count(const pnr_tsdf* v, void* ws, size_t ws_bytes, int64_t* n_points, hipStream_t st) {
  TsdfArgs a;
  if (!tsdf_args(v, a) || !n_points) return PNR_E_ARG;
  if (!ws || ws_bytes < tsdf_workspace_bytes(v)) return PNR_E_WORKSPACE;
  TsdfWs w;
  const int64_t n_rows = (int64_t)a.max_blocks * kRowsPerSlot;
  ws_layout(ws, n_rows, false, a.max_blocks, &w);
  const int cus = device_cu_count();
  const int grid = a.max_blocks < 8 * cus ? a.max_blocks : 8 * cus;
  hipLaunchKernelGGL(k_tsdf_extract<false>, dim3((unsigned)grid), dim3(256), 0, st, a, w.flags, nullptr, nullptr,
                     nullptr);
  int rc = scan_exclusive(w.flags, w.offs, n_rows, w.scratch, st);
  if (rc) return rc;
  hipLaunchKernelGGL(k_tsdf_total, dim3(1), dim3(1), 0, st, w.offs, n_rows, n_points);
  return hip_status(hipGetLastError());
}

int launch_tsdf_extract_emit(const pnr_tsdf* v, const void* ws, size_t ws_bytes, float* xyz, float* rgb,
                             hipStream_t st) {
  TsdfArgs a;
  if (!tsdf_args(v, a) || !xyz || (rgb && !a.rgb)) return PNR_E_ARG;
  if (!ws || ws_bytes < tsdf_workspace_bytes(v)) return PNR_E_WORKSPACE;
  TsdfWs w;
  ws_layout(const_cast<void*>(ws), (int64_t)a.max_blocks * kRowsPerSlot, false, a.max_blocks, &w);
  const int cus = device_cu_count();
  const int grid = a.max_blocks < 8 * cus ? a.max_blocks : 8 * cus;
  hipLaunchKernelGGL(k_tsdf_extract<true>, dim3((unsigned)grid), dim3(256), 0, st, a, nullptr, w.offs, xyz, rgb);
  return hip_status(hipGetLastError());
}

// A volume can be meshed when max_blocks cells' worth of faces fits an int32 whatever the surface (3 vertices
// per voxel always do): the counts come back on the device, so the limit is checked on the size.
static bool mesh_args(const pnr_tsdf* v, TsdfArgs& a, bool need_buffers) {
  return tsdf_args(v, a, need_buffers) && (int64_t)a.max_blocks * kVox * MC_MAX_TRI <= (int64_t)INT_MAX;
}

size_t tsdf_mesh_workspace_bytes(const pnr_tsdf* v) {
  TsdfArgs a;
  if (!mesh_args(v, a, false)) return 0;
  return mesh_ws_layout(nullptr, a.max_blocks, nullptr);
}

int launch_tsdf_mesh_count(const pnr_tsdf* v, void* ws, size_t ws_bytes, int64_t* n_vertices, int64_t* n_faces,
                           hipStream_t st) {
  TsdfArgs a;
  if (!mesh_args(v, a, true) || !n_vertices || !n_faces || ((uintptr_t)ws & 7)) return PNR_E_ARG;
  if (!ws || ws_bytes < tsdf_mesh_workspace_bytes(v)) return PNR_E_WORKSPACE;
  MeshWs w;
  mesh_ws_layout(ws, a.max_blocks, &w);
  const int cus = device_cu_count();
  const int grid = a.max_blocks < 8 * cus ? a.max_blocks : 8 * cus;
  hipLaunchKernelGGL(k_tsdf_mesh<false>, dim3((unsigned)grid), dim3(256), 0, st, a, w, MeshOut{nullptr, nullptr, nullptr});
  int rc = scan_exclusive(w.vcnt, w.voff, a.max_blocks, w.scratch, st);
  if (rc) return rc;
  rc = scan_exclusive(w.fcnt, w.foff, a.max_blocks, w.scratch, st);
  if (rc) return rc;
  hipLaunchKernelGGL(k_tsdf_mesh_total, dim3(1), dim3(1), 0, st, w.voff, w.foff, (int64_t)a.max_blocks, n_vertices,
                     n_faces);
  return hip_status(hipGetLastError());
}

int launch_tsdf_mesh_emit(const pnr_tsdf* v, const void* ws, size_t ws_bytes, float* xyz, float* rgb, int32_t* faces,
                          hipStream_t st) {
  TsdfArgs a;
  if (!mesh_args(v, a, true) || !xyz || !faces || (rgb && !a.rgb) || ((uintptr_t)ws & 7)) return PNR_E_ARG;
  if (!ws || ws_bytes < tsdf_mesh_workspace_bytes(v)) return PNR_E_WORKSPACE;
  MeshWs w;
  mesh_ws_layout(const_cast<void*>(ws), a.max_blocks, &w);
  const int cus = device_cu_count();
  const int grid = a.max_blocks < 8 * cus ? a.max_blocks : 8 * cus;
  hipLaunchKernelGGL(k_tsdf_mesh<true>, dim3((unsigned)grid), dim3(256), 0, st, a, w, MeshOut{xyz, rgb, faces});
  return hip_status(hipGetLastError());
}

}  // namespace pnr
