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
// Integer atomics only; vector stores only.
#include <float.h>
#include <limits.h>

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

}  // namespace pnr
