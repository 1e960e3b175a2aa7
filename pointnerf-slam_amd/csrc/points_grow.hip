// points_grow.hip -- growing the neural-point map from a keyframe's depth.
//
// The reference has no neural-point stage; Point-SLAM's Mapper calls this step add_neural_points.  It is
// build-defined: include/pnr.h (pnr_points_add_frame) states the rules and tests/points_grow_ref.py
// restates them on the CPU.  One call, stream-ordered, no host read:
//   k_add_candidates  one thread per candidate (pixel x depth offset): depth load, backproject
//                     (window_sample.h: the ray k_get_rays builds and the position on it; shared with
//                     the mesh bound, bound.hip), the bound test, and the test against the
//                     existing points through the cloud's index -- base_cell, the 8 bucket headers of
//                     the 2x2x2 probe block (own bucket or colliding bucket; a foreign bucket is not
//                     read), the buckets' points until the first one inside the ball.  Coalesced
//                     float4 position and flag-byte stores; the valid / free counts leave each block
//                     as one 64-bit integer atomic on one of 64 spread counters.
//   k_add_thin_claim  a free candidate claims its voxel's entry of an open-addressed table (64-bit
//                     cell_key words by atomicCAS, linear probing on the full key) and lowers the
//                     entry's 32-bit minimum candidate index (atomicMin).  Integer min commutes: the
//                     winner is the same whatever order the lanes arrive in.
//   k_add_thin_mark   the candidate whose index is its voxel's minimum is kept; 0 / 1 keep words.
//   scan_exclusive    (points.hip) keep words -> the rank of each kept candidate in candidate order.
//   k_add_emit        8 lanes per candidate: the kept ones of rank < capacity - n write their xyz row
//                     (12 B) and their 128-B feature row (one 16-B store per lane when the buffers
//                     are 16-B aligned, four 4-B stores otherwise) at row n + rank.
//   k_add_counters    the five counters.
// No float atomics anywhere, and no atomic decides where a row goes.
#include "pnr_internal.h"
#include "points_hash.h"
#include "window_sample.h"

namespace pnr {

namespace {

constexpr uint64_t kEmptyKey = ~0ull;  // cell_key uses 63 bits: never a voxel
constexpr int kCntLists = 64;          // spread block counters, one per 128-B line

static inline size_t a256(size_t x) { return (x + 255) / 256 * 256; }

static int64_t thin_table_size(int64_t n_cand) {
  int64_t t = 2;
  while (t < 2 * n_cand) t <<= 1;
  return t;
}

struct AddView {
  unsigned long long* cnt;  // [kCntLists * 16]: valid | free << 32 per list
  float4* pos;              // [n] (x, y, z, 0)
  int32_t* slot;            // [n] table entry of a free candidate
  int32_t* keep;            // [n] 0 / 1
  int32_t* rank;            // [n + 1] exclusive scan of keep
  int32_t* scratch;         // scan scratch
  unsigned long long* keys; // [Tn]
  uint32_t* mins;           // [Tn], directly after keys (one fill)
  uint8_t* flags;           // [n]
  int64_t Tn;
};

static AddView add_view(void* base, int64_t n, size_t* bytes) {
  AddView v{};
  char* b = static_cast<char*>(base);
  size_t off = 0;
  auto take = [&](size_t k) {
    char* p = b ? b + off : nullptr;
    off += a256(k);
    return p;
  };
  const int64_t m = n > 0 ? n : 1;
  v.Tn = thin_table_size(m);
  v.cnt = reinterpret_cast<unsigned long long*>(take((size_t)kCntLists * 16 * 8));
  v.pos = reinterpret_cast<float4*>(take((size_t)m * 16));
  v.slot = reinterpret_cast<int32_t*>(take((size_t)m * 4));
  v.keep = reinterpret_cast<int32_t*>(take((size_t)m * 4));
  v.rank = reinterpret_cast<int32_t*>(take((size_t)(m + 1) * 4));
  v.scratch = reinterpret_cast<int32_t*>(take((size_t)scan_scratch_ints(m) * 4));
  char* tab = take((size_t)v.Tn * 12);
  v.keys = reinterpret_cast<unsigned long long*>(tab);
  v.mins = reinterpret_cast<uint32_t*>(tab ? tab + (size_t)v.Tn * 8 : nullptr);
  v.flags = reinterpret_cast<uint8_t*>(take((size_t)m));
  if (bytes) *bytes = off;
  return v;
}

struct AddArgs {
  pnr_points_add a;
  int64_t n_cand;
  int64_t n_live, room;  // existing rows, rows left below capacity
  int32_t nW;            // lattice columns (stride mode)
  HashGrid g;
  const int4* hdr;       // null: an empty cloud, no neighbour test
  const float4* sorted;
  float r2, inv_thin;
  uint32_t tmask;
  AddView v;
  float* xyz;
  float* feats;
  int vec4;  // feats and init_feats are 16-B aligned (a Parameter inside an optimiser's flat buffer need not be)
  int64_t* counters;
};

__global__ __launch_bounds__(256) void k_add_candidates(AddArgs a) {
  PNR_FP_STRICT
  __shared__ uint32_t s_cnt[4][2];
  const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
  float px = 0.f, py = 0.f, pz = 0.f;
  bool valid = false, fre = false;
  if (c < a.n_cand) {
    const int64_t rank = c / a.a.n_rho;
    const int o = (int)(c - rank * a.a.n_rho);
    int u, v;
    bool inimg = true;
    if (a.a.pixels) {
      const int64_t pix = a.a.pixels[rank];
      inimg = pix >= 0 && pix < (int64_t)a.a.H * a.a.W;
      v = inimg ? (int)(pix / a.a.W) : 0;
      u = inimg ? (int)(pix - (int64_t)v * a.a.W) : 0;
    } else {
      const int64_t row = rank / a.nW;
      v = (int)row * a.a.stride;
      u = (int)(rank - row * a.nW) * a.a.stride;
    }
    if (inimg) {
      const float d = a.a.depth[(int64_t)v * a.a.W + u];
      float rho = a.a.rho[0];  // (a select chain: a per-lane index into the arguments would go through scratch)
#pragma unroll
      for (int k = 1; k < PNR_MAX_RHO; ++k) rho = o == k ? a.a.rho[k] : rho;
      const float z = d * (1.0f + rho);
      backproject((float)u, (float)v, z, a.a.fx, a.a.fy, a.a.cx, a.a.cy, a.a.c2w, px, py, pz);
      valid = d > 0.f && d <= 3.402823466e+38f && px > a.a.bound[0] && px < a.a.bound[1] && py > a.a.bound[2] &&
              py < a.a.bound[3] && pz > a.a.bound[4] && pz < a.a.bound[5];
    }
    fre = valid;
    if (valid && a.hdr) {
      int bx, by, bz;
      base_cell(px, a.g.o0, a.g.inv, bx);
      base_cell(py, a.g.o1, a.g.inv, by);
      base_cell(pz, a.g.o2, a.g.inv, bz);
      int4 h[8];  // all 8 headers in flight before the first is used
#pragma unroll
      for (int n = 0; n < 8; ++n)
        h[n] = a.hdr[cell_hash(bx + (n & 1), by + ((n >> 1) & 1), bz + (n >> 2), a.g.mask)];
      bool hit = false;
#pragma unroll
      for (int n = 0; n < 8; ++n) {
        const uint64_t hk = (uint64_t)(uint32_t)h[n].z | ((uint64_t)(uint32_t)h[n].w << 32);
        const bool coll = (hk & kCollision) != 0;
        const bool own = (hk & ~kCollision) == cell_key(bx + (n & 1), by + ((n >> 1) & 1), bz + (n >> 2));
        // (every point read is an existing point and the distance test is exact, so a colliding
        // bucket needs no per-point cell test here: a hit through any bucket is a hit)
        if (!hit && (coll || own) && h[n].y > h[n].x) {
          for (int j = h[n].x; j < h[n].y; ++j) {
            const float4 q = a.sorted[j];
            const float d0 = px - q.x, d1 = py - q.y, d2 = pz - q.z;
            if ((d0 * d0 + d1 * d1) + d2 * d2 <= a.r2) {
              hit = true;
              break;
            }
          }
        }
      }
      fre = !hit;
    }
    a.v.pos[c] = make_float4(px, py, pz, 0.f);
    a.v.flags[c] = (uint8_t)((valid ? PNR_ADD_VALID : 0) | (fre ? PNR_ADD_FREE : 0));
    if (a.a.cand_xyz) {
      a.a.cand_xyz[c * 3 + 0] = px;
      a.a.cand_xyz[c * 3 + 1] = py;
      a.a.cand_xyz[c * 3 + 2] = pz;
    }
  }
  const uint64_t mv = __ballot(valid), mf = __ballot(fre);
  if ((threadIdx.x & 63) == 0) {
    s_cnt[threadIdx.x >> 6][0] = (uint32_t)__popcll(mv);
    s_cnt[threadIdx.x >> 6][1] = (uint32_t)__popcll(mf);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const uint64_t nv = s_cnt[0][0] + s_cnt[1][0] + s_cnt[2][0] + s_cnt[3][0];
    const uint64_t nf = s_cnt[0][1] + s_cnt[1][1] + s_cnt[2][1] + s_cnt[3][1];
    if (nv) atomicAdd(a.v.cnt + (blockIdx.x & (kCntLists - 1)) * 16, (unsigned long long)(nv | (nf << 32)));
  }
}

__global__ __launch_bounds__(256) void k_add_thin_claim(AddArgs a) {
  const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= a.n_cand || !(a.v.flags[c] & PNR_ADD_FREE)) return;
  const float4 p = a.v.pos[c];
  const unsigned long long key = cell_key(cell_coord(p.x, a.g.o0, a.inv_thin), cell_coord(p.y, a.g.o1, a.inv_thin),
                                          cell_coord(p.z, a.g.o2, a.inv_thin));
  uint32_t h = (uint32_t)mix64(key) & a.tmask;
  // at most half of the entries are ever claimed, so the probe ends at a match or an empty entry
  while (true) {
    unsigned long long cur = a.v.keys[h];
    if (cur == kEmptyKey) cur = atomicCAS(a.v.keys + h, kEmptyKey, key);
    if (cur == kEmptyKey || cur == key) break;
    h = (h + 1) & a.tmask;
  }
  atomicMin(a.v.mins + h, (uint32_t)c);
  a.v.slot[c] = (int32_t)h;
}

__global__ __launch_bounds__(256) void k_add_thin_mark(AddArgs a) {
  const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= a.n_cand) return;
  uint8_t f = a.v.flags[c];
  bool keep = (f & PNR_ADD_FREE) != 0;
  if (keep && a.inv_thin > 0.f) keep = a.v.mins[a.v.slot[c]] == (uint32_t)c;
  if (keep) f |= PNR_ADD_KEPT;
  a.v.keep[c] = keep ? 1 : 0;
  if (a.a.cand_flags) a.a.cand_flags[c] = f;
}

__global__ __launch_bounds__(256) void k_add_emit(AddArgs a) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t c = t >> 3;
  const int part = (int)(t & 7);
  if (c >= a.n_cand || !a.v.keep[c]) return;
  const int64_t r = a.v.rank[c];
  if (r >= a.room) return;
  const int64_t row = a.n_live + r;
  if (a.vec4) {
    reinterpret_cast<float4*>(a.feats)[row * 8 + part] =
        a.a.init_feats ? reinterpret_cast<const float4*>(a.a.init_feats)[c * 8 + part] : make_float4(0.f, 0.f, 0.f, 0.f);
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e)
      a.feats[row * 32 + part * 4 + e] = a.a.init_feats ? a.a.init_feats[c * 32 + part * 4 + e] : 0.f;
  }
  if (part < 3) {
    const float4 p = a.v.pos[c];
    a.xyz[row * 3 + part] = part == 0 ? p.x : (part == 1 ? p.y : p.z);
  }
}

__global__ __launch_bounds__(64) void k_add_counters(AddArgs a) {
  unsigned long long w = a.v.cnt[threadIdx.x * 16];
  unsigned long long nv = w & 0xFFFFFFFFull, nf = w >> 32;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    nv += __shfl_xor(nv, o);
    nf += __shfl_xor(nf, o);
  }
  if (threadIdx.x == 0) {
    const int64_t kept = a.n_cand > 0 ? (int64_t)a.v.rank[a.n_cand] : 0;
    a.counters[0] = a.n_cand;
    a.counters[1] = (int64_t)nv;
    a.counters[2] = (int64_t)nf;
    a.counters[3] = kept;
    a.counters[4] = kept > a.room ? kept - a.room : 0;
  }
}

}  // namespace

int64_t points_add_candidates(const pnr_points_add& a) {
  if (a.H < 1 || a.W < 1 || a.n_rho < 1 || a.n_rho > PNR_MAX_RHO) return -1;
  int64_t n_pix;
  if (a.pixels) {
    if (a.n_pixels < 0) return -1;
    n_pix = a.n_pixels;
  } else {
    if (a.stride < 1) return -1;
    n_pix = (int64_t)((a.H + a.stride - 1) / a.stride) * ((a.W + a.stride - 1) / a.stride);
  }
  if (n_pix > 0x7FFFFFFFll / a.n_rho) return -1;
  return n_pix * a.n_rho;
}

size_t points_add_workspace_bytes(int64_t n_cand) {
  size_t b = 0;
  add_view(nullptr, n_cand, &b);
  return b;
}

int launch_points_add(const pnr_points& pts, int64_t capacity, float* xyz, float* feats, const pnr_points_add& ar,
                      void* ws, size_t ws_bytes, int64_t* counters, hipStream_t st) {
  const int64_t n = points_add_candidates(ar);
  if (n < 0) return PNR_E_ARG;
  size_t need = 0;
  AddArgs a{};
  a.v = add_view(ws, n, &need);
  if (!ws || ws_bytes < need) return PNR_E_WORKSPACE;
  a.a = ar;
  a.n_cand = n;
  a.n_live = pts.n_points;
  a.room = capacity - pts.n_points;
  a.nW = ar.pixels ? 1 : (ar.W + ar.stride - 1) / ar.stride;
  a.g = make_grid(pts);
  if (pts.n_points > 0) {
    const IndexView iv = index_view(pts.index, pts.n_points, pts.table_bits, nullptr);
    a.hdr = iv.hdr;
    a.sorted = iv.sorted;
  }
  a.r2 = ar.radius_add * ar.radius_add;
  a.inv_thin = ar.thin > 0.f ? 1.0f / ar.thin : 0.f;
  a.tmask = (uint32_t)(a.v.Tn - 1);
  a.xyz = xyz;
  a.feats = feats;
  a.vec4 = ((reinterpret_cast<uintptr_t>(feats) | reinterpret_cast<uintptr_t>(ar.init_feats)) & 15) == 0;
  a.counters = counters;
  if (hipMemsetAsync(a.v.cnt, 0, (size_t)kCntLists * 16 * 8, st) != hipSuccess) return (int)hipGetLastError();
  if (n > 0) {
    const unsigned nb = (unsigned)((n + 255) / 256);
    hipLaunchKernelGGL(k_add_candidates, dim3(nb), dim3(256), 0, st, a);
    if (ar.thin > 0.f) {
      if (hipMemsetAsync(a.v.keys, 0xFF, (size_t)a.v.Tn * 12, st) != hipSuccess) return (int)hipGetLastError();
      hipLaunchKernelGGL(k_add_thin_claim, dim3(nb), dim3(256), 0, st, a);
    }
    hipLaunchKernelGGL(k_add_thin_mark, dim3(nb), dim3(256), 0, st, a);
    const int rc = scan_exclusive(a.v.keep, a.v.rank, n, a.v.scratch, st);
    if (rc) return rc;
    hipLaunchKernelGGL(k_add_emit, dim3((unsigned)((n * 8 + 255) / 256)), dim3(256), 0, st, a);
  }
  hipLaunchKernelGGL(k_add_counters, dim3(1), dim3(64), 0, st, a);
  return hip_status(hipGetLastError());
}

}  // namespace pnr
