// keypoints.hip -- SuperPoint's post-processing on the device (src/demo_superpoint.py:158-293): threshold,
// greedy non-maximum suppression, border cut, and the bilinear descriptor sample.
//
// Rank.  Candidate p (heat[p] >= conf_thresh, p = y W + x) ranks above q when heat[p] > heat[q], or the two
// are equal and p < q: a total order.  Greedy NMS walks the candidates in rank order, keeps one that is not
// yet suppressed, and lets it suppress every candidate within Chebyshev distance nms_dist.  Equivalently
//   p is kept  <=>  no kept candidate of higher rank lies in p's window
// which defines kept / suppressed uniquely by induction over the rank.  It is solved as a fixed point on one
// int32 state per pixel (none, undecided, kept, suppressed):
//   an undecided p becomes suppressed when it sees a kept higher-ranked candidate in its window,
//   and kept when it sees no kept and no undecided higher-ranked one; otherwise it waits.
// A decision is only taken from decisions that are final, so every written state is the greedy one whatever
// the order in which pixels are visited and however stale a neighbour's state is read (a stale read can only
// make p wait): the result does not depend on scheduling.  Progress: the highest-ranked undecided candidate
// of a pass over a set of pixels always decides, so a loop "until a pass changes nothing" ends with nothing
// undecided among the pixels of a workgroup that can see all its own writes.
//   k_kp_classify  state = undecided | none, the counters cleared.
//   k_nms          a workgroup sweeps its tile of pixels until a sweep changes nothing.  Three launches with
//                  32 x 32 tiles (a tile waits only for chains that enter it from another tile), each adding
//                  the number of pixels it leaves undecided to a counter; a launch returns at once when the
//                  one before left none.  Then one workgroup with the whole image as its tile, which cannot
//                  end with an undecided pixel: it is the guarantee, and normally returns at once.
//   k_kp_emit      kept pixels with border <= x < W - border, border <= y < H - border append the key
//                    heat bits << 32 | (0xFFFFFFFF - p)         (heat > 0: its bits order as the floats do)
//                  to the key list through an integer atomic counter; the caller sorts the keys descending,
//                  which is the output order (confidence descending, then p ascending) whatever the append
//                  order was.
//   k_sample_desc  one workgroup per keypoint, one thread per channel: the bilinear sample of the coarse map
//                  at (x / 8 - 0.5, y / 8 - 0.5) with zero padding (grid_sample, align_corners = False), the
//                  256 squares summed in a fixed order (wave shuffles, then the four wave sums), divided by
//                  the root.
// Integer atomics only, vector stores only.
#include "pnr_internal.h"

namespace pnr {

namespace {

constexpr int kNone = 0, kUndecided = 1, kKept = 2, kSuppressed = 3;
constexpr int kTileLaunches = 3;
constexpr int kNmsTile = 32;
constexpr size_t kHeaderBytes = 64;  // int32 counters: [0] keys appended, [1..3] undecided after tile launch 0..2

__device__ __forceinline__ int ld_state(const int32_t* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void st_state(int32_t* p, int v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(256) void k_kp_classify(const float* __restrict__ heat, int32_t n, float thresh,
                                                     int32_t* __restrict__ state, int32_t* __restrict__ ctr) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p < 16) ctr[p] = 0;
  if (p < n) state[p] = heat[p] >= thresh ? kUndecided : kNone;
}

__global__ void k_nms(const float* __restrict__ heat, int32_t* state, int32_t H, int32_t W, int32_t d, int32_t th,
                      int32_t tw, int32_t tiles_x, const int32_t* left_before, int32_t* left_after) {
  if (left_before && *left_before == 0) return;
  const int t = threadIdx.x;
  const int y0 = (int)(blockIdx.x / tiles_x) * th, x0 = (int)(blockIdx.x % tiles_x) * tw;
  const int hh = min(th, H - y0), ww = min(tw, W - x0);
  const int n = hh * ww;
  int changed;
  do {
    changed = 0;
    for (int e = t; e < n; e += blockDim.x) {
      const int y = y0 + e / ww, x = x0 + e % ww;
      const int p = y * W + x;
      if (ld_state(state + p) != kUndecided) continue;
      const float hp = heat[p];
      bool kept_above = false, undecided_above = false;
      for (int yy = max(0, y - d); yy <= min(H - 1, y + d); ++yy)
        for (int xx = max(0, x - d); xx <= min(W - 1, x + d); ++xx) {
          const int q = yy * W + xx;
          const int s = ld_state(state + q);
          if (q == p || (s != kKept && s != kUndecided)) continue;
          const float hq = heat[q];
          if (hq > hp || (hq == hp && q < p)) {
            kept_above |= s == kKept;
            undecided_above |= s == kUndecided;
          }
        }
      if (kept_above || !undecided_above) {
        st_state(state + p, kept_above ? kSuppressed : kKept);
        changed = 1;
      }
    }
    changed = __syncthreads_or(changed);
  } while (changed);
  if (left_after) {
    int left = 0;
    for (int e = t; e < n; e += blockDim.x) left += ld_state(state + (y0 + e / ww) * W + x0 + e % ww) == kUndecided;
    if (left) atomicAdd(left_after, left);
  }
}

__global__ __launch_bounds__(256) void k_kp_emit(const float* __restrict__ heat, const int32_t* __restrict__ state,
                                                 int32_t H, int32_t W, int32_t border,
                                                 unsigned long long* __restrict__ keys, int32_t* __restrict__ count) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= H * W || state[p] != kKept) return;
  const int y = p / W, x = p % W;
  if (x < border || x >= W - border || y < border || y >= H - border) return;
  const int pos = atomicAdd(count, 1);
  keys[pos] = ((unsigned long long)__float_as_uint(heat[p]) << 32) | (unsigned long long)(0xFFFFFFFFu - (uint32_t)p);
}

__global__ __launch_bounds__(256) void k_sample_desc(const float* __restrict__ coarse, int32_t Hc, int32_t Wc,
                                                     const float* __restrict__ pts, int32_t N,
                                                     float* __restrict__ desc) {
  __shared__ float s_sum[4];
  const int k = blockIdx.x, c = threadIdx.x;
  const float ix = pts[k] * 0.125f - 0.5f, iy = pts[N + k] * 0.125f - 0.5f;
  const float fx = floorf(ix), fy = floorf(iy);
  const int xa = (int)fx, ya = (int)fy;
  const float wx = ix - fx, wy = iy - fy;
  const float* m = coarse + (int64_t)c * Hc * Wc;
  auto at = [&](int yy, int xx) { return (yy >= 0 && yy < Hc && xx >= 0 && xx < Wc) ? m[yy * Wc + xx] : 0.f; };
  const float v = (at(ya, xa) * (1.f - wx) + at(ya, xa + 1) * wx) * (1.f - wy) +
                  (at(ya + 1, xa) * (1.f - wx) + at(ya + 1, xa + 1) * wx) * wy;
  float ss = v * v;
#pragma unroll
  for (int s = 1; s < 64; s <<= 1) ss += __shfl_xor(ss, s);
  if ((c & 63) == 0) s_sum[c >> 6] = ss;
  __syncthreads();
  const float tot = (s_sum[0] + s_sum[1]) + (s_sum[2] + s_sum[3]);
  desc[(int64_t)c * N + k] = v / sqrtf(tot);
}

bool size_ok(int32_t H, int32_t W) {
  return H > 0 && W > 0 && H % 8 == 0 && W % 8 == 0 && (int64_t)H * W < (1ll << 28);
}

}  // namespace

// workspace: counters (64 B) | keys uint64[H W] | state int32[H W]; 0 for sizes the call refuses
size_t superpoint_workspace_bytes(int32_t H, int32_t W) {
  if (!size_ok(H, W)) return 0;
  return kHeaderBytes + (size_t)H * W * 12;
}

int launch_superpoint_keypoints(const float* heat, int32_t H, int32_t W, float thresh, int32_t nms_dist,
                                int32_t border, void* ws, size_t ws_bytes, hipStream_t st) {
  if (!heat || !ws || !size_ok(H, W) || !(thresh > 0.f) || nms_dist < 0 || nms_dist > 64 || border < 0) return PNR_E_ARG;
  if (reinterpret_cast<uintptr_t>(ws) & 7) return PNR_E_ARG;
  if (ws_bytes < superpoint_workspace_bytes(H, W)) return PNR_E_WORKSPACE;
  const int n = H * W;
  int32_t* ctr = static_cast<int32_t*>(ws);
  unsigned long long* keys = reinterpret_cast<unsigned long long*>(static_cast<char*>(ws) + kHeaderBytes);
  int32_t* state = reinterpret_cast<int32_t*>(keys + n);
  const unsigned blocks = (unsigned)((n + 255) / 256);
  hipLaunchKernelGGL(k_kp_classify, dim3(blocks), dim3(256), 0, st, heat, n, thresh, state, ctr);
  const int tx = (W + kNmsTile - 1) / kNmsTile, ty = (H + kNmsTile - 1) / kNmsTile;
  for (int j = 0; j < kTileLaunches; ++j)
    hipLaunchKernelGGL(k_nms, dim3((unsigned)(tx * ty)), dim3(256), 0, st, heat, state, H, W, nms_dist, kNmsTile,
                       kNmsTile, tx, j ? ctr + j : nullptr, ctr + j + 1);
  hipLaunchKernelGGL(k_nms, dim3(1), dim3(1024), 0, st, heat, state, H, W, nms_dist, H, W, 1, ctr + kTileLaunches,
                     (int32_t*)nullptr);
  hipLaunchKernelGGL(k_kp_emit, dim3(blocks), dim3(256), 0, st, heat, state, H, W, border, keys, ctr);
  return hip_status(hipGetLastError());
}

int launch_superpoint_sample_desc(const float* coarse, int32_t Hc, int32_t Wc, const float* pts, int64_t N,
                                  float* desc, hipStream_t st) {
  if (Hc <= 0 || Wc <= 0 || N < 0 || N >= (1ll << 23) || 256ll * Hc * Wc >= (1ll << 31)) return PNR_E_ARG;
  if (N == 0) return PNR_OK;
  if (!coarse || !pts || !desc) return PNR_E_ARG;
  hipLaunchKernelGGL(k_sample_desc, dim3((unsigned)N), dim3(256), 0, st, coarse, Hc, Wc, pts, (int32_t)N, desc);
  return hip_status(hipGetLastError());
}

}  // namespace pnr
