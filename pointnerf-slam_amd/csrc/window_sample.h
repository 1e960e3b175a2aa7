// window_sample.h -- the window sampler's block body (k_window_sample, render.hip) shared with the
// grouped head launch (k_sample_pack, mlp16_pack.hip), and the small helpers it uses.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#include <cstdint>

namespace pnr {

__device__ __forceinline__ float max_nanf(float m, float v) { return (v > m || v != v) ? v : m; }
__device__ __forceinline__ float block_max_256(float m, float* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = max_nanf(m, __shfl_xor(m, o));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
  __syncthreads();
  return max_nanf(max_nanf(red[0], red[1]), max_nanf(red[2], red[3]));
}

// rays: dirs = [(i-cx)/fx, -(j-cy)/fy, -1]; rays_d = sum(dirs * c2w[:3,:3], -1); rays_o = c2w[:3,3]
__device__ __forceinline__ void make_ray(float i, float j, float fx, float fy, float cx, float cy,
                                         const float* __restrict__ c2w, int ld, float* o, float* d) {
#pragma clang fp contract(off)  // (render.hip's rule: the reference's unfused float arithmetic)
  const float dx = (i - cx) / fx, dy = -((j - cy) / fy), dzv = -1.f;
  for (int r = 0; r < 3; ++r) {
    // torch.sum over the last dim of 3 products: ((a0 + a1) + a2), products rounded
    const float p0 = dx * c2w[r * ld + 0], p1 = dy * c2w[r * ld + 1], p2 = dzv * c2w[r * ld + 2];
    d[r] = (p0 + p1) + p2;
    o[r] = c2w[r * ld + 3];
  }
}

// World position of pixel (u, v) at depth z along make_ray's float32 ray: p = rays_o + rays_d z, unfused.
// One statement of it for the map growth (points_grow.hip k_add_candidates) and the mesh bound (bound.hip).
__device__ __forceinline__ void backproject(float u, float v, float z, float fx, float fy, float cx, float cy,
                                            const float* __restrict__ c2w, float& px, float& py, float& pz) {
#pragma clang fp contract(off)
  float ro[3], rd[3];
  make_ray(u, v, fx, fy, cx, cy, c2w, 4, ro, rd);
  px = ro[0] + rd[0] * z;
  py = ro[1] + rd[1] * z;
  pz = ro[2] + rd[2] * z;
}

// A mapping iteration's whole window batch in ONE launch, drawn on the device: the uniform pixels
// (torch.randint(H*W) per ray in Mapper.py:560-606's get_samples), the regulation jitter t_rand
// (torch.rand, Renderer.py:293), the rays and gt of k_window_rays, and the batch far clamp
// max(1.2 gt) (k_gt_max, Renderer.py:112) -- in place of randint + rand (+ the two seed / offset
// fills torch's RNG records in a captured graph) + the gt max.  The draws are a counter-based hash
// (splitmix64 finaliser of seed, batch and draw index), not torch's Philox stream: the same
// distribution, a different sequence.  The state holds the batch counter (advanced by the block
// that takes the last ticket, so a captured graph draws a fresh batch per replay), the ticket and
// the per-block maxima.
constexpr int kSampleParts = 64;
struct SampleState {
  int64_t batch;
  uint32_t ticket;
  uint32_t pad;
  uint64_t part[kSampleParts];  // per-block gt maxima (float bits), written and read by 8-B atomics
};
static_assert(sizeof(SampleState) == 16 + 8 * kSampleParts, "sampler state layout");
__device__ __forceinline__ uint64_t mix64(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
struct WindowSampleArgs {
  uint64_t seed;
  SampleState* stt;
  int64_t n, per_frame, hw;
  int W;
  float fx, fy, cx, cy;
  const float* c2w;
  const float* depth;
  const float* color;
  int S;
  float* ro;
  float* rd;
  float* gd;
  float* gc;
  float* t_rand;
  int64_t* idx_out;
  float* far_out;
};
// blocks of a sampler launch: ray blocks, then jitter blocks (4 values per thread)
inline int window_sample_blocks(int64_t n, int S) {
  const int64_t nbr = n < (int64_t)kSampleParts * 256 ? (n + 255) / 256 : kSampleParts;
  const int64_t nj = (n * (S > 0 ? S : 0) + 1023) / 1024;
  return (int)(nbr + (nj < 192 ? nj : 192));
}
// block `bid` of `nblk` sampler blocks (the ticket counts these alone: the launch may hold others)
__device__ __forceinline__ void window_sample_block(const WindowSampleArgs& a, const int bid, const int nblk) {
#pragma clang fp contract(off)
  const uint64_t seed = a.seed;
  SampleState* __restrict__ stt = a.stt;
  const int64_t n = a.n, per_frame = a.per_frame, hw = a.hw;
  const int W = a.W, S = a.S;
  const float fx = a.fx, fy = a.fy, cx = a.cx, cy = a.cy;
  const float* __restrict__ c2w = a.c2w;
  const float* __restrict__ depth = a.depth;
  const float* __restrict__ color = a.color;
  float* __restrict__ ro = a.ro;
  float* __restrict__ rd = a.rd;
  float* __restrict__ gd = a.gd;
  float* __restrict__ gc = a.gc;
  float* __restrict__ t_rand = a.t_rand;
  int64_t* __restrict__ idx_out = a.idx_out;
  float* __restrict__ far_out = a.far_out;
  __shared__ float red[4];
  __shared__ uint32_t last;
  const int64_t batch = stt->batch;
  const uint64_t base = mix64(seed + (uint64_t)batch * 0x9E3779B97F4A7C15ull);
  // blocks [0, nbr) draw the rays (and their gt maxima, part[0..nbr)); the others draw the jitter,
  // one value per thread (a thread per ray drawing its 32 values serially was the launch's latency)
  const int nbr = (int)(n < (int64_t)kSampleParts * 256 ? (n + 255) / 256 : kSampleParts);
  float m = -INFINITY;
  if ((int)bid < nbr) {
    for (int64_t k = (int64_t)bid * 256 + threadIdx.x; k < n; k += (int64_t)nbr * 256) {
      const int64_t f = k / per_frame;
      const uint64_t r = mix64(base + (uint64_t)k * 0xD1B54A32D192ED03ull);
      const int64_t pix = (int64_t)(((r >> 32) * (uint64_t)hw) >> 32);  // uniform in [0, hw) (hw < 2^32)
      if (idx_out) idx_out[k] = pix;
      make_ray((float)(pix % W), (float)(pix / W), fx, fy, cx, cy, c2w + f * 16, 4, ro + k * 3, rd + k * 3);
      const int64_t q = f * hw + pix;
      const float d = depth[q];
      gd[k] = d;
      gc[k * 3 + 0] = color[q * 3 + 0];
      gc[k * 3 + 1] = color[q * 3 + 1];
      gc[k * 3 + 2] = color[q * 3 + 2];
      m = max_nanf(m, d * 1.2f);
    }
  } else {
    const int64_t ns = n * S, stride = (int64_t)(nblk - nbr) * 256;
    for (int64_t e = (int64_t)(bid - nbr) * 256 + threadIdx.x; e < ns; e += stride) {
      // 24-bit uniforms in [0, 1), like torch.rand's float32: value (k, s) is draw n + k S + s
      const uint64_t u = mix64(base + (uint64_t)(n + e) * 0xD1B54A32D192ED03ull);
      t_rand[e] = (float)(uint32_t)(u >> 40) * 0x1p-24f;
    }
  }
  m = block_max_256(m, red);
  // ticket hand-off as k_map_loss (8-B agent atomics both sides); the last block reduces the maxima
  // and advances the batch
  if (threadIdx.x == 0) {
    if ((int)bid < nbr) atomicExch(stt->part + bid, (unsigned long long)__float_as_uint(m));
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const uint32_t t = atomicAdd(&stt->ticket, 1u);
    last = t == (uint32_t)(nblk - 1) ? 1u : 0u;
  }
  __syncthreads();
  if (!last) return;
  __shared__ float red2[4];
  const float v = block_max_256(
      (int)threadIdx.x < nbr ? __uint_as_float((uint32_t)atomicAdd(stt->part + threadIdx.x, 0ull)) : -INFINITY, red2);
  if (threadIdx.x == 0) {
    if (far_out) far_out[0] = v;
    stt->batch = batch + 1;
    stt->ticket = 0u;
  }
}

inline WindowSampleArgs window_sample_args(uint64_t seed, void* state, int64_t n, int64_t per_frame, int H, int W, float fx,
                                    float fy, float cx, float cy, const float* c2w, const float* depth,
                                    const float* color, int S, float* ro, float* rd, float* gd, float* gc,
                                    float* t_rand, int64_t* idx, float* far_out) {
  return WindowSampleArgs{seed, (SampleState*)state, n, per_frame, (int64_t)H * W, W, fx, fy, cx, cy, c2w, depth, color,
                          S, ro, rd, gd, gc, t_rand, idx, far_out};
}

}  // namespace pnr
