// pose.hip -- bundle adjustment in the Mapper iteration (src/Mapper.py:460-500, 567-581, 657-692): the
// keyframe camera tensors as a second parameter group of Mapper.optimize_map.
//
//   k_map_ray_grads   dL/drays_o, dL/drays_d of the map pass: per ray, the sum over its regulation,
//                     coarse and importance rows of the delta chain's dL/dx (k_ray_grads' sums over the
//                     three row segments of pnr_map_fwd)
//   k_pose_step       per window frame: dL/dt = sum g_o, dL/dR = sum g_d dir^T (the adjoint of
//                     get_rays_from_uv, src/common.py:74-89), the chain through quad2rotation
//                     (src/common.py:137-160, with its 2 / sum q^2 term) into the (F,7) camera-tensor
//                     gradient, Adam on the frames that are not fixed, and their c2w rows rewritten from
//                     the stepped tensors -- one launch
#include <hip/hip_runtime.h>

#include "adam.h"
#include "pnr_internal.h"

#pragma clang fp contract(off)  // render.hip's rule: the reference's unfused arithmetic

namespace pnr {

namespace {
inline unsigned nblk(int64_t n, int b) { return (unsigned)((n + b - 1) / b); }
}  // namespace

// Rows of the map pass (capi.cpp MapWS): regulation [0, n S) | coarse [pr, pr + n S) | importance
// [r1, r1 + n I); gx is the delta chain's dL/dx over all of them (with the gather backward's dL/dp
// already added, neural points).  dL/do = sum g_x; dL/dd = sum g_x z + g_nrm d/|d|: the regulation z is
// k_reg_z's float32 z (recomputed from gt, t_vals and t_rand), the render z the saved float64 z; the
// importance z carries no gradient of its own (Renderer.py:190 detaches it).  float64 sums in row order.
__global__ __launch_bounds__(128) void k_map_ray_grads(pnr_render_params prm, const float* __restrict__ rd,
                                                       const float* __restrict__ gt,
                                                       const float* __restrict__ t_rand,
                                                       const double* __restrict__ zc, const double* __restrict__ zi,
                                                       const float* __restrict__ gx, int64_t pr, int64_t r1,
                                                       const float* __restrict__ g_nrm, int64_t n_rays,
                                                       float* __restrict__ g_o, float* __restrict__ g_d) {
  const int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= n_rays) return;
  const int S = prm.n_samples, I = prm.n_importance;
  double o[3] = {0, 0, 0}, d[3] = {0, 0, 0};
  {  // k_reg_z's float arithmetic: the z the forward used
    const float far = gt[n] * 0.85f;
    auto z0 = [&](int k) { return (0.0f * (1.f - prm.t_vals[k])) + far * prm.t_vals[k]; };
    for (int s = 0; s < S; ++s) {
      const float zs = z0(s);
      const float lower = s > 0 ? .5f * (zs + z0(s - 1)) : zs;
      const float upper = s < S - 1 ? .5f * (z0(s + 1) + zs) : zs;
      const float z = lower + (upper - lower) * t_rand[n * S + s];
      for (int c = 0; c < 3; ++c) {
        const double g = gx[(n * S + s) * 3 + c];
        o[c] += g;
        d[c] += g * (double)z;
      }
    }
  }
  for (int s = 0; s < S; ++s)
    for (int c = 0; c < 3; ++c) {
      const double g = gx[(pr + n * S + s) * 3 + c];
      o[c] += g;
      d[c] += g * zc[n * S + s];
    }
  for (int s = 0; s < I; ++s)
    for (int c = 0; c < 3; ++c) {
      const double g = gx[(r1 + n * I + s) * 3 + c];
      o[c] += g;
      d[c] += g * zi[n * I + s];
    }
  const float* dv = rd + n * 3;
  const float gn = g_nrm[n];
  // |d| as the ray kernels form it (render.hip ray_norm)
  const float nrm = sqrtf(__builtin_fmaf(dv[2], dv[2], __builtin_fmaf(dv[1], dv[1], dv[0] * dv[0])));
  for (int c = 0; c < 3; ++c) {
    g_o[n * 3 + c] = (float)o[c];
    const float extra = nrm > 0.f ? gn * dv[c] / nrm : 0.f;
    g_d[n * 3 + c] = (float)d[c] + extra;
  }
}

int launch_map_ray_grads(const pnr_render_params& prm, const float* rd, const float* gt, const float* t_rand,
                         const double* zc, const double* zi, const float* gx, int64_t pr, int64_t r1,
                         const float* g_nrm, int64_t n, float* g_o, float* g_d, hipStream_t st) {
  if (n <= 0) return 0;
  hipLaunchKernelGGL(k_map_ray_grads, dim3(nblk(n, 128)), dim3(128), 0, st, prm, rd, gt, t_rand, zc, zi, gx, pr, r1,
                     g_nrm, n, g_o, g_d);
  return hip_status(hipGetLastError());
}

// ---------------------------------------------------------------------------------------------
// The pose step.  Grid: `bpf` blocks per frame; block (f, b) adds the twelve sums of its rays of frame
// f (3 of dL/dt, 9 of dL/dR) in float64 -- a fixed order: thread-strided, wave butterfly, four waves --
// and hands its partial to the block that takes the last ticket (k_map_loss's hand-off: 8-B agent
// atomics both sides, the storing wave's vmcnt(0), then the ticket).  That block adds each frame's
// partials in block order, so the result does not depend on which block finishes last, and runs the
// per-frame tail on one thread per frame.
constexpr int kPoseBlock = 256;
constexpr int kPoseMaxBpf = 16;
struct PoseArgs {
  const float* g_o;
  const float* g_d;
  const int64_t* idx;
  int64_t npf, hw;
  int F, bpf, W, adam;
  float fx, fy, cx, cy;
  float* cam;            // (F,7) qw qx qy qz tx ty tz
  const uint8_t* fixed;  // (F) or null
  float* m;
  float* v;
  float lr, beta1, beta2, eps;
  int32_t* step;  // completed Adam steps (advanced here)
  float* c2w;     // (F,4,4)
  float* g_cam;   // (F,7)
  uint32_t* ticket;
  double* part;  // [F * bpf][12]
};

// R = quad2rotation(q) as pnr.common restates it: two_s = 2 / sum q^2, R = I + two_s A(q)
__device__ __forceinline__ void quad_rotation(const double q[4], double R[9]) {
  const double r = q[0], i = q[1], j = q[2], k = q[3];
  const double ts = 2.0 / (r * r + i * i + j * j + k * k);
  R[0] = 1.0 - ts * (j * j + k * k);
  R[1] = ts * (i * j - k * r);
  R[2] = ts * (i * k + j * r);
  R[3] = ts * (i * j + k * r);
  R[4] = 1.0 - ts * (i * i + k * k);
  R[5] = ts * (j * k - i * r);
  R[6] = ts * (i * k - j * r);
  R[7] = ts * (j * k + i * r);
  R[8] = 1.0 - ts * (i * i + j * j);
}

__global__ __launch_bounds__(kPoseBlock) void k_pose_step(PoseArgs a) {
  __shared__ double red[kPoseBlock / 64][12];
  __shared__ uint32_t last;
  const int f = (int)blockIdx.x / a.bpf, b = (int)blockIdx.x % a.bpf;
  const int tid = (int)threadIdx.x;
  double acc[12];
#pragma unroll
  for (int t = 0; t < 12; ++t) acc[t] = 0.0;
  for (int64_t r = (int64_t)b * kPoseBlock + tid; r < a.npf; r += (int64_t)a.bpf * kPoseBlock) {
    const int64_t k = (int64_t)f * a.npf + r;
    int64_t pix = a.idx[k];
    pix = pix < 0 ? 0 : (pix >= a.hw ? a.hw - 1 : pix);  // k_window_rays' clamp
    float dir[3];
    {  // make_ray's float32 directions: the adjoint of the rays the forward built
      const float i = (float)(pix % a.W), j = (float)(pix / a.W);
      dir[0] = (i - a.cx) / a.fx;
      dir[1] = -((j - a.cy) / a.fy);
      dir[2] = -1.f;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      acc[c] += (double)a.g_o[k * 3 + c];
      const double gd = (double)a.g_d[k * 3 + c];
#pragma unroll
      for (int e = 0; e < 3; ++e) acc[3 + c * 3 + e] += gd * (double)dir[e];
    }
  }
#pragma unroll
  for (int t = 0; t < 12; ++t) {
    double s = acc[t];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if ((tid & 63) == 0) red[tid >> 6][t] = s;
  }
  __syncthreads();
  if (tid < 12) {
    const double s = (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]);
    atomicExch(reinterpret_cast<unsigned long long*>(a.part) + (int64_t)blockIdx.x * 12 + tid,
               (unsigned long long)__double_as_longlong(s));
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  }
  __syncthreads();
  if (tid == 0) {
    const uint32_t t = atomicAdd(a.ticket, 1u);
    last = t == gridDim.x - 1 ? 1u : 0u;
  }
  __syncthreads();
  if (!last) return;
  const int32_t step = a.adam ? *a.step : 0;
  for (int fr = tid; fr < a.F; fr += kPoseBlock) {
    const bool fix = a.fixed && a.fixed[fr];
    if (fix) {  // a fixed frame takes no gradient and is not written
#pragma unroll
      for (int t = 0; t < 7; ++t) a.g_cam[fr * 7 + t] = 0.f;
      continue;
    }
    double G[12];
#pragma unroll
    for (int t = 0; t < 12; ++t) G[t] = 0.0;
    for (int bb = 0; bb < a.bpf; ++bb)
#pragma unroll
      for (int t = 0; t < 12; ++t)
        G[t] += __longlong_as_double((long long)atomicAdd(
            reinterpret_cast<unsigned long long*>(a.part) + ((int64_t)fr * a.bpf + bb) * 12 + t, 0ull));
    const double* gR = G + 3;  // dL/dR[i][j] at gR[i * 3 + j]
    double q[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) q[t] = (double)a.cam[fr * 7 + t];
    const double r = q[0], i = q[1], j = q[2], k = q[3];
    const double ts = 2.0 / (r * r + i * i + j * j + k * k);
    // R = I + ts A(q): dL/dts = sum G A, dts/dq = -ts^2 q
    const double A[9] = {-(j * j + k * k), i * j - k * r, i * k + j * r, i * j + k * r, -(i * i + k * k),
                         j * k - i * r, i * k - j * r, j * k + i * r, -(i * i + j * j)};
    double gts = 0.0;
#pragma unroll
    for (int t = 0; t < 9; ++t) gts += gR[t] * A[t];
    const double dr = -k * gR[1] + j * gR[2] + k * gR[3] - i * gR[5] - j * gR[6] + i * gR[7];
    const double di = j * gR[1] + k * gR[2] + j * gR[3] - 2.0 * i * gR[4] - r * gR[5] + k * gR[6] + r * gR[7] -
                      2.0 * i * gR[8];
    const double dj = -2.0 * j * gR[0] + i * gR[1] + r * gR[2] + i * gR[3] + k * gR[5] - r * gR[6] + k * gR[7] -
                      2.0 * j * gR[8];
    const double dk = -2.0 * k * gR[0] - r * gR[1] + i * gR[2] + r * gR[3] - 2.0 * k * gR[4] + j * gR[5] +
                      i * gR[6] + j * gR[7];
    const double dq[4] = {dr, di, dj, dk};
    float g7[7];
#pragma unroll
    for (int t = 0; t < 4; ++t) g7[t] = (float)(ts * dq[t] - gts * ts * ts * q[t]);
#pragma unroll
    for (int t = 0; t < 3; ++t) g7[4 + t] = (float)G[t];
#pragma unroll
    for (int t = 0; t < 7; ++t) a.g_cam[fr * 7 + t] = g7[t];
    if (!a.adam) continue;
    const AdamCoef coef = adam_coef(step, a.lr, a.beta1, a.beta2);
    float p7[7];
#pragma unroll
    for (int t = 0; t < 7; ++t) {
      float mi = a.m[fr * 7 + t], vi = a.v[fr * 7 + t];
      p7[t] = adam_update(g7[t], mi, vi, a.cam[fr * 7 + t], a.beta1, a.beta2, a.eps, coef);
      a.m[fr * 7 + t] = mi;
      a.v[fr * 7 + t] = vi;
      a.cam[fr * 7 + t] = p7[t];
    }
    // the frame's c2w row from the stepped tensor (get_camera_from_tensor), bottom row 0 0 0 1
    const double qn[4] = {(double)p7[0], (double)p7[1], (double)p7[2], (double)p7[3]};
    double R[9];
    quad_rotation(qn, R);
    float* M = a.c2w + (int64_t)fr * 16;
#pragma unroll
    for (int rr = 0; rr < 3; ++rr) {
#pragma unroll
      for (int cc = 0; cc < 3; ++cc) M[rr * 4 + cc] = (float)R[rr * 3 + cc];
      M[rr * 4 + 3] = p7[4 + rr];
    }
    M[12] = 0.f;
    M[13] = 0.f;
    M[14] = 0.f;
    M[15] = 1.f;
  }
  __syncthreads();  // every frame's thread has read the step before it advances
  if (tid == 0) {
    if (a.adam) *a.step = step + 1;
    *a.ticket = 0u;  // zero again for the next call on this workspace
  }
}

int pose_step_bpf(int64_t npf) {
  const int64_t b = (npf + kPoseBlock - 1) / kPoseBlock;
  return (int)(b < 1 ? 1 : (b > kPoseMaxBpf ? kPoseMaxBpf : b));
}
// ticket word (8 bytes) + the block partials
int64_t pose_step_workspace_bytes(int64_t F, int64_t npf) {
  return 8 + F * pose_step_bpf(npf) * 12 * (int64_t)sizeof(double);
}

int launch_pose_step(const float* g_o, const float* g_d, const int64_t* idx, int F, int64_t npf, int H, int W,
                     float fx, float fy, float cx, float cy, float* cam, const uint8_t* fixed, float* m, float* v,
                     float lr, float beta1, float beta2, float eps, int32_t* step, int adam, float* c2w,
                     float* g_cam, void* ws, hipStream_t st) {
  PoseArgs a{};
  a.g_o = g_o;
  a.g_d = g_d;
  a.idx = idx;
  a.npf = npf;
  a.hw = (int64_t)H * W;
  a.F = F;
  a.bpf = pose_step_bpf(npf);
  a.W = W;
  a.adam = adam;
  a.fx = fx;
  a.fy = fy;
  a.cx = cx;
  a.cy = cy;
  a.cam = cam;
  a.fixed = fixed;
  a.m = m;
  a.v = v;
  a.lr = lr;
  a.beta1 = beta1;
  a.beta2 = beta2;
  a.eps = eps;
  a.step = step;
  a.c2w = c2w;
  a.g_cam = g_cam;
  a.ticket = static_cast<uint32_t*>(ws);
  a.part = reinterpret_cast<double*>(static_cast<char*>(ws) + 8);
  hipLaunchKernelGGL(k_pose_step, dim3((unsigned)(F * a.bpf)), dim3(kPoseBlock), 0, st, a);
  return hip_status(hipGetLastError());
}

}  // namespace pnr
