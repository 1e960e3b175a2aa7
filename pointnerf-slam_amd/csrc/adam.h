// adam.h -- the Adam arithmetic shared by k_adam_multi (render.hip) and k_reduce_adam_multi
// (wgrad16.hip): one expression tree for both kernels, so they give the same bits
// (tests/test_gpu_step_tail.py compares them).  No FMA contraction: each product and sum is rounded,
// as in torch's elementwise Adam.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace pnr {

// bias corrections of step `step + 1` (pnr_adam_step's host arithmetic: double pow, then float)
struct AdamCoef {
  float step_size, bc2_sqrt;
};
__device__ __forceinline__ AdamCoef adam_coef(int32_t step, float lr, float beta1, float beta2) {
#pragma clang fp contract(off)
  const double t = (double)(step + 1);
  const double bc1 = 1.0 - pow((double)beta1, t), bc2 = 1.0 - pow((double)beta2, t);
  return AdamCoef{(float)((double)lr / bc1), (float)sqrt(bc2)};
}

// torch.optim.Adam (amsgrad=False, weight_decay=0) on one element: m, v updated in place, returns p'
__device__ __forceinline__ float adam_update(float g, float& m, float& v, float p, float beta1, float beta2, float eps,
                                             const AdamCoef c) {
#pragma clang fp contract(off)  // torch's unfused float arithmetic, whichever kernel inlines this
  const float mn = m + (1.f - beta1) * (g - m);
  const float vn = v * beta2 + (1.f - beta2) * g * g;
  m = mn;
  v = vn;
  const float denom = sqrtf(vn) / c.bc2_sqrt + eps;
  return p + (-c.step_size) * (mn / denom);
}

// the f16 images' power-of-two scale of a tensor with max|W| = mx: s = 2^e, e = floor(log2(2^14 / mx))
// clamped to [-20, 20] (e = 20 for an all-zero tensor); scl = s, inv = 1/s, both exact
__device__ __forceinline__ void wscale_from_max(float mx, float* scl, float* inv) {
  int e = 20;
  if (mx > 0.f) {
    int ex;
    frexpf(16384.f / mx, &ex);  // 16384/max = f 2^ex, f in [0.5,1)
    e = ex - 1;                 // 2^e <= 16384/max
    e = e < -20 ? -20 : (e > 20 ? 20 : e);
  }
  *scl = ldexpf(1.f, e);
  *inv = ldexpf(1.f, -e);
}

}  // namespace pnr
