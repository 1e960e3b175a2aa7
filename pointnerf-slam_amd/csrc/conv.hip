// conv.hip -- implicit-GEMM convolution for the SuperPoint network (src/demo_superpoint.py:78-131): float32
// planar (Cin,H,W) -> (Cout,H,W), batch 1, stride 1, 3x3 with zero padding 1 or 1x1.
//
//   out[co][y][x] = bias[co] + sum over (tap, ci) of w[tap][ci][co] x[ci][y + dy - pad][x + dx - pad]
//
// k_conv (Cin a multiple of the chunk).  GEMM rows = output channels (A = weights), columns = pixels (B = the
// input): after v_mfma_f32_32x32x2_f32 lane (hh, i) holds pixel i of its wave's row segment and 16 channels
// perm(r, hh), so a planar store of one channel is 32 consecutive floats.
//   tile      one workgroup = 2 rows x 32 columns of pixels x TC = 64 NACC output channels, four waves:
//             wave w owns row w >> 1 and the NACC 32-channel blocks (w & 1) NACC + j.  NACC = 1 for every
//             plain layer; 2 (TC = 128 >= 65) for SOFTMAX_HEATMAP and 4 (TC = 256) for L2NORM, whose
//             reductions over the channels then stay inside one workgroup.
//   staging   no im2col.  Per cin chunk (CK = 8 for 3x3, 16 for 1x1) LDS holds, k-major,
//               patch [ci][py][px]      the halo patch, (2 + KS - 1) rows x (32 + KS - 1) columns, row pitch 40
//                                       (3x3) or 48 (1x1) so that a ci plane is 160 / 96 floats = 32 banks
//                                       modulo 64: the two k-planes of a B read fall on disjoint banks
//               slab  [tap][ci][co]     row stride TC + 32 (the same rule for the A read)
//             The B operand of tap (dy, dx) is the window patch[ci][row + dy][dx + i]: 32 consecutive floats
//             per k-plane, a shifted view of the one patch.  Two such buffers (2 x 32 KiB for 3x3: two
//             workgroups per CU); the next chunk's global loads (5 patch floats and 5 float4 of weights per
//             thread for 3x3) are in flight in registers while this chunk's MFMAs run and are stored to the
//             other buffer before the chunk's one barrier.
//   order     every output is one fp32 chain by one wave: acc = bias, then cin chunks ascending, inside a
//             chunk the taps ascending (ky major), inside a tap the cin pairs ascending (one MFMA each).
//   edges     a patch element outside the image is staged as 0 and never loaded; stores are guarded by
//             y < H, x < W, co < Cout; the packed weights are zero-padded to a multiple of 64 channels.
//   epilogues NONE, RELU: guarded planar stores.  RELU_POOL2: the tile's ReLU outputs go through LDS and
//             each thread writes four 2x2 maxima (tiles start on even rows and columns; H, W even).
//             SOFTMAX_HEATMAP (Cout = 65): semi is stored as NONE stores it, e = expf(semi), the 65-term sum
//             is reduced over registers, the half waves (one shuffle) and the row's two waves (LDS), and
//             heat[8 y + (c >> 3)][8 x + (c & 7)] = e_c / (sum + 1e-5f) for c < 64.  L2NORM (Cout = 256): the
//             sum of squares is reduced the same way and every output is divided by its square root.
// k_conv_c1 (Cin = 1, conv1a): one thread per pixel, 9 inputs in registers, one fma chain per channel in
// ascending tap.  K = 9 would fill 9 of 16 k-steps of a padded MFMA tile and the layer is bound by its
// 64-channel store (0.9 GFLOP against 209 MB at 680 x 1200), so it stays on the VALU.
// Vector stores only, no atomics.
#include "pnr_internal.h"

namespace pnr {

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kTW = 32;  // tile columns: the 32 MFMA columns of one wave
constexpr int kTH = 2;   // tile rows: one per pair of waves
constexpr int kPoolLd = 72;  // RELU_POOL2 exchange: channel stride (4 x 72 = 32 banks modulo 64)

template <int KS>
struct ConvCfg {
  static constexpr int T = KS * KS;
  static constexpr int PAD = KS / 2;
  static constexpr int CK = KS == 3 ? 8 : 16;
  static constexpr int PR = kTH + KS - 1;
  static constexpr int PW = kTW + KS - 1;
  static constexpr int PITCH = KS == 3 ? 40 : 48;
  static constexpr int PLANE = PR * PITCH;
  static constexpr int PATCH = CK * PLANE;
  static constexpr int NPE = CK * PR * PW;      // patch elements per chunk
  static constexpr int NP = (NPE + 255) / 256;  // per thread
};
static_assert(ConvCfg<3>::PLANE % 64 == 32 && ConvCfg<1>::PLANE % 64 == 32, "k-planes on disjoint banks");

struct ConvArgs {
  const float* x;
  const float* w;     // [T][Cin][cout_pad]
  const float* bias;  // [Cout]
  float* out;
  float* heat;
  int32_t Cin, Cout, cout_pad, H, W, tiles_x, tiles_y;
};

template <int KS, int NACC, int EPI>
__global__ __launch_bounds__(256) void k_conv(ConvArgs a) {
  using C = ConvCfg<KS>;
  constexpr int TC = 64 * NACC, WLD = TC + 32, SLAB = C::T * C::CK * WLD, BUF = SLAB + C::PATCH;
  constexpr int NW4 = C::T * C::CK * TC / 4, NWQ = (NW4 + 255) / 256;
  static_assert(WLD % 64 == 32 && 2 * BUF * 4 <= 65536 && 2 * BUF >= 64 * kPoolLd, "LDS layout");
  __shared__ __attribute__((aligned(16))) float lds[2 * BUF];
  const int t = threadIdx.x;
  const int lane = t & 63, hh = lane >> 5, i = lane & 31;
  const int w = __builtin_amdgcn_readfirstlane(t >> 6);
  const int row = w >> 1, chalf = w & 1;
  int b = blockIdx.x;
  const int x0 = (b % a.tiles_x) * kTW;
  b /= a.tiles_x;
  const int y0 = (b % a.tiles_y) * kTH;
  const int cb0 = (b / a.tiles_y) * TC;
  const int HW = a.H * a.W;

  // this thread's patch elements: global offset inside a chunk (-1: outside the image, staged as 0) and LDS
  // offset (-1: past the patch)
  int goff[C::NP], loff[C::NP];
#pragma unroll
  for (int q = 0; q < C::NP; ++q) {
    const int e = t + 256 * q;
    const int c = e / (C::PR * C::PW), rem = e % (C::PR * C::PW);
    const int py = rem / C::PW, px = rem % C::PW;
    const int gy = y0 - C::PAD + py, gx = x0 - C::PAD + px;
    const bool in = e < C::NPE;
    const bool ok = in && gy >= 0 && gy < a.H && gx >= 0 && gx < a.W;
    goff[q] = ok ? c * HW + gy * a.W + gx : -1;
    loff[q] = in ? c * C::PLANE + py * C::PITCH + px : -1;
  }
  // and its float4 pieces of the weight slab: row (tap, ci) of the chunk, four channels
  int wrow[NWQ], wcol[NWQ];
#pragma unroll
  for (int q = 0; q < NWQ; ++q) {
    const int e = t + 256 * q;
    wrow[q] = e < NW4 ? e / (TC / 4) : -1;
    wcol[q] = (e % (TC / 4)) * 4;
  }

  float pv[C::NP];
  float4 wv[NWQ];
  auto load_chunk = [&](int c0) {
    const float* xs = a.x + (int64_t)c0 * HW;
#pragma unroll
    for (int q = 0; q < C::NP; ++q) pv[q] = goff[q] >= 0 ? xs[goff[q]] : 0.f;
#pragma unroll
    for (int q = 0; q < NWQ; ++q) {
      wv[q] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (wrow[q] >= 0) {
        const int tap = wrow[q] / C::CK, c = wrow[q] % C::CK;
        wv[q] = *reinterpret_cast<const float4*>(a.w + ((int64_t)tap * a.Cin + c0 + c) * a.cout_pad + cb0 + wcol[q]);
      }
    }
  };
  auto store_chunk = [&](float* s) {
#pragma unroll
    for (int q = 0; q < C::NP; ++q)
      if (loff[q] >= 0) s[SLAB + loff[q]] = pv[q];
#pragma unroll
    for (int q = 0; q < NWQ; ++q)
      if (wrow[q] >= 0) *reinterpret_cast<float4*>(s + wrow[q] * WLD + wcol[q]) = wv[q];
  };

  // lane (hh, i), accumulator j, register r: channel cb0 + 32 (chalf NACC + j) + perm(r, hh), pixel (y0 + row, x0 + i)
  f32x16 acc[NACC];
#pragma unroll
  for (int j = 0; j < NACC; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int ch = cb0 + 32 * (chalf * NACC + j) + perm(r, hh);
      acc[j][r] = ch < a.Cout ? a.bias[ch] : 0.f;
    }

  load_chunk(0);
  store_chunk(lds);
  __syncthreads();
  int buf = 0;
  for (int c0 = 0; c0 < a.Cin; c0 += C::CK) {
    const bool more = c0 + C::CK < a.Cin;
    if (more) load_chunk(c0 + C::CK);
    const float* ws = lds + buf * BUF + hh * WLD + 32 * chalf * NACC + i;
    const float* ps = lds + buf * BUF + SLAB + hh * C::PLANE + row * C::PITCH + i;
#pragma unroll
    for (int tap = 0; tap < C::T; ++tap) {
      const int dy = tap / KS, dx = tap % KS;
#pragma unroll
      for (int kk = 0; kk < C::CK / 2; ++kk) {
        const float bv = ps[2 * kk * C::PLANE + dy * C::PITCH + dx];
#pragma unroll
        for (int j = 0; j < NACC; ++j)
          acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(ws[(tap * C::CK + 2 * kk) * WLD + 32 * j], bv, acc[j], 0, 0, 0);
      }
    }
    buf ^= 1;
    if (more) store_chunk(lds + buf * BUF);  // last read one barrier ago
    __syncthreads();
  }

  const int y = y0 + row, x = x0 + i;
  const bool pix_ok = y < a.H && x < a.W;
  if (EPI == PNR_CONV_NONE || EPI == PNR_CONV_RELU) {
#pragma unroll
    for (int j = 0; j < NACC; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int ch = cb0 + 32 * (chalf * NACC + j) + perm(r, hh);
        const float v = EPI == PNR_CONV_RELU ? fmaxf(acc[j][r], 0.f) : acc[j][r];
        if (pix_ok && ch < a.Cout) a.out[(int64_t)ch * HW + y * a.W + x] = v;
      }
  } else if (EPI == PNR_CONV_RELU_POOL2) {
    static_assert(EPI != PNR_CONV_RELU_POOL2 || NACC == 1, "the pool exchange holds 64 channels");
#pragma unroll
    for (int r = 0; r < 16; ++r)
      lds[(32 * chalf + perm(r, hh)) * kPoolLd + 32 * row + i] = fmaxf(acc[0][r], 0.f);
    __syncthreads();
    const int Ho = a.H >> 1, Wo = a.W >> 1;
    const int oy = y0 >> 1;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int o = t + 256 * q;
      const int xo = o & 15, chl = o >> 4;
      const int ch = cb0 + chl, ox = (x0 >> 1) + xo;
      if (ch < a.Cout && oy < Ho && ox < Wo) {
        const float* s = lds + chl * kPoolLd + 2 * xo;
        a.out[(int64_t)ch * Ho * Wo + oy * Wo + ox] = fmaxf(fmaxf(s[0], s[1]), fmaxf(s[32], s[33]));
      }
    }
  } else {
    // a reduction over the channels of each pixel: registers, the other half wave, the row's other wave
    float e[NACC][16];
    float sum = 0.f;
#pragma unroll
    for (int j = 0; j < NACC; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int ch = cb0 + 32 * (chalf * NACC + j) + perm(r, hh);
        const float v = acc[j][r];
        if (EPI == PNR_CONV_SOFTMAX_HEATMAP) {
          if (pix_ok && ch < a.Cout) a.out[(int64_t)ch * HW + y * a.W + x] = v;
          e[j][r] = ch < a.Cout ? expf(v) : 0.f;
          sum += e[j][r];
        } else {
          e[j][r] = v;
          sum += v * v;
        }
      }
    sum += __shfl_xor(sum, 32);
    if (hh == 0) lds[32 * w + i] = sum;
    __syncthreads();
    const float tot = lds[64 * row + i] + lds[64 * row + 32 + i];
    if (EPI == PNR_CONV_SOFTMAX_HEATMAP) {
      const float den = tot + 1e-5f;
      if (chalf == 0 && pix_ok) {
#pragma unroll
        for (int j = 0; j < NACC; ++j)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int ch = 32 * j + perm(r, hh);  // < 64: the dustbin is channel 64, in the other wave
            a.heat[(int64_t)(8 * y + (ch >> 3)) * (8 * a.W) + 8 * x + (ch & 7)] = e[j][r] / den;
          }
      }
    } else {
      const float nrm = sqrtf(tot);
#pragma unroll
      for (int j = 0; j < NACC; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int ch = cb0 + 32 * (chalf * NACC + j) + perm(r, hh);
          if (pix_ok && ch < a.Cout) a.out[(int64_t)ch * HW + y * a.W + x] = e[j][r] / nrm;
        }
    }
  }
}

__global__ __launch_bounds__(256) void k_conv_c1(ConvArgs a, int relu) {
  const int HW = a.H * a.W;
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= HW) return;
  const int y = p / a.W, x = p % a.W;
  float v[9];
#pragma unroll
  for (int tap = 0; tap < 9; ++tap) {
    const int yy = y + tap / 3 - 1, xx = x + tap % 3 - 1;
    v[tap] = (yy >= 0 && yy < a.H && xx >= 0 && xx < a.W) ? a.x[yy * a.W + xx] : 0.f;
  }
  for (int ch = 0; ch < a.Cout; ++ch) {
    float acc = a.bias[ch];
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) acc = fmaf(a.w[tap * a.cout_pad + ch], v[tap], acc);
    a.out[(int64_t)ch * HW + p] = relu ? fmaxf(acc, 0.f) : acc;
  }
}

template <int KS, int NACC, int EPI>
int launch_one(ConvArgs a, hipStream_t st) {
  a.tiles_x = (a.W + kTW - 1) / kTW;
  a.tiles_y = (a.H + kTH - 1) / kTH;
  const int64_t grid = (int64_t)a.tiles_x * a.tiles_y * (a.cout_pad / (64 * NACC));
  if (grid >= (1ll << 31)) return PNR_E_ARG;
  hipLaunchKernelGGL((k_conv<KS, NACC, EPI>), dim3((unsigned)grid), dim3(256), 0, st, a);
  return hip_status(hipGetLastError());
}

template <int KS>
int launch_plain(const ConvArgs& a, int epi, hipStream_t st) {
  if (epi == PNR_CONV_NONE) return launch_one<KS, 1, PNR_CONV_NONE>(a, st);
  if (epi == PNR_CONV_RELU) return launch_one<KS, 1, PNR_CONV_RELU>(a, st);
  return launch_one<KS, 1, PNR_CONV_RELU_POOL2>(a, st);
}

}  // namespace

int launch_conv2d(const float* x, const float* w, const float* bias, float* out, float* heat, int32_t Cin,
                  int32_t Cout, int32_t H, int32_t W, int32_t ksize, int32_t epi, hipStream_t st) {
  if (!x || !w || !bias || !out || H <= 0 || W <= 0) return PNR_E_ARG;
  if (Cin != 1 && Cin != 64 && Cin != 128 && Cin != 256) return PNR_E_ARG;
  if (Cout != 64 && Cout != 128 && Cout != 256 && Cout != 65) return PNR_E_ARG;
  if ((ksize != 1 && ksize != 3) || epi < PNR_CONV_NONE || epi > PNR_CONV_L2NORM) return PNR_E_ARG;
  if ((reinterpret_cast<uintptr_t>(w) & 15) != 0) return PNR_E_ARG;
  const int64_t cmax = Cin > Cout ? Cin : Cout;
  if (cmax * H * W >= (1ll << 31)) return PNR_E_ARG;  // offsets are int32
  if (epi == PNR_CONV_RELU_POOL2 && ((H | W) & 1)) return PNR_E_ARG;
  if (epi == PNR_CONV_SOFTMAX_HEATMAP && (Cout != 65 || ksize != 1 || !heat || 64ll * H * W >= (1ll << 31))) return PNR_E_ARG;
  if (epi == PNR_CONV_L2NORM && (Cout != 256 || ksize != 1)) return PNR_E_ARG;
  ConvArgs a{x, w, bias, out, heat, Cin, Cout, (Cout + 63) / 64 * 64, H, W, 0, 0};
  if (Cin == 1) {
    if (ksize != 3 || epi > PNR_CONV_RELU) return PNR_E_ARG;
    hipLaunchKernelGGL(k_conv_c1, dim3((unsigned)(((int64_t)H * W + 255) / 256)), dim3(256), 0, st, a,
                       (int)(epi == PNR_CONV_RELU));
    return hip_status(hipGetLastError());
  }
  if (epi == PNR_CONV_SOFTMAX_HEATMAP) return launch_one<1, 2, PNR_CONV_SOFTMAX_HEATMAP>(a, st);
  if (epi == PNR_CONV_L2NORM) return launch_one<1, 4, PNR_CONV_L2NORM>(a, st);
  return ksize == 3 ? launch_plain<3>(a, epi, st) : launch_plain<1>(a, epi, st);
}

}  // namespace pnr
