/*
 * pnr.h -- C ABI of the MI355X (gfx950) neural volume renderer `libpnr.so`.
 *
 * Drop-in boundary for the `render_batch_ray` hot path of thua919/pointNeRF-SLAM
 * (src/utils/Renderer.py + src/common.py + src/conv_onet/models/decoder.py).  The Python
 * host mirror `pnr` (pointnerf-slam_amd/pnr/) binds these symbols with ctypes; any other
 * FFI (cgo, JNI, N-API) can bind them the same way -- see INTEGRATION.md.
 *
 * Conventions
 *  - Every pointer argument is a DEVICE pointer owned by the caller, except `pnr_render_params`
 *    and the `const float* const*` parameter-table arrays, which are HOST structs holding device
 *    pointers.  The library allocates no device memory and keeps no per-call state; scratch comes
 *    from the caller's workspace (size from the matching *_workspace_bytes query).
 *  - `stream` is a hipStream_t passed as void* (0 = legacy default stream).  All calls are
 *    asynchronous and stream-ordered; they are re-entrant (the only global state is the opt-in
 *    kernel-timing record of pnr_timing_enable).
 *  - Return value: 0 on success, a negative PNR_E* code on argument errors, or a positive
 *    hipError_t when a launch fails.  No exception ever crosses the ABI.
 *  - Dtypes follow the reference exactly: sample depths z / points / depth / variance are
 *    float64, rays / colours / densities / MLP weights are float32.
 *
 * Decoder parameter table (`params[11]`), the reference state_dict order
 * (src/conv_onet/models/decoder.py:128-159; src/conv_onet/config.py:29-31):
 *    0 embedder._B            (3,93)      1 pts_linears.0.weight (256,93)   2 pts_linears.0.bias (256)
 *    3 pts_linears.1.weight   (256,256)   4 pts_linears.1.bias   (256)
 *    5 pts_linears.2.weight   (256,256)   6 pts_linears.2.bias   (256)
 *    7 pts_linears.3.weight   (256,256)   8 pts_linears.3.bias   (256)
 *    9 output_linear.weight   (4,256)    10 output_linear.bias   (4)
 * all contiguous row-major float32.
 */
#ifndef PNR_H_
#define PNR_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PNR_ABI_VERSION 14
#define PNR_N_PARAMS 11
#define PNR_MAX_SAMPLES 64      /* N_samples + N_importance per ray */
#define PNR_C_DIM 32            /* neural-point feature width (decoder.py:122-125 fc_c input) */
#define PNR_MAX_K 8             /* neighbours per sample of the point gather */
#define PNR_N_FC_PARAMS 8       /* fc_c.{0..3}.weight (256,32), fc_c.{0..3}.bias (256), interleaved */

enum {
  PNR_OK = 0,
  PNR_E_ARG = -1,        /* bad argument (null pointer, negative size, unsupported config) */
  PNR_E_WORKSPACE = -2,  /* workspace smaller than *_workspace_bytes */
  PNR_E_BLAS = -3,       /* reserved (no BLAS library is used) */
};

/* ---- neural points (build-defined, no reference counterpart) --------
 * Feature of a sample p: the (up to) k neighbours x_i with the smallest (|p-x_i|^2, i) among
 *   PNR_GATHER_IDW:       |p - x_i| <= radius,           weight w_i = 1 / max(|p - x_i|, eps)
 *   PNR_GATHER_TRILINEAR: |p_a - x_i,a| < spacing_a (all a), w_i = prod_a (1 - |p_a - x_i,a| / spacing_a)
 * c(p) = sum_k (w_k / sum w) f_k, 0 without neighbours (oracle/ref_points.py is the spec).  With
 * points on a lattice, TRILINEAR reproduces MLP.sample_grid_feature's F.grid_sample
 * (src/conv_onet/models/decoder.py:168-175) on interior samples.  The decoder then injects c
 * into every hidden layer: h = relu(W h + b) + fc_c[i](c) (decoder.py:196-197).
 * Search structure: a spatial hash of cubic cells (edge `cell`, corner `origin`) into
 * 2^table_bits buckets, bucket-sorted copies of the positions; built on the device by
 * pnr_points_build into the caller's `index` buffer.  `cell` must be >= 2 * radius * (1 + 2^-9)
 * (IDW) or >= 2 * max(spacing) * (1 + 2^-9) (TRILINEAR): the search visits the 2x2x2 cells
 * covering [p - reach, p + reach], and the margin absorbs the f32 rounding of cell coordinates. */
enum { PNR_GATHER_IDW = 0, PNR_GATHER_TRILINEAR = 1 };

/* Arithmetic of the decoder matmuls (build-defined; the reference runs torch fp32 matmuls).
 *   PNR_PREC_FP32:   v_mfma_f32_32x32x2_f32, an exact fp32 fma chain (bitwise the CPU order per
 *                    product; only the summation order differs from torch CPU).
 *   PNR_PREC_F16X3:  (default) every fp32 operand split x = hi + lo into two f16 parts (22
 *                    significant bits), W x computed as Wh xh + Wh xl + Wl xh on
 *                    v_mfma_f32_32x32x16_f16 with fp32 accumulation (~2^-21 relative per product),
 *                    5.3x the fp32 MFMA rate.  The packer scales each weight tensor by a power of two
 *                    (max |W| s <= 2^14) and the kernel scales the accumulator back exactly.  The
 *                    forward needs |activations| < 65504 (f16 range): a larger value sets
 *                    PNR_STATUS_F16_RANGE in *prm->status.
 *   PNR_PREC_BF16X3: the same split in bf16 parts (16 significant bits, no range limit).
 *   PNR_PREC_BF16:   plain bf16 forward operands, fp32 accumulation (BASELINE config C3).
 * Fourier features, bias, ReLU, compositing and all float64 work stay fp32 / fp64 in every mode.
 * Backward of every mode but PNR_PREC_FP32 (which runs fp32 MFMA throughout): the delta chain is
 * f16x3 with an exact per-point power-of-two scale (any gradient magnitude), and the weight-gradient
 * GEMMs dW0..dW3, dWc are f16x3 on fp32-stored activations and deltas (per-wave power-of-two scale of
 * the deltas; delta4 = (Wo^T g_out) masked is not stored but rebuilt in fp32 FMAs inside the dW3
 * GEMM); dWo and dB are fp32 FMA reductions.  Point features (the fc_c operand) are split under a
 * power-of-two scale of their own in both directions (forward: per wave; dWc: per-wave running
 * scale), so they keep 22 bits whatever their magnitude (the reference's fine-grid features have
 * std 1e-4).  Hidden activations and the Fourier features are split unscaled (|e| <= 1, activations
 * checked < 65504): 22 bits for values >= 2^-3 and an absolute error <= 2^-25 below.  In a
 * weight-gradient element dW[i][j] = sum_p delta_i h_j that bounds each term's error by
 * |delta_i| 2^-25: an element whose unit j stays below ~3e-5 at every point carries more than 1e-3
 * relative error, but is itself < 1e-6 of a typical element.  (A per-point scale of the activation
 * rows, measured this round, cost 32% of the weight-gradient time.)  Every GEMM accumulates in fp32. */
enum { PNR_PREC_FP32 = 0, PNR_PREC_BF16X3 = 1, PNR_PREC_BF16 = 2, PNR_PREC_F16X3 = 3 };

/* Status bits (ABI 7) the kernels OR into the caller's device word pnr_render_params.status:
 *   PNR_STATUS_F16_RANGE  an F16X3 forward met a value >= 65504 to split into f16 parts (the result
 *                         of that call is not fp32-faithful; re-run it in PNR_PREC_FP32). */
enum { PNR_STATUS_F16_RANGE = 1 };

typedef struct pnr_points {
  const float* xyz;         /* (M,3) float32 point positions                                  */
  const float* feats;       /* (M,32) float32 point features                                  */
  int64_t n_points;         /* M                                                              */
  int32_t mode;             /* PNR_GATHER_IDW / PNR_GATHER_TRILINEAR                          */
  int32_t k;                /* neighbours kept, 1..PNR_MAX_K                                  */
  float radius;             /* IDW ball radius                                                */
  float eps;                /* IDW distance floor                                             */
  float spacing[3];         /* TRILINEAR lattice spacing per axis                             */
  float cell;               /* hash cell edge                                                 */
  float origin[3];          /* hash cell origin                                               */
  int32_t table_bits;       /* 10..24                                                         */
  void* index;              /* device buffer of pnr_points_index_bytes() bytes                */
  const float* fc_packed;   /* fc_c weight image (pnr_fc_pack) for the decoder; may be NULL for
                               the standalone gather                                           */
  float* g_feats;           /* backward: dL/dfeats (M,32) ACCUMULATED, or NULL                */
  float* const* g_fc;       /* backward: host array of 8 device ptrs accumulating dL/dfc_c, or NULL */
  int32_t feat_half;        /* ABI 6: 1 = `feats` holds (M,32) float16 (read-only copy of an fp32
                               master; sums, weights and g_feats stay float32), 0 = float32     */
} pnr_points;

/* Renderer configuration: the cfg keys Renderer.__init__ reads (src/utils/Renderer.py:6-21)
 * plus host-computed torch.linspace tables (Renderer.py:157, common.py:33). */
typedef struct pnr_render_params {
  int32_t n_samples;        /* cfg['rendering']['N_samples']  (<= 64)            */
  int32_t n_importance;     /* cfg['rendering']['N_importance'] (n_samples+n_importance <= 64) */
  int32_t lindisp;          /* cfg['rendering']['lindisp']                       */
  int32_t far_mode;         /* 0: clamp far to max(1.2*gt) of THIS batch (Renderer.py:112);
                               1: clamp to `far_clamp` (global max supplied by a sharded caller);
                               2: clamp to *far_clamp_dev (a device float32, e.g. the all-reduced
                                  max of a sharded batch: no host round trip, graph-capturable) */
  double bound[6];          /* slam.bound (3,2) float64 row-major: x0,x1,y0,y1,z0,z1   */
  double far_clamp;         /* used when far_mode == 1                                 */
  float t_vals[PNR_MAX_SAMPLES];   /* torch.linspace(0,1,n_samples) float32           */
  float u_vals[PNR_MAX_SAMPLES];   /* torch.linspace(0,1,n_importance) float32        */
  int32_t save_for_backward;       /* 1: keep MLP activations in the workspace for pnr_render_bwd;
                                      2 (ABI 8): keep only the ReLU masks and inputs -- the backward
                                      then computes NO decoder / fc_c weight gradients (grads and
                                      g_fc must be NULL: the Tracker's camera-only backward); the
                                      split precisions skip the 4 KB/point activation stores
                                      (PNR_PREC_FP32 saves everything either way) */
  int32_t need_ray_grads;          /* backward also produces dL/drays_o, dL/drays_d (tracking) */
  const pnr_points* points;        /* neural-point features, NULL = the reference decoder (c_dim=0) */
  int32_t precision;               /* PNR_PREC_* of the decoder matmuls                           */
  int32_t grads_overwrite;         /* ABI 11, backward: 0 = add the decoder / fc_c weight gradients
                                      into `grads` / `g_fc` (autograd's accumulation), 1 = store them
                                      (the caller need not zero them first; point-feature gradients
                                      always accumulate)                                          */
  int32_t* status;                 /* ABI 7: device int32 receiving PNR_STATUS_* bits (ORed), or NULL */
  const float* far_clamp_dev;      /* ABI 7: device float32 far clamp of far_mode 2                */
} pnr_render_params;

/* ---- library identity -------------------------------------------------------------------- */
int pnr_abi_version(void);
const char* pnr_build_info(void);

/* ---- decoder: MLP.forward / eval_points -------------------------------------------------- */
/* Number of float32 words of the packed (MFMA-fragment-ordered) weight image: the fp32 fragment
 * images plus the bf16 split images of the PNR_PREC_BF16X3 / PNR_PREC_BF16 kernels. */
size_t pnr_mlp_packed_floats(void);
/* Builds the packed image from the 11 reference tensors (params: host array of device ptrs).
 * Must be re-run after every optimizer step (the image is a pure function of the weights). */
int pnr_mlp_pack(const float* const* params, float* packed, void* stream);
/* ABI 14: pnr_mlp_pack with flags.  PNR_PACK_F16X3_ONLY: only the images the PNR_PREC_F16X3 kernels
 * read (the weight scales, the forward and delta-chain images and the raw table; the fp32 and bf16
 * images are left as they were) -- a Mapper iteration's repack after its Adam step, on the critical
 * path.  Those images are bit for bit those of pnr_mlp_pack.  flags 0 = pnr_mlp_pack. */
#define PNR_PACK_F16X3_ONLY 2
int pnr_mlp_pack2(const float* const* params, float* packed, int32_t flags, void* stream);

/* Renderer.eval_points (src/utils/Renderer.py:23-61): raw[P,4] = MLP(p) with raw[:,3] := 100
 * where p is not strictly inside `bound6`.  p float64 (P,3).  `precision`: PNR_PREC_*. */
int pnr_eval_points(const float* packed, const double* p, int64_t P, const double* bound6,
                    float* raw_out, int32_t precision, void* stream);
/* Same for float32 points (MLP.forward on f32 input, decoder.py:177-203); bound6 may be NULL
 * (then no masking).  The mask comparison is done in float32 as torch does for f32 points. */
int pnr_eval_points_f32(const float* packed, const float* p, int64_t P, const double* bound6,
                        float* raw_out, int32_t precision, void* stream);

/* MLP.forward with autograd (decoder.py:177-203 on float32 points, no bound mask): the forward
 * keeps activations in `ws` (size pnr_mlp_train_workspace_bytes(P)); pnr_mlp_bwd consumes them.
 * g_raw (P,4) float32; grads accumulated (+=); g_p (P,3) written when non-NULL. */
size_t pnr_mlp_train_workspace_bytes(int64_t P);
int pnr_mlp_fwd_train(const float* packed, const float* p, int64_t P, float* raw_out, void* ws, size_t ws_bytes,
                      int32_t precision, void* stream);
size_t pnr_mlp_bwd_workspace_bytes(int64_t P);
int pnr_mlp_bwd(const float* packed, int64_t P, const float* g_raw, float* const* grads, float* g_p, void* ws,
                size_t ws_bytes, void* bwd_ws, size_t bwd_bytes, int32_t precision, void* stream);

/* ---- map pass (ABI 10): one Mapper iteration's two decoder passes as ONE pass --------------------
 * src/Mapper.py:623-655 renders the window batch with gt depth (render_batch_ray: N_samples coarse +
 * N_importance importance samples, Renderer.py:63-203) and queries the density at N_samples jittered
 * depths per ray (regulation, Renderer.py:263-301).  pnr_map_fwd runs both with shared MLP launches:
 * launch A over the regulation + coarse samples, launch B over the importance samples; the points and
 * their bound tests are formed by the ray kernels in the reference's dtypes (float32 regulation,
 * float64 render).  Outputs: depth, var (n) float64, rgb (n,3), sigma (n, N_samples) float32 -- bit for
 * bit those of pnr_render_fwd + pnr_regulation_fwd with the same t_rand (tests/test_gpu_mapping.py).
 * pnr_map_bwd takes dL/ddepth, dL/drgb, dL/dsigma and runs ONE delta chain / weight-gradient pass over
 * every sample (grads accumulated, +=; neural points as in pnr_render_bwd); no ray gradients
 * (pnr_map_bwd_rays is the form with them).
 * prm: save_for_backward / need_ray_grads ignored (the pass always trains the decoder); n_importance > 0;
 * far_mode as pnr_render_fwd; t_rand (n, N_samples) float32 in [0,1). */
size_t pnr_map_workspace_bytes(const pnr_render_params* prm, int64_t n_rays);
int pnr_map_fwd(const pnr_render_params* prm, const float* packed, const float* rays_o, const float* rays_d,
                const float* gt_depth, const float* t_rand, int64_t n, double* depth, double* var, float* rgb,
                float* sigma, void* workspace, size_t ws_bytes, void* stream);
size_t pnr_map_bwd_workspace_bytes(const pnr_render_params* prm, int64_t n_rays);
int pnr_map_bwd(const pnr_render_params* prm, const float* packed, const float* rays_d, int64_t n,
                const double* g_depth, const float* g_rgb, const float* g_sigma, float* const* grads, void* workspace,
                size_t ws_bytes, void* bwd_ws, size_t bwd_bytes, void* stream);

/* ---- neural points ------------------------------------------------------------------------ */
size_t pnr_points_index_bytes(int64_t n_points, int32_t table_bits);
/* (Re)builds pts->index from pts->xyz (after any change of positions / cell / origin). */
int pnr_points_build(const pnr_points* pts, void* stream);
/* Growing the map from a keyframe's depth (build-defined, as the gather is; tests/points_grow_ref.py
 * is the spec).  Candidate c = pixel_rank * n_rho + o is pixel (u, v) of the list (`pixels`, flat
 * v W + u, any order, repeats allowed) or of the `stride` lattice in row-major order, at depth
 * z = depth[v,u] * (1 + rho[o]) (float32), position p = rays_o + rays_d * z with pnr_get_rays' own
 * float32 ray.  A candidate is VALID when its depth is finite and > 0 and bound[2a] < p_a <
 * bound[2a+1] on every axis (a pixel index outside the image is invalid, p = 0); FREE when no
 * existing point (rows [0, n_points), through pts->index) has (dx dx + dy dy) + dz dz <=
 * radius_add^2 in unfused float32; with thin > 0 only the smallest candidate index of each voxel
 * (edge `thin`, the hash origin, the 3 x 21-bit cell identity) is KEPT, with thin == 0 every free
 * one.  The kept candidates are appended in candidate order at rows [n_points, n_points + n_new) of
 * xyz_rw (capacity,3) / feats_rw (capacity,32) -- row c of init_feats, or zeros -- up to `capacity`;
 * no other row is written.  counters_dev: device int64[5] = {candidates, valid, free, kept, dropped
 * (kept rows beyond capacity)}, n_new = kept - dropped.  The result depends on nothing but the
 * arguments (integer atomics only, none in the output order).  Requires radius_add <= cell / (2 (1 +
 * 2^-9)) -- the 2x2x2 probe then covers the ball -- and an index built for the n_points rows;
 * the caller rebuilds it (pnr_points_build) with the new count afterwards.  At most 2^31 - 1
 * candidates per call.  pnr_points_add_workspace_bytes(n_cand): n_cand = pixels x n_rho. */
#define PNR_MAX_RHO 8
#define PNR_ADD_VALID 1
#define PNR_ADD_FREE 2
#define PNR_ADD_KEPT 4
typedef struct pnr_points_add {
  const float* depth;       /* (H,W) float32, device                                          */
  const float* c2w;         /* (4,4) float32 row-major, device                                */
  int32_t H, W;
  float fx, fy, cx, cy;
  const int64_t* pixels;    /* (n_pixels) flat pixel indices, device; NULL = the stride lattice */
  int64_t n_pixels;         /* length of `pixels` (ignored when NULL)                         */
  int32_t stride;           /* >= 1: pixels (0, s, 2s, ...) of both axes when `pixels` is NULL */
  int32_t n_rho;            /* 1..PNR_MAX_RHO                                                 */
  float rho[PNR_MAX_RHO];   /* relative depth offsets                                         */
  float radius_add;         /* > 0                                                            */
  float thin;               /* voxel edge of the thinning, 0 = none                           */
  float bound[6];           /* x0,x1,y0,y1,z0,z1 (float32: the test runs in the positions' type) */
  const float* init_feats;  /* (n_cand,32) float32 initial features per candidate, NULL = zeros */
  float* cand_xyz;          /* out, optional: (n_cand,3) candidate positions                  */
  uint8_t* cand_flags;      /* out, optional: (n_cand) PNR_ADD_* bits                         */
} pnr_points_add;
size_t pnr_points_add_workspace_bytes(int64_t n_cand);
int pnr_points_add_frame(const pnr_points* pts, int64_t capacity, float* xyz_rw, float* feats_rw,
                         const pnr_points_add* args, void* ws, size_t ws_bytes, int64_t* counters_dev, void* stream);
/* Standalone gather: c (P,32) float32 for float64 points p (P,3).  idx (P,k) int32 (-1 = none)
 * and w (P,k) float32 normalised weights are written when non-NULL (needed by the backward).
 * ws: pnr_point_gather_workspace_bytes(P) bytes (work list of samples with candidates). */
size_t pnr_point_gather_workspace_bytes(int64_t P);
int pnr_point_gather(const pnr_points* pts, const double* p, int64_t P, float* c, int32_t* idx, float* w,
                     void* ws, size_t ws_bytes, void* stream);
/* Backward of pnr_point_gather: g_c (P,32) -> pts->g_feats (+=, when non-NULL) and g_p (P,3)
 * (written, when non-NULL: dL/dp through the weights).  ws: pnr_point_gather_bwd_workspace_bytes
 * (ABI 10).  The feature gradient is DETERMINISTIC (ABI 10): every term w_k dL/dc is rounded once to
 * an int64 multiple of 2^-s, the terms are added exactly with 64-bit integer atomics, and the sum is
 * converted once into g_feats.  Any order of the additions gives the same bits.  The fixed point, in
 * full (tests/gather_bwd_model.py restates it): a sample row takes part when idx[row][0] >= 0; guard
 * = the smallest integer >= 1 with 2^guard > P, at most 40 (ceil(log2(P+1)) for P >= 1); gmax = max
 * |dL/dc| over every channel of the rows that take part; e = its frexp exponent (gmax = m 2^e, 0.5 <=
 * m < 1); s = 62 - guard - e, or 0 when gmax is 0, so |term| 2^s < 2^(62 - guard) and no sum of P
 * terms overflows.  A term is rint(ldexp(fl32(w_k dL/dc), s)): the float32 product, scaled exactly,
 * rounded half to even; the result g_feats = fl32(g_feats + fl32(float64(sum) 2^-s)).  The absolute
 * error of an element before that conversion is at most (its term count) x 2^-(s + 1) = (count) x
 * 2^-(63 - guard) x 2^e, under (count) x 2^-(62 - guard) x max |dL/dc|: fp32-class for any element
 * above ~2^-14 of the largest term.  A non-finite dL/dc in a row that takes part makes every element
 * of the feature rows the call's samples name NaN; rows no sample names are left untouched (ABI 12)
 * in sparse and dense calls alike (a dense call, P k >= 4 n_points, adds +0 to them: only a -0 there
 * changes, to +0), and a dL/dc row without neighbours has no effect at all. */
size_t pnr_point_gather_bwd_workspace_bytes(const pnr_points* pts, int64_t P);
int pnr_point_gather_bwd(const pnr_points* pts, const double* p, int64_t P, const int32_t* idx, const float* w,
                         const float* c, const float* g_c, float* g_p, void* ws, size_t ws_bytes, void* stream);
/* Diagnostics (ABI 10): the 64-bit atomic add instructions (32 lanes x 8 B = 256 B each) the last
 * pnr_point_gather_bwd with workspace `ws` issued (synchronises `stream`). */
int pnr_point_gather_bwd_atomics(const pnr_points* pts, const void* ws, int64_t P, int64_t* n_instr, void* stream);
/* fc_c weight image of the decoder (MLP(c_dim=32)): fc_params = host array of the 8 tensors
 * fc_c.0.weight, fc_c.0.bias, ..., fc_c.3.bias (contiguous float32). */
size_t pnr_fc_packed_floats(void);
int pnr_fc_pack(const float* const* fc_params, float* fc_packed, void* stream);
/* ABI 14: pnr_fc_pack with the pnr_mlp_pack2 flags. */
int pnr_fc_pack2(const float* const* fc_params, float* fc_packed, int32_t flags, void* stream);
/* MLP.forward with per-point features c (P,32): eval (bound6 may be NULL) and training
 * variants.  pnr_mlp_bwd_c also writes g_c (P,32) and accumulates the 8 fc_c grads. */
int pnr_eval_points_c(const float* packed, const float* fc_packed, const double* p, const float* c, int64_t P,
                      const double* bound6, float* raw_out, int32_t precision, void* stream);
int pnr_mlp_fwd_train_c(const float* packed, const float* fc_packed, const float* p, const float* c, int64_t P,
                        float* raw_out, void* ws, size_t ws_bytes, int32_t precision, void* stream);
size_t pnr_mlp_bwd_workspace_bytes_c(int64_t P);
int pnr_mlp_bwd_c(const float* packed, const float* fc_packed, const float* c, int64_t P, const float* g_raw,
                  float* const* grads, float* const* g_fc, float* g_c, float* g_p, void* ws, size_t ws_bytes,
                  void* bwd_ws, size_t bwd_bytes, int32_t precision, void* stream);

/* ---- render_batch_ray (src/utils/Renderer.py:63-203) ------------------------------------- */
size_t pnr_render_workspace_bytes(const pnr_render_params* prm, int64_t n_rays);
/* Forward.  depth, var: float64 (N); rgb float32 (N,3).  gt_depth may be NULL (gt_depth=None).
 * The workspace must stay untouched between this call and pnr_render_bwd. */
int pnr_render_fwd(const pnr_render_params* prm, const float* packed,
                   const float* rays_o, const float* rays_d, const float* gt_depth, int64_t n_rays,
                   double* depth, double* var, float* rgb,
                   void* workspace, size_t ws_bytes, void* stream);
/* Backward of the final (44-sample) pass.  Inputs are dL/ddepth, dL/dvar (float64, may be NULL
 * = zero), dL/drgb (float32, may be NULL).  Outputs: `grads` = host array of 11 device pointers
 * receiving dL/dparam (ACCUMULATED: +=, reference layout), or NULL for no decoder weight gradients
 * (ABI 5: the Tracker's camera-only backward skips every weight-gradient launch), g_rays_o / g_rays_d (N,3) float32
 * written (not accumulated) when prm->need_ray_grads, else ignored (may be NULL).
 * `params` = the same 11 raw tensors (needed for the transposed weight images). */
size_t pnr_render_bwd_workspace_bytes(const pnr_render_params* prm, int64_t n_rays);
int pnr_render_bwd(const pnr_render_params* prm, const float* packed, const float* const* params,
                   const float* rays_o, const float* rays_d, int64_t n_rays,
                   const double* g_depth, const double* g_var, const float* g_rgb,
                   float* const* grads, float* g_rays_o, float* g_rays_d,
                   void* workspace, size_t ws_bytes,
                   void* bwd_workspace, size_t bwd_ws_bytes, void* stream);

/* ---- Renderer.regulation (src/utils/Renderer.py:263-301) --------------------------------- */
/* sigma[N*n_samples] = density at z = lower + (upper-lower)*t_rand in [0, 0.85*gt], float32 z.
 * t_rand (N, n_samples) float32 replaces the reference's torch.rand draw (Renderer.py:293). */
size_t pnr_regulation_workspace_bytes(const pnr_render_params* prm, int64_t n_rays);
int pnr_regulation_fwd(const pnr_render_params* prm, const float* packed,
                       const float* rays_o, const float* rays_d, const float* gt_depth,
                       const float* t_rand, int64_t n_rays, float* sigma,
                       void* workspace, size_t ws_bytes, void* stream);
size_t pnr_regulation_bwd_workspace_bytes(const pnr_render_params* prm, int64_t n_rays);
int pnr_regulation_bwd(const pnr_render_params* prm, const float* packed, const float* const* params,
                       const float* rays_o, const float* rays_d, int64_t n_rays,
                       const float* g_sigma, float* const* grads, float* g_rays_o, float* g_rays_d,
                       void* workspace, size_t ws_bytes,
                       void* bwd_workspace, size_t bwd_ws_bytes, void* stream);

/* ---- rays (src/common.py:74-89, 248-266) ------------------------------------------------- */
/* Full-frame rays, row-major (H,W,3) float32; c2w (3,4) or (4,4) float32 row-major on device. */
int pnr_get_rays(int32_t H, int32_t W, float fx, float fy, float cx, float cy, const float* c2w,
                 float* rays_o, float* rays_d, void* stream);
/* Rays for pixel coordinates i (column), j (row), float32 (n). */
int pnr_rays_from_uv(const float* i, const float* j, int64_t n, float fx, float fy, float cx, float cy,
                     const float* c2w, float* rays_o, float* rays_d, void* stream);
/* ABI 10: a Mapper iteration's pixel batch over its keyframe window in one launch (src/Mapper.py:560-606:
 * per window frame get_samples(0, H, 0, W, pixs_per_image, ...), src/common.py:110-134).  Ray r uses
 * frame f = r / n_per_frame and pixel idx[r] (int64, uniform over the H x W image, row-major: column
 * idx % W, row idx / W; clamped into the image as select_uv clamps); c2w (F,4,4) float32, depth
 * (F,H,W) float32, color (F,H,W,3) float32.  Writes rays_o, rays_d (n,3), gt_depth (n), gt_color (n,3):
 * the same values as pnr_rays_from_uv + the reference's depth / colour gathers. */
int pnr_window_rays(const int64_t* idx, int64_t n, int64_t n_per_frame, int32_t H, int32_t W, float fx, float fy,
                    float cx, float cy, const float* c2w, const float* depth, const float* color, float* rays_o,
                    float* rays_d, float* gt_depth, float* gt_color, void* stream);

/* ABI 11: the same batch with its draws made on the device, plus the regulation jitter and the far
 * clamp, in ONE launch (a captured Mapper iteration replays it without torch's RNG launches):
 * pixel r ~ uniform over [0, H*W) (get_samples' torch.randint), t_rand (n, n_samples) ~ uniform
 * [0,1) with 24-bit resolution (Renderer.py:293's torch.rand), far_clamp[0] = max(1.2 * gt_depth)
 * (Renderer.py:112; pass it as far_clamp_dev, far_mode 2).  The draws are a counter-based hash of
 * (seed, batch, draw index) -- the reference's distribution, not torch's Philox sequence.  `state`
 * (pnr_window_sample_state_bytes(), zero-filled before the first call, not shared by concurrent
 * calls) holds the batch counter, advanced by each call on the device.  idx (n, int64) receives the
 * drawn pixels and may be NULL; far_clamp may be NULL.  Rays and gt equal pnr_window_rays on idx. */
size_t pnr_window_sample_state_bytes(void);
int pnr_window_sample(uint64_t seed, void* state, int64_t n, int64_t n_per_frame, int32_t H, int32_t W, float fx,
                      float fy, float cx, float cy, const float* c2w, const float* depth, const float* color,
                      int32_t n_samples, float* rays_o, float* rays_d, float* gt_depth, float* gt_color,
                      float* t_rand, int64_t* idx, float* far_clamp, void* stream);

/* ---- optimizer (src/Mapper.py:498-502, 657-662: torch.optim.Adam, default betas/eps) ----- */
/* One Adam step over `n` float32 words: p -= lr * mhat / (sqrt(vhat) + eps).  step >= 1. */
int pnr_adam_step(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1,
                  float beta2, float eps, int64_t step, void* stream);
/* The same step with the step number read on the device: step = *step_count + 1, where
 * step_count (int32, device) counts completed steps and is advanced by pnr_step_advance after the
 * step's last Adam launch.  Host-free, so a captured graph (hipGraph / torch.cuda.CUDAGraph) of a
 * whole mapping iteration replays with the right bias corrections. */
int pnr_adam_step_dev(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1,
                      float beta2, float eps, const int32_t* step_count, void* stream);
int pnr_step_advance(int32_t* step_count, void* stream);
/* ABI 10: Adam over n_seg (1..4) learning-rate segments of one flat parameter buffer -- segment q is
 * p[seg_offset[q] .. + seg_n[q]) with its own moments m[q], v[q] (device pointers, host array) and
 * lr seg_lr[q] -- AND the step advance, in ONE launch: step2 (int32[2], device) = {completed steps,
 * 0}; every element uses step = step2[0] + 1, and the launch leaves {step2[0] + 1, 0}.  Same
 * arithmetic as pnr_adam_step_dev per segment followed by pnr_step_advance. */
int pnr_adam_multi_dev(float* p, const float* g, int32_t n_seg, const int64_t* seg_offset, const int64_t* seg_n,
                       float* const* m, float* const* v, const float* seg_lr, float beta1, float beta2, float eps,
                       int32_t* step2, void* stream);
/* ABI 12: pnr_adam_multi_dev that also writes float16(p) of every updated element of segment q into
 * half_copy[q][0 .. seg_n[q]) when half_copy (host array of n_seg device pointers) and half_copy[q]
 * are non-NULL: the float16 feature copy the gather reads (pnr_points.feat_half), refreshed in the
 * same pass instead of a separate conversion of the whole table (round to nearest even, as torch's
 * float16 copy). */
int pnr_adam_multi_dev_h(float* p, const float* g, int32_t n_seg, const int64_t* seg_offset, const int64_t* seg_n,
                         float* const* m, float* const* v, const float* seg_lr, float beta1, float beta2, float eps,
                         uint16_t* const* half_copy, int32_t* step2, void* stream);

/* Mapper loss terms and their gradients (src/Mapper.py:628-655, the loss of Mapper.optimize_map
 * built from render_batch_ray's depth / colour and regulation's sigma), in one pass (ABI 9):
 *   *loss   = sum_{i<n, gt_depth_i > 0} |gt_depth_i - depth_i| + w_color sum_{i<n} |gt_color_i - color_i|_1
 *           + w_reg sum_{j<n_sigma} |sigma_j|                                          (float64)
 *   g_depth = -sign(gt_depth - depth) [gt_depth > 0]  (float64, n)
 *   g_color = -w_color sign(gt_color - color)         (float32, n x 3)
 *   g_sigma = w_reg sign(sigma)                       (float32, n_sigma)
 * sign(0) = 0 as torch's abs backward.  Either part may be empty (n = 0 or n_sigma = 0, its
 * pointers NULL).  The sum has a fixed order (deterministic).  workspace:
 * pnr_map_loss_workspace_bytes() bytes of device scratch, ZERO-FILLED before its first use (ABI 10: it
 * holds a ticket word that lets the last block add the partial sums, one launch; each call leaves it
 * zero-filled again, so a caller reuses one workspace for the calls of one stream).  Replaces the ~20
 * elementwise / reduction launches the torch form of the loss and its autograd backward cost. */
size_t pnr_map_loss_workspace_bytes(void);
int pnr_map_loss(const float* gt_depth, const double* depth, const float* gt_color, const float* color, int64_t n,
                 float w_color, const float* sigma, int64_t n_sigma, float w_reg, double* loss, double* g_depth,
                 float* g_color, float* g_sigma, void* workspace, void* stream);

/* One Mapper iteration's loss and decoder / fc_c / point-feature gradients in ONE call (ABI 13;
 * src/Mapper.py:623-655): pnr_map_fwd, pnr_map_loss and pnr_map_bwd on the same inputs.  Up to
 * 32,768 rays the final compositing, the loss terms and the compositing backward run as ONE fused
 * wave-per-ray launch (k_fine_loss_w): the gradients are bit for bit those of the three-call form,
 * the loss differs from pnr_map_loss's only in summation order (fixed: deterministic).  Larger
 * batches run the three calls' kernels.  No depth / colour / sigma outputs.
 *   workspace: pnr_map_step_workspace_bytes(prm, n); bwd_ws: pnr_map_bwd_workspace_bytes(prm, n);
 *   loss_ws: a pnr_map_loss workspace (zero-filled before its first use, left zero-filled);
 *   grads / prm->grads_overwrite / prm->points as pnr_map_bwd; *loss float64 on the device.
 * n = 0: *loss = 0 and (grads_overwrite) zero decoder / fc_c gradients. */
size_t pnr_map_step_workspace_bytes(const pnr_render_params* prm, int64_t n_rays);
int pnr_map_step(const pnr_render_params* prm, const float* packed, const float* rays_o, const float* rays_d,
                 const float* gt_depth, const float* gt_color, const float* t_rand, int64_t n, float w_color,
                 float w_reg, double* loss, float* const* grads, void* workspace, size_t ws_bytes, void* bwd_ws,
                 size_t bwd_bytes, void* loss_ws, void* stream);

/* The step with its optimiser (additions to ABI 14): pnr_map_step whose weight-gradient reduction also
 * takes the Adam step of pnr_adam_multi_dev (one segment) on every element it has just summed, and
 * leaves the weight scales of the next PNR_PACK_F16X3_ONLY pack -- ONE launch (k_reduce_adam_multi)
 * where the reduction, the Adam kernel and the pack's scale stage were three.  Bit for bit what
 * pnr_map_step + pnr_adam_multi_dev + pnr_mlp_pack2's scales give.
 *   p, g: the flat parameter / gradient buffers (n floats; the eleven grads[i] must tile [g, g + n)
 *   exactly -- only the elements the reduction owns are stepped -- else PNR_E_ARG); m, v: the moments
 *   of [0, n); step2 as pnr_adam_multi_dev;
 *   scales: pnr_step_tail_floats() floats, ZERO-FILLED before the first use and owned by this step
 *   (not shared by concurrent calls): floats [0, 5) receive the scales of W0..W3, Wo and [5, 10)
 *   their inverses (the rest is the kernel's hand-off scratch), for pnr_mlp_pack_scaled.
 * The fused tail runs, and *fused = 1, only when the precision is a split one, grads is given, there
 * are no neural points, n > 0, n_rays > 0, the backward is a single chunk and prm->grads_overwrite
 * is set; otherwise the call is pnr_map_step unchanged, *fused = 0, and the caller runs Adam. */
typedef struct pnr_adam_tail {
  float* p;
  float* g;
  float* m;
  float* v;
  int64_t n;
  float lr, beta1, beta2, eps;
  int32_t* step2;
  float* scales;
} pnr_adam_tail;
size_t pnr_step_tail_floats(void);
int pnr_map_step_adam(const pnr_render_params* prm, const float* packed, const float* rays_o, const float* rays_d,
                      const float* gt_depth, const float* gt_color, const float* t_rand, int64_t n, float w_color,
                      float w_reg, double* loss, float* const* grads, void* workspace, size_t ws_bytes, void* bwd_ws,
                      size_t bwd_bytes, void* loss_ws, const pnr_adam_tail* tail, int32_t* fused, void* stream);
/* pnr_mlp_pack2(PNR_PACK_F16X3_ONLY) with the scales given (scales[0..5) and their inverses
 * [5..10), device floats, e.g. pnr_map_step_adam's): the images' launch alone, which also copies the
 * ten floats into the image's raw table.  Bit for bit the full pack when the scales are the tensors'. */
int pnr_mlp_pack_scaled(const float* const* params, float* packed, const float* scales, void* stream);
/* pnr_window_sample and pnr_mlp_pack_scaled as ONE launch (blocks of either kind: the two do not depend
 * on each other, and each sat at the launch-latency floor).  Same outputs as the two calls. */
int pnr_window_sample_pack(uint64_t seed, void* state, int64_t n, int64_t n_per_frame, int32_t H, int32_t W, float fx,
                           float fy, float cx, float cy, const float* c2w, const float* depth, const float* color,
                           int32_t n_samples, float* rays_o, float* rays_d, float* gt_depth, float* gt_color,
                           float* t_rand, int64_t* idx, float* far_clamp, const float* const* params, float* packed,
                           const float* scales, void* stream);

/* ---- bundle adjustment (src/Mapper.py:460-500, 542-543, 567-581, 675-692; additions to ABI 14) ----
 * With mapping.BA the Mapper's loss also reaches the camera tensors of the window's keyframes, through
 * rays_o, rays_d and |rays_d|.  The map pass in its ray-gradient form: the delta chain also emits dL/dx
 * per sample, the gather backward (neural points) adds its dL/dp into the same buffer, and ONE more
 * launch (k_map_ray_grads) sums per ray, over its regulation, coarse and importance rows,
 *   dL/drays_o = sum g_x,   dL/drays_d = sum g_x z + g_nrm d / |d|       (float64 sums, a fixed order)
 * with the regulation's float32 z (Renderer.py:284-294, recomputed from gt_depth, t_vals and t_rand),
 * the render's saved float64 z, and no gradient through the importance z (detached, Renderer.py:190)
 * or near / far.  g_rays_o, g_rays_d: (n,3) float32, written.  Everything else -- the decoder / fc_c /
 * feature gradients, the loss, the fused tail -- is bit for bit that of the form without ray gradients.
 * pnr_map_bwd_rays = pnr_map_bwd (+ gt_depth, t_rand of the forward); pnr_map_step_rays = pnr_map_step
 * (tail NULL; fused may be NULL) or pnr_map_step_adam (tail given).  n = 0: as those calls, the ray
 * gradients (no rows) untouched. */
int pnr_map_bwd_rays(const pnr_render_params* prm, const float* packed, const float* rays_d, const float* gt_depth,
                     const float* t_rand, int64_t n, const double* g_depth, const float* g_rgb, const float* g_sigma,
                     float* const* grads, float* g_rays_o, float* g_rays_d, void* workspace, size_t ws_bytes,
                     void* bwd_ws, size_t bwd_bytes, void* stream);
int pnr_map_step_rays(const pnr_render_params* prm, const float* packed, const float* rays_o, const float* rays_d,
                      const float* gt_depth, const float* gt_color, const float* t_rand, int64_t n, float w_color,
                      float w_reg, double* loss, float* const* grads, void* workspace, size_t ws_bytes, void* bwd_ws,
                      size_t bwd_bytes, void* loss_ws, const pnr_adam_tail* tail, int32_t* fused, float* g_rays_o,
                      float* g_rays_d, void* stream);

/* The pose gradient, the camera Adam step and the pose table in ONE launch.  The n = n_frames *
 * n_per_frame rays are those of pnr_window_rays: frame f's rays at [f n_per_frame, (f+1) n_per_frame),
 * pixel idx[r] (int64, row-major in the H x W image, clamped as there).  Per frame
 *   dL/dt = sum g_rays_o,   dL/dR[i][j] = sum g_rays_d[i] dir[j],   dir = ((i-cx)/fx, -(j-cy)/fy, -1)
 * (the adjoint of get_rays_from_uv, src/common.py:74-89; dir in float32 as the forward forms it, the
 * sums in float64), chained through quad2rotation (src/common.py:137-160: R = I + two_s A(q) with
 * two_s = 2 / sum q^2, so a non-unit quaternion's normalisation term is part of the gradient) into
 *   g_cam (F,7) float32: dL/d(qw, qx, qy, qz, tx, ty, tz), written; a fixed frame's row is zero.
 * adam = 1: every frame with fixed[f] == 0 then takes torch.optim.Adam's step (lr, beta1, beta2, eps;
 * moments m, v (F,7); step number *step + 1, *step a device int32 of completed steps that this launch
 * advances by one) on its row of cam (F,7), and its c2w (F,4,4) row is rewritten from the stepped
 * tensor (get_camera_from_tensor, bottom row 0 0 0 1).  A fixed frame's cam, m, v and c2w rows are
 * not written at all.  adam = 0: gradients only (cam is read; m, v, step, c2w may be NULL).
 * fixed: (F) bytes, or NULL = no frame fixed.  workspace: pnr_pose_step_workspace_bytes(n_frames,
 * n_per_frame) bytes, 8-byte aligned, ZERO-FILLED before its first use (a ticket word; each call leaves
 * it zero) and not shared by concurrent calls.  Deterministic: float64 block partials in a fixed order,
 * added by the block that takes the last ticket in block order; no floating-point atomics.
 * n_frames = 0 or n_per_frame = 0: a no-op that leaves the poses (and g_cam) untouched. */
size_t pnr_pose_step_workspace_bytes(int64_t n_frames, int64_t n_per_frame);
int pnr_pose_step(const float* g_rays_o, const float* g_rays_d, const int64_t* idx, int64_t n_frames,
                  int64_t n_per_frame, int32_t H, int32_t W, float fx, float fy, float cx, float cy, float* cam,
                  const uint8_t* fixed, float* m, float* v, float lr, float beta1, float beta2, float eps,
                  int32_t* step, int32_t adam, float* c2w, float* g_cam, void* workspace, size_t ws_bytes,
                  void* stream);

/* ---- mesh extraction (src/utils/Mesher.py:349-574; additions to ABI 14) -------------------------
 * Mesher.point_masks (:53-212) for one chunk of P float32 points (the caller splits by
 * points_batch_size as the reference does: PNR_MASK_DEPTH_TEST's max_depth is a maximum over the
 * points of ONE call).  w2c (K,4,4) float32 row-major = the host inverse of each keyframe's c2w.
 *   PNR_MASK_POSES      get_mask_use_all_frames: frustum tests only (depth, max_depth NULL)
 *   PNR_MASK_MAX_DEPTH  depth_test=False: both masks also need -cam.z < max_depth[k], a device
 *                       float32 (K) the caller fills with 1.1 * max(depth_k)
 *   PNR_MASK_DEPTH_TEST depth_test=True: depth (K,H,W) float32 is sampled at uv (F.grid_sample,
 *                       bilinear, align_corners=True, zero padding); forecast needs -cam.z < the
 *                       maximum sample of the call, seen needs |-cam.z - sample| < 2.4
 * seen / forecast: P bytes each (0 / 1), forecast already without the seen points.  ws:
 * pnr_point_masks_workspace_bytes(P, K, mode) bytes (0 for the first two modes).  Deterministic. */
enum { PNR_MASK_POSES = 0, PNR_MASK_MAX_DEPTH = 1, PNR_MASK_DEPTH_TEST = 2 };
size_t pnr_point_masks_workspace_bytes(int64_t P, int32_t K, int32_t mode);
int pnr_point_masks(const float* points, int64_t P, const float* w2c, int32_t K, int32_t H, int32_t W, float fx,
                    float fy, float cx, float cy, int32_t mode, const float* depth, const float* max_depth,
                    uint8_t* seen, uint8_t* forecast, void* ws, size_t ws_bytes, void* stream);

/* Marching cubes over a float32 volume of nx x ny x nz samples; sample (ix,iy,iz) is
 * vol[ix*sx + iy*sy + iz*sz] (element strides, so the Mesher's (iy*nx + ix)*nz + iz grid order needs no
 * transposed copy).  A corner is "below" when sample < level; an edge with exactly one below corner
 * carries one vertex at origin + (i + t) * spacing, t = (level - a) / (b - a) in float64.  Each vertex
 * is shared by the faces around it; vertices are ordered by owning grid point ((ix*ny + iy)*nz + iz,
 * then x, y, z edge), faces by cell and case-table order; the winding is skimage's default.  No atomic
 * decides a position: equal volumes give equal bits.  Two calls with the same arguments and workspace:
 *   pnr_marching_cubes_count  fills ws and writes the vertex / face counts to two device int64
 *   pnr_marching_cubes_emit   writes vertices (n_vertices,3) float64 and faces (n_faces,3) int32
 * (the caller reads the counts and allocates in between; a volume without a crossing gives 0, 0).
 * origin, spacing: HOST double[3].  nx*ny*nz <= pnr_marching_cubes_max_points(). */
size_t pnr_marching_cubes_workspace_bytes(int64_t nx, int64_t ny, int64_t nz);
int64_t pnr_marching_cubes_max_points(void);
int pnr_marching_cubes_count(const float* vol, int64_t nx, int64_t ny, int64_t nz, int64_t sx, int64_t sy,
                             int64_t sz, double level, void* ws, size_t ws_bytes, int64_t* n_vertices,
                             int64_t* n_faces, void* stream);
int pnr_marching_cubes_emit(const float* vol, int64_t nx, int64_t ny, int64_t nz, int64_t sx, int64_t sy,
                            int64_t sz, double level, const double* origin, const double* spacing, const void* ws,
                            size_t ws_bytes, double* vertices, int32_t* faces, void* stream);

/* ---- mesh bound from the keyframes (src/utils/Mesher.py:214-279, applied at :426-433 / :475-485;
 * additions to ABI 14) --------------------------------------------------------------------------
 * The reference bounds the mesh by the convex hull of a TSDF surface fused from the keyframes' depth
 * (Mesher.py:214-279).  Here the hull is taken over the point set P itself, and the device supplies
 * the three passes over P or over the grid; the combinatorics run on the host (pnr/bound.py).
 * P, with its index space:
 *   depth pixels   keyframe k < K, pixel (v, u) of the `stride` lattice (v, u multiples of stride), depth
 *                  d finite, 0 < d <= depth_trunc (Mesher.py:253's depth_trunc): index k H W + v W + u,
 *                  position pnr_points_add_frame's with rho = 0 (the same device function): the float32
 *                  ray of pnr_get_rays, p = rays_o + rays_d d, unfused
 *   extra points   n_extra float32 rows (the camera centres c2w[:3,3], Mesher.py:262-267): index
 *                  K H W + e; a row with a NaN coordinate is invalid
 * K H W + n_extra < 2^31. */
typedef struct pnr_bound_frames {
  const float* depth;      /* (K,H,W) float32, device                                          */
  const float* c2w;        /* (K,4,4) float32 row-major, device                                */
  int32_t K, H, W, stride; /* K >= 0, stride >= 1                                              */
  float fx, fy, cx, cy, depth_trunc;
  const float* extra_xyz;  /* (n_extra,3) float32, device; NULL when n_extra == 0              */
  int64_t n_extra;
} pnr_bound_frames;
/* The support function of P (the pass quickhull makes per round, Mesher.py:270's hull): for each of the
 * D <= pnr_bound_support_max_dirs() float32 directions n, h = max over the valid points of
 * (x nx + y ny) + z nz in unfused float32 (a NaN product never wins) and arg = the smallest index that
 * attains it; no valid point: h = -inf, arg = -1, and the call still returns 0.  Max and min-index
 * commute, so the result depends on nothing but the arguments: persistent workgroups write per-workgroup
 * (value, index) rows with plain stores and one fixed-order launch reduces them; no float atomics.
 * ws: pnr_bound_support_workspace_bytes(frames, D) bytes (0 for bad arguments). */
int32_t pnr_bound_support_max_dirs(void);
size_t pnr_bound_support_workspace_bytes(const pnr_bound_frames* frames, int32_t n_dirs);
int pnr_bound_support(const pnr_bound_frames* frames, const float* dirs, int32_t D, float* h, int64_t* arg,
                      void* ws, size_t ws_bytes, void* stream);
/* Positions (n,3) float32 of the points of P with the given indices (the hull's vertices, Mesher.py:270);
 * an index outside [0, K H W + n_extra), off the lattice or of an invalid point gives a NaN row. */
int pnr_bound_points(const pnr_bound_frames* frames, const int64_t* idx, int64_t n, float* xyz, void* stream);
/* The hull mask of Mesher.py:426 (`mesh_bound.contains`): inside[i] = 1 when (x a + y b) + z c <= d in
 * unfused float64 for every plane (a, b, c, d) of `planes` (F,4) float64 (float32 points are widened
 * first), else 0; F = 0 gives all ones. */
int pnr_bound_contains_f32(const float* p, int64_t P, const double* planes, int32_t F, uint8_t* inside,
                           void* stream);
int pnr_bound_contains_f64(const double* p, int64_t P, const double* planes, int32_t F, uint8_t* inside,
                           void* stream);

/* ---- block-sparse TSDF volume fused from keyframe depth (src/utils/Mesher.py:231-266: open3d's
 * ScalableTSDFVolume.integrate per keyframe; additions to ABI 14) -----------------------------------
 * Geometry.  Blocks of 16^3 voxels of edge voxel_length; block_length = 16 voxel_length.  A dense int32
 * directory of dims[0] x dims[1] x dims[2] entries, entry index e = (bz dims[1] + by) dims[0] + bx, covers
 * the box that starts at `origin`; it replaces open3d's unbounded hash, and surface outside it is dropped.
 * Global voxel g_a = 16 b_a + i_a has its centre at X_a = origin_a + ((float)g_a + 0.5f) voxel_length
 * (open3d's convention); voxel (i, j, k) of a block has voxel index (k 16 + j) 16 + i.  An entry >= 0 is the
 * block's slot; a negative entry means no block (-1: dropped for want of a slot, INT32_MIN: never touched).
 * `directory` holds pnr_tsdf_directory_bytes() bytes: int32 n_blocks, int32 dropped_blocks, padding to 256
 * bytes, then the entries.  The slot arrays are the caller's, structure of arrays, max_blocks slots: tsdf
 * and weight (max_blocks, 4096), rgb (max_blocks, 3, 4096), block_index (max_blocks) = the slot's entry
 * index.  Rows at or above n_blocks are never read, so the arrays need no clearing.
 * Required: 0 < sdf_trunc < block_length, fx, fy > 0, 1 <= max_blocks <= 2^17, dims >= 1 with a product
 * <= 2^27, every pointer but rgb non-null (rgb NULL: no colour is kept).  All arithmetic is unfused float32.
 *
 * pnr_tsdf_integrate fuses K frames, depth (K,H,W), colour (K,H,W,3) or NULL, c2w (K,4,4), in call order:
 *   valid depth   d finite and 0 < d <= depth_trunc.
 *   allocate      for every valid pixel of frame k: p = rays_o + rays_d d on pnr_get_rays' float32 ray (the
 *                 device function of pnr_points_add_frame / pnr_bound_frames); a non-finite p is skipped.
 *                 Per axis the blocks floorf(((p_a - sdf_trunc) - origin_a) / block_length) ..
 *                 floorf(((p_a + sdf_trunc) - origin_a) / block_length), clipped to the directory (open3d's
 *                 touch rule: at most 8 blocks when 2 sdf_trunc <= block_length, 27 otherwise).  A touched
 *                 entry without a block is born at the first frame k that touches it.  The new blocks take
 *                 the slots after the existing ones in ascending entry index; those past max_blocks are
 *                 dropped in that order, become -1 for good, and are counted once in dropped_blocks.  The
 *                 call still returns 0.  No host read; the assignment depends on the arguments alone.
 *   integrate     every block, for the frames k at or after its birth (a block that existed before the
 *                 call: all K), every voxel, with R = c2w[:3,:3], t = c2w[:3,3], q = X - t:
 *                   P_c = (R[0][c] q_0 + R[1][c] q_1) + R[2][c] q_2      (camera looks down -z, y up)
 *                   zc = -P_2;                                           skip unless zc > 0
 *                   uf = ((fx P_0) / zc + cx) + 0.5f, vf = ((-(fy P_1)) / zc + cy) + 0.5f
 *                   u = floorf(uf), v = floorf(vf);                      skip unless 0 <= uf < W, 0 <= vf < H
 *                   d = depth[k][v][u];                                  skip unless valid
 *                   a = (u - cx) / fx, b = (v - cy) / fy, m = sqrtf((a a + b b) + 1)
 *                   sdf = (d - zc) m;                                    skip if sdf <= -sdf_trunc
 *                   s = fminf(1, sdf / sdf_trunc), w1 = w + 1
 *                   tsdf = (tsdf w + s) / w1, rgb_c = (rgb_c w + colour[k][v][u][c]) / w1, w = w1
 *                 (open3d's IntegrateWithDepthToCameraDistanceMultiplier as recalled; THIS statement is the
 *                 contract).  So the volume depends on the sequence of frames alone, not on how calls
 *                 batch them; only the slot order does.  A block is read once and written once per 64
 *                 frames of a call; a conservative per-block frustum test skips frames that cannot reach
 *                 the block and never changes a result.
 * pnr_tsdf_extract_count / _emit give the zero crossings between neighbouring voxels: for every voxel of
 * every block with w > 0 and each of its +x, +y, +z neighbours (axis a = 0, 1, 2; found through the directory
 * when it lies in the next block, skipped when that block is absent) with w > 0, a point when tsdf0 and
 * tsdf1 have strictly opposite signs (tsdf0 tsdf1 < 0):
 *   s = tsdf0 / (tsdf0 - tsdf1);  xyz = X0, xyz_a = X0_a + voxel_length s;  rgb_c = rgb0_c + (rgb1_c - rgb0_c) s
 * in order of (slot, voxel index, axis): equal arguments give equal bits.  _count writes the number of
 * points to *n_points (device) and leaves the offsets in the workspace for _emit; xyz, rgb (n_points,3)
 * float32, rgb may be NULL (and must be when the volume keeps no colour).
 * ws: pnr_tsdf_workspace_bytes() bytes (0 for bad arguments), 4-byte aligned, any contents.  Bad arguments:
 * PNR_E_ARG; a short workspace: PNR_E_WORKSPACE; nothing is launched.
 *
 * pnr_tsdf_mesh_count / _emit give the volume's coloured triangle mesh: marching cubes at level 0, slot by
 * slot over the blocks, neighbour blocks found through the directory.
 *   corner     a voxel of a live block (entry >= 0) with w > 0 is valid; its sample is its tsdf, and it is
 *              below when tsdf < 0 (pnr_marching_cubes' rule with level 0).
 *   cell       belongs to the voxel (i, j, k) of slot s at its lowest corner; the other seven corners are at
 *              +1 along the axes, in the same block or in one of the seven +x/+y/+z neighbour blocks.  A cell
 *              is valid when all eight corners are: a cell that touches an absent or dropped block, the edge of
 *              the directory or a w == 0 voxel emits nothing (open3d's rule).  Case index and triangles are
 *              pnr_marching_cubes' (corner c = (c & 1, c >> 1 & 1, c >> 2) sets bit c; the same edge numbers).
 *   vertex     an edge belongs to the voxel at its lower end and has an axis a.  It carries a vertex when
 *              exactly one end is below and at least one of the up to four cells around it is valid, so every
 *              vertex is referenced.  s = tsdf0 / (tsdf0 - tsdf1), xyz = X0, xyz_a = X0_a + voxel_length s,
 *              rgb_c = rgb0_c + (rgb1_c - rgb0_c) s in unfused float32: a vertex whose edge has
 *              tsdf0 tsdf1 < 0 is bit for bit a point of pnr_tsdf_extract_emit.  The faces around a vertex
 *              share it, across block faces too.
 *   order      vertices by (slot, voxel index, axis), faces by (slot, voxel index of the cell, case-table
 *              order).  No atomic decides a position: equal volumes give equal bits.
 *   winding    the table's, unchanged: with below = tsdf < 0 the normal (v1 - v0) x (v2 - v0) points towards
 *              positive tsdf, the free space in front of the surface.
 * _count writes V and F to *n_vertices, *n_faces (device) and leaves in the workspace what _emit needs; xyz,
 * rgb (V,3) float32, rgb may be NULL (and must be when the volume keeps no colour), faces (F,3) int32.
 * V, F < 2^31: a volume whose max_blocks 4096 5 faces would not fit (max_blocks > 104,857) has a workspace
 * size of 0 and is refused with PNR_E_ARG by both calls, since the counts are known on the device only.
 * ws: pnr_tsdf_mesh_workspace_bytes() bytes, 8-byte aligned, any contents before _count.  After it: int32
 * vertex and face totals per slot (2 max_blocks), their exclusive scans (2 (max_blocks + 1)), the scan's
 * scratch, and per slot 256 uint64 rank rows, row (k, j): bits 0-15, 16-31, 32-47 mark the voxels i whose
 * x, y, z edge carries a vertex, bits 48-63 count the slot's vertices before the row.  A vertex index is the
 * owning slot's scanned offset + the row's count + the marks before (i, a) in (voxel, axis) order.
 * Bad arguments: PNR_E_ARG; a short workspace: PNR_E_WORKSPACE; nothing is launched. */
typedef struct pnr_tsdf {
  float origin[3];
  float voxel_length, sdf_trunc, depth_trunc;
  int32_t dims[3];      /* directory entries per axis                                          */
  int32_t max_blocks;
  int32_t H, W;
  float fx, fy, cx, cy;
  int32_t* directory;   /* pnr_tsdf_directory_bytes                                            */
  float* tsdf;          /* (max_blocks, 4096)                                                  */
  float* weight;        /* (max_blocks, 4096)                                                  */
  float* rgb;           /* (max_blocks, 3, 4096) or NULL                                       */
  int32_t* block_index; /* (max_blocks)                                                        */
} pnr_tsdf;
size_t pnr_tsdf_directory_bytes(const pnr_tsdf* vol);
size_t pnr_tsdf_workspace_bytes(const pnr_tsdf* vol);
/* Empties the volume: every entry INT32_MIN, both counters 0. */
int pnr_tsdf_reset(const pnr_tsdf* vol, void* stream);
int pnr_tsdf_integrate(const pnr_tsdf* vol, const float* depth, const float* color, const float* c2w, int32_t K,
                       void* ws, size_t ws_bytes, void* stream);
int pnr_tsdf_extract_count(const pnr_tsdf* vol, void* ws, size_t ws_bytes, int64_t* n_points, void* stream);
int pnr_tsdf_extract_emit(const pnr_tsdf* vol, const void* ws, size_t ws_bytes, float* xyz, float* rgb, void* stream);
size_t pnr_tsdf_mesh_workspace_bytes(const pnr_tsdf* vol);
int pnr_tsdf_mesh_count(const pnr_tsdf* vol, void* ws, size_t ws_bytes, int64_t* n_vertices, int64_t* n_faces,
                        void* stream);
int pnr_tsdf_mesh_emit(const pnr_tsdf* vol, const void* ws, size_t ws_bytes, float* xyz, float* rgb, int32_t* faces,
                       void* stream);

/* ---- two-way descriptor matching (src/Tracker.py:398-440, nn_match_two_way; additions to ABI 14) ----
 * desc1 (D,N), desc2 (D,M): float32 row-major with unit-norm columns (the reference's SuperPoint layout);
 * D a multiple of 32 in [32, 512], N, M <= 2^20.  dot = desc1^T desc2 on v_mfma_f32_32x32x2_f32 (each
 * element one fp32 fma chain in ascending k), clipped to [-1, 1]; per row i the column j* of the largest
 * dot and per column the row of the largest dot, the lowest index among bitwise-equal dots (np.argmin's
 * first occurrence on the distance).  Row i is kept when score = sqrtf(2 - 2 dot[i][j*]) < nn_thresh and
 * column j* chose row i.  The L kept rows are written in ascending i: idx1[0..L) = i, idx2[0..L) = j*
 * (int32), score[0..L) (float32), *count = L (int32); idx1, idx2, score hold N elements, of which the
 * call writes the first L only.  N = 0 or M = 0: *count = 0.  The N x M product never reaches memory, and
 * equal arguments give equal bits (integer atomics only).  Non-finite descriptors are the caller's error
 * (a NaN dot counts as -1).
 * workspace: pnr_match_workspace_bytes(N, M) bytes (0 for sizes the call refuses), 8-byte aligned, any
 * contents.  After the call it holds uint64 row_key[N] then col_key[M]:
 *   key = u << 32 | (0xFFFFFFFF - index of the best partner)
 *   u   = the dot's float32 bits b mapped monotonically: b | 0x80000000 for b >= 0, ~b for a negative dot
 * so a caller can read every row's nearest column, kept or not.
 * D unsupported, nn_thresh negative or NaN, a size out of range, a null pointer: PNR_E_ARG; a short
 * workspace: PNR_E_WORKSPACE; nothing is launched. */
size_t pnr_match_workspace_bytes(int64_t N, int64_t M);
int pnr_match_two_way(const float* desc1, const float* desc2, int32_t D, int64_t N, int64_t M, float nn_thresh,
                      int32_t* idx1, int32_t* idx2, float* score, int32_t* count, void* workspace,
                      size_t workspace_bytes, void* stream);

/* ---- SuperPoint on the device (src/demo_superpoint.py:78-293; additions to ABI 14) --------------------
 * One convolution layer of the network: x (Cin,H,W) -> out, float32 planar, batch 1, stride 1, ksize 3 with
 * zero padding 1 or ksize 1.  Cin in {1, 64, 128, 256}, Cout in {64, 128, 256, 65}; Cin = 1 is served for
 * ksize 3 with NONE / RELU only.  H, W > 0 need no alignment.
 *   w_packed  [ksize^2][Cin][cout_pad] float32, cout_pad = Cout rounded up to a multiple of 64 and the padding
 *             zero: w_packed[ky ksize + kx][ci][co] = conv.weight[co][ci][ky][kx]; 16-byte aligned
 *   bias      [Cout]
 * Arithmetic: v_mfma_f32_32x32x2_f32 (Cin = 1: fmaf).  Every output is one fp32 chain formed by one wave:
 * acc = bias, then cin chunks ascending (8 channels for ksize 3, 16 for ksize 1), inside a chunk the taps
 * ascending (ky major), inside a tap the cin pairs ascending; Cin = 1: bias, then the 9 taps ascending.  A
 * pixel outside the image contributes 0.  Equal arguments give equal bits; every output element is written.
 * Epilogues:
 *   NONE             out (Cout,H,W) = the chain
 *   RELU             out (Cout,H,W) = max(chain, 0)
 *   RELU_POOL2       out (Cout,H/2,W/2) = 2 x 2 / stride 2 max of the RELU output; H and W even
 *   SOFTMAX_HEATMAP  Cout = 65, ksize 1: out (65,H,W) = the chain (bitwise NONE's), and
 *                    heat[8 y + (c >> 3)][8 x + (c & 7)] = expf(out[c][y][x]) / (sum over the 65 channels of
 *                    expf(out[.][y][x]) + 1e-5f) for c < 64 into heat (8 H, 8 W); no maximum is subtracted
 *                    (demo_superpoint.py:248-258 as it stands)
 *   L2NORM           Cout = 256, ksize 1: out (256,H,W) = chain / sqrtf(sum over the 256 channels of chain^2)
 * heat is read by SOFTMAX_HEATMAP only.  Anything else, a null pointer, or a tensor of 2^31 elements or
 * more: PNR_E_ARG, nothing is launched. */
typedef enum pnr_conv_epilogue {
  PNR_CONV_NONE = 0,
  PNR_CONV_RELU = 1,
  PNR_CONV_RELU_POOL2 = 2,
  PNR_CONV_SOFTMAX_HEATMAP = 3,
  PNR_CONV_L2NORM = 4
} pnr_conv_epilogue;
int pnr_conv2d_fwd(const float* x, const float* w_packed, const float* bias, float* out, float* heat, int32_t Cin,
                   int32_t Cout, int32_t H, int32_t W, int32_t ksize, int32_t epilogue, void* stream);
/* Keypoints of a heatmap (H,W) float32, H and W positive multiples of 8, H W < 2^28 (demo_superpoint.py:158-275).
 * Candidates: heat >= conf_thresh (conf_thresh > 0).  Candidate p = y W + x ranks above q when heat[p] >
 * heat[q], or they are equal and p < q.  Greedy NMS in that order: a candidate not yet suppressed is kept and
 * suppresses every candidate at Chebyshev distance <= nms_dist (0 <= nms_dist <= 64).  Then kept points with
 * x < border, x >= W - border, y < border or y >= H - border are dropped.  The result does not depend on
 * scheduling (a fixed point whose decisions are final; csrc/keypoints.hip).
 * workspace: pnr_superpoint_workspace_bytes(H, W) bytes (0 for sizes the call refuses), 8-byte aligned, any
 * contents.  After the call it holds int32 count at byte 0 and, from byte 64, `count` uint64 keys in no
 * particular order:  key = heat bits << 32 | (0xFFFFFFFF - p).  Sorted descending they are the reference's
 * output order (confidence descending; ties, which numpy leaves to an unstable sort, by ascending p).
 * Bad arguments: PNR_E_ARG; a short workspace: PNR_E_WORKSPACE; nothing is launched. */
size_t pnr_superpoint_workspace_bytes(int32_t H, int32_t W);
int pnr_superpoint_keypoints(const float* heat, int32_t H, int32_t W, float conf_thresh, int32_t nms_dist,
                             int32_t border, void* workspace, size_t workspace_bytes, void* stream);
/* Descriptors of N keypoints (demo_superpoint.py:277-292): pts (3,N) float32 rows x, y, confidence in pixels
 * of the full image; coarse (256,Hc,Wc) the L2NORM output.  desc (256,N) float32: the bilinear sample of
 * coarse at (x / 8 - 0.5, y / 8 - 0.5) with zeros outside (grid_sample, align_corners = False), divided by
 * its Euclidean norm -- the layout pnr_match_two_way takes.  N = 0 launches nothing. */
int pnr_superpoint_sample_desc(const float* coarse, int32_t Hc, int32_t Wc, const float* pts, int64_t N, float* desc,
                               void* stream);

/* ---- relative pose from matches (src/Tracker.py:356-360 estimatePose, :458-610; additions to ABI 14) ----
 * All float64.  x1, x2: (L,2) normalised image coordinates of the matches in the first and the second view
 * (cv2.findEssentialMat's points1, points2: x2^T E x1 = 0); 5 <= L <= 2^20, 1 <= S <= 2^16 samples.
 * The draw.  Sample s takes 5 distinct match indices: draw d = 0..4 tries retry = 0, 1, ...
 *   z = (seed << 32 | s) * 0x9E3779B97F4A7C15 + (d << 32 | retry) * 0xD1B54A32D192ED03        (mod 2^64)
 *   z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9;  z = (z ^ z >> 27) * 0x94D049BB133111EB;  z ^= z >> 31
 *   index = ((z >> 32) * L) >> 32
 * and keeps the first index that differs from the draws before it; after 64 refusals it walks index + 1
 * (mod L) instead.  The draws depend on (seed, s, L) alone, not on the launch.
 * The solver (Nister's five-point method) gives sample s up to 10 essential matrices, unit Frobenius norm,
 * at hypotheses 10 s + r in ascending order of the root z of the degree-10 polynomial; unused slots and
 * rank-deficient samples are flagged invalid and hold zeros.
 * Scoring.  err = (x2^T E x1)^2 / (a0^2 + a1^2 + b0^2 + b1^2), a = E x1, b = E^T x2 (cv2's Sampson error); a
 * match is an inlier when err <= threshold^2.  The best hypothesis has the most inliers, the lowest index
 * among equal counts: equal arguments give equal bits.
 * pose (37): E (9) | R (9) | t (3) | Trc (16), row-major, x2 ~ R x1 + t, Trc = [R t; 0 1].  R, t: E = U diag V^T
 * by one-sided Jacobi, R1 = U W V^T, R2 = U W^T V^T (determinants +1), t = +-u3; the inliers are triangulated
 * under (R1,t), (R2,t), (R1,-t), (R2,-t) and the first candidate with the most points of depth in (0, 50) in
 * both views wins (cv2.recoverPose).  mask (L) uint8 and *count: the inliers of E, from a plain float64
 * evaluation.  No valid hypothesis: count 0, mask 0, E = 0, R = I, t = 0.
 * workspace: pnr_relpose_workspace_bytes(L, S) bytes (0 for sizes the call refuses), 8-byte aligned, any
 * contents.  After the call: uint64 best key = count << 32 | (0xFFFFFFFF - hypothesis) at byte 0 (0: none);
 * from byte 64 the candidates (10 S, 9) float64; then the samples (S,5) int32 (rounded up to 8 bytes); then
 * valid (10 S) uint8.
 * A size out of range, a negative or NaN threshold, a null pointer: PNR_E_ARG; a short workspace:
 * PNR_E_WORKSPACE; nothing is launched. */
size_t pnr_relpose_workspace_bytes(int64_t L, int64_t S);
int pnr_relpose_estimate(const double* x1, const double* x2, int64_t L, int64_t S, uint32_t seed, double threshold,
                         double* pose, uint8_t* mask, int32_t* count, void* workspace, size_t workspace_bytes,
                         void* stream);
/* The solver alone: x1, x2 (S,5,2) -> E (S,10,9), valid (S,10) as above.  0 <= S <= 2^16. */
int pnr_fivept_solve(const double* x1, const double* x2, int64_t S, double* E, uint8_t* valid, void* stream);
/* DLT triangulation (src/utils/utils_geom.py:140-207).  Tcw_1, Tcw_2: (4,4) row-major world-to-camera poses;
 * kpn_1, kpn_2: (L,2) normalised keypoints.  Per match the rows x P[2] - P[0], y P[2] - P[1] of both views
 * form A (4,4); X is its right singular vector of the smallest singular value by one-sided Jacobi on A;
 * pts3d (L,3) = X[:3] / X[3], good (L) uint8 = X[3] != 0.  With K (3,3) not null also, per view, q = K (Rcw p +
 * tcw): uv (L,2) = q[:2] / q[2] and z (L) = q[2] (src/camera.py:62-68).  L = 0 launches nothing. */
int pnr_triangulate(const double* Tcw_1, const double* Tcw_2, const double* kpn_1, const double* kpn_2, int64_t L,
                    const double* K, double* pts3d, uint8_t* good, double* uv1, double* z1, double* uv2, double* z2,
                    void* stream);
/* The pseudo-depth map (Tracker.py:571-610).  uv (n,2) float64 pixels (u column, v row), depth (n) float64,
 * out (H,W) float32.  Background 0.  Point i paints rows [int(v - patch), int(v + patch)) x columns
 * [int(u - patch), int(u + patch)) when patch < v < H - patch and patch < u < W - patch, else the pixel
 * (int(v), int(u)) when 0 < v < H and 0 < u < W; a pixel painted more than once keeps the highest i.
 * workspace: pnr_paint_depth_workspace_bytes(H, W) = 4 H W bytes (0 when H W >= 2^30 or a side < 1), 4-byte
 * aligned, any contents.  Deviations from the reference: it pairs every coordinate with every depth (each
 * patch ends with the last depth), compares u with H, and fills the background with rand / 10000. */
size_t pnr_paint_depth_workspace_bytes(int32_t H, int32_t W);
int pnr_paint_depth(const double* uv, const double* depth, int64_t n, int32_t H, int32_t W, int32_t patch, float* out,
                    void* workspace, size_t workspace_bytes, void* stream);

/* ---- reconstruction metrics (src/tools/eval_recon.py calc_3d_metric; additions to ABI 14) ------------------
 * All float64; point sets are (n,3) row-major.  Sizes up to 2^28 points.
 *
 * Exact nearest neighbour by brute force over all Q R pairs on the float64 MFMA.  dist (Q) and idx (Q) int64:
 *  - dist[i] is the float64 distance |query[i] - ref[idx[i]]| from coordinate differences,
 *    sqrt((dx dx + dy dy) + dz dz) with every operation rounded once: exact to rounding.
 *  - idx[i] is chosen by the expansion d^2 = |a|^2 + (|b|^2 - 2 a.b) over the clouds centred on the query's
 *    bounding-box centre, compared on its leading 28 mantissa bits, ties to the lower index.  Its squared
 *    distance is at most d^2_min (1 + 2^-27) + 2 E with E = 16 * 2^-53 * max (|a| + |b|)^2 over the centred
 *    clouds, the rounding bound of the four-term expansion.  Wherever the runner-up is farther than that,
 *    idx[i] is the argmin.
 *  - With max_dist finite, a query whose chosen point is farther than max_dist (dist <= max_dist keeps it) gets
 *    idx -1 and dist +inf.  Pass +inf for no limit; a negative or NaN max_dist is PNR_E_ARG.
 *  - Equal arguments give equal bits, whatever the slice count.  slices = 0 lets the call split the ref columns
 *    over workgroups as it sees fit (small Q still fills the chip); 1 <= slices <= min(chunks of 512 ref
 *    points, max(automatic count, 4)) forces a count (larger: PNR_E_ARG).
 *  - Q = 0 or R = 0 launches nothing and writes nothing.  Non-finite coordinates are the caller's fault: the
 *    outputs are then unspecified, but every access stays in bounds.
 * workspace: pnr_nn_workspace_bytes(Q, R) bytes (0 for sizes the call refuses), 16-byte aligned, any contents. */
size_t pnr_nn_workspace_bytes(int64_t Q, int64_t R);
int pnr_nn_search(const double* query, int64_t Q, const double* ref, int64_t R, double max_dist, int32_t slices,
                  double* dist, int64_t* idx, void* workspace, size_t workspace_bytes, void* stream);
/* Surface sampling by trimesh.sample.sample_surface's rule.  verts (V,3), faces (F,3) int64.
 * pnr_face_areas: area (F) = half the cross-product norm; a face with an index outside [0, V) has area 0.
 * pnr_sample_surface: cum_area (F) is the inclusive prefix sum of the areas (the caller's scan).  Sample i
 * takes uniforms (u0, u1, u2) in [0, 1): row i of `uniforms` (count,3) when it is given, else
 *   base = mix(seed * 0x9E3779B97F4A7C15), u_k = (mix(base + (3 i + k) * 0xD1B54A32D192ED03) >> 11) * 2^-53
 * with mix the splitmix64 finaliser (as in pnr_relpose_estimate), so the samples depend on (seed, i) alone.
 * The face is the first with cum_area >= u0 * total and cum_area > 0 (never a zero-area face); (u1, u2) become
 * (1 - u1, 1 - u2) when u1 + u2 > 1; the point is ((v1 - v0) u1 + (v2 - v0) u2) + v0, unfused.  points
 * (count,3), face_idx (count) int64.  A total area that is zero or not finite gives NaN points and face -1.
 * The rule is trimesh's; its random stream is not reproduced (numpy's generator is not built). */
int pnr_face_areas(const double* verts, int64_t V, const int64_t* faces, int64_t F, double* area, void* stream);
int pnr_sample_surface(const double* verts, const int64_t* faces, const double* cum_area, int64_t F, int64_t count,
                       uint64_t seed, const double* uniforms, double* points, int64_t* face_idx, void* stream);
/* out[0] = the sum of dist (n), out[1] = the number of entries < dist_th, both summed in float64 in a fixed
 * order (per-block partials, then one block): equal arguments give equal bits.  1 <= n <= 2^28.
 * workspace: pnr_dist_stats_workspace_bytes() bytes, 8-byte aligned, any contents. */
size_t pnr_dist_stats_workspace_bytes(void);
int pnr_dist_stats(const double* dist, int64_t n, double dist_th, double* out, void* workspace, size_t workspace_bytes,
                   void* stream);
/* out (n,3) = R p + t for T = [R t; 0 1] (4,4) row-major on the device; out is a buffer of its own. */
int pnr_transform_points(const double* pts, int64_t n, const double* T, double* out, void* stream);
/* One step of point-to-point ICP (open3d registration_icp): src (N,3) is moved by T_in, every moved point
 * takes its nearest dst (M,3) point within `threshold` (pnr_nn_search with max_dist = threshold), and
 * stats (3) = fitness (matched / N), inlier RMSE (0 without a match), matched count describe T_in.
 * T_out = [R t; 0 1] T_in where (R, t) is the least-squares rigid motion of the matched pairs: Kabsch on the
 * cross-covariance about the centroids, sums in a fixed order, SVD by one-sided Jacobi, the weakest singular
 * pair replaced by cross products so that det R = +1 (the reflection fix).  No match: T_out = T_in.  T_in and
 * T_out are distinct (4,4) row-major device matrices.  The caller iterates and tests convergence.
 * workspace: pnr_icp_workspace_bytes(N, M) bytes (0 for sizes the call refuses), 16-byte aligned, any
 * contents; afterwards it starts with the moved points (N,3), then dist (N) and idx (N) int64 from byte
 * offsets round16(24 N) and round16(24 N) + round16(8 N). */
size_t pnr_icp_workspace_bytes(int64_t N, int64_t M);
int pnr_icp_step(const double* src, int64_t N, const double* dst, int64_t M, const double* T_in, double threshold,
                 double* T_out, double* stats, void* workspace, size_t workspace_bytes, void* stream);

/* ---- mesh depth rasteriser (src/tools/eval_recon.py calc_2d_metric, check_proj; src/tools/cull_mesh.py;
 * additions to ABI 14) ------------------------------------------------------------------------------------------
 * Depth images of a triangle mesh, float64 arithmetic, float32 images.  The rendering rule:
 *  - Camera.  c2w (n,4,4) row-major float64 = [R t] per view with OpenCV axes (x right, y down, z forward), what
 *    calc_2d_metric hands open3d as inv(extrinsic).  R is taken as orthonormal: a world point x has camera
 *    coordinates p = R^T (x - t), each component ((r0 d0 + r1 d1) + r2 d2) with d = x - t.  The last row is not read.
 *  - Projection.  p = (x, y, z) has homogeneous image coordinates q = (fx x + cx z, fy y + cy z, z).
 *  - Pixels.  The centre of pixel (row i, column j) is s = (j, i, 1): integer coordinates are pixel centres
 *    (cx = W / 2 - 0.5 centres the image).
 *  - Homogeneous edge functions (Olano-Greer): nothing is clipped at the near plane for coverage.  For a face
 *    with vertices 0, 1, 2 the edge opposite vertex k has E_k(s) = (q_i x q_j) . s with (i, j) = (k + 1, k + 2)
 *    mod 3, evaluated (n_x j + n_y i) + n_z, and det = q_0 . (q_1 x q_2) = (q0_x n_x + q0_y n_y) + q0_z n_z.  The
 *    pixel is covered iff det != 0 and E_k sign(det) >= 0 for k = 0, 1, 2; its depth is
 *    z = det / ((E_0 + E_1) + E_2); the sample is kept iff z_near <= z <= z_far.
 *  - Output.  depth[view][i][j] is the least kept z over all faces, rounded once to float32; 0 without one.
 *  - Two-sided: both orientations render (the reference's mesh_show_back_face = True).
 *  - A face with a vertex index outside [0, V) or with det = 0 contributes nothing.
 *  - Watertight.  An edge's cross product is formed with the lower vertex index first and negated if that
 *    swapped the operands, so the two faces of a shared edge see exactly negated edge values and no pixel centre
 *    falls between them; a centre exactly on the edge is covered by both, harmless under a minimum.
 *  - Reproducible.  A minimum: equal arguments give equal bits, whatever the view batch and the bin order.
 *  - Every operation is rounded once (no fused multiply-add).  Non-finite coordinates are the caller's fault:
 *    the image is then unspecified, but every access stays in bounds.
 * Deviations from open3d's OpenGL capture, stated: z_near is a parameter (calc_2d_metric's default here 0.01;
 * open3d derives its own from the scene) and must be > 0; z_far (finite, >= z_near) defaults to 20, the
 * reference's set_constant_z_far; the background is 0; no anti-aliasing and no top-left fill rule.
 *
 * Three calls render the n_views of a pnr_raster, with 32 x 32-pixel tiles, T = ceil(W / 32) ceil(H / 32):
 *   pnr_raster_count   counts (n_views T) int32 = per (view, tile) the faces whose conservative pixel box (of
 *                      the part with z >= z_near, widened by 2^-8 pixel, clamped to the image) overlaps the tile.
 *   (the caller)       ends (n_views T) int64 = the inclusive prefix sum of counts; pairs = its last entry.
 *   pnr_raster_fill    the face ids into the tile lists of the workspace (list order depends on scheduling).
 *   pnr_raster_tiles   depth (n_views, H, W) float32 from the lists; every pixel is written.
 * counts, ends and pairs of fill and tiles are those of the count call on the same pnr_raster; other values
 * leave the image unspecified and every access in bounds.  1 <= n_views <= 4096, 1 <= H, W <= 8192,
 * n_views T <= 2^24, V, F <= 2^28, pairs <= 2^30: otherwise PNR_E_ARG, and pnr_raster_counters and
 * pnr_raster_workspace_bytes return 0.  The caller batches the views to stay inside those bounds.
 * workspace: pnr_raster_workspace_bytes(r, pairs) bytes, 16-byte aligned, any contents before fill; tiles reads
 * what fill left. */
typedef struct pnr_raster {
  const double* verts; /* (V,3) */
  int64_t V;
  const int64_t* faces; /* (F,3) */
  int64_t F;
  const double* c2w; /* (n_views,4,4) */
  int32_t n_views, H, W, reserved;
  double fx, fy, cx, cy, z_near, z_far;
} pnr_raster;
int64_t pnr_raster_counters(const pnr_raster* r); /* n_views T */
size_t pnr_raster_workspace_bytes(const pnr_raster* r, int64_t pairs);
int pnr_raster_count(const pnr_raster* r, int32_t* counts, void* stream);
int pnr_raster_fill(const pnr_raster* r, const int32_t* counts, const int64_t* ends, int64_t pairs, void* workspace,
                    size_t workspace_bytes, void* stream);
int pnr_raster_tiles(const pnr_raster* r, const int32_t* counts, const int64_t* ends, int64_t pairs, float* depth,
                     const void* workspace, size_t workspace_bytes, void* stream);
/* out (n) float64 = per image the mean of |a - b| over its hw pixels: a, b (n, hw) float32, differences and sums
 * in float64 in a fixed order (per-block partials, then one block): equal arguments give equal bits.
 * 1 <= n <= 65535, 1 <= hw <= 2^26.  workspace: pnr_depth_l1_workspace_bytes(n) bytes, 8-byte aligned. */
size_t pnr_depth_l1_workspace_bytes(int64_t n);
int pnr_depth_l1(const float* a, const float* b, int64_t n, int64_t hw, double* out, void* workspace,
                 size_t workspace_bytes, void* stream);
/* check_proj's frustum test for every (point, view): with p and q as above, zz = z + 1e-5, the view sees the
 * point iff zz > 0, 0 < q_x / zz < W and 0 < q_y / zz < H.  view_any (n) uint8 = 1 where the view sees any of
 * the points (the view sampler's rejection), point_any (P) uint8 = 1 where any view sees the point
 * (cull_mesh.py), else 0; either may be null.  Float64 where the reference computes in float32, and OpenCV
 * poses where it flips an OpenGL pose: its guard is z - 1e-5 >= 0 on the same axis. */
int pnr_frustum_seen(const double* points, int64_t P, const double* c2w, int32_t n, int32_t H, int32_t W, double fx,
                     double fy, double cx, double cy, uint8_t* view_any, uint8_t* point_any, void* stream);

/* ---- diagnostics (not on the reference API) ----------------------------------------------- */
/* Kernel timing: while enabled, every launch of the timed kernels is bracketed by hipEvents on
 * its own stream.  pnr_timing_read synchronises those events and returns, for `kernel`
 *   0 = fused MLP forward (k_mlp_fwd / k_mlp_fwd16), units = points
 *   1 = MLP delta chain (k_mlp_bwd / k_mlp_bwd16), units = points
 *   2 = ray kernels, units = rays
 *   3 = weight-gradient GEMMs (k_wgrad / k_wgrad16 / k_wgrad_skinny, each with its fixed-order
 *       partial reduction k_part_reduce), units = points of the K dimension
 *   4 = neural-point gather (pnr_point_gather and the render's gathers: probe, group scan /
 *       scatter and search as one bracket), units = samples
 *   5 = neural-point gather backward (k_gather_bwd_probe + k_gather_bwd), units = samples
 *   6 = the grouped split weight-gradient launch (k_wgrad16_group: every f16x3 GEMM of a backward
 *       chunk but dWo / dB), units = multiply-adds / 65,536 (one 256 x 256 layer over one point = 1)
 *       -- kind 3 then holds the dWo / dB launches and the fp32-mode GEMMs
 * the launch count, the summed device milliseconds and the summed units, then clears that
 * kernel's record.  Process-global, mutex-protected; off by default. */
int pnr_timing_enable(int on);
int pnr_timing_read(int kernel, int64_t* launches, double* ms, int64_t* units);

#ifdef __cplusplus
}
#endif
#endif /* PNR_H_ */
