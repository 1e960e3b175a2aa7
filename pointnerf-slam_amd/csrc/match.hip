// match.hip -- two-way nearest-neighbour matching of unit descriptors (src/Tracker.py:398-440,
// nn_match_two_way, the SuperPoint step ahead of the weak-depth Tracker).
//
//   dot[i][j] = sum_k desc1[k][i] desc2[k][j]        desc1 (D,N), desc2 (D,M) float32 row-major
//   dist      = sqrt(2 - 2 clip(dot, -1, 1))
//   a row i is kept when dist[i][j*] < nn_thresh for j* = argmin_j dist[i][.] and argmin_i dist[.][j*] = i
//
// Both operands are k-major, which is the layout v_mfma_f32_32x32x2_f32 wants with no transpose: a slab
// [k][row] in LDS feeds the A operand (lane l reads row l & 31 of k-plane l >> 5: 32 consecutive floats
// per k-plane) and the B operand alike.  The row stride of the slab is kLd = 160 floats = 32 banks
// modulo 64, so the two k-planes of a read fall on disjoint banks: conflict-free.
//   k_match_clear     zeroes row_key[N] | col_key[M] (the caller's workspace may be dirty).
//   k_match_dots      one 64 x 64 tile of dot per workgroup, four waves, one 32 x 32 accumulator each
//                     (a 1,024 x 1,024 call is 256 workgroups: one per CU).  k is walked in slabs of 32
//                     through two LDS buffers: the next slab is in flight in registers (16 coalesced 4-B
//                     loads per thread, any N and M: columns past the end load 0) while the MFMAs of this
//                     one run; one barrier per slab.  The N x M matrix never reaches memory: the epilogue
//                     clips the accumulator, maps each element to its orderable uint32 image (a padded
//                     row or column to 0, below every real image), reduces every accumulator row over
//                     the 32 lanes of its half wave (5 __shfl_xor steps on the image, then a ballot picks
//                     the lowest column among the maxima) and every column over the 16 registers and the
//                     two half waves, and merges both into the key arrays with one 64-bit atomicMax per
//                     row / column and wave.
//                       key = image(clipped dot) << 32 | (0xFFFFFFFF - index)
//                     so the larger dot wins and, among bitwise-equal dots, the lowest index: np.argmin's
//                     first occurrence on the distance.  Every dot is formed by exactly one wave as one
//                     fma chain in ascending k, and max is order-free: equal inputs give equal bits.
//   k_match_finalize  one workgroup: per row decode j* and the dot, score = sqrtf(2 - 2 dot), keep when
//                     score < nn_thresh and col_key[j*] decodes to the row; the kept rows are compacted in
//                     ascending row order (ballot + a scan of the wave totals per 1,024 rows).
// Integer atomics only, vector stores only.
#include "pnr_internal.h"

namespace pnr {

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kMT = 64;        // tile edge (rows of desc1^T and of desc2^T per workgroup)
constexpr int kKS = 32;        // k rows per slab
constexpr int kLd = 160;       // slab row stride in floats: [A 64 | B 64 | pad 32]
constexpr int kSlab = kKS * kLd;
constexpr int kLoads = kKS * 2 * kMT / 256;  // 4-B loads per thread and slab
constexpr int kMatchMaxDim = 512;
constexpr int64_t kMatchMaxCols = 1 << 20;   // N, M: the tile grid stays below 2^31, indices in int32

// monotone map float -> uint32 (a < b <=> image(a) < image(b)); x + 0 folds -0 into +0
__device__ __forceinline__ uint32_t image_of(float x) {
  const uint32_t u = __float_as_uint(x + 0.f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float dot_of(uint32_t img) {
  return __uint_as_float((img & 0x80000000u) ? (img & 0x7FFFFFFFu) : ~img);
}
__device__ __forceinline__ unsigned long long key_of(uint32_t img, uint32_t index) {
  return ((unsigned long long)img << 32) | (unsigned long long)(0xFFFFFFFFu - index);
}
__device__ __forceinline__ uint32_t index_of(unsigned long long key) { return 0xFFFFFFFFu - (uint32_t)key; }

__global__ __launch_bounds__(256) void k_match_clear(unsigned long long* __restrict__ keys, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) keys[i] = 0ull;
}

struct MatchArgs {
  const float* d1;  // (D,N)
  const float* d2;  // (D,M)
  int32_t D, N, M;
  int32_t tiles_m;  // column tiles
  unsigned long long* row_key;
  unsigned long long* col_key;
};

__global__ __launch_bounds__(256) void k_match_dots(MatchArgs a) {
  __shared__ float lds[2 * kSlab];
  const int t = threadIdx.x;
  const int lane = t & 63, hh = lane >> 5, i = lane & 31;
  const int w = __builtin_amdgcn_readfirstlane(t >> 6);
  const int wr = w >> 1, wc = w & 1;
  const int n0 = (int)(blockIdx.x / a.tiles_m) * kMT;
  const int m0 = (int)(blockIdx.x % a.tiles_m) * kMT;

  // this thread's column of the slab: c < 64 = column n0 + c of desc1, else column m0 + c - 64 of desc2
  const int c = t & 127, par = t >> 7;
  const bool isA = c < kMT;
  const int col = isA ? n0 + c : m0 + c - kMT;
  const int ld = isA ? a.N : a.M;
  const bool ok = col < ld;
  const float* src = (isA ? a.d1 : a.d2) + (ok ? col : 0);

  float v[kLoads];
  auto load_slab = [&](int k0) {
#pragma unroll
    for (int q = 0; q < kLoads; ++q) v[q] = ok ? src[(int64_t)(k0 + 2 * q + par) * ld] : 0.f;
  };
  auto store_slab = [&](float* s) {
#pragma unroll
    for (int q = 0; q < kLoads; ++q) s[(2 * q + par) * kLd + c] = v[q];
  };

  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;

  load_slab(0);
  store_slab(lds);
  __syncthreads();
  int buf = 0;
  for (int k0 = 0; k0 < a.D; k0 += kKS) {
    const bool more = k0 + kKS < a.D;
    if (more) load_slab(k0 + kKS);
    const float* s = lds + buf * kSlab;
    const float* sa = s + hh * kLd + wr * 32 + i;
    const float* sb = s + hh * kLd + kMT + wc * 32 + i;
    float av[kKS / 2], bv[kKS / 2];  // the slab's operands up front: the reads run under the MFMA chain
#pragma unroll
    for (int kk = 0; kk < kKS / 2; ++kk) {
      av[kk] = sa[2 * kk * kLd];
      bv[kk] = sb[2 * kk * kLd];
    }
    __builtin_amdgcn_sched_barrier(0);  // (the scheduler otherwise sinks each read to its MFMA)
#pragma unroll
    for (int kk = 0; kk < kKS / 2; ++kk) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[kk], bv[kk], acc, 0, 0, 0);
    buf ^= 1;
    if (more) store_slab(lds + buf * kSlab);  // last read one barrier ago
    __syncthreads();
  }

  // lane (hh, i), register r: dot of row n0 + 32 wr + perm(r, hh) and column m0 + 32 wc + i
  const int colj = m0 + 32 * wc + i;
  const int rowb = n0 + 32 * wr;
  const bool col_ok = colj < a.M;
  uint32_t cbest = 0, crow = 0;      // this lane's column: best image over its 16 rows, lowest row of it
  unsigned long long rkey = 0ull;    // lane i < 16 ends up with the key of row perm(i, hh)
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int row = rowb + perm(r, hh);  // ascending in r
    const float d = fminf(fmaxf(acc[r], -1.f), 1.f);
    const uint32_t img = (col_ok && row < a.N) ? image_of(d) : 0u;
    if (img > cbest) {
      cbest = img;
      crow = (uint32_t)row;
    }
    uint32_t mx = img;
#pragma unroll
    for (int s = 1; s < 32; s <<= 1) {
      const uint32_t o = (uint32_t)__shfl_xor((int)mx, s);
      mx = o > mx ? o : mx;
    }
    const unsigned long long eq = __ballot(img == mx);
    const uint32_t half = (uint32_t)(eq >> (32 * hh));     // never 0: the maximum's own lane is in it
    const uint32_t jmin = (uint32_t)(m0 + 32 * wc) + (uint32_t)(__ffs((int)half) - 1);
    if (i == r) rkey = mx ? key_of(mx, jmin) : 0ull;
  }
  if (i < 16) {
    const int row = rowb + perm(i, hh);
    if (row < a.N && rkey) atomicMax(&a.row_key[row], rkey);
  }
  // the other half wave holds the column's other 16 rows
  const uint32_t obest = (uint32_t)__shfl_xor((int)cbest, 32);
  const uint32_t orow = (uint32_t)__shfl_xor((int)crow, 32);
  if (obest > cbest || (obest == cbest && orow < crow)) {
    cbest = obest;
    crow = orow;
  }
  if (hh == 0 && col_ok && cbest) atomicMax(&a.col_key[colj], key_of(cbest, crow));
}

__global__ __launch_bounds__(1024) void k_match_finalize(const unsigned long long* __restrict__ row_key,
                                                         const unsigned long long* __restrict__ col_key, int32_t N,
                                                         int32_t M, float thresh, int32_t* __restrict__ idx1,
                                                         int32_t* __restrict__ idx2, float* __restrict__ score,
                                                         int32_t* __restrict__ count) {
  __shared__ int s_tot[16];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  int base = 0;
  for (int i0 = 0; i0 < N; i0 += 1024) {
    const int row = i0 + t;
    bool keep = false;
    uint32_t j = 0;
    float sc = 0.f;
    if (row < N) {
      const unsigned long long key = row_key[row];
      j = index_of(key);
      sc = sqrtf(2.f - 2.f * dot_of((uint32_t)(key >> 32)));
      keep = sc < thresh && j < (uint32_t)M && index_of(col_key[j]) == (uint32_t)row;
    }
    const unsigned long long m = __ballot(keep);
    if (lane == 0) s_tot[w] = __popcll(m);
    __syncthreads();
    int before = 0, all = 0;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int n = s_tot[q];
      before += q < w ? n : 0;
      all += n;
    }
    if (keep) {
      const int pos = base + before + __popcll(m & ((1ull << lane) - 1ull));
      idx1[pos] = row;
      idx2[pos] = (int32_t)j;
      score[pos] = sc;
    }
    base += all;
    __syncthreads();  // s_tot is rewritten by the next round
  }
  if (t == 0) *count = base;
}

}  // namespace

// workspace: row_key[N] | col_key[M], 8 B each; 0 for sizes the call refuses
size_t match_workspace_bytes(int64_t N, int64_t M) {
  if (N < 0 || M < 0 || N > kMatchMaxCols || M > kMatchMaxCols) return 0;
  const int64_t n = N + M;
  return (size_t)(n > 0 ? n : 1) * 8;
}

int launch_match_two_way(const float* d1, const float* d2, int32_t D, int64_t N, int64_t M, float thresh,
                         int32_t* idx1, int32_t* idx2, float* score, int32_t* count, void* ws, size_t ws_bytes,
                         hipStream_t st) {
  if (D < 32 || D > kMatchMaxDim || D % 32 != 0 || !(thresh >= 0.f)) return PNR_E_ARG;
  if (N < 0 || M < 0 || N > kMatchMaxCols || M > kMatchMaxCols || !count) return PNR_E_ARG;
  unsigned long long* keys = static_cast<unsigned long long*>(ws);
  if (N == 0 || M == 0) {  // np.zeros((3, 0)): the count alone
    hipLaunchKernelGGL(k_match_finalize, dim3(1), dim3(1024), 0, st, keys, keys, 0, 0, thresh, idx1, idx2, score, count);
    return hip_status(hipGetLastError());
  }
  if (!d1 || !d2 || !idx1 || !idx2 || !score || !ws || (reinterpret_cast<uintptr_t>(ws) & 7)) return PNR_E_ARG;
  if (ws_bytes < match_workspace_bytes(N, M)) return PNR_E_WORKSPACE;
  MatchArgs a{d1, d2, D, (int32_t)N, (int32_t)M, (int32_t)((M + kMT - 1) / kMT), keys, keys + N};
  const int64_t tiles = ((N + kMT - 1) / kMT) * a.tiles_m;
  hipLaunchKernelGGL(k_match_clear, dim3((unsigned)((N + M + 255) / 256)), dim3(256), 0, st, keys, N + M);
  hipLaunchKernelGGL(k_match_dots, dim3((unsigned)tiles), dim3(256), 0, st, a);
  hipLaunchKernelGGL(k_match_finalize, dim3(1), dim3(1024), 0, st, a.row_key, a.col_key, a.N, a.M, thresh, idx1,
                     idx2, score, count);
  return hip_status(hipGetLastError());
}

}  // namespace pnr
