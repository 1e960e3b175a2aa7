// points_hash.h -- the neural-point spatial hash's cell arithmetic, shared by the index build and the
// gather (points.hip) and by the insertion pass (points_grow.hip): every kernel that names a cell
// forms it from the same float32 expression.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/pnr.h"

namespace pnr {

#define PNR_FP_STRICT _Pragma("clang fp contract(off)")

struct HashGrid {
  float o0, o1, o2;
  float inv;       // 1 / cell
  uint32_t mask;   // T - 1
  uint32_t omask;  // occupancy bits - 1
};

inline int occ_bits_log2(int32_t bits) { return bits + 6 < 26 ? bits + 6 : 26; }

inline HashGrid make_grid(const pnr_points& p) {
  HashGrid g;
  g.o0 = p.origin[0];
  g.o1 = p.origin[1];
  g.o2 = p.origin[2];
  g.inv = 1.0f / p.cell;
  g.mask = (uint32_t)((1ll << p.table_bits) - 1);
  g.omask = (uint32_t)((1ll << occ_bits_log2(p.table_bits)) - 1);
  return g;
}

__device__ __forceinline__ int cell_coord(float x, float o, float inv) {
  PNR_FP_STRICT
  float f = floorf((x - o) * inv);
  f = fminf(fmaxf(f, -1.0e9f), 1.0e9f);  // far-away / non-finite samples: any cell, never UB
  return (int)f;
}

// lower of the two cells per axis that cover [x - reach, x + reach] when cell >= 2 reach
__device__ __forceinline__ void base_cell(float x, float o, float inv, int& b) {
  PNR_FP_STRICT
  float t = (x - o) * inv;
  t = fminf(fmaxf(t, -1.0e9f), 1.0e9f);
  const float f = floorf(t);
  b = (int)f - (t - f < 0.5f ? 1 : 0);
}

__device__ __forceinline__ uint32_t cell_hash(int cx, int cy, int cz, uint32_t mask) {
  return (((uint32_t)cx * 73856093u) ^ ((uint32_t)cy * 19349663u) ^ ((uint32_t)cz * 83492791u)) & mask;
}

// exact cell identity: 3 x 21-bit two's complement (scenes stay far below 2^20 cells per axis)
__device__ __forceinline__ uint64_t cell_key(int cx, int cy, int cz) {
  return (uint64_t)((uint32_t)cx & 0x1FFFFFu) | ((uint64_t)((uint32_t)cy & 0x1FFFFFu) << 21) |
         ((uint64_t)((uint32_t)cz & 0x1FFFFFu) << 42);
}
constexpr uint64_t kCollision = 1ull << 63;

}  // namespace pnr
