// The 32-row bf16 tile primitives of the embedding ILD (ild.hip), shared with
// the history-distance kernels (history_dist.hip): a tile holds 32 table rows
// as MFMA fragments, lane l -> row (l & 31), k-slice 8*(l >> 5) + 16*s, and the
// same fragment serves as A (rows) and B (columns) operand of
// v_mfma_f32_32x32x16_bf16.
#pragma once

#include "common.h"

namespace dr {

// This lane's fragments of table row `row` (h = lane >> 5, col = lane & 31
// throughout).
template <int D>
__device__ __forceinline__ void gather_row(const __bf16* __restrict__ E, int64_t row, int h,
                                           bf16x8 (&f)[D / 16]) {
  const uint4* src = reinterpret_cast<const uint4*>(E + row * D + 8 * h);
#pragma unroll
  for (int s = 0; s < D / 16; ++s) f[s] = __builtin_bit_cast(bf16x8, src[2 * s]);
}

template <int D>
__device__ __forceinline__ f32x16 gram_tile(const bf16x8 (&x)[D / 16], const bf16x8 (&y)[D / 16]) {
  f32x16 acc = f32x16{};
#pragma unroll
  for (int s = 0; s < D / 16; ++s)
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(x[s], y[s], acc, 0, 0, 0);
  return acc;
}

// Element (c, c) of a Gram tile is register diag_reg(c) of the lane with
// col = c in the half-wave that diag_owner(col, h) is true for.
__device__ constexpr int diag_reg(int col) { return (col & 3) + 4 * (col >> 3); }
__device__ __forceinline__ bool diag_owner(int col, int h) { return ((col >> 2) & 1) == h; }

// Distance of a pair from its Gram element g and the per-row terms of its two
// rows: 1/|e| (cosine), unused (dot), |e|^2 (euclidean).
template <int KIND>
__device__ __forceinline__ float pair_dist(float g, float wi, float wj) {
  if constexpr (KIND == DR_ILD_COSINE) return fmaf(-g, wi * wj, 1.f);
  else if constexpr (KIND == DR_ILD_DOT) return g;
  else return sqrtf(fmaxf(wi + wj - 2.f * g, 0.f));
}

}  // namespace dr
