// Row runs: the layout and the run primitive of the training-step kernels
// (bpr_kernel, mse_kernel, gather_dot_bwd_rows), which are bound by fp32 atomics.
//
// A group of 32 lanes owns an embedding row and lane l handles its elements
// l, l+32, l+64, ... (E = ceil(d / 32) per lane, any d <= 512): every load
// and every atomic wave-instruction then covers contiguous 128-B row segments,
// the shape at which global_atomic_add_f32 runs at its full rate
// (MI355X_MICROARCH.md, Global float atomics; cdna_hip_programming.md
// Guideline 12). 16-B-per-lane chunks scatter each atomic instruction over
// 16-B strides and measured 3.9x slower.
//
// A RowRun is one table side of a group that walks a CONTIGUOUS span of the
// batch: the row of the current id is read once per run of equal ids, its
// gradient contributions are summed in registers and added with ONE row of
// atomics when the run ends. The reference's own batches are such runs
// (PairWiseDataset's m x m product: one user for m*m triples, each positive
// repeated m times in a row, base_datasets.py:94-107; interaction files
// grouped by user), so the atomics per sample drop to ~1 row there; uniform
// random ids (runs of 1) cost one row per side.
#pragma once

#include <algorithm>
#include <type_traits>

#include "common.h"

namespace dr {

__device__ __forceinline__ bool in_rows(int64_t r, int64_t n) { return r >= 0 && r < n; }

// ---------------------------------------------------------------- device
// This lane's place in its 32-lane group, and the group's index in a grid of
// `block`-thread workgroups.
__device__ __forceinline__ int row_lane() { return threadIdx.x & 31; }
__device__ __forceinline__ int64_t row_group(int block) {
  return ((int64_t)blockIdx.x * block + threadIdx.x) >> 5;
}

template <int E>  // v = this lane's elements of a row of d floats, 0 past the end
__device__ __forceinline__ void load_row(const float* row, int64_t d, int gl, float (&v)[E]) {
#pragma unroll
  for (int e = 0; e < E; ++e) {
    const int64_t x = e * 32 + gl;
    v[e] = x < d ? row[x] : 0.f;
  }
}

template <int E>  // row r of table += v: one row of atomics
__device__ __forceinline__ void atomic_add_row(float* table, int64_t r, int64_t d, int gl,
                                               const float (&v)[E]) {
#pragma unroll
  for (int e = 0; e < E; ++e) {
    const int64_t x = e * 32 + gl;
    if (x < d) atomicAdd(table + r * d + x, v[e]);
  }
}

// Every lane: each value's sum over its group, the values' exchanges of a step
// issued together (xor < 32 stays inside the 32-lane group).
template <typename... F>
__device__ __forceinline__ void group_sum_f32(F&... v) {
#pragma unroll
  for (int m = 16; m > 0; m >>= 1) ((v += __shfl_xor(v, m)), ...);
}

// kGrad = false is the forward-only form: g is never touched, so neither the
// gradient registers nor the atomics are compiled.
template <int E, bool kGrad = true>
struct RowRun {
  int64_t id = -1;  // the current run's row (-1 = none)
  float v[E];       // that row
  float g[E];       // its summed gradient contributions

  __device__ __forceinline__ RowRun() {
    if (kGrad) {
#pragma unroll
      for (int e = 0; e < E; ++e) g[e] = 0.f;
    }
  }
  // ends the run: g goes to row id of grad_table (may be NULL) and is cleared
  __device__ __forceinline__ void flush(float* grad_table, int64_t d, int gl) {
    if (!kGrad) return;
    if (grad_table && id >= 0) atomic_add_row(grad_table, id, d, gl, g);
#pragma unroll
    for (int e = 0; e < E; ++e) g[e] = 0.f;
  }
  // row r (in range) of table becomes the current row
  __device__ __forceinline__ void move_to(int64_t r, const float* table, float* grad_table,
                                          int64_t d, int gl) {
    if (r == id) return;
    flush(grad_table, d, gl);
    id = r;
    load_row(table + r * d, d, gl, v);
  }
};

// ---------------------------------------------------------------- host
// Contiguous spans of the batch per 32-lane group, up to 8 workgroups per CU,
// at least 16 samples per span (so runs are summed in small batches too).
struct SpanPlan { int64_t span, grid; };
inline SpanPlan span_plan(int64_t batch, int block) {
  const int64_t groups = 256 * 8 * (block / 32);
  const int64_t span = std::max<int64_t>(16, ceil_div(batch, groups));
  return {span, ceil_div(ceil_div(batch, span), block / 32)};
}

// Workgroups for `items` at per_block each, capped (the kernel grid-strides
// the rest, Guideline 11) and at least 1.
inline int capped_grid(int64_t items, int64_t per_block, int64_t cap) {
  return (int)std::min(std::max<int64_t>(ceil_div(items, per_block), 1), cap);
}

// f(std::integral_constant<int, E>) for the smallest listed E >= elems.
template <int... Es, typename F>
inline void for_row_elems(int64_t elems, F&& f) {
  (void)((elems <= Es && (f(std::integral_constant<int, Es>{}), true)) || ...);
}

}  // namespace dr
