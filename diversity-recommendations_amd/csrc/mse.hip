// Point-wise MSE training step: the fused pair gather + squared error +
// embedding gradient scatter of point_wise_train_loop (reference
// divrec/train/utils.py:108-115) with MSELoss (divrec/losses/mse_loss.py:6-10).
//
// mse_fwd_bwd is HBM/atomic-bound like bpr_fwd_bwd (bpr.hip): per pair it reads
// two fp32 rows (2*d*4 B), 16 B of ids and a 4-B target, writes pred/loss, and
// adds 2*d*4 B of gradient with fp32 atomics. Same shape as bpr_kernel: a
// group of 32 lanes owns a contiguous span of pairs and lane l handles row
// elements l, l+32, l+64, ..., so every load and every no-return atomic
// wave-instruction covers contiguous 128-B row segments, the shape at which
// global_atomic_add_f32 runs at its full rate (MI355X_MICROARCH.md, Global
// float atomics; cdna_hip_programming.md Guideline 12). Any d <= 512.
// Out-of-range ids are range-checked (include/divrec_hip.h): such a pair reads
// and adds nothing.
#include <algorithm>

#include "common.h"

namespace {

constexpr int kBlock = 256;

__device__ __forceinline__ bool in_rows(int64_t r, int64_t n) { return r >= 0 && r < n; }

// E: row elements per lane, ceil(d / 32). kGrad = false is the forward-only
// form (both gradient tables NULL): no gradient registers, no atomics.
template <int E, bool kGrad>
__global__ __launch_bounds__(kBlock) void mse_kernel(
    const float* __restrict__ U, int64_t nu, const float* __restrict__ I, int64_t ni, int64_t d,
    const int64_t* __restrict__ uid, const int64_t* __restrict__ iid,
    const float* __restrict__ target, int64_t batch, int64_t span, float grad_scale,
    float* __restrict__ pred, float* __restrict__ loss, float* __restrict__ gU,
    float* __restrict__ gI, int32_t* __restrict__ err) {
  // Each 32-lane group walks a CONTIGUOUS span of pairs and keeps one run per
  // table side: the current user and item rows are read once per run of equal
  // ids, and their gradient contributions are summed in registers and added
  // with ONE row of atomics when the run ends. Interaction files are typically
  // grouped by user, so an unshuffled epoch pays ~1 row of atomics per pair
  // (the item side); uniform random pairs (runs of 1) pay both.
  const int gl = threadIdx.x & 31;
  const int64_t group = ((int64_t)blockIdx.x * kBlock + threadIdx.x) >> 5;
  const int64_t b0 = group * span;
  const int64_t b1 = b0 + span < batch ? b0 + span : batch;
  int bad = 0;
  int64_t cu = -1, ci = -1;  // ids of the current runs (-1 = none)
  float uv[E], iv[E];        // their rows
  float gu[E], gi[E];        // their summed gradient contributions
#pragma unroll
  for (int e = 0; e < E; ++e) gu[e] = gi[e] = 0.f;
  auto load = [&](const float* tab, int64_t r, float (&v)[E]) {
    const float* row = tab + r * d;
#pragma unroll
    for (int e = 0; e < E; ++e) {
      const int64_t x = e * 32 + gl;
      v[e] = x < d ? row[x] : 0.f;
    }
  };
  auto flush = [&](float* g, int64_t r, float (&acc)[E]) {  // one row of atomics
    if (!kGrad) return;
    if (g && r >= 0) {
#pragma unroll
      for (int e = 0; e < E; ++e) {
        const int64_t x = e * 32 + gl;
        if (x < d) atomicAdd(g + r * d + x, acc[e]);
      }
    }
#pragma unroll
    for (int e = 0; e < E; ++e) acc[e] = 0.f;
  };
  for (int64_t b = b0; b < b1; ++b) {
    const int64_t u = uid[b], i = iid[b];
    if (!in_rows(u, nu) || !in_rows(i, ni)) {  // uniform in the group
      if (gl == 0) {
        if (pred) pred[b] = __builtin_nanf("");
        if (loss) loss[b] = __builtin_nanf("");
        bad += 1;
      }
      continue;
    }
    if (u != cu) {
      flush(gU, cu, gu);
      cu = u;
      load(U, u, uv);
    }
    if (i != ci) {
      flush(gI, ci, gi);
      ci = i;
      load(I, i, iv);
    }
    float s = 0.f;
#pragma unroll
    for (int e = 0; e < E; ++e) s = fmaf(uv[e], iv[e], s);
#pragma unroll
    for (int m = 16; m > 0; m >>= 1) s += __shfl_xor(s, m);  // xor < 32: inside the group
    const float er = target[b] - s;
    if (gl == 0) {
      if (pred) pred[b] = s;
      if (loss) loss[b] = er * er;
    }
    if (kGrad) {
      const float g = -2.f * er * grad_scale;  // d/ds of (t - s)^2, scaled
#pragma unroll
      for (int e = 0; e < E; ++e) {
        gu[e] += g * iv[e];
        gi[e] += g * uv[e];
      }
    }
  }
  flush(gU, cu, gu);
  flush(gI, ci, gi);
  if (bad && err) atomicAdd(err, bad);
}

}  // namespace

extern "C" int dr_mse_fwd_bwd(const float* user_table, int64_t n_user_rows,
                              const float* item_table, int64_t n_item_rows, int64_t d,
                              const int64_t* user_id, const int64_t* item_id,
                              const float* target, int64_t batch, float grad_scale, float* pred,
                              float* loss, float* grad_user, float* grad_item, int32_t* err,
                              dr_stream_t stream) {
  DR_CHECK_ARG(batch >= 0 && n_user_rows >= 0 && n_item_rows >= 0, "sizes must be >= 0");
  if (batch == 0) return DR_OK;
  DR_CHECK_ARG(user_table && item_table && user_id && item_id && target, "null pointer");
  DR_CHECK_ARG(d >= 1 && d <= 512, "d must be in [1, 512]");
  hipStream_t s = (hipStream_t)stream;
  // contiguous spans of pairs per 32-lane group, up to 8 workgroups per CU
  // (at least 16 per span, so runs are summed in small batches too)
  constexpr int64_t kGroups = 256 * 8 * (kBlock / 32);
  const int64_t span = std::max<int64_t>(16, dr::ceil_div(batch, kGroups));
  const int64_t grid = dr::ceil_div(dr::ceil_div(batch, span), kBlock / 32);
  const bool train = grad_user || grad_item;
#define DR_MSE_K(EE, GG)                                                                       \
  hipLaunchKernelGGL((mse_kernel<EE, GG>), dim3((unsigned)grid), dim3(kBlock), 0, s,           \
                     user_table, n_user_rows, item_table, n_item_rows, d, user_id, item_id,    \
                     target, batch, span, grad_scale, pred, loss, grad_user, grad_item, err)
#define DR_MSE(EE)          \
  do {                      \
    if (train)              \
      DR_MSE_K(EE, true);   \
    else                    \
      DR_MSE_K(EE, false);  \
  } while (0)
  switch ((int)dr::ceil_div(d, 32)) {
    case 1: DR_MSE(1); break;
    case 2: DR_MSE(2); break;
    case 3: DR_MSE(3); break;
    case 4: DR_MSE(4); break;
    case 5: DR_MSE(5); break;
    case 6: DR_MSE(6); break;
    case 7: DR_MSE(7); break;
    case 8: DR_MSE(8); break;
    case 9: case 10: case 11: case 12: DR_MSE(12); break;
    default: DR_MSE(16); break;
  }
#undef DR_MSE
#undef DR_MSE_K
  DR_CHECK_LAUNCH();
  return DR_OK;
}
