// Point-wise MSE training step: the fused pair gather + squared error +
// embedding gradient scatter of point_wise_train_loop (reference
// divrec/train/utils.py:108-115) with MSELoss (divrec/losses/mse_loss.py:6-10).
//
// mse_fwd_bwd is HBM/atomic-bound like bpr_fwd_bwd (bpr.hip): per pair it reads
// two fp32 rows (2*d*4 B), 16 B of ids and a 4-B target, writes pred/loss, and
// adds 2*d*4 B of gradient with fp32 atomics, in the row-run layout of
// row_runs.h. Any d <= 512. Out-of-range ids are range-checked
// (include/divrec_hip.h): such a pair reads and adds nothing.
#include "row_runs.h"

namespace {

using dr::in_rows;

constexpr int kBlock = 256;

// E: row elements per lane, ceil(d / 32). kGrad = false is the forward-only
// form (both gradient tables NULL): no gradient registers, no atomics.
template <int E, bool kGrad>
__global__ __launch_bounds__(kBlock) void mse_kernel(
    const float* __restrict__ U, int64_t nu, const float* __restrict__ I, int64_t ni, int64_t d,
    const int64_t* __restrict__ uid, const int64_t* __restrict__ iid,
    const float* __restrict__ target, int64_t batch, int64_t span, float grad_scale,
    float* __restrict__ pred, float* __restrict__ loss, float* __restrict__ gU,
    float* __restrict__ gI, int32_t* __restrict__ err) {
  // one run per table side over this group's span of pairs (row_runs.h): an
  // unshuffled epoch pays ~1 row of atomics per pair (the item side)
  const int gl = dr::row_lane();
  const int64_t b0 = dr::row_group(kBlock) * span;
  const int64_t b1 = b0 + span < batch ? b0 + span : batch;
  int bad = 0;
  dr::RowRun<E, kGrad> ur, ir;  // the current user and item rows
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
    ur.move_to(u, U, gU, d, gl);
    ir.move_to(i, I, gI, d, gl);
    float s = 0.f;
#pragma unroll
    for (int e = 0; e < E; ++e) s = fmaf(ur.v[e], ir.v[e], s);
    dr::group_sum_f32(s);
    const float er = target[b] - s;
    if (gl == 0) {
      if (pred) pred[b] = s;
      if (loss) loss[b] = er * er;
    }
    if (kGrad) {
      const float g = -2.f * er * grad_scale;  // d/ds of (t - s)^2, scaled
#pragma unroll
      for (int e = 0; e < E; ++e) {
        ur.g[e] += g * ir.v[e];
        ir.g[e] += g * ur.v[e];
      }
    }
  }
  ur.flush(gU, d, gl);
  ir.flush(gI, d, gl);
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
  const dr::SpanPlan plan = dr::span_plan(batch, kBlock);
  auto launch = [&](auto kern) {
    hipLaunchKernelGGL(kern, dim3((unsigned)plan.grid), dim3(kBlock), 0, s, user_table,
                       n_user_rows, item_table, n_item_rows, d, user_id, item_id, target, batch,
                       plan.span, grad_scale, pred, loss, grad_user, grad_item, err);
  };
  const bool train = grad_user || grad_item;
  dr::for_row_elems<1, 2, 3, 4, 5, 6, 7, 8, 12, 16>(dr::ceil_div(d, 32), [&](auto E) {
    if (train)
      launch(mse_kernel<decltype(E)::value, true>);
    else
      launch(mse_kernel<decltype(E)::value, false>);
  });
  DR_CHECK_LAUNCH();
  return DR_OK;
}
