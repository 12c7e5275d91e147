// WARP step (Weston, Bengio, Usunier 2011, as LightFM implements it; not in the
// reference): per (user, positive) pair, draw negatives until one violates the
// margin, weight the update by the rank that the number of draws implies, and
// add the gradients of that one triple. include/divrec_hip.h states the
// semantics; the result is defined by trial order alone.
//
// One 32-lane group per pair over contiguous spans, in the row-run layout of
// row_runs.h: the user row and the positive row are RowRuns (an unshuffled
// interaction file is runs of one user), the violator's row is added directly.
// Every lane of a group draws the same candidates and searches the same
// sorted lists (uniform, broadcast loads), so no lane exchange is needed
// beyond the dot products' xor tree.
//
// A serial trial costs one random HBM row fetch. The kernel therefore draws
// and loads kRound candidate rows per round, all loads in flight together,
// and takes the first violator in trial order: the outcome is that of
// rounds of 1, the rows fetched past the violator are wasted bytes. The first
// round is trial 0 alone (kFirst): on an untrained or easy pair it violates,
// and rows loaded beside it measured 16 % on the whole step (DESIGN.md
// §3.6c). A skipped draw (the positive itself, a listed positive, an
// excluded item) uses up its trial; its row is fetched with the round's
// others and never scored. The reported loss's hinge is re-evaluated in
// float64 for the one chosen triple. Per pair: (2 + scored trials) rows
// read, 3 rows of fp32 atomics with a violator, none without. Any d <= 512.
#include <cmath>

#include "row_runs.h"

// Candidate rows in flight in the first round and in every later one: the
// measured choices of DESIGN.md §3.6c, which change no result.
#ifndef DR_WARP_FIRST
#define DR_WARP_FIRST 1
#endif
#ifndef DR_WARP_ROUND
#define DR_WARP_ROUND 4
#endif

namespace {

using dr::in_rows;

constexpr int kBlock = 256;
constexpr int kFirst = DR_WARP_FIRST;
constexpr int kRound = DR_WARP_ROUND;
constexpr int kMaxTrials = 4096;
static_assert(kRound >= 1 && kRound <= 8, "DR_WARP_ROUND must be in [1, 8]");
static_assert(kFirst >= 1 && kFirst <= 8, "DR_WARP_FIRST must be in [1, 8]");

struct WarpArgs {
  const float* U;
  int64_t nu;
  const float* I;
  int64_t ni, d;
  const int64_t* uid;
  const int64_t* pid;
  int64_t batch, span;
  const int64_t* pos_rowptr;
  const int32_t* pos_items;
  const int64_t* excl_rowptr;
  const int32_t* excl_items;
  int max_trials;
  float margin;
  uint64_t seed;
  int64_t pair_base;
  float grad_scale;
  float* loss;
  int64_t* neg;
  int32_t* trials;
  float* gU;
  float* gI;
  int32_t* err;
};

// row u of an optional CSR: its sorted items and their count (0 without the CSR)
struct SortedRow {
  const int32_t* items = nullptr;
  int64_t n = 0;
  __device__ __forceinline__ SortedRow(const int64_t* rowptr, const int32_t* all, int64_t u) {
    if (rowptr) {
      items = all + rowptr[u];
      n = rowptr[u + 1] - rowptr[u];
    }
  }
  __device__ __forceinline__ bool holds(int32_t c) const {
    return n && dr::sorted_contains(items, n, c);
  }
};

template <int E>  // row elements per lane: ceil(d / 32)
__global__ __launch_bounds__(kBlock) void warp_kernel(const WarpArgs a) {
  const int gl = dr::row_lane();
  const int64_t b0 = dr::row_group(kBlock) * a.span;
  const int64_t b1 = b0 + a.span < a.batch ? b0 + a.span : a.batch;
  const int64_t d = a.d;
  int bad = 0;
  dr::RowRun<E> ur, pr;  // the current user and positive rows
  for (int64_t b = b0; b < b1; ++b) {
    const int64_t u = a.uid[b], p = a.pid[b];
    if (!in_rows(u, a.nu) || !in_rows(p, a.ni)) {  // uniform in the group
      if (gl == 0) {
        if (a.loss) a.loss[b] = __builtin_nanf("");
        if (a.neg) a.neg[b] = -1;
        if (a.trials) a.trials[b] = 0;
        bad += 1;
      }
      continue;
    }
    ur.move_to(u, a.U, a.gU, d, gl);
    pr.move_to(p, a.I, a.gI, d, gl);
    float sp = 0.f;
#pragma unroll
    for (int e = 0; e < E; ++e) sp = fmaf(ur.v[e], pr.v[e], sp);
    dr::group_sum_f32(sp);
    const float bar = sp - a.margin;  // a candidate above it violates the margin
    const SortedRow positives(a.pos_rowptr, a.pos_items, u);
    const SortedRow excluded(a.excl_rowptr, a.excl_items, u);

    int n_trials = a.max_trials;
    int64_t violator = -1;
    float pair_loss = 0.f;
    // the first violator in trial order: its loss, and its triple's gradients
    auto take = [&](int t, int32_t c, const float (&nv)[E]) {
      n_trials = t + 1;
      violator = c;
      const int64_t rank = (a.ni - 1) / n_trials;  // integer division
      const float w = rank > 1 ? logf((float)rank) : 0.f;
      if (a.loss && w != 0.f) {
        // The reported hinge margin - s_p + s_n = margin + <u, c - p> of this
        // one triple in float64: w (up to log n_items) times the fp32 error of
        // the two dot products is past the loss bound where the hinge is near
        // 0. The violation test above stays the fp32 one.
        double h = 0.0;
#pragma unroll
        for (int e = 0; e < E; ++e)
          h = fma((double)ur.v[e], (double)nv[e] - (double)pr.v[e], h);
#pragma unroll
        for (int m = 16; m > 0; m >>= 1) h += __shfl_xor(h, m);
        pair_loss = (float)((double)w * ((double)a.margin + h));
      }
      const float g = w * a.grad_scale;
      if (g == 0.f) return;  // log 1: the violator is reported, nothing is added
      float gn[E];
#pragma unroll
      for (int e = 0; e < E; ++e) {
        ur.g[e] += g * nv[e] - g * pr.v[e];
        pr.g[e] += -g * ur.v[e];
        gn[e] = g * ur.v[e];
      }
      if (a.gI) dr::atomic_add_row(a.gI, (int64_t)c, d, gl, gn);
    };
    // one round: trials t0 .. t0 + R - 1
    auto round = [&](auto rows, int t0) {
      constexpr int R = decltype(rows)::value;
      int32_t c[R];
      bool scored[R];
      float nv[R][E], sn[R];
#pragma unroll
      for (int r = 0; r < R; ++r) {  // the round's draws, every row load in flight
        c[r] = (int32_t)(dr::draw_bits(a.seed, a.pair_base + b, 0, t0 + r) % (uint64_t)a.ni);
        scored[r] = t0 + r < a.max_trials && c[r] != p && !positives.holds(c[r]) &&
                    !excluded.holds(c[r]);
        dr::load_row(a.I + (int64_t)c[r] * d, d, gl, nv[r]);
      }
#pragma unroll
      for (int r = 0; r < R; ++r) {
        sn[r] = 0.f;
#pragma unroll
        for (int e = 0; e < E; ++e) sn[r] = fmaf(ur.v[e], nv[r][e], sn[r]);
      }
#pragma unroll
      for (int m = 16; m > 0; m >>= 1) {  // the round's xor trees, issued together
#pragma unroll
        for (int r = 0; r < R; ++r) sn[r] += __shfl_xor(sn[r], m);
      }
#pragma unroll
      for (int r = 0; r < R; ++r) {
        if (violator < 0 && scored[r] && sn[r] > bar) take(t0 + r, c[r], nv[r]);
      }
    };
    round(std::integral_constant<int, kFirst>{}, 0);
    for (int t0 = kFirst; t0 < a.max_trials && violator < 0; t0 += kRound)
      round(std::integral_constant<int, kRound>{}, t0);
    if (gl == 0) {
      if (a.loss) a.loss[b] = pair_loss;
      if (a.neg) a.neg[b] = violator;
      if (a.trials) a.trials[b] = n_trials;
    }
  }
  ur.flush(a.gU, d, gl);
  pr.flush(a.gI, d, gl);
  if (bad && a.err) atomicAdd(a.err, bad);
}

}  // namespace

extern "C" int dr_warp_fwd_bwd(const float* user_table, int64_t n_user_rows,
                               const float* item_table, int64_t n_item_rows, int64_t d,
                               const int64_t* user_id, const int64_t* pos_id, int64_t batch,
                               const int64_t* pos_rowptr, const int32_t* pos_items,
                               const int64_t* excl_rowptr, const int32_t* excl_items,
                               int max_trials, float margin, uint64_t seed, int64_t pair_base,
                               float grad_scale, float* loss, int64_t* neg_id, int32_t* trials,
                               float* grad_user, float* grad_item, int32_t* err,
                               dr_stream_t stream) {
  DR_CHECK_ARG(batch >= 0 && n_user_rows >= 0 && n_item_rows >= 0, "sizes must be >= 0");
  DR_CHECK_ARG(n_item_rows < 0x7fffffffLL, "n_item_rows must be < 2^31 - 1");
  DR_CHECK_ARG(max_trials >= 1 && max_trials <= kMaxTrials, "max_trials must be in [1, 4096]");
  DR_CHECK_ARG(d >= 1 && d <= 512, "d must be in [1, 512]");
  DR_CHECK_ARG(std::isfinite(margin), "margin must be finite");
  DR_CHECK_ARG(pair_base >= 0, "pair_base must be >= 0");
  DR_CHECK_ARG((pos_rowptr == nullptr) == (pos_items == nullptr),
               "pos_rowptr and pos_items must both be set or both be NULL");
  DR_CHECK_ARG((excl_rowptr == nullptr) == (excl_items == nullptr),
               "excl_rowptr and excl_items must both be set or both be NULL");
  if (batch == 0) return DR_OK;
  DR_CHECK_ARG(user_table && item_table && user_id && pos_id, "null pointer");
  const dr::SpanPlan plan = dr::span_plan(batch, kBlock);
  const WarpArgs a{user_table, n_user_rows, item_table, n_item_rows, d, user_id, pos_id, batch,
                   plan.span, pos_rowptr, pos_items, excl_rowptr, excl_items, max_trials, margin,
                   seed, pair_base, grad_scale, loss, neg_id, trials, grad_user, grad_item, err};
  dr::for_row_elems<1, 2, 3, 4, 5, 6, 7, 8, 12, 16>(dr::ceil_div(d, 32), [&](auto E) {
    hipLaunchKernelGGL(warp_kernel<decltype(E)::value>, dim3((unsigned)plan.grid), dim3(kBlock),
                       0, (hipStream_t)stream, a);
  });
  DR_CHECK_LAUNCH();
  return DR_OK;
}

extern "C" int dr_warp_round(void) { return kRound; }

extern "C" int dr_warp_candidates(uint64_t seed, int64_t pair_base, int64_t n_pairs,
                                  int max_trials, int64_t n_items, int32_t* out) {
  DR_CHECK_ARG(n_pairs >= 0 && pair_base >= 0, "n_pairs and pair_base must be >= 0");
  DR_CHECK_ARG(max_trials >= 1 && max_trials <= kMaxTrials, "max_trials must be in [1, 4096]");
  DR_CHECK_ARG(n_items >= 1 && n_items < 0x7fffffffLL, "1 <= n_items < 2^31 - 1 required");
  if (n_pairs == 0) return DR_OK;
  DR_CHECK_ARG(out, "null pointer");
  for (int64_t b = 0; b < n_pairs; ++b)
    for (int t = 0; t < max_trials; ++t)
      out[b * max_trials + t] =
          (int32_t)(dr::draw_bits(seed, pair_base + b, 0, t) % (uint64_t)n_items);
  return DR_OK;
}
