// Calibrated re-rank over item partition labels (Steck, "Calibrated
// Recommendations", RecSys 2018): top-C candidates -> k_out picks per user,
// each pick maximising lambda * score - (1 - lambda) * KL(p || q~(list + pick)),
// p the label distribution of the user's history, q~ that of the list. There
// is no reference symbol, as for MMR and DPP; the spec is the build's own
// (include/divrec_hip.h). Beside it: the label histogram of a history CSR
// (dr_label_profile) and the KL of finished lists (dr_calibration_kl).
//
// Layout: there are no item rows, so a user's whole state
// fits one wave and no workgroup barrier separates the steps of a user.
//   * lane g < G is category g: it keeps p_g, log p_g and the count n_g;
//   * candidate position j * 64 + lane (j < 16) is register j of the lane:
//     lambda * score (-inf once picked or never live) and the label as a
//     ds_bpermute address.
// A step: every category lane forms its two KL terms (the list as it stands,
// and with one more of its own label), one DPP wave sum gives the base, and
// KL_c = base - a_c + b_c is the value of adding label c: two logf per lane,
// no G x G loop. Each lane then reads the gain of its 16 labels across lanes,
// keeps its best candidate, and a DPP wave argmax (the best value, then the
// lowest position that holds it) makes the pick. Waves of a workgroup run different users; the grid is
// persistent over users.
#include <float.h>

#include "common.h"
#include "rerank_args.h"

namespace {

constexpr int kWaves = 4;                 // users in flight per workgroup
constexpr int kThreads = kWaves * 64;
constexpr int kPer = 16;                  // candidates per lane
constexpr int kMaxC = kPer * 64;          // 1024
constexpr int kMaxG = DR_CALIB_MAX_LABELS;
static_assert(kMaxG == 64, "one lane per category");

using dr::profile_entry;  // lane g's entry of the normalised profile row

// p log(p / q~) with q~ = (1 - alpha) share + alpha p (>= alpha p, so finite); 0 where p = 0
__device__ __forceinline__ float kl_term(float p, float logp, float share) {
  const float q = fmaf(1.f - DR_CALIB_ALPHA, share, DR_CALIB_ALPHA * p);
  return p > 0.f ? p * (logp - logf(q)) : 0.f;
}

// Label of item `it`, or -1 with *nbad counted when the id or the label is out
// of range (ids < 0 are empty slots: -1, not counted). The label of an id past
// the table is never read.
__device__ __forceinline__ int label_of(int64_t it, const int32_t* __restrict__ labels,
                                        int64_t n_items, int G, int& nbad) {
  if (it < 0) return -1;
  if (it < n_items) {
    const int lab = labels[it];
    if ((unsigned)lab < (unsigned)G) return lab;
  }
  ++nbad;
  return -1;
}

__global__ __launch_bounds__(kThreads) void calib_pick_kernel(
    const int32_t* __restrict__ cand_items, const float* __restrict__ cand_scores, int C,
    const int32_t* __restrict__ labels, int64_t n_items, int G, const float* __restrict__ profile,
    int64_t n_users, int k_out, float lambda, int32_t* __restrict__ out_items,
    float* __restrict__ out_kl, int32_t* __restrict__ err) {
  __shared__ uint16_t s_pos[kWaves][kMaxC];  // the picks' positions, in pick order
  __shared__ uint8_t s_lab[kWaves][kMaxC];   // label per position (read once per pick)
  __shared__ float s_inv[kMaxC];             // 1 / (t + 1), the same for every user
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t n_waves = (int64_t)gridDim.x * kWaves;
  const float mu = 1.f - lambda;
  for (int i = threadIdx.x; i < k_out; i += kThreads) s_inv[i] = 1.f / (float)(i + 1);
  __syncthreads();  // the only workgroup barrier: from here on a wave is on its own

  for (int64_t u = (int64_t)blockIdx.x * kWaves + w; u < n_users; u += n_waves) {
    const float p = profile_entry(profile + u * G, G, lane);
    const float logp = p > 0.f ? logf(p) : 0.f;
    const int32_t* items = cand_items + u * C;
    const float* scores = cand_scores + u * C;

    // ids, then labels and scores, as three batches of independent loads (an
    // index that must not be read is replaced by one that may: entry C - 1,
    // label 0; n_items >= 1)
    int32_t it[kPer];
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
      const int pos = j * 64 + lane;
      const int32_t id = items[pos < C ? pos : C - 1];
      it[j] = pos < C ? id : -1;
    }
    float ls[kPer];  // lambda * score; -inf: not live (any more)
    int la[kPer];    // label << 2: the byte address ds_bpermute reads the gain from
    int nbad = 0;
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
      const int pos = j * 64 + lane;
      const bool inside = it[j] >= 0 && (int64_t)it[j] < n_items;
      const int lab = labels[inside ? it[j] : 0];
      const float sc = scores[pos < C ? pos : C - 1];
      const bool live = inside && (unsigned)lab < (unsigned)G;
      nbad += (it[j] >= 0 && !live) ? 1 : 0;
      // a live candidate's value stays above -inf: -inf and NaN scores count as -FLT_MAX
      ls[j] = live ? lambda * fmaxf(sc, -FLT_MAX) : -INFINITY;
      la[j] = (live ? lab : 0) << 2;
      s_lab[w][pos] = (uint8_t)(live ? lab : 0);
    }
    if (nbad && err) atomicAdd(err, nbad);
    dr::wave_lds_sync();

    float cnt = 0.f;  // n_g of this lane's category (an exact integer)
    float kl = 0.f;   // KL(p || q~) of the list as it stands
    int t = 0;
    for (; t < k_out; ++t) {
      const float inv = s_inv[t];
      const float a = kl_term(p, logp, cnt * inv);
      const float b = kl_term(p, logp, (cnt + 1.f) * inv);
      const float base = dr::wave_sum_dpp_f32(a);
      if (t == 0) kl = base;  // n = 0: the empty list's KL, whatever the divisor
      const float klc = (base - a) + b;  // the list with one more of category `lane`
      const int gain = __float_as_int(-(mu * klc));

      float g[kPer];  // all 16 cross-lane reads in flight before the first is used
#pragma unroll
      for (int j = 0; j < kPer; ++j)
        g[j] = __int_as_float(__builtin_amdgcn_ds_bpermute(la[j], gain));
      float best = -INFINITY;
      int bj = 0;
#pragma unroll
      for (int j = 0; j < kPer; ++j) {
        const float v = ls[j] + g[j];
        const bool take = v > best;  // strict: the lowest of a lane's equal positions stays
        best = take ? v : best;
        bj = take ? j : bj;
      }
      // wave argmax in two 32-bit DPP reductions: the best value's order key
      // (0: no live candidate; a live one never maps to 0), then the lowest
      // position among the lanes that hold it
      const uint32_t ord = best > -INFINITY ? dr::f32_to_ord(best) : 0u;
      const uint32_t top = dr::wmax_u32<64>(ord);
      if (top == 0u) break;  // no live candidate left: the list ends here
      const int pc = (int)dr::wave_min_u32_64(ord == top ? (uint32_t)(bj * 64 + lane) : ~0u);
      const int off = pc - lane;
#pragma unroll
      for (int j = 0; j < kPer; ++j) ls[j] = off == j * 64 ? -INFINITY : ls[j];
      const int c = __builtin_amdgcn_readfirstlane((int)s_lab[w][pc]);
      kl = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(klc), c));
      cnt += lane == c ? 1.f : 0.f;
      if (lane == 0) {
        s_pos[w][t] = (uint16_t)pc;
        if (out_kl) out_kl[u * k_out + t] = kl;
      }
    }
    dr::wave_lds_sync();
    // picks [0, t) by position; the rest -1, with the KL of the list as it stands
    for (int i = lane; i < k_out; i += 64) {
      out_items[u * k_out + i] = i < t ? items[s_pos[w][i]] : -1;
      if (i >= t && out_kl) out_kl[u * k_out + i] = kl;
    }
    dr::wave_lds_sync();  // the next user overwrites s_lab / s_pos
  }
}

// A wave's label histogram of the ids id(i), i = first + lane, + 64, ... < end,
// in its LDS row hist[kMaxG]: n is this lane's category's count,
// total the count of all labelled ids (every lane). An id or a label out of
// range is counted into *err; a negative id too where NEG_IS_BAD (a history
// has no empty slots), elsewhere it is an empty slot. The caller syncs the
// wave (wave_lds_sync) before its next call.
struct LabelCount { int n, total; };
template <bool NEG_IS_BAD, typename Idx, typename IdAt>
__device__ __forceinline__ LabelCount label_histogram(int* hist, int lane, Idx first, Idx end,
                                                      IdAt id, const int32_t* labels,
                                                      int64_t n_items, int G, int32_t* err) {
  hist[lane] = 0;
  dr::wave_lds_sync();
  int nbad = 0;
  for (Idx i = first + lane; i < end; i += 64) {
    const auto it = id(i);
    const int lab = label_of(it, labels, n_items, G, nbad);
    if (NEG_IS_BAD && it < 0) ++nbad;
    if (lab >= 0) atomicAdd(&hist[lab], 1);
  }
  if (nbad && err) atomicAdd(err, nbad);
  dr::wave_lds_sync();
  const int n = hist[lane];
  int total = n;
#pragma unroll
  for (int m = 32; m > 0; m >>= 1) total += __shfl_xor(total, m);
  return {n, total};
}

// One wave per CSR row: labels of the row's items counted into the wave's LDS
// histogram, then out[row, g] = n_g / total (one fp32 divide of two integers).
__global__ __launch_bounds__(kThreads) void label_profile_kernel(
    const int64_t* __restrict__ rowptr, const int32_t* __restrict__ items,
    const int32_t* __restrict__ labels, int64_t n_items, int G, int64_t n_rows,
    float* __restrict__ out, int32_t* __restrict__ err) {
  __shared__ int s_hist[kWaves][kMaxG];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t n_waves = (int64_t)gridDim.x * kWaves;
  for (int64_t r = (int64_t)blockIdx.x * kWaves + w; r < n_rows; r += n_waves) {
    const LabelCount c = label_histogram<true>(
        s_hist[w], lane, rowptr[r], rowptr[r + 1], [&](int64_t i) { return items[i]; }, labels,
        n_items, G, err);
    if (lane < G) out[r * G + lane] = c.total > 0 ? (float)c.n / (float)c.total : 0.f;
    dr::wave_lds_sync();
  }
}

// One wave per list: out[u] = KL(p || q~) with q the label shares of the
// list's valid entries (q = 0 for a list without any).
template <typename RecT>
__global__ __launch_bounds__(kThreads) void calibration_kl_kernel(
    const RecT* __restrict__ recs, int64_t n_users, int k, const int32_t* __restrict__ labels,
    int64_t n_items, int G, const float* __restrict__ profile, float* __restrict__ out,
    int32_t* __restrict__ err) {
  __shared__ int s_hist[kWaves][kMaxG];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t n_waves = (int64_t)gridDim.x * kWaves;
  for (int64_t u = (int64_t)blockIdx.x * kWaves + w; u < n_users; u += n_waves) {
    const LabelCount c = label_histogram<false>(
        s_hist[w], lane, 0, k, [&](int i) { return recs[u * k + i]; }, labels, n_items, G, err);
    const float p = profile_entry(profile + u * G, G, lane);
    const float logp = p > 0.f ? logf(p) : 0.f;
    const float inv = c.total > 0 ? 1.f / (float)c.total : 0.f;
    const float kl = dr::wave_sum_dpp_f32(kl_term(p, logp, (float)c.n * inv));
    if (lane == 0) out[u] = kl;
    dr::wave_lds_sync();
  }
}

// dr::persistent_grid of one-wave workers, each wave looping over the units
// (users, rows); 4 workgroups per CU if the occupancy query fails.
template <typename Kernel>
dim3 wave_grid(Kernel kernel, int64_t units) {
  return dr::persistent_grid(kernel, kThreads, dr::ceil_div(units, kWaves), 4);
}

// The label-table arguments the three calls share.
int check_labels(const char* fn, int64_t n_items, int G) {
  if (G > kMaxG) {
    dr::set_error(std::string(fn) + ": G must be <= 64");
    return DR_EUNSUPPORTED;
  }
  if (G < 1 || n_items < 0 || n_items >= 0x7fffffffLL) {
    dr::set_error(std::string(fn) + ": G must be >= 1 and n_items in [0, 2^31)");
    return DR_EINVAL;
  }
  if (n_items == 0) {
    dr::set_error(std::string(fn) + ": empty label table");
    return DR_EINVAL;
  }
  return DR_OK;
}

}  // namespace

extern "C" int dr_calibrated_rerank(const int32_t* cand_items, const float* cand_scores,
                                    int64_t n_users, int C, const int32_t* item_labels,
                                    int64_t n_items, int G, const float* profile, int k_out,
                                    float lambda, int32_t* out_items, float* out_kl, int32_t* err,
                                    dr_stream_t stream) {
  static_assert(kMaxC == dr::kRerankMaxC, "the shared check's bound");
  DR_CHECK_RC(
      dr::check_candidates(__func__, n_users, C, k_out, lambda, dr::kCalibratedArgs));
  DR_CHECK_RC(check_labels(__func__, n_items, G));
  if (n_users == 0) return DR_OK;
  DR_CHECK_ARG(cand_items && cand_scores && item_labels && profile && out_items, "null pointer");
  hipLaunchKernelGGL(calib_pick_kernel, wave_grid(calib_pick_kernel, n_users), dim3(kThreads), 0,
                     (hipStream_t)stream, cand_items, cand_scores, C, item_labels, n_items, G,
                     profile, n_users, k_out, lambda, out_items, out_kl, err);
  DR_CHECK_LAUNCH();
  return DR_OK;
}

extern "C" int dr_label_profile(const int64_t* rowptr, const int32_t* items, int64_t n_rows,
                                const int32_t* item_labels, int64_t n_items, int G, float* out,
                                int32_t* err, dr_stream_t stream) {
  DR_CHECK_ARG(n_rows >= 0, "n_rows must be >= 0");
  DR_CHECK_RC(check_labels(__func__, n_items, G));
  if (n_rows == 0) return DR_OK;
  DR_CHECK_ARG(rowptr && item_labels && out, "null pointer");  // items may be NULL: all rows empty
  hipLaunchKernelGGL(label_profile_kernel, wave_grid(label_profile_kernel, n_rows), dim3(kThreads), 0,
                     (hipStream_t)stream, rowptr, items, item_labels, n_items, G, n_rows, out, err);
  DR_CHECK_LAUNCH();
  return DR_OK;
}

extern "C" int dr_calibration_kl(const void* recs, int rec_dtype, int64_t n_users, int k,
                                 const int32_t* item_labels, int64_t n_items, int G,
                                 const float* profile, float* out, int32_t* err,
                                 dr_stream_t stream) {
  DR_CHECK_ARG(n_users >= 0 && k >= 0, "n_users and k must be >= 0");
  DR_CHECK_ARG(rec_dtype == DR_I32 || rec_dtype == DR_I64, "recs must be DR_I32 or DR_I64");
  DR_CHECK_RC(check_labels(__func__, n_items, G));
  if (n_users == 0) return DR_OK;
  DR_CHECK_ARG((recs || k == 0) && item_labels && profile && out, "null pointer");
  hipStream_t s = (hipStream_t)stream;
  if (rec_dtype == DR_I32)
    hipLaunchKernelGGL(calibration_kl_kernel<int32_t>,
                       wave_grid(calibration_kl_kernel<int32_t>, n_users), dim3(kThreads), 0, s,
                       (const int32_t*)recs, n_users, k, item_labels, n_items, G, profile, out, err);
  else
    hipLaunchKernelGGL(calibration_kl_kernel<int64_t>,
                       wave_grid(calibration_kl_kernel<int64_t>, n_users), dim3(kThreads), 0, s,
                       (const int64_t*)recs, n_users, k, item_labels, n_items, G, profile, out, err);
  DR_CHECK_LAUNCH();
  return DR_OK;
}
