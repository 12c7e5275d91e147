// xQuAD aspect-aware re-rank over a multi-hot item-aspect matrix (Santos,
// Macdonald, Ounis, WWW 2010; Vargas & Castells, RecSys 2011): top-C candidates
// -> k_out picks per user, each pick maximising lambda * score + (1 - lambda) *
// sum_a m_a c_{i,a}, m the profile mass the list has not covered yet. There is
// no reference symbol; the spec is the build's own (include/divrec_hip.h).
// Beside it: the aspect profile of a history CSR (dr_aspect_profile) and the
// expected aspect coverage of finished lists (dr_aspect_coverage).
//
// Layout: every candidate carries a row of G coverages, so a
// user's clamped C x G block lives in LDS, aspect-major with an odd row stride
// S = C | 1: a step reads one aspect across candidates (consecutive lanes,
// consecutive banks), and the prologue's row-wise gather writes a candidate's
// G aspects to G different banks. One 256-thread workgroup per user:
//   * candidate position j * 256 + thread (j < 4) is register j of the thread:
//     lambda * score (-inf once picked or never live) and the running
//     diversity term div = sum_a m_a c_a;
//   * lane a < G of EVERY wave keeps m_a (four identical copies: no barrier
//     orders the update against the next step's reads).
// A step: each thread's best of four as a 64-bit key (value order key, then the
// lowest position), the wave's best in one DPP reduction (wave_max_u64), four
// partials through LDS and one barrier that waits for LDS alone.
// Then the pick's row is read across lanes, and each aspect it covers
// (c_pick,a != 0: a wave-uniform loop over a ballot) takes delta_a = m_a c_pick,a
// off m_a and delta_a c_{i,a} off every div_i: with genre-like rows that is one
// to three of the G columns, not the C x G dot product again.
// Every product and sum below is a separate fp32 operation (contraction off):
// tests/xquad_checks.py restates them one by one.
#include <float.h>

#include "common.h"
#include "rerank_args.h"

namespace {

constexpr int kWaves = 4;
constexpr int kThreads = kWaves * 64;
constexpr int kPer = 4;                 // candidates per thread
constexpr int kMaxC = kPer * kThreads;  // 1024
constexpr int kMaxG = DR_XQUAD_MAX_ASPECTS;
constexpr int kGather = 8;    // row elements in flight per lane and group of 64 (prologue)
constexpr int kRowBatch = 8;  // rows in flight per wave in the two small kernels
static_assert(kMaxG == 64, "one lane per aspect");

// The user block's LDS cells G * (C | 1), in three kernel instances: four, two
// and one workgroup per CU beside their 64 B of partials (160 KiB of LDS).
constexpr int kCellsSmall = 8256, kCellsMid = 19968;
constexpr int kCellsMax = DR_XQUAD_MAX_CELLS + kMaxG;  // C * G + G >= G * (C | 1)
static_assert(4 * (kCellsSmall * 4 + 64) <= 163840 && 2 * (kCellsMid * 4 + 64) <= 163840 &&
                  kCellsMax * 4 + 64 <= 163840, "LDS budget");

__device__ __forceinline__ float clamp01(float x) {  // NaN -> 0 (fmaxf keeps the number)
  return fminf(fmaxf(x, 0.f), 1.f);
}

template <int CELLS>
__global__ __launch_bounds__(kThreads) void xquad_pick_kernel(
    const int32_t* __restrict__ cand_items, const float* __restrict__ cand_scores, int C,
    const float* __restrict__ aspects, int64_t n_items, int G, const float* __restrict__ profile,
    int64_t n_users, int k_out, float lambda, int32_t* __restrict__ out_items,
    float* __restrict__ out_cov, int32_t* __restrict__ err) {
#pragma clang fp contract(off)
  __shared__ float s_c[CELLS];           // c[a * S + position], clamped; 0 where not live
  __shared__ uint64_t s_key[2][kWaves];  // the waves' best keys, by step parity
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int S = C | 1;
  const float mu = 1.f - lambda;
  // the gather's walk over a group of 64 candidates' rows, element e = lane +
  // 64 i of the 64 x G block: candidate e / G, aspect e % G, advanced by 64
  const int cw0 = lane / G, a0 = lane - cw0 * G;
  const int step_c = 64 / G, step_a = 64 - step_c * G;
  int pj[kPer];  // this thread's positions, clamped into the list for LDS reads
#pragma unroll
  for (int j = 0; j < kPer; ++j) pj[j] = min(j * kThreads + tid, C - 1);

  for (int64_t u = blockIdx.x; u < n_users; u += gridDim.x) {
    const float p = dr::profile_entry(profile + u * G, G, lane);
    const int32_t* items = cand_items + u * C;
    const float* scores = cand_scores + u * C;

    int32_t it[kPer];  // the id; -1: not live
    float ls[kPer];    // lambda * score; -inf: not live (any more)
    int nbad = 0;
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
      const bool in = j * kThreads + tid < C;
      const int32_t id = items[pj[j]];
      const float sc = scores[pj[j]];
      const bool past = in && (int64_t)id >= n_items;
      const bool live = in && id >= 0 && !past;
      nbad += past ? 1 : 0;
      it[j] = live ? id : -1;
      // a live candidate's value stays above -inf: -inf and NaN scores count as -FLT_MAX
      ls[j] = live ? lambda * fmaxf(sc, -FLT_MAX) : -INFINITY;
    }
    if (nbad && err) atomicAdd(err, nbad);

    // prologue: a wave gathers the rows of its own four groups of 64
    // candidates, G consecutive lanes on one row; the walk is the same in
    // every group, so kGather elements of all four are in flight at once (a
    // row that must not be read is replaced by row 0; n_items >= 1)
    int cw = cw0, a = a0;
    for (int i0 = 0; i0 < G; i0 += kGather) {
      float x[kPer][kGather];
      int at[kGather], cb[kGather];  // a * S + the candidate in its group; that candidate
#pragma unroll
      for (int b = 0; b < kGather; ++b) {
        const bool on = i0 + b < G;  // then cw < 64
        at[b] = a * S + cw;
        cb[b] = on ? cw : kMaxC;  // past every list
#pragma unroll
        for (int j = 0; j < kPer; ++j) {
          const int id = __shfl(it[j], cw & 63);
          const bool rd = on && id >= 0;  // -1 also past C: it[j] of such a position
          const float v = aspects[rd ? (int64_t)id * G + a : 0];
          x[j][b] = rd ? v : 0.f;
        }
        a += step_a, cw += step_c;
        if (a >= G) a -= G, ++cw;
      }
#pragma unroll
      for (int b = 0; b < kGather; ++b) {
#pragma unroll
        for (int j = 0; j < kPer; ++j) {
          const int base = j * kThreads + w * 64;
          if (base + cb[b] < C) s_c[at[b] + base] = clamp01(x[j][b]);
        }
      }
    }
    dr::lds_barrier();

    float m = p;  // lane a: the uncovered mass of aspect a
    float div[kPer] = {0.f, 0.f, 0.f, 0.f};
    for (int a = 0; a < G; ++a) {
      const float pa = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(p), a));
#pragma unroll
      for (int j = 0; j < kPer; ++j) div[j] = div[j] + pa * s_c[a * S + pj[j]];
    }

    float cov = 0.f;  // sum_a (p_a - m_a), as the sum of the steps' gains
    int t = 0;
    for (; t < k_out; ++t) {
      // a candidate's key: the value's order key above the complement of its
      // position, so the largest key is the highest value at the lowest
      // position; 0: not live (a live value never maps to order key 0)
      uint64_t key = 0ull;
#pragma unroll
      for (int j = 0; j < kPer; ++j) {
        const float v = ls[j] + mu * div[j];
        const uint64_t kj = ((uint64_t)dr::f32_to_ord(v) << 32) | (uint32_t)~(j * kThreads + tid);
        key = dr::umax64(key, v > -INFINITY ? kj : 0ull);
      }
      key = dr::wave_max_u64(key);
      if (lane == 0) s_key[t & 1][w] = key;
      dr::lds_barrier();  // the step's only barrier: the partials alternate by parity
      uint64_t gkey = 0ull;
#pragma unroll
      for (int i = 0; i < kWaves; ++i) gkey = dr::umax64(gkey, s_key[t & 1][i]);
      if (gkey == 0ull) break;  // no live candidate left: the list ends here (all threads agree)
      const int pick = __builtin_amdgcn_readfirstlane((int)~(uint32_t)gkey);
      if (tid == (pick & (kThreads - 1))) {  // the pick's owner
#pragma unroll
        for (int j = 0; j < kPer; ++j)
          if ((pick >> 8) == j) {
            out_items[u * k_out + t] = it[j];
            ls[j] = -INFINITY;
          }
      }
      // the pick's row across lanes; each aspect it covers, in aspect order
      const float cp = lane < G ? s_c[lane * S + pick] : 0.f;
      const float delta = m * cp;
      m = m - delta;
      uint64_t covers = __ballot(cp != 0.f);
      while (covers) {
        const int a = __builtin_ctzll(covers);
        covers &= covers - 1;
        const float da = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(delta), a));
        cov = cov + da;
#pragma unroll
        for (int j = 0; j < kPer; ++j) div[j] = div[j] - da * s_c[a * S + pj[j]];
      }
      if (tid == 0 && out_cov) out_cov[u * k_out + t] = cov;
    }
    // picks [0, t) are written; the rest -1, with the coverage of the list as it stands
    for (int i = t + tid; i < k_out; i += kThreads) {
      out_items[u * k_out + i] = -1;
      if (out_cov) out_cov[u * k_out + i] = cov;
    }
    dr::lds_barrier();  // the next user overwrites s_c and the partials
  }
}

// The clamped aspect rows of the ids id(i), i in [first, end), of one wave:
// use(c) is called once per valid id, in order, lane a < G holding c_{id,a}
// (lanes >= G hold column 0's and are the caller's to ignore). 64 ids are
// loaded at a time, kRowBatch rows are in flight. An id >= n_items is skipped
// and counted into *err; a negative id too where NEG_IS_BAD (a history has no
// empty slots), elsewhere it is an empty slot.
template <bool NEG_IS_BAD, typename Idx, typename IdAt, typename Use>
__device__ __forceinline__ void for_each_aspect_row(int lane, Idx first, Idx end, IdAt id,
                                                    const float* __restrict__ aspects,
                                                    int64_t n_items, int G, int32_t* err, Use use) {
  const int col = lane < G ? lane : 0;
  int nbad = 0;
  for (Idx base = first; base < end; base += 64) {
    const int n = (int)(end - base < 64 ? end - base : 64);
    const int64_t mine = lane < n ? (int64_t)id(base + lane) : -1;
    const bool ok = mine >= 0 && mine < n_items;
    nbad += (lane < n && !ok && (NEG_IS_BAD || mine >= 0)) ? 1 : 0;
    const int row = ok ? (int)mine : -1;
    for (int i0 = 0; i0 < n; i0 += kRowBatch) {  // i0 + b <= 63
      int r[kRowBatch];
      float x[kRowBatch];
#pragma unroll
      for (int b = 0; b < kRowBatch; ++b) {
        r[b] = __builtin_amdgcn_readlane(row, __builtin_amdgcn_readfirstlane(i0 + b));
        x[b] = aspects[(int64_t)(r[b] < 0 ? 0 : r[b]) * G + col];  // row 0 for a skipped id
      }
#pragma unroll
      for (int b = 0; b < kRowBatch; ++b)
        if (r[b] >= 0) use(clamp01(x[b]));  // wave-uniform
    }
  }
  if (nbad && err) atomicAdd(err, nbad);
}

// One wave per CSR row: lane a sums c_{i,a} in the row's order, one DPP tree
// over the aspects gives the denominator, one divide the value.
__global__ __launch_bounds__(kThreads) void aspect_profile_kernel(
    const int64_t* __restrict__ rowptr, const int32_t* __restrict__ items,
    const float* __restrict__ aspects, int64_t n_items, int G, int64_t n_rows,
    float* __restrict__ out, int32_t* __restrict__ err) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t n_waves = (int64_t)gridDim.x * kWaves;
  for (int64_t r = (int64_t)blockIdx.x * kWaves + w; r < n_rows; r += n_waves) {
    float acc = 0.f;
    for_each_aspect_row<true>(
        lane, rowptr[r], rowptr[r + 1], [&](int64_t i) { return items[i]; }, aspects, n_items, G,
        err, [&](float c) { acc = acc + c; });
    const float num = lane < G ? acc : 0.f;
    const float total = dr::wave_sum_dpp_f32(num);
    if (lane < G) out[r * G + lane] = total > 0.f ? num / total : 0.f;
  }
}

// One wave per list: lane a runs m_a <- m_a - m_a c_{j,a} over the list's valid
// entries (the re-rank's own update), out[u] = sum_a (p_a - m_a).
template <typename RecT>
__global__ __launch_bounds__(kThreads) void aspect_coverage_kernel(
    const RecT* __restrict__ recs, int64_t n_users, int k, const float* __restrict__ aspects,
    int64_t n_items, int G, const float* __restrict__ profile, float* __restrict__ out,
    int32_t* __restrict__ err) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t n_waves = (int64_t)gridDim.x * kWaves;
  for (int64_t u = (int64_t)blockIdx.x * kWaves + w; u < n_users; u += n_waves) {
    const float p = dr::profile_entry(profile + u * G, G, lane);
    float m = p;
    for_each_aspect_row<false>(
        lane, 0, k, [&](int i) { return recs[u * k + i]; }, aspects, n_items, G, err,
        [&](float c) { m = m - m * c; });
    const float cov = dr::wave_sum_dpp_f32(lane < G ? p - m : 0.f);
    if (lane == 0) out[u] = cov;
  }
}

// dr::persistent_grid of one-wave workers, each wave looping over the units
// (rows, lists); 8 workgroups per CU if the occupancy query fails.
template <typename Kernel>
dim3 wave_grid(Kernel kernel, int64_t units) {
  return dr::persistent_grid(kernel, kThreads, dr::ceil_div(units, kWaves), 8);
}

template <int CELLS>
void launch_pick(hipStream_t s, const int32_t* cand_items, const float* cand_scores, int C,
                 const float* aspects, int64_t n_items, int G, const float* profile,
                 int64_t n_users, int k_out, float lambda, int32_t* out_items, float* out_cov,
                 int32_t* err) {
  const dim3 grid = dr::persistent_grid(xquad_pick_kernel<CELLS>, kThreads, n_users,
                                        163840 / (CELLS * 4 + 64));
  hipLaunchKernelGGL(xquad_pick_kernel<CELLS>, grid, dim3(kThreads), 0, s, cand_items, cand_scores,
                     C, aspects, n_items, G, profile, n_users, k_out, lambda, out_items, out_cov,
                     err);
}

}  // namespace

extern "C" int dr_xquad_rerank(const int32_t* cand_items, const float* cand_scores, int64_t n_users,
                               int C, const float* item_aspects, int64_t n_items, int G,
                               const float* profile, int k_out, float lambda, int32_t* out_items,
                               float* out_cov, int32_t* err, dr_stream_t stream) {
  static_assert(kMaxC == dr::kRerankMaxC, "the shared check's bound");
  DR_CHECK_RC(dr::check_candidates(__func__, n_users, C, k_out, lambda, dr::kXquadArgs));
  DR_CHECK_RC(dr::check_aspects(__func__, n_items, G, C));
  if (n_users == 0) return DR_OK;
  DR_CHECK_RC(dr::check_aspects_filled(__func__, n_items));
  DR_CHECK_ARG(cand_items && cand_scores && item_aspects && profile && out_items, "null pointer");
  const int cells = G * (C | 1);  // <= kCellsMax by the checks above
  auto launch = cells <= kCellsSmall ? launch_pick<kCellsSmall>
                : cells <= kCellsMid ? launch_pick<kCellsMid>
                                     : launch_pick<kCellsMax>;
  launch((hipStream_t)stream, cand_items, cand_scores, C, item_aspects, n_items, G, profile,
         n_users, k_out, lambda, out_items, out_cov, err);
  DR_CHECK_LAUNCH();
  return DR_OK;
}

extern "C" int dr_aspect_profile(const int64_t* rowptr, const int32_t* items, int64_t n_rows,
                                 const float* item_aspects, int64_t n_items, int G, float* out,
                                 int32_t* err, dr_stream_t stream) {
  DR_CHECK_ARG(n_rows >= 0, "n_rows must be >= 0");
  DR_CHECK_RC(dr::check_aspects(__func__, n_items, G));
  if (n_rows == 0) return DR_OK;
  DR_CHECK_RC(dr::check_aspects_filled(__func__, n_items));
  DR_CHECK_ARG(rowptr && item_aspects && out, "null pointer");  // items may be NULL: all rows empty
  hipLaunchKernelGGL(aspect_profile_kernel, wave_grid(aspect_profile_kernel, n_rows),
                     dim3(kThreads), 0, (hipStream_t)stream, rowptr, items, item_aspects, n_items,
                     G, n_rows, out, err);
  DR_CHECK_LAUNCH();
  return DR_OK;
}

extern "C" int dr_aspect_coverage(const void* recs, int rec_dtype, int64_t n_users, int k,
                                  const float* item_aspects, int64_t n_items, int G,
                                  const float* profile, float* out, int32_t* err,
                                  dr_stream_t stream) {
  DR_CHECK_ARG(n_users >= 0 && k >= 0, "n_users and k must be >= 0");
  DR_CHECK_ARG(rec_dtype == DR_I32 || rec_dtype == DR_I64, "recs must be DR_I32 or DR_I64");
  DR_CHECK_RC(dr::check_aspects(__func__, n_items, G));
  if (n_users == 0) return DR_OK;
  DR_CHECK_RC(dr::check_aspects_filled(__func__, n_items));
  DR_CHECK_ARG((recs || k == 0) && item_aspects && profile && out, "null pointer");
  hipStream_t s = (hipStream_t)stream;
  if (rec_dtype == DR_I32)
    hipLaunchKernelGGL(aspect_coverage_kernel<int32_t>,
                       wave_grid(aspect_coverage_kernel<int32_t>, n_users), dim3(kThreads), 0, s,
                       (const int32_t*)recs, n_users, k, item_aspects, n_items, G, profile, out,
                       err);
  else
    hipLaunchKernelGGL(aspect_coverage_kernel<int64_t>,
                       wave_grid(aspect_coverage_kernel<int64_t>, n_users), dim3(kThreads), 0, s,
                       (const int64_t*)recs, n_users, k, item_aspects, n_items, G, profile, out,
                       err);
  DR_CHECK_LAUNCH();
  return DR_OK;
}
