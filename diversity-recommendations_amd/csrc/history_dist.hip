// Distance of list items from a user's own history through the item
// embeddings (unexpectedness / serendipity, Kaminskas & Bridge 2016):
//   dr_history_distance    out[u, p] = min | mean over h in H_u of 1 - cos(e_{r[u,p]}, e_h)
//   dr_serendipity_rerank  the k_out best of lambda * score + (1 - lambda) * dist,
//                          one register sort per user
//   dr_list_item_mean      per-list mean of a per-item value (novelty)
// There is no reference symbol; the spec is the build's own (include/divrec_hip.h).
//
// Layout: a cross Gram between two gathered row sets. The
// candidate side stays in registers: a wave owns a GROUP of TG candidate tiles
// of 32 rows (TG = 4, 4, 2, 1 at d = 32, 64, 128, 256: at most 64 VGPRs of
// fragments, so nothing spills) with 1/|e| of its column's
// row; the history streams past in 32-row tiles gathered through the cache
// (rows are read once from HBM per user; the other waves of the user and the
// later groups of a wave hit L2). A history tile is the A operand (rows), a
// candidate tile the B operand (columns), so a lane holds 16 history rows of
// ONE candidate: the reduction over the history runs down the lane's
// registers and ends with one exchange between the two half-waves. No LDS
// beyond 32 floats per wave (the history tile's 1/|e| by row), no workgroup
// barrier, no atomics on floats.
// One wave serves a user when C <= 128 (four users per workgroup); above, the
// four waves of a workgroup take the user's groups round-robin.
#include <float.h>
#include <type_traits>

#include "common.h"
#include "ild_tiles.h"
#include "rerank_args.h"

namespace {

using dr::bf16x8;
using dr::f32x16;

constexpr int kWaves = 4;
constexpr int kThreads = kWaves * 64;
constexpr int kMaxC = dr::kRerankMaxC;
constexpr int kWaveMaxC = 128;  // one wave per user up to here

// candidate tiles a wave keeps in registers (the macros are for A/B variant
// builds: build_native.py --variant NAME -D DR_HIST_TG128=2)
#ifndef DR_HIST_TG128
#define DR_HIST_TG128 2
#endif
#ifndef DR_HIST_TG256
#define DR_HIST_TG256 1
#endif
template <int D>
constexpr int tiles_per_group() { return D <= 64 ? 4 : D == 128 ? DR_HIST_TG128 : DR_HIST_TG256; }

// 1/|e| of row `col` of a tile, in every lane of that column (both
// half-waves), from the diagonal of the tile's Gram with itself; 0 for a row
// whose sum of squares is 0 (cosine 0 with every row).
template <int D>
__device__ __forceinline__ float tile_inv_norm(const bf16x8 (&x)[D / 16], int col, int h) {
  const f32x16 g = dr::gram_tile<D>(x, x);
  const int ri = dr::diag_reg(col);
  float v = g[0];
#pragma unroll
  for (int q = 1; q < 16; ++q) v = (ri == q) ? g[q] : v;
  const float other = __shfl_xor(v, 32);
  v = dr::diag_owner(col, h) ? v : other;
  return v > 0.f ? 1.f / sqrtf(v) : 0.f;
}

// The distances of one user's list positions in groups g_first, g_first +
// g_step, ... to dst[0, C) (global memory or LDS): the one device function
// behind both entry points. hist[0, hn) is the user's history row; w is the
// wave's 32 floats of LDS. Ids >= n_items of the wave's positions, and (where
// count_hist) history entries outside the table, are added to nbad by the
// lanes that saw them.
template <int D>
__device__ __forceinline__ void user_distances(const int32_t* __restrict__ list, int C,
                                               const __bf16* __restrict__ E, int64_t n_items,
                                               const int32_t* __restrict__ hist, int64_t hn,
                                               int reduce, int g_first, int g_step, float* dst,
                                               float* w, bool count_hist, int& nbad) {
  constexpr int KS = D / 16;
  constexpr int TG = tiles_per_group<D>();
  const int lane = dr::lane_id();
  const int h = lane >> 5, col = lane & 31;
  const int ngroups = (C + 32 * TG - 1) / (32 * TG);
  const int64_t nht = (hn + 31) / 32;

  for (int g = g_first; g < ngroups; g += g_step) {
    bf16x8 x[TG][KS];
    int32_t cid[TG];  // the id; -1: empty slot or past the list; -2: outside the table
    float wc[TG];
#pragma unroll
    for (int t = 0; t < TG; ++t) {
      const int p = 32 * (g * TG + t) + col;
      const int32_t id = p < C ? list[p] : -1;
      const bool past = (int64_t)id >= n_items;
      cid[t] = id < 0 ? -1 : past ? -2 : id;
      nbad += (past && h == 0) ? 1 : 0;
      dr::gather_row<D>(E, cid[t] >= 0 ? cid[t] : 0, h, x[t]);  // row 0 is never used: n_items >= 1
    }
#pragma unroll
    for (int t = 0; t < TG; ++t) wc[t] = tile_inv_norm<D>(x[t], col, h);

    float mn[TG];
    double sm[TG];
#pragma unroll
    for (int t = 0; t < TG; ++t) mn[t] = INFINITY, sm[t] = 0.0;
    int nvalid = 0;
    int32_t hid = col < hn ? hist[col] : -1;  // the next tile's entry, one tile ahead of its rows
    for (int64_t ht = 0; ht < nht; ++ht) {
      const int64_t e = 32 * ht + col;
      const bool in = e < hn;
      const bool ok = in && hid >= 0 && (int64_t)hid < n_items;
      const int32_t row = ok ? hid : 0;
      if (count_hist && g == g_first) nbad += (in && !ok && h == 0) ? 1 : 0;
      hid = e + 32 < hn ? hist[e + 32] : -1;
      const uint32_t vmask = (uint32_t)__ballot(ok);  // rows of the tile that count (lanes 0..31)
      if (vmask == 0u) continue;                      // wave-uniform: none of its rows is read
      nvalid += __popc(vmask);
      bf16x8 y[KS];
      dr::gather_row<D>(E, row, h, y);
      const float wy = tile_inv_norm<D>(y, col, h);
      dr::wave_lds_sync();  // the previous tile's reads of w are done
      if (h == 0) w[col] = wy;
      dr::wave_lds_sync();
      float wi[16];
      bool rv[16];
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        wi[q] = w[dr::tile_row(q, h)];
        rv[q] = (vmask >> dr::tile_row(q, h)) & 1u;
      }
#pragma unroll
      for (int t = 0; t < TG; ++t) {
        if (32 * (g * TG + t) < C) {  // wave-uniform
          // gm[q] = <history row tile_row(q, h), candidate col>
          const f32x16 gm = dr::gram_tile<D>(y, x[t]);
          if (reduce == DR_HIST_MIN) {
#pragma unroll
            for (int q = 0; q < 16; ++q) {
              const float dist = dr::pair_dist<DR_ILD_COSINE>(gm[q], wi[q], wc[t]);
              mn[t] = rv[q] ? fminf(mn[t], dist) : mn[t];
            }
          } else {
            float part = 0.f;  // <= 16 terms in fp32, the tile sums in double
#pragma unroll
            for (int q = 0; q < 16; ++q) {
              const float dist = dr::pair_dist<DR_ILD_COSINE>(gm[q], wi[q], wc[t]);
              part += rv[q] ? dist : 0.f;
            }
            sm[t] += (double)part;
          }
        }
      }
    }
#pragma unroll
    for (int t = 0; t < TG; ++t) {
      float r;
      if (reduce == DR_HIST_MIN) {
        r = fminf(mn[t], __shfl_xor(mn[t], 32));
      } else {
        const double s = sm[t] + __shfl_xor(sm[t], 32);
        r = (float)(s / (double)(nvalid > 0 ? nvalid : 1));
      }
      if (nvalid == 0 || cid[t] == -1) r = 0.f;
      if (cid[t] == -2) r = __builtin_nanf("");
      const int p = 32 * (g * TG + t) + col;
      if (h == 0 && p < C) dst[p] = r;
    }
  }
}

__device__ __forceinline__ void add_errors(int nbad, int32_t* err) {
#pragma unroll
  for (int m = 32; m > 0; m >>= 1) nbad += __shfl_xor(nbad, m);
  if (nbad && err && dr::lane_id() == 0) atomicAdd(err, nbad);
}

// Workgroup b of the persistent loop serves users [b * upb, b * upb + upb):
// upb = 4 with one wave each (wpu = 1), or one user on four waves.
template <int D>
__global__ __launch_bounds__(kThreads, 2) void history_distance_kernel(
    const int32_t* __restrict__ lists, int64_t n_users, int C, const __bf16* __restrict__ E,
    int64_t n_items, const int64_t* __restrict__ rowptr, const int32_t* __restrict__ hist,
    int reduce, float* __restrict__ out, int32_t* __restrict__ err) {
  __shared__ float s_w[kWaves][32];
  const int wave = threadIdx.x >> 6;
  const int wpu = C <= kWaveMaxC ? 1 : kWaves;
  const int upb = kWaves / wpu;
  const int64_t nblocks = (n_users + upb - 1) / upb;
  int nbad = 0;
  for (int64_t b = blockIdx.x; b < nblocks; b += gridDim.x) {
    const int64_t u = b * upb + (wpu == 1 ? wave : 0);
    if (u >= n_users) continue;  // wave-uniform; the kernel has no workgroup barrier
    const int64_t h0 = rowptr[u], h1 = rowptr[u + 1];
    const int gw = wpu == 1 ? 0 : wave;
    user_distances<D>(lists + u * C, C, E, n_items, hist + h0, h1 > h0 ? h1 - h0 : 0, reduce, gw,
                      wpu, out + u * C, s_w[wave], gw == 0, nbad);
  }
  add_errors(nbad, err);
}

// value = lambda * score + (1 - lambda) * dist: two multiplies and one add
__device__ __forceinline__ float blend(float lambda, float mu, float score, float dist) {
#pragma clang fp contract(off)
  const float a = lambda * fmaxf(score, -FLT_MAX);  // -inf and NaN count as -FLT_MAX
  const float b = mu * dist;
  return a + b;
}

// P keys per lane: P = 2 is one wave per user (C <= 128, four users per
// workgroup, no workgroup barrier), P = 16 one workgroup per user whose wave 0
// sorts the 1024 keys.
template <int D, int P>
__global__ __launch_bounds__(kThreads, 2) void serendipity_rerank_kernel(
    const int32_t* __restrict__ cand_items, const float* __restrict__ cand_scores, int64_t n_users,
    int C, const __bf16* __restrict__ E, int64_t n_items, const int64_t* __restrict__ rowptr,
    const int32_t* __restrict__ hist, int reduce, int k_out, float lambda,
    int32_t* __restrict__ out_items, float* __restrict__ out_dist, int32_t* __restrict__ err) {
  constexpr int WPU = P == 2 ? 1 : kWaves;
  constexpr int UPB = kWaves / WPU;
  constexpr int NKEY = 64 * P;
  static_assert((WPU == 1 && NKEY == kWaveMaxC) || (WPU == kWaves && NKEY == kMaxC), "key count");
  __shared__ float s_w[kWaves][32];
  __shared__ float s_dist[UPB][NKEY];
  const int lane = dr::lane_id();
  const int wave = threadIdx.x >> 6;
  const float mu = 1.f - lambda;
  const int64_t nblocks = (n_users + UPB - 1) / UPB;
  int nbad = 0;
  for (int64_t b = blockIdx.x; b < nblocks; b += gridDim.x) {
    const int64_t u = b * UPB + (WPU == 1 ? wave : 0);
    const bool have = u < n_users;  // workgroup-uniform where WPU > 1
    float* dist = s_dist[WPU == 1 ? wave : 0];
    if (have) {
      const int64_t h0 = rowptr[u], h1 = rowptr[u + 1];
      const int gw = WPU == 1 ? 0 : wave;
      user_distances<D>(cand_items + u * C, C, E, n_items, hist + h0, h1 > h0 ? h1 - h0 : 0, reduce,
                        gw, WPU, dist, s_w[wave], gw == 0, nbad);
    }
    if constexpr (WPU == 1) dr::wave_lds_sync();
    else __syncthreads();
    if (have && (WPU == 1 || wave == 0)) {
      const int32_t* items = cand_items + u * C;
      const float* scores = cand_scores + u * C;
      // key: the value's order key above the complement of the position, so
      // descending keys are descending values, ties at the lowest position
      // first; 0: not live (a live value never maps to order key 0)
      uint64_t key[P];
#pragma unroll
      for (int i = 0; i < P; ++i) {
        const int pos = lane * P + i;
        const int32_t id = pos < C ? items[pos] : -1;
        const bool live = id >= 0 && (int64_t)id < n_items;
        const float sc = pos < C ? scores[pos] : 0.f;
        const float v = blend(lambda, mu, sc, live ? dist[pos] : 0.f);
        key[i] = live ? dr::make_key(v, (uint32_t)pos) : 0ull;
      }
      dr::wave_sort_desc<P>(key);
#pragma unroll
      for (int i = 0; i < P; ++i) {
        const int e = lane * P + i;
        if (e < k_out) {
          const bool got = key[i] != 0ull;
          const int pos = got ? (int)dr::key_item(key[i]) : 0;
          out_items[u * k_out + e] = got ? items[pos] : -1;
          if (out_dist) out_dist[u * k_out + e] = got ? dist[pos] : 0.f;
        }
      }
    }
    // the next user's distances overwrite s_dist
    if constexpr (WPU == 1) dr::wave_lds_sync();
    else __syncthreads();
  }
  add_errors(nbad, err);
}

// One wave per list: 64 entries are read at a time (coalesced) and their
// values gathered together, then added lane by lane, so the fp32 sum runs in
// position order and is reproducible (a skipped entry adds nothing).
template <typename R>
__global__ __launch_bounds__(kThreads) void list_item_mean_kernel(
    const R* __restrict__ recs, int64_t n_users, int k, const float* __restrict__ values,
    int64_t n_items, float* __restrict__ out, int32_t* __restrict__ err) {
  const int lane = dr::lane_id();
  const int64_t n_waves = (int64_t)gridDim.x * kWaves;
  int nbad = 0;
  for (int64_t u = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6); u < n_users; u += n_waves) {
    float sum = 0.f;
    int n = 0;
    for (int base = 0; base < k; base += 64) {
      const int p = base + lane;
      const int64_t id = p < k ? (int64_t)recs[u * k + p] : -1;
      const bool ok = id >= 0 && id < n_items;
      nbad += (id >= n_items) ? 1 : 0;
      const float v = ok ? values[id] : 0.f;
      uint64_t live = __ballot(ok);
      n += __popcll(live);
      while (live) {  // wave-uniform: the valid entries in position order
        const int l = __builtin_ctzll(live);
        live &= live - 1;
        sum += __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l));
      }
    }
    if (lane == 0) out[u] = n ? sum / (float)n : 0.f;
  }
  add_errors(nbad, err);
}

// Host side: f(std::integral_constant<int, D>{}) for the width that has a kernel.
template <class F>
bool for_width(int d, F&& f) {
  switch (d) {
    case 32: f(std::integral_constant<int, 32>{}); return true;
    case 64: f(std::integral_constant<int, 64>{}); return true;
    case 128: f(std::integral_constant<int, 128>{}); return true;
    case 256: f(std::integral_constant<int, 256>{}); return true;
  }
  return false;
}

int check_history_args(const char* fn, int64_t n_users, int64_t n_items, int d, int reduce) {
  if (n_users < 0) return dr::arg_error(fn, DR_EINVAL, "n_users must be >= 0");
  DR_CHECK_RC(dr::check_item_rows(fn, n_items));
  if (reduce != DR_HIST_MIN && reduce != DR_HIST_MEAN)
    return dr::arg_error(fn, DR_EINVAL, "reduce must be DR_HIST_MIN or DR_HIST_MEAN");
  if (d != 32 && d != 64 && d != 128 && d != 256)
    return dr::arg_error(fn, DR_EUNSUPPORTED, "d must be one of 32, 64, 128, 256");
  return DR_OK;
}

// the candidate rules of dr_serendipity_rerank: C in [1, 1024] (DR_EINVAL), k_out in [1, C]
constexpr dr::CandidateRules kSerendipityArgs{false, false, kMaxC};

}  // namespace

extern "C" int dr_history_distance(const int32_t* lists, int64_t n_users, int C,
                                   const void* item_table, int64_t n_items, int d,
                                   const int64_t* hist_rowptr, const int32_t* hist_items,
                                   int reduce, float* out, int32_t* err, dr_stream_t stream) {
  DR_CHECK_ARG(C >= 1 && C <= kMaxC, "C must be in [1, 1024]");
  DR_CHECK_RC(check_history_args(__func__, n_users, n_items, d, reduce));
  if (n_users == 0) return DR_OK;
  DR_CHECK_RC(dr::check_item_table_filled(__func__, n_items));
  DR_CHECK_ARG(lists && item_table && hist_rowptr && out, "null pointer");  // hist_items may be NULL: all rows empty
  const int upb = C <= kWaveMaxC ? kWaves : 1;
  for_width(d, [&](auto D) {
    const auto kernel = history_distance_kernel<D>;
    const dim3 grid = dr::persistent_grid(kernel, kThreads, dr::ceil_div(n_users, upb), 2);
    hipLaunchKernelGGL(kernel, grid, dim3(kThreads), 0, (hipStream_t)stream, lists, n_users, C,
                       (const __bf16*)item_table, n_items, hist_rowptr, hist_items, reduce, out,
                       err);
  });
  DR_CHECK_LAUNCH();
  return DR_OK;
}

extern "C" int dr_serendipity_rerank(const int32_t* cand_items, const float* cand_scores,
                                     int64_t n_users, int C, const void* item_table,
                                     int64_t n_items, int d, const int64_t* hist_rowptr,
                                     const int32_t* hist_items, int reduce, int k_out,
                                     float lambda, int32_t* out_items, float* out_dist,
                                     int32_t* err, dr_stream_t stream) {
  DR_CHECK_RC(dr::check_candidates(__func__, n_users, C, k_out, lambda, kSerendipityArgs));
  DR_CHECK_RC(check_history_args(__func__, n_users, n_items, d, reduce));
  if (n_users == 0) return DR_OK;
  DR_CHECK_RC(dr::check_item_table_filled(__func__, n_items));
  DR_CHECK_ARG(cand_items && cand_scores && item_table && hist_rowptr && out_items, "null pointer");
  for_width(d, [&](auto D) {
    const auto launch = [&](auto kernel, int upb) {
      const dim3 grid = dr::persistent_grid(kernel, kThreads, dr::ceil_div(n_users, upb), 2);
      hipLaunchKernelGGL(kernel, grid, dim3(kThreads), 0, (hipStream_t)stream, cand_items,
                         cand_scores, n_users, C, (const __bf16*)item_table, n_items, hist_rowptr,
                         hist_items, reduce, k_out, lambda, out_items, out_dist, err);
    };
    if (C <= kWaveMaxC) launch(serendipity_rerank_kernel<D, 2>, kWaves);
    else launch(serendipity_rerank_kernel<D, 16>, 1);
  });
  DR_CHECK_LAUNCH();
  return DR_OK;
}

extern "C" int dr_list_item_mean(const void* recs, int rec_dtype, int64_t n_users, int k,
                                 const float* item_values, int64_t n_items, float* out,
                                 int32_t* err, dr_stream_t stream) {
  DR_CHECK_ARG(n_users >= 0 && k >= 0, "n_users and k must be >= 0");
  DR_CHECK_ARG(rec_dtype == DR_I32 || rec_dtype == DR_I64, "recs must be DR_I32 or DR_I64");
  DR_CHECK_RC(dr::check_item_rows(__func__, n_items));
  if (n_users == 0) return DR_OK;
  DR_CHECK_ARG((recs || k == 0) && (item_values || n_items == 0) && out, "null pointer");
  const int64_t blocks = dr::ceil_div(n_users, kWaves);
  hipStream_t s = (hipStream_t)stream;
  if (rec_dtype == DR_I32)
    hipLaunchKernelGGL(list_item_mean_kernel<int32_t>,
                       dr::persistent_grid(list_item_mean_kernel<int32_t>, kThreads, blocks, 8),
                       dim3(kThreads), 0, s, (const int32_t*)recs, n_users, k, item_values, n_items,
                       out, err);
  else
    hipLaunchKernelGGL(list_item_mean_kernel<int64_t>,
                       dr::persistent_grid(list_item_mean_kernel<int64_t>, kThreads, blocks, 8),
                       dim3(kThreads), 0, s, (const int64_t*)recs, n_users, k, item_values, n_items,
                       out, err);
  DR_CHECK_LAUNCH();
  return DR_OK;
}
