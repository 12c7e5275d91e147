// Full-catalog user x item scoring with a fused top-K: the MI355X form of
// get_model_recommendations (reference divrec/train/utils.py:53-77), whose
// per-user loop scores every RankingDataset candidate (base_datasets.py:136-171)
// with MatrixFactorization.forward (matrix_factorization.py:26-28) and keeps
// candidates[argsort(scores, descending=True)][:k].
//
// Kernels:
// score_scan_kernel (score_scan.h; instantiated per table dtype in
//   score_scan_bf16.hip and score_scan_f32.hip) — the streaming MFMA scan with
//   the fused threshold top-k into per-user candidate buffers.
// topk_threshold_kernel — one wave per user: ks-th best key of the sample scan.
// topk_finalize_kernel — one wave per user: gather the candidates of all
//   chunks, drop excluded items, bitonic sort, write the k best.
// topk_merge_kernel / topk_merge_stream_kernel — merge sorted partial lists
//   (the exchange step of the item-sharded multi-GPU top-k).
//
// Keys encode (score desc, item asc) as one 64-bit unsigned order, so the
// result is a deterministic total order and any item partition (chunks,
// GPUs) gives bit-identical top-k lists.
#include <algorithm>
#include <cmath>
#include <cstdlib>

#include "score_scan_plan.h"

namespace {

using namespace dr_topk;

// ------------------------------------------------------------------ per-user gather
// Where a user's candidate buffers live (Plan / TopkArgs): every user has its
// chunk-0 buffer at row = its position; a user of a split tail block has
// chunks - 1 more at rows n_users_pad + (j - 1) * tail_pad + (u - head_users).
// kMaxTailChunks: the most buffers a user has (the planner's bound on a tail
// block's chunks, and the static bound of gather_candidates' unrolled loop).
constexpr int kMaxTailChunks = 16;

struct BufMap {
  int64_t n_users_pad;
  int64_t head_users;  // positions below this have one buffer
  int64_t tail_pad;    // users of the split tail blocks
  int chunks;          // buffers of a tail user
  __device__ int64_t row(int64_t u, int j) const {
    return j == 0 ? u : n_users_pad + (int64_t)(j - 1) * tail_pad + (u - head_users);
  }
  __device__ int n(int64_t u) const { return u < head_users ? 1 : chunks; }
};

BufMap buf_map(const Plan& p) {
  return BufMap{p.n_users_pad, p.head_users(), (p.n_ublocks - p.n_head) * p.users_per_wg,
                p.tail_chunks};
}

// Drop the keys of excluded items (sorted exclusion list of n items):
// lower_bound of every key's item by binary lifting, one runtime loop over the
// (uniform) steps around the unrolled per-key work, so key[] keeps static
// indices (P independent searches, each a loop of its own, left key[] in
// scratch at P >= 16).
template <int P>
__device__ __forceinline__ void drop_excluded(uint64_t (&key)[P], const int32_t* __restrict__ list,
                                              int n) {
  if (n <= 0) return;
  int lo[P];
#pragma unroll
  for (int i = 0; i < P; ++i) lo[i] = 0;
  int step = 1;
  while (2 * step <= n) step *= 2;
  for (; step > 0; step >>= 1) {
#pragma unroll
    for (int i = 0; i < P; ++i) {
      const int c = lo[i] + step;
      if (c <= n && list[c - 1] < (int32_t)dr::key_item(key[i])) lo[i] = c;
    }
  }
#pragma unroll
  for (int i = 0; i < P; ++i)
    if (key[i] != 0ull && lo[i] < n && list[lo[i]] == (int32_t)dr::key_item(key[i])) key[i] = 0ull;
}

// The k best of a sorted key array (element e = lane*P + i) to output row
// `row`, decoded; empty slots (key 0) as score -inf, item -1.
template <int P>
__device__ __forceinline__ void write_best(const uint64_t (&key)[P], int k,
                                           float* __restrict__ out_s, int32_t* __restrict__ out_i,
                                           int64_t row) {
  const int lane = dr::lane_id();
#pragma unroll
  for (int i = 0; i < P; ++i) {
    const int e = lane * P + i;
    if (e < k) {
      const bool empty = key[i] == 0ull;
      out_s[row * k + e] = empty ? -INFINITY : dr::key_score(key[i]);
      out_i[row * k + e] = empty ? -1 : (int32_t)dr::key_item(key[i]);
    }
  }
}

// A threshold strictly below score s, so that every score >= s passes the
// scan's `score > thr` test; -inf (no pruning) for NaN and infinite scores.
__device__ __forceinline__ float below_score(float s) {
  const float b = s - fmaxf(fabsf(s) * 0x1p-20f, 0x1p-100f);
  return b < s ? b : -INFINITY;
}

// The best 1024 of `total` streamed keys, sorted, in elements [0, 1024) of a
// 2048-key register array: load(x0, lane0) puts the keys at stream positions
// x0 + (lane - lane0) * 32 + i into key[i] of the lanes >= lane0 (0 past the
// end). Every round re-sorts the running best with the next 1024 keys, which
// enter elements [1024, 2048).
template <typename Load>
__device__ __forceinline__ void stream_best_1024(uint64_t (&key)[32], int64_t total, Load load) {
  load(0, 0);
  dr::wave_sort_desc<32>(key);
  for (int64_t next = 64 * 32; next < total; next += 32 * 32) {
    load(next, 32);
    dr::wave_sort_desc<32>(key);
  }
}

// One user's candidate keys of every buffer into registers (element e =
// lane*P + i), excluded items dropped; 0 = empty. The plan bounds the count
// by 64*P.
template <int P>
__device__ __forceinline__ void gather_candidates(const uint64_t* __restrict__ cand,
                                                  const int32_t* __restrict__ cnt, const BufMap m,
                                                  int cap, int64_t u,
                                                  const int64_t* __restrict__ excl_rowptr,
                                                  const int32_t* __restrict__ excl_items,
                                                  int64_t er, uint64_t (&key)[P]) {
  const int lane = dr::lane_id();
#pragma unroll
  for (int i = 0; i < P; ++i) key[i] = 0ull;
  const int nc = m.n(u);
  int off = 0;
  // chunk loop unrolled to its static bound so key[] stays in registers
#pragma unroll
  for (int c = 0; c < kMaxTailChunks; ++c) {
    if (c < nc) {
      const int64_t r = m.row(u, c);
      const int n = cnt[r];
      const uint64_t* src = cand + (size_t)r * cap;
#pragma unroll
      for (int i = 0; i < P; ++i) {
        const int e = lane * P + i;
        if (e >= off && e < off + n) key[i] = src[e - off];
      }
      off += n;
    }
  }
  if (excl_rowptr) {  // er: the user's exclusion row
    const int64_t e0 = excl_rowptr[er], e1 = excl_rowptr[er + 1];
    drop_excluded<P>(key, excl_items + e0, (int)(e1 - e0));
  }
}

// ------------------------------------------------------------------ finalize
// One wave per user of [u0, n_users): all its candidate buffers -> drop
// excluded items -> wave-wide register bitonic sort -> k best, decoded.
//   * Guessed-threshold scans (fail_cnt != NULL): a user left with fewer than
//     k keys may have lost items to a threshold guessed too high; it is
//     appended to the fail list (its user row and position) for the rescan.
//   * The rescan's finalize (pos_map != NULL): list entry u is written to the
//     caller's position pos_map[u]; the count comes from the device.
template <int P>
__global__ __launch_bounds__(256) void topk_finalize_kernel(
    const uint64_t* __restrict__ cand, const int32_t* __restrict__ cnt, const BufMap m, int cap,
    int64_t u0, int64_t n_users, int k, const int64_t* __restrict__ excl_rowptr,
    const int32_t* __restrict__ excl_items, float* __restrict__ out_s,
    int32_t* __restrict__ out_i, const int64_t* __restrict__ pos_map,
    const int32_t* __restrict__ n_users_dev, const int64_t* __restrict__ user_ids,
    int32_t* __restrict__ fail_cnt, int64_t* __restrict__ fail_rows,
    int64_t* __restrict__ fail_pos, const float* __restrict__ fail_thr_src,
    float* __restrict__ fail_thr) {
  const int lane = dr::lane_id();
  const int64_t u = u0 + (((int64_t)blockIdx.x * 256 + threadIdx.x) >> 6);
  if (n_users_dev) {
    const int64_t n = *n_users_dev;
    n_users = n < n_users ? n : n_users;
  }
  if (u >= n_users) return;  // wave-uniform
  const int64_t op = pos_map ? pos_map[u] : u;  // output and exclusion row
  uint64_t key[P];
  gather_candidates<P>(cand, cnt, m, cap, u, excl_rowptr, excl_items, op, key);
  dr::wave_sort_desc<P>(key);
  write_best<P>(key, k, out_s, out_i, op);
  if (fail_cnt && lane == (k - 1) / P && dr::select_key<P>(key, (k - 1) % P) == 0ull) {
    const int32_t f = atomicAdd(fail_cnt, 1);
    fail_rows[f] = user_ids ? user_ids[u] : u;
    fail_pos[f] = op;
    if (fail_thr) fail_thr[f] = fail_thr_src[u];  // the user's second-tier threshold
  }
}

// ------------------------------------------------------------------ second-tier finalize
// Users of a second-tier rescan (dev_split chunk plan, device count): one
// wave per user streams the keys of all its chunk buffers, any number of
// them, through a 2048-key register sort that keeps the running best 1024
// (elements [0, 1024)); new keys enter elements [1024, 2048). Excluded items
// are dropped, the k best written to the caller's position pos_map[u]; a user
// left with fewer than k keys (its second-tier threshold was still too high)
// goes to the third-tier list.
struct DevSplitArgs {
  int upwg, grid, max_c;
  int64_t buf_blocks, n_items, stage_items;
};

__global__ __launch_bounds__(256) void topk_finalize_stream_kernel(
    const uint64_t* __restrict__ cand, const int32_t* __restrict__ cnt, const DevSplitArgs dsa,
    int cap, int64_t n_users_max, int k, const int64_t* __restrict__ excl_rowptr,
    const int32_t* __restrict__ excl_items, float* __restrict__ out_s, int32_t* __restrict__ out_i,
    const int64_t* __restrict__ pos_map, const int32_t* __restrict__ n_users_dev,
    const int64_t* __restrict__ user_ids, int32_t* __restrict__ fail_cnt,
    int64_t* __restrict__ fail_rows, int64_t* __restrict__ fail_pos) {
  constexpr int P = 32;
  const int lane = dr::lane_id();
  const int64_t u = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 6;
  int64_t n = *n_users_dev;
  n = n < n_users_max ? n : n_users_max;
  if (u >= n) return;  // wave-uniform
  const int64_t nb = (n + dsa.upwg - 1) / dsa.upwg;
  const DevSplit ds = dev_split_plan(nb, dsa.grid, dsa.max_c, dsa.buf_blocks, dsa.n_items,
                                     dsa.stage_items);
  const int64_t rows_per_chunk = nb * dsa.upwg;  // chunk j of user u: row j * rows_per_chunk + u
  int64_t total = 0;
  for (int j = 0; j < ds.chunks; ++j) total += cnt[j * rows_per_chunk + u];
  const int64_t op = pos_map[u];
  const int32_t* ex = nullptr;
  int exn = 0;
  if (excl_rowptr) {
    ex = excl_items + excl_rowptr[op];
    exn = (int)(excl_rowptr[op + 1] - excl_rowptr[op]);
  }
  // keys at flat positions [x0, x0 + 64 * P) of the concatenated buffers into
  // elements e = lane * P + i with lane >= lane0
  uint64_t key[P];
#pragma unroll
  for (int i = 0; i < P; ++i) key[i] = 0ull;
  auto load = [&](int64_t x0, int lane0) {
    if (lane < lane0) return;
    uint64_t nk[P];
#pragma unroll
    for (int i = 0; i < P; ++i) nk[i] = 0ull;
    int64_t off = 0;
    for (int j = 0; j < ds.chunks; ++j) {
      const int64_t r = j * rows_per_chunk + u;
      const int64_t nj = cnt[r];
      const uint64_t* src = cand + (size_t)r * cap;
#pragma unroll
      for (int i = 0; i < P; ++i) {
        const int64_t x = x0 + (int64_t)(lane - lane0) * P + i;
        if (x >= off && x < off + nj) nk[i] = src[x - off];
      }
      off += nj;
    }
    drop_excluded<P>(nk, ex, exn);
#pragma unroll
    for (int i = 0; i < P; ++i) key[i] = nk[i];
  };
  stream_best_1024(key, total, load);
  write_best<P>(key, k, out_s, out_i, op);
  if (lane == (k - 1) / P && dr::select_key<P>(key, (k - 1) % P) == 0ull) {
    const int32_t f = atomicAdd(fail_cnt, 1);
    fail_rows[f] = user_ids[u];
    fail_pos[f] = op;
  }
}

// ------------------------------------------------------------------ threshold
// One wave per user position of [u0, u1) of the sample scan: the starting
// threshold of the main scan, strictly below the user's k-th best
// (non-excluded) sample score, so every score >= it passes the scan's
// `score > thr` test. -inf when the sample holds fewer than k candidates;
// +inf for padding positions (no user).
// thr[u] is taken at sample rank k1 (the first tier: the main scan's
// threshold), thr2[u] at rank k (the safe rank: a second-tier rescan's, for
// users whose first-tier guess fails); thr2 may be NULL.
template <int P>
__global__ __launch_bounds__(256) void topk_threshold_kernel(
    const uint64_t* __restrict__ cand, const int32_t* __restrict__ cnt, const BufMap m, int cap,
    int64_t u0, int64_t u1, int64_t n_users, int k, int k1, float* __restrict__ thr,
    float* __restrict__ thr2) {
  const int lane = dr::lane_id();
  const int64_t u = u0 + (((int64_t)blockIdx.x * 256 + threadIdx.x) >> 6);
  if (u >= u1) return;  // wave-uniform
  if (u >= n_users) {
    if (lane == 0) {
      thr[u] = INFINITY;
      if (thr2) thr2[u] = INFINITY;
    }
    return;
  }
  uint64_t key[P];
  gather_candidates<P>(cand, cnt, m, cap, u, nullptr, nullptr, u, key);
  dr::wave_sort_desc<P>(key);
  auto below_key = [](uint64_t kk) {  // an empty slot: fewer than that many candidates
    return kk != 0ull ? below_score(dr::key_score(kk)) : -INFINITY;
  };
  if (lane == (k1 - 1) / P) thr[u] = below_key(dr::select_key<P>(key, (k1 - 1) % P));
  if (thr2 && lane == (k - 1) / P) thr2[u] = below_key(dr::select_key<P>(key, (k - 1) % P));
}

// The same thresholds from the dense tile maxima of a gmax == 2 sample scan
// (TopkArgs::tmax): one THREAD per user position of [0, n_pad) streams its
// column ([user / 32][tile][user % 32]: a wave reads two 128-B lines per tile,
// 8 tiles in flight) into a descending register array of its KS best maxima.
// A maximum above the lane's cut (its KS-th best at the last merge) is
// appended to the lane's LDS list (kDenseBuf slots); when some lane's list
// could overflow, every lane merges its list through a branch-free insertion
// network, new[j] = max(old[j], min(old[j-1], v)) (2 VALU per entry), and
// raises its cut. Appends cost ~3 VALU per tile; merges run ~KS (1 + ln(T /
// KS)) / kDenseBuf times per wave instead of once per tile (the wave's lanes
// insert at different tiles: a per-tile network ran on nearly every tile).
// Values at or below the cut cannot change the KS-th order statistic. The
// k-th best tile maximum equals the k-th best key of the compaction path's
// buffer (same maxima, same rank), so the thresholds are bit-identical to it.
// NaN maxima (a tile whose 32 scores are all NaN) rank nothing: a lower bound
// either way. KS >= k >= k1.
constexpr int kDenseMaxKs = 72;
constexpr int kDenseBuf = 24;
constexpr double kDenseMaxGiB = 16.0;

template <int KS>
__global__ __launch_bounds__(256) void topk_threshold_dense_kernel(
    const float* __restrict__ tmax, int64_t T, int64_t n_pad, int64_t n_users, int k, int k1,
    float* __restrict__ thr, float* __restrict__ thr2) {
  constexpr int kIn = 8;
  static_assert(kDenseBuf >= kIn, "a merge leaves room for one batch");
  __shared__ float lst[4][kDenseBuf][64];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (__builtin_amdgcn_readfirstlane((int)(((int64_t)blockIdx.x * 256 + (threadIdx.x & ~63)) >= n_pad)))
    return;  // whole wave past the end
  const bool live = u < n_users;
  const float* src = tmax + (size_t)((live ? u : 0) >> 5) * (size_t)T * 32 + (u & 31);
  float best[KS];
#pragma unroll
  for (int j = 0; j < KS; ++j) best[j] = -INFINITY;
  float cut = -INFINITY;
  int n = 0;
  auto merge = [&]() {
    for (int i = 0; __builtin_amdgcn_ballot_w64(i < n) != 0ull; ++i) {
      const float v = i < n ? lst[wave][i][lane] : -INFINITY;
#pragma unroll
      for (int j = KS - 1; j > 0; --j) best[j] = fmaxf(best[j], fminf(best[j - 1], v));
      best[0] = fmaxf(best[0], v);
    }
    n = 0;
    cut = best[KS - 1];
  };
  auto add = [&](float v) {
    v = v == v ? v : -INFINITY;
    if (v > cut) lst[wave][n++][lane] = v;
  };
  int64_t t = 0;
  if (live) {
    for (; t + kIn <= T; t += kIn) {
      float v[kIn];
#pragma unroll
      for (int i = 0; i < kIn; ++i) v[i] = src[(size_t)(t + i) * 32];
#pragma unroll
      for (int i = 0; i < kIn; ++i) add(v[i]);
      if (__builtin_amdgcn_ballot_w64(n > kDenseBuf - kIn) != 0ull) merge();
    }
    for (; t < T; ++t) {
      add(src[(size_t)t * 32]);
      if (__builtin_amdgcn_ballot_w64(n >= kDenseBuf) != 0ull) merge();
    }
  }
  merge();
  if (u >= n_pad) return;
  if (!live) {
    thr[u] = INFINITY;
    if (thr2) thr2[u] = INFINITY;
    return;
  }
  float v1 = -INFINITY, v2 = -INFINITY;
#pragma unroll
  for (int j = 0; j < KS; ++j) {
    if (j == k1 - 1) v1 = best[j];
    if (j == k - 1) v2 = best[j];
  }
  thr[u] = below_score(v1);
  if (thr2) thr2[u] = below_score(v2);
}

// Launch topk_threshold_dense_kernel for ranks (k1, k) over positions [0, n_pad).
bool launch_threshold_dense(const float* tmax, int64_t T, int64_t n_pad, int64_t n_users, int k,
                            int k1, float* thr, float* thr2, hipStream_t s) {
  const dim3 grid((unsigned)dr::ceil_div(n_pad, 256));
  auto go = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, grid, dim3(256), 0, s, tmax, T, n_pad, n_users, k, k1, thr, thr2);
    return true;
  };
  if (k <= 8) return go(topk_threshold_dense_kernel<8>);
  if (k <= 16) return go(topk_threshold_dense_kernel<16>);
  if (k <= 24) return go(topk_threshold_dense_kernel<24>);
  if (k <= 32) return go(topk_threshold_dense_kernel<32>);
  if (k <= 48) return go(topk_threshold_dense_kernel<48>);
  if (k <= 72) return go(topk_threshold_dense_kernel<72>);
  return false;
}

// ------------------------------------------------------------------ merge
// One wave per user: gather parts*k_in (score, item) pairs, sort, keep k_out.
template <int P>
__global__ __launch_bounds__(256) void topk_merge_kernel(const float* __restrict__ in_s,
                                                         const int32_t* __restrict__ in_i,
                                                         int parts, int64_t n_users, int k_in,
                                                         int k_out, float* __restrict__ out_s,
                                                         int32_t* __restrict__ out_i) {
  const int lane = dr::lane_id();
  const int64_t u = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 6;
  if (u >= n_users) return;  // wave-uniform
  const int total = parts * k_in;
  uint64_t key[P];
#pragma unroll
  for (int i = 0; i < P; ++i) {
    const int e = lane * P + i;
    uint64_t kk = 0ull;
    if (e < total) {
      const int p = e / k_in, j = e % k_in;
      const size_t o = ((size_t)p * n_users + u) * k_in + j;
      const int32_t it = in_i[o];
      kk = it < 0 ? 0ull : dr::make_key(in_s[o], (uint32_t)it);
    }
    key[i] = kk;
  }
  dr::wave_sort_desc<P>(key);
  write_best<P>(key, k_out, out_s, out_i, u);
}

int p_for(int total) {
  for (int p = 2; p <= 32; p <<= 1)
    if (total <= 64 * p) return p;
  return -1;
}

// ------------------------------------------------------------------ planning
// Plans take w, the row width in bf16 units (d for bf16 tables, 2d for fp32).
// Workgroup slots = CUs (one 512-thread workgroup per CU). DR_KNOB_SCAN_SLOTS
// overrides the count so that tests can reach the split-tail plans with
// small inputs; the result is identical for any plan.
size_t al256(size_t x) { return (x + 255) & ~(size_t)255; }

int knob_int(int id, int fallback) {
  double v;
  return dr::plan_knob(id, &v) ? (int)v : fallback;
}

int scan_slots() {  // an override, not the cap of dr::persistent_cus() (common.h)
  const int slots = knob_int(DR_KNOB_SCAN_SLOTS, 0);
  return slots > 0 ? slots : dr::device_cus();
}

// Smallest candidate capacity that leaves at least 32 keys of headroom above
// k + kSlack once a stage's worth of new keys (the margin) is reserved.
int cap_for(int w, int k) {
  for (int cap = 512; cap <= 2048; cap <<= 1)
    if (k + kSlack + 32 <= cap - stage_items(w, cap)) return cap;
  return -1;
}

// Compaction slack and flush gap of the sample scan (ks <= ~70 keys per user).
constexpr int kSampleSlack = 32;
constexpr int kSampleGap = 96;
constexpr int kSampleGmax = 1;  // sample scans keep tile maxima (TopkArgs::gmax)
// The finalize of a split-tail user sorts every chunk's end-compacted keys
// (<= k + kSlack each) in one wave; at most 1024 of them keeps its sort at
// P = 16 (a 2048-key sort costs ~6x the 512-key one of a whole-catalog user).
constexpr int kMaxTailKeys = 1024;

// Grid tail: U users make B = ceil(U / UPWG) user blocks for `slots`
// workgroups. Whole-catalog units run in ceil(B / slots) rounds, the last one
// with B % slots of the CUs busy (1M users at d = 128: 977 blocks, the 4th
// round on 209 of 256 CUs, 4.6 % of the scan idle). The plan keeps
// H = floor(B / slots) * slots "head" blocks whole and splits each of the T
// tail blocks into c catalog chunks, c chosen to minimise
// H / slots + ceil(T c / slots) / c (in whole-unit times); the chunks'
// buffers are merged by the finalize. With B < slots, H = 0 and the chunks
// fill the idle CUs instead.
//
// Measured (tools/variant_bench.py, 1M users, d = 128, k = 100, lists
// identical; profiles/r02_scan/ab_split_*.json): the split gains less than the
// idle-CU count suggests, because the chip clocks up while a last round runs on
// fewer CUs: +0.7 % at 1.25M items (an 8-way shard), and at 10M items +1.5 %
// together with the seeding it needs (a chunk scanned from -inf pays its own
// survivor stream), which alone costs 1.1 % there at the 1/32 sample stride
// and breaks even at 1/128. So a head/tail split is planned only for
// catalogs the guess can seed (seedable); a grid smaller than the CU count
// (H = 0) is chunked in any case, as before.
// Small catalogs (round 6): with at most kKeepAllItems rows the candidate
// buffer is sized to hold every row (CAP >= n_items, at most 2048: the finalize
// sort's bound), so the scan never compacts (TopkArgs::keep_all) and the
// finalize sorts all keys. Config 1's 943 users x 1682 rows ran ONE
// workgroup whose waves compacted each user's buffer several times from -inf.
// Measured against the compacting plan (lists identical,
// profiles/r06/keep_all/): 943 x 1682 d = 32 3.40 -> 1.55 ms, d = 64 2.07 ->
// 1.56, 10K x 2000 k = 100 4.18 -> 2.07; config 1's whole evaluation step
// 9.09 -> 5.23 ms. The 2048-key finalize per user grows with the users
// (60K x 2048 k = 10: 2.35 -> 3.30 ms, break-even near 20K), so the rule
// takes calls of at most kKeepAllUsers users. Such calls have few user
// blocks, so their catalog is split into stage-long chunks over more CUs (no
// chunk compacts; the finalize gathers every chunk's keys): 943 x 1682 d = 64
// 1.55 -> 0.86 ms, 10K x 2000 k = 100 2.05 -> 1.10, config 1's step 3.17 ->
// 2.43 ms. Unseeded main scans only (the caller says so: allow_keep_all).
constexpr int64_t kKeepAllItems = 2048;
constexpr int64_t kKeepAllUsers = 16384;

Plan make_plan(int64_t n_users, int64_t n_items, int w, int k, bool seedable,
               bool allow_keep_all = false) {
  Plan p{};
  p.cap = cap_for(w, k);
  if (allow_keep_all && !seedable && p.cap > 0 && n_items <= kKeepAllItems &&
      n_users <= kKeepAllUsers && w <= 256) {  // CAP-2048 instances exist for w <= 256
    p.keep_all = 1;
    p.all_keys = n_items;
    while (p.cap < n_items) p.cap <<= 1;
  }
  p.users_per_wg = users_per_wg(w);
  p.n_ublocks = dr::ceil_div(n_users, p.users_per_wg);
  p.n_users_pad = p.n_ublocks * p.users_per_wg;
  const int64_t slots = scan_slots();
  const int64_t stage_items = dr_topk::stage_items(w, p.cap);
  int max_c_override = 0;
  const int64_t B = p.n_ublocks;
  const int64_t H = (B / slots) * slots;
  // each chunk stays long enough to amortise its start (B fragments, ring
  // fill) and its end compaction; a grid smaller than the CU count (H = 0)
  // may split down to 8192-row chunks: a catalog shorter than 2^17 rows
  // otherwise ran on one CU (1000 users x 100K items: 12.85 -> 4.24 ms).
  // Shorter chunks lose: every chunk compacts each of its users once at its
  // end (~0.9 ms per workgroup), which config 1's 1682-row catalog split in 3
  // paid (5.1 -> 6.0 ms).
  // keep-all plans (small catalogs, no compaction) split down to one stage
  // per chunk: no chunk pays an end compaction, and the few user blocks of
  // such a call would otherwise scan on as many CUs
  const int64_t min_chunk = p.keep_all ? stage_items
                          : H > 0 ? 65536 : std::max<int64_t>(stage_items, 8192);
  if (H > 0 && !seedable) max_c_override = 1;
  const int64_t T = B - H;
  int best_c = 1;
  double best = (double)H / slots + (double)dr::ceil_div(T, slots);
  int max_c = max_c_override > 0 ? max_c_override : kMaxTailChunks;
  if (const int c = knob_int(DR_KNOB_SCAN_SPLIT, 0); c > 0) max_c = c;  // A/B knob
  // a head user's finalize already sorts 2048 keys when its flush bound
  // passes 1024 (k >= ~800): the tail may then gather as many
  const int head_flush = std::min(k + kSlack + kFlushGap, p.cap - (int)stage_items);
  int max_keys = head_flush > kMaxTailKeys ? 2048 : kMaxTailKeys;
  if (const int m = knob_int(DR_KNOB_TAIL_KEYS, 0); m > 0) max_keys = m;  // A/B knob
  for (int c = 2; c <= max_c && T > 0; ++c) {
    if (n_items / c < min_chunk) break;
    if (!p.keep_all && c * k > max_keys) break;  // each chunk keeps at least k keys
    const double t = (double)H / slots + (double)dr::ceil_div(T * c, slots) / c;
    if (t < best * 0.99) {  // a smaller split unless a larger one gains > 1 %
      best = t;
      best_c = c;
    }
  }
  p.n_head = best_c > 1 ? H : B;
  p.tail_chunks = best_c;
  p.chunk_items = best_c > 1
      ? dr::ceil_div(dr::ceil_div(n_items, best_c), stage_items) * stage_items : n_items;
  p.chunk_floor = n_items;  // equal chunks (grade_tail_chunks)
  p.slack = kSlack;
  // Long lists: once k + kSlack + kFlushGap passes 1024 keys the head finalize
  // sorts 2048 keys anyway, so a buffer may fill to CAP - margin before its
  // first compaction at no finalize cost. A seeded k = 1000 scan admits ~1.5 k
  // survivors (the guess's rank): with the flush at k + 128 = 1128 every user
  // compacted a ~1.1K-key buffer 3-4 times in the last third of the catalog;
  // at CAP - margin = 1792 most users never compact.
  p.gap = head_flush > kMaxTailKeys ? p.cap - (int)stage_items - k - kSlack : kFlushGap;
  // a tail chunk ends with at most end_keep >= k keys, so c of them fit the
  // finalize's max_keys
  p.end_keep = best_c > 1 && !p.keep_all ? std::min(k + kSlack, max_keys / best_c) : 0;
  // Long lists (the flush bound above 1024 keys): every whole-catalog unit ends
  // with a compaction to at most kMaxTailKeys keys (slack kMaxTailKeys - k), so
  // the finalize sorts 1024 keys per user instead of 2048 (k = 1000: the
  // 2048-key sort cost ~24 ms per 1M users).
  p.head_keep = head_flush > kMaxTailKeys && k + 8 <= kMaxTailKeys ? kMaxTailKeys : 0;
  p.buf_rows = p.n_users_pad + (int64_t)(best_c - 1) * (B - p.n_head) * p.users_per_wg;
  const int64_t units = p.n_head + (B - p.n_head) * best_c;
  p.grid = (int)(units < slots ? units : slots);
  p.cand_bytes = (size_t)p.buf_rows * p.cap * sizeof(uint64_t);
  p.cnt_bytes = al256((size_t)p.buf_rows * sizeof(int32_t));
  return p;
}

// Graded tail chunks, for a scan whose workgroups claim their units from the
// queue (TopkArgs::unit_queue) and have more units than workgroups: the c
// chunks of a tail block halve from the first down to a floor
// (tail_chunk_bounds) instead of being equal, so the last units claimed are
// short and the CUs finish close together (1M x 10M: the last 418 of 2022
// units are 1/32 of the catalog, ~12 ms, instead of 1/6, ~67 ms). Same chunk
// count, buffer rows and end_keep; Plan::chunk_items stays the nominal equal
// length. Without the queue a workgroup's units are fixed (b, b + grid, ...):
// graded chunks would then make the workgroups' sums differ by up to half a
// catalog pass, so those scans keep equal chunks.
// The floor: every chunk ends by compacting all its users (~0.9 ms per
// workgroup), so chunks must stay long against that; never below the 2^16
// rows of the planner's own minimum chunk. DR_KNOB_SCAN_FLOOR overrides it
// (tests force one-stage chunks on small catalogs; a value >= n_items / c
// gives equal chunks). Chosen at 1M x 1.25M, k = 100 (9 rounds, one process,
// lists identical; profiles/scan_units/ab_shard_1250k.json): chunks of 625K,
// 312K and 4 x 78K rows 217.4 ms [217.1-217.9] against 220.6 [219.9-221.3] on
// the queue with six equal chunks of 208K (what a floor of 2^17 gives there)
// and 220.8 [220.1-222.3] for the static loop. At 1M x 10M (halving down to
// 312K rows) 1499.0 ms; a floor of 400 000 rows (1/2, 1/4, 1/8, 3 x 1/24)
// 1500.8, inside the spread.
constexpr int64_t kChunkFloor = 65536;

void grade_tail_chunks(Plan& p, int64_t n_items) {
  const int64_t units = p.n_head + (p.n_ublocks - p.n_head) * p.tail_chunks;
  if (p.tail_chunks <= 1 || units <= p.grid) return;
  double v;
  p.chunk_floor = dr::plan_knob(DR_KNOB_SCAN_FLOOR, &v) ? (int64_t)v : kChunkFloor;
}

// Largest candidate count the finalize of a head / split-tail user gathers.
// A whole-catalog buffer ends with at most flush_at keys (the scan compacts
// every buffer above flush_at = min(k + kSlack + kFlushGap, CAP - margin) at
// each stage end, the last included), so k = 100 sorts 256 keys, not CAP = 512
// (the sort instances start at 256 keys).
int flush_keys(const Plan& p, int w, int k) {
  // never compacted: every row's key (and rank k reached: every output slot written)
  if (p.keep_all) return (int)std::max<int64_t>(p.all_keys, k);
  const int f = k + p.slack + p.gap;
  const int m = p.cap - stage_items(w, p.cap);
  return f < m ? f : m;
}
int head_keys(const Plan& p, int w, int k) {
  const int n = p.head_keep > 0 ? p.head_keep : flush_keys(p, w, k);
  return n > 256 ? n : 256;
}
int tail_keys(const Plan& p, int w, int k) {
  if (p.tail_chunks <= 1) return head_keys(p, w, k);
  // keep-all chunks are never compacted (not even to head_keep): all their
  // keys, at most n_items <= 2048 over the chunks
  if (p.keep_all) return std::max(256, flush_keys(p, w, k));
  const int n = p.tail_chunks * p.end_keep;
  return n > 256 ? n : 256;
}

// Guessed thresholds, for catalogs of >= kGuessMinItems rows. A scan that
// starts at -inf stores every running top-k record of a user:
// ~k * (1 + ln(I / k)) keys, the survivor
// stream that dominates short catalogs (47 % of wave time at d=64 over 1M
// items). Instead a first scan over a strided sample of S = I / kGuessStride
// rows keeps each user's ks best, and the main scan starts from just below the
// ks-th best sample score. ks is the mean number of the user's true top k
// inside the sample plus kGuessSigma standard deviations (+3), so for
// exchangeable catalogs the guess is below the true k-th best score for all
// but ~1e-8 of users. The guess is verified, not trusted: the finalize
// appends every user left with fewer than k keys to a fail list, and those
// users are rescanned from -inf (device-side count, no host sync). Results are
// bit-identical to the plain scan in every case; a catalog whose sampled rows
// are unrepresentative only pays the rescan (one extra unit scan per 1024
// failing users). Used up to kGuessMaxItems rows (measured, 6-sigma margin:
// +14 % at d=64 over 1M items, +6 % at d=128 over 1.25M, +1.7 % over 5M,
// -0.3 to -0.8 % over 10M).
struct Guess {
  int64_t S = 0;       // sample rows (0 = plain scan)
  int64_t stride = 0;  // sample row i is slice row i * stride
  int ks = 0;          // safe rank of the guessed threshold in the sample (second tier)
  int ks1 = 0;         // first-tier rank (<= ks): the main scan's threshold
};

constexpr double kGuessSigma = 6.0;
// Two-tier guess (round 3): the main scan starts from the sample's
// ks1-th best score; the users it fails are rescanned from their safe
// (6-sigma) threshold by a second-tier scan spread over every CU, and the
// rare users that fail that too by the whole-catalog rescan from -inf.
// ks1 (round 5) is the smallest rank whose Poisson(mu) tail P(X >= ks1) is at
// most kGuessTail = 0.5 % (the share of users expected to fail it); the
// round-3 rule mu + 3 sigma + 1 had tails of 0.12-0.15 %. Measured with the
// z knob giving the same ranks (profiles/r05/ab19/, ab20/, lists identical):
// config 2 (ks1 10 -> 9) -1.05 %, d = 32 -2.7 %, an 8-way shard's 1.25M rows
// -0.8 %, k = 1000 (50 -> 48) -0.2 %; the headline keeps 5 (the 0.84 % tail
// of 4 measured +0.1 %).
int poisson_tail_rank(double mu, double tail) {
  double pmf = std::exp(-mu), cdf = 0.0;
  for (int j = 1; j < 4096; ++j) {
    cdf += pmf;                         // P(X <= j - 1)
    if (1.0 - cdf <= tail) return j;    // P(X >= j)
    pmf *= mu / (double)j;
  }
  return 4096;
}
constexpr double kGuessTail = 0.005;
// catalog chunks per user block of a second-tier rescan: 128 lets the usual
// one or two failing blocks fill the grid (round 6, 64 -> 128: the headline's
// rescan 6.8 -> ~3.9 ms, call -2.9 ms; k = 1000 -1.9 ms; lists identical,
// profiles/r06/rescan_chunks/)
constexpr int kMaxRescanChunks = 128;
constexpr int64_t kGuessStride = 32;
constexpr int64_t kGuessMinItems = 1 << 18;
constexpr int64_t kGuessMaxItems = 1ll << 23;  // measured: +1.7 % at 5M rows, -0.3 % at 10M
// Long lists pay a survivor stream of ~k (1 + ln(I / k)) keys per user from
// -inf (10K keys at k = 1000 over 10M items: 3.5x the k = 100 scan), which the
// guess removes at any catalog length.
constexpr int kGuessLongK = 256;

// A plan with a split tail is always seeded (from kGuessMinItems rows): an
// unseeded chunk pays the survivor stream of its own catalog part from -inf,
// ~c times the keys of one whole-catalog pass for its users.
Guess guess_for(int64_t n_items, int k, bool split_tail) {
  Guess g;
  if (n_items < kGuessMinItems) return g;
  const int force = knob_int(DR_KNOB_SCAN_SEED, -1);  // A/B knob: 0 never, 1 always
  if (force == 0) return g;
  if (n_items > kGuessMaxItems && k < kGuessLongK && !split_tail && force != 1) return g;
  // Long catalogs sample more sparsely: the sample scan starts from -inf and
  // is survivor-dense (~1.5x the per-row cost of the seeded scan), so about
  // 2^16 sample rows are kept (stride 32 up to 2^22 rows, 64 from 4.2M,
  // 128 from 8.4M). Measured with the split tail at 1M x 10M, d = 128:
  // stride 32 / 64 / 128 / 256 = 1912 / 1879 / 1873 / 1880 ms
  // (profiles/r02_scan/ab_stride_10m.json). Long lists too since round 6
  // (k = 1000 at 1M x 10M, lists identical, profiles/r06/k1000_stride/:
  // stride 32 / 64 / 128 = 1990.8 / 1971.8 / 1963.9 ms; 128 also puts the
  // sample on the dense tile-max path, 9.8 GB instead of 39 GB at 32).
  g.stride = kGuessStride;
  while (g.stride < 128 && n_items / (2 * g.stride) >= 65536) g.stride *= 2;
  if (const int st = knob_int(DR_KNOB_GUESS_STRIDE, 0); st > 1) g.stride = st;  // A/B knob
  // a whole number of 32-row tiles: the sample is stored tile-transposed
  // (sample_rows_kernel), and rows left out only lower the sample's order
  // statistics, so the guess stays a lower bound
  g.S = n_items / g.stride / kTileItems * kTileItems;
  const double mu = (double)k * (double)g.S / (double)n_items;
  int ks = (int)ceil(mu + kGuessSigma * sqrt(mu) + 3.0);
  g.ks = ks < k ? ks : k;
  int ks1 = poisson_tail_rank(mu, kGuessTail);
  double z1 = 3.0, c1 = 1.0;
  const bool zk = dr::plan_knob(DR_KNOB_GUESS_Z1, &z1);  // A/B knobs: the round-3 form
  const bool ck = dr::plan_knob(DR_KNOB_GUESS_C1, &c1);
  if (zk || ck) ks1 = (int)ceil(mu + z1 * sqrt(mu) + c1);
  if (ks1 < 1) ks1 = 1;
  if (knob_int(DR_KNOB_GUESS_TIGHT, 1) == 0) ks1 = g.ks;  // A/B knob: one tier (ks1 = ks)
  g.ks1 = ks1 < g.ks ? ks1 : g.ks;
  return g;
}

size_t diag_bytes() {
#ifdef DR_TOPK_DIAG
  return (size_t)scan_slots() * kWavesScan * kDgSlots * sizeof(uint64_t);
#else
  return 0;
#endif
}

// Workspace layout, 256-B aligned pieces:
//   [cand | cnt | thr (tier 1, tier 2) | sample rows | fail rows | fail positions |
//    fail thresholds | tier-2 fail rows | tier-2 fail positions | fail counts | diag].
// The sample scan, the main scan and the rescans run one after the other on
// the stream and share the candidate region.
// The sample scan keeps dense tile maxima (TopkArgs::gmax == 2) when its rank
// fits the dense threshold kernel and the [users][tiles] float matrix fits
// kDenseMaxGiB (it shares the candidate region: the main scan starts after
// the thresholds are read); else the compaction path (gmax == 1).
// DR_KNOB_SAMPLE_DENSE = 0 forces the compaction path (A/B and the
// bit-identity test of the two); a value > 1 is the budget in GiB.
bool sample_dense(int ks, int64_t n_users_pad, int64_t S) {
  double gib = kDenseMaxGiB;
  if (dr::plan_knob(DR_KNOB_SAMPLE_DENSE, &gib) && gib <= 0.0) return false;
  if (gib <= 1.0) gib = kDenseMaxGiB;  // 1: on, default budget
  return ks <= kDenseMaxKs && (double)n_users_pad * (double)(S / kTileItems) * 4.0 <= gib * 1073741824.0;
}
size_t dense_bytes(int64_t n_users_pad, int64_t S) {
  return (size_t)n_users_pad * (size_t)(S / kTileItems) * 4;
}

// The sample scan of the guessed thresholds, as dr_score_topk and
// dr_sample_thresholds both run it: S tile-transposed sample rows scanned from
// -inf for each user's ks best tile maxima.
struct SampleScan {
  Plan plan{};         // over the S rows at rank ks, compacted tighter (kSampleSlack / kSampleGap)
  int64_t S = 0;       // sample rows, whole tiles (0: no sample)
  int ks = 0;
  bool dense = false;  // dense tile maxima (gmax == 2) instead of the compaction path
  size_t cand_bytes = 0;  // what the scan needs of the candidate region
  int64_t tiles() const { return S / kTileItems; }
};

SampleScan sample_scan_for(int64_t n_users, int64_t S, int w, int ks) {
  SampleScan ss;
  ss.S = S;
  ss.ks = ks;
  if (S == 0) return ss;
  ss.plan = make_plan(n_users, S, w, ks, false);
  ss.plan.slack = kSampleSlack;
  ss.plan.gap = kSampleGap;
  ss.dense = sample_dense(ks, ss.plan.n_users_pad, S);
  ss.cand_bytes = ss.dense ? al256(dense_bytes(ss.plan.n_users_pad, S)) : ss.plan.cand_bytes;
  return ss;
}

struct Layout {
  Plan main;
  SampleScan sample;
  Guess g;
  bool queued = false;  // the main scan's workgroups claim units from fcnt[3] (TopkArgs::unit_queue)
  size_t cand = 0, cnt = 0, thr = 0, samp = 0, frows = 0, fpos = 0, fthr = 0, fcnt = 0, diag = 0;
  size_t off_thr() const { return cand + cnt; }
  size_t off_samp() const { return off_thr() + 2 * thr; }
  size_t off_frows() const { return off_samp() + samp; }
  size_t off_fpos() const { return off_frows() + frows; }
  size_t off_fthr() const { return off_fpos() + fpos; }
  size_t off_frows2() const { return off_fthr() + fthr; }
  size_t off_fpos2() const { return off_frows2() + frows; }
  size_t off_fcnt() const { return off_fpos2() + fpos; }
  size_t off_diag() const { return off_fcnt() + fcnt; }
  size_t total() const { return off_diag() + diag; }
};

Layout make_layout(int64_t n_users, int64_t n_items, int w, int k) {
  Layout L{};
  L.main = make_plan(n_users, n_items, w, k, n_items >= kGuessMinItems, true);
  L.g = guess_for(n_items, k, L.main.tail_chunks > 1);
  L.cand = L.main.cand_bytes;
  L.cnt = L.main.cnt_bytes;
  if (L.g.S > 0) {
    L.sample = sample_scan_for(n_users, L.g.S, w, L.g.ks);
    L.cand = std::max(L.cand, L.sample.cand_bytes);
    L.cnt = std::max(L.cnt, L.sample.plan.cnt_bytes);
    L.thr = al256((size_t)L.main.n_users_pad * sizeof(float));
    L.samp = al256((size_t)L.g.S * w * 2);
    L.frows = al256((size_t)n_users * sizeof(int64_t));
    L.fpos = al256((size_t)n_users * sizeof(int64_t));
    L.fthr = al256((size_t)n_users * sizeof(float));
    L.fcnt = 256;
    // the seeded main scan claims its units from a device queue (A/B knob: 0 = static loop)
    L.queued = knob_int(DR_KNOB_SCAN_QUEUE, 1) != 0;
    if (L.queued) grade_tail_chunks(L.main, n_items);
  }
  L.diag = diag_bytes();
  return L;
}

// Sample rows, tile-transposed: the S = 32 T sample rows j * stride (j < S)
// are stored so that sample j = q T + r sits in row q of tile r, i.e. output
// row p = 32 r + q. A tile (the GMAX sample scan keeps one max per user and
// tile) then holds samples T apart — catalog rows T * stride apart — so items
// that cluster by id (e.g. ids ordered by popularity) fall into different
// tiles. dr_sample_thresholds' caller gathered its sample already: stride 1.
// 16 B per thread.
__global__ __launch_bounds__(256) void sample_rows_kernel(const uint4* __restrict__ I,
                                                          int64_t stride, int64_t S, int cpr,
                                                          uint4* __restrict__ out) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= S * cpr) return;
  const int64_t p = t / cpr, c = t % cpr;
  const int64_t T = S / kTileItems;
  const int64_t j = (p % kTileItems) * T + p / kTileItems;
  out[t] = I[j * stride * cpr + c];
}


// Row width in bf16 units for a table dtype and embedding width, or -1 when
// no scan is instantiated for it (the host pads other widths with zero
// columns, which change no dot product).
int width_for(int dtype, int d) {
  if (dtype == DR_BF16 && (d == 32 || d == 64 || d == 128 || d == 256 || d == 512)) return d;
  if (dtype == DR_F32 && (d == 32 || d == 64 || d == 128 || d == 256)) return 2 * d;
  return -1;
}

bool launch_scan(const Plan& p, const TopkArgs& a, int dtype, int w, bool seeded, hipStream_t s) {
  return dtype == DR_F32 ? launch_scan_f32(p, a, w, seeded, s)
                         : launch_scan_bf16(p, a, w, seeded, s);
}

// ------------------------------------------------------------------ host-side launch sequence
// The entry points below are written out of these steps. Each takes the entry
// point's name `fn` for its error text and returns a DR_* code.
#define DR_TRY(expr)                   \
  do {                                 \
    const int rc_ = (expr);            \
    if (rc_ != DR_OK) return rc_;      \
  } while (0)

int arg_error(const char* fn, const char* msg) {
  dr::set_error(std::string(fn) + ": " + msg);
  return DR_EINVAL;
}
int plan_error(const char* fn, const char* what) {
  dr::set_error(std::string(fn) + ": internal plan error (" + what + ")");
  return DR_EUNSUPPORTED;
}
int launch_status(const char* fn) {
  const hipError_t e = hipGetLastError();
  if (e == hipSuccess) return DR_OK;
  dr::set_error(std::string(fn) + ": hipGetLastError() -> " + hipGetErrorString(e));
  return DR_EHIP;
}

// The argument checks of dr_score_topk and dr_score_topk_seeded (thr_ok: the
// seeded call's threshold pointer is set); *w = the row width. DR_OK with
// n_users == 0 means "nothing to do": the pointers are not looked at then.
int check_score_call(const char* fn, const void* user_table, int64_t n_users,
                     const void* item_table, int64_t n_items, int64_t item_base, int dtype, int d,
                     int k, const int64_t* excl_rowptr, const int32_t* excl_items,
                     const float* out_scores, const int32_t* out_items, bool thr_ok, int* w) {
  if (!(n_users >= 0 && n_items >= 0)) return arg_error(fn, "negative size");
  if (!(k >= 1 && k <= 1024)) return arg_error(fn, "k must be in [1, 1024]");
  if (!(dtype == DR_BF16 || dtype == DR_F32))
    return arg_error(fn, "tables must be DR_BF16 or DR_F32");
  *w = width_for(dtype, d);
  if (!(*w > 0))
    return arg_error(fn, dtype == DR_BF16 ? "bf16 d must be one of 32, 64, 128, 256, 512"
                                          : "fp32 d must be one of 32, 64, 128, 256");
  if (!(cap_for(*w, k) > 0)) return arg_error(fn, "k too large for this d");
  if (!(item_base >= 0 && item_base + n_items < 0x7fffffffLL))
    return arg_error(fn, "global item ids must fit int32");
  if ((excl_rowptr == nullptr) != (excl_items == nullptr))
    return arg_error(fn, "excl_rowptr and excl_items must both be set or both be NULL");
  if (n_users == 0) return DR_OK;
  if (!(user_table && out_scores && out_items && thr_ok)) return arg_error(fn, "null pointer");
  if (n_items == 0) return arg_error(fn, "empty catalog");
  if (!item_table) return arg_error(fn, "null item_table");
  return DR_OK;
}

// The 256-B aligned base of the caller's workspace; NULL (error set; the
// caller returns DR_EWORKSPACE) when fewer than `need` bytes follow it.
char* workspace_base(const char* fn, void* workspace, size_t workspace_bytes, size_t need) {
  char* ws = (char*)al256((uintptr_t)workspace);
  if (workspace && (size_t)(ws - (char*)workspace) + need <= workspace_bytes) return ws;
  dr::set_error(std::string(fn) + ": workspace too small (need " + std::to_string(need + 256) +
                " bytes)");
  return nullptr;
}

// TopkArgs of a scan under plan p: the plan's units and compaction bounds over
// the caller's tables, with the candidate keys at ws and the counts cand_bytes
// after them. Everything else is zero (item base 0, no exclusions, unseeded,
// host-side user count, no diag block): the caller states what it changes.
TopkArgs args_for(const Plan& p, const void* user_table, const int64_t* user_ids, int64_t n_users,
                  const void* item_rows, int64_t n_items, int k, char* ws, size_t cand_bytes) {
  TopkArgs a{};
  a.U = (const char*)user_table;
  a.user_ids = user_ids;
  a.n_users = n_users;
  a.n_users_pad = p.n_users_pad;
  a.I = (const char*)item_rows;
  a.n_items = n_items;
  a.k = k;
  a.n_ublocks = p.n_ublocks;
  a.n_head = p.n_head;
  a.tail_chunks = p.tail_chunks;
  a.chunk_items = p.chunk_items;
  a.chunk_floor = p.chunk_floor;
  a.end_keep = p.end_keep;
  a.head_keep = p.head_keep;
  a.slack = p.slack;
  a.gap = p.gap;
  a.keep_all = p.keep_all;
  a.cand = (uint64_t*)ws;
  a.cnt = (int32_t*)(ws + cand_bytes);
  return a;
}

int run_scan(const char* fn, const Plan& p, const TopkArgs& a, int dtype, int w, bool seeded,
             hipStream_t s) {
  if (!launch_scan(p, a, dtype, w, seeded, s)) return plan_error(fn, "no scan instance");
  return launch_status(fn);
}

// One finalize: which buffers, where the lists go, and (rescans) whose they
// are; see topk_finalize_kernel.
struct FinalizeArgs {
  const uint64_t* cand;
  const int32_t* cnt;
  BufMap map;
  int cap, k;
  const int64_t* excl_rowptr;
  const int32_t* excl_items;
  float* out_s;
  int32_t* out_i;
  const int64_t* user_ids;               // the users' table rows (for the fail list)
  const int64_t* pos_map = nullptr;      // rescans: list entry -> the caller's position
  const int32_t* n_users_dev = nullptr;  // rescans: the list's length, on the device
  // guessed scans: users left with fewer than k keys are appended here
  int32_t* fail_cnt = nullptr;
  int64_t* fail_rows = nullptr;
  int64_t* fail_pos = nullptr;
  const float* fail_thr_src = nullptr;  // [position] second-tier thresholds, copied to
  float* fail_thr = nullptr;            // [fail list entry]
};

// Finalize users [u0, u1), one wave each, sorting at most `keys` keys per
// user; false when no sort instance holds that many.
bool launch_finalize(const FinalizeArgs& f, int64_t u0, int64_t u1, int keys, hipStream_t s) {
  const dim3 grid((unsigned)dr::ceil_div(u1 - u0, 4));
  auto go = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, grid, dim3(256), 0, s, f.cand, f.cnt, f.map, f.cap, u0, u1, f.k,
                       f.excl_rowptr, f.excl_items, f.out_s, f.out_i, f.pos_map, f.n_users_dev,
                       f.user_ids, f.fail_cnt, f.fail_rows, f.fail_pos, f.fail_thr_src, f.fail_thr);
    return true;
  };
  switch (p_for(keys)) {
    case 4: return go(topk_finalize_kernel<4>);
    case 8: return go(topk_finalize_kernel<8>);
    case 16: return go(topk_finalize_kernel<16>);
    case 32: return go(topk_finalize_kernel<32>);
    default: return false;
  }
}

int finalize_range(const char* fn, const FinalizeArgs& f, int64_t u0, int64_t u1, int keys,
                   hipStream_t s) {
  if (u1 <= u0) return DR_OK;
  if (!launch_finalize(f, u0, u1, keys, s)) return plan_error(fn, "candidate sort");
  return launch_status(fn);
}

// Plan p's users: the head blocks' (one buffer each), then the split tail's
// (their chunks' buffers), each range with the sort its key count needs.
int finalize_head_and_tail(const char* fn, const FinalizeArgs& f, const Plan& p, int w,
                           int64_t n_users, hipStream_t s) {
  const int64_t head_end = std::min(p.head_users(), n_users);
  DR_TRY(finalize_range(fn, f, 0, head_end, head_keys(p, w, f.k), s));
  return finalize_range(fn, f, head_end, n_users, tail_keys(p, w, f.k), s);
}

// Thresholds of positions [u0, u1) from the compaction path's sample buffers
// (topk_threshold_kernel); false when no sort instance holds `keys` keys.
struct ThresholdArgs {
  const uint64_t* cand;
  const int32_t* cnt;
  BufMap map;
  int cap;
  int64_t n_users;  // positions from here on are padding: +inf
  int ks, ks1;      // ranks of thr2 (safe) and thr (first tier)
  float* thr;
  float* thr2;
};

bool launch_threshold(const ThresholdArgs& t, int64_t u0, int64_t u1, int keys, hipStream_t s) {
  const dim3 grid((unsigned)dr::ceil_div(u1 - u0, 4));
  auto go = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, grid, dim3(256), 0, s, t.cand, t.cnt, t.map, t.cap, u0, u1,
                       t.n_users, t.ks, t.ks1, t.thr, t.thr2);
    return true;
  };
  switch (p_for(keys)) {
    case 4: return go(topk_threshold_kernel<4>);
    case 8: return go(topk_threshold_kernel<8>);
    case 16: return go(topk_threshold_kernel<16>);
    case 32: return go(topk_threshold_kernel<32>);
    default: return false;
  }
}

// TopkArgs of the sample scan over `rows` (ss.S tile-transposed sample rows):
// sample ids are sample rows, so no exclusions and no item base. The
// candidate region starts at ws (the scan uses ss.cand_bytes of it: keys, or
// the dense tile maxima), the counts cand_bytes after it.
TopkArgs sample_args(const SampleScan& ss, const void* user_table, const int64_t* user_ids,
                     int64_t n_users, const char* rows, char* ws, size_t cand_bytes) {
  TopkArgs a = args_for(ss.plan, user_table, user_ids, n_users, rows, ss.S, ss.ks, ws, cand_bytes);
  a.gmax = ss.dense ? 2 : kSampleGmax;
  a.tmax = (float*)ws;
  a.tmax_tiles = ss.tiles();
  return a;
}

// The guess's first two steps: the sample scan (a = sample_args), then each
// position's thresholds at sample ranks ks1 (thr) and ss.ks (thr2, may be
// NULL), dense or by sorting the compaction path's buffers. Positions
// [0, n_pos) are written; those from a.n_users on (padding) get +inf.
int sample_scan_thresholds(const char* fn, const SampleScan& ss, const TopkArgs& a, int dtype,
                           int w, int ks1, int64_t n_pos, float* thr, float* thr2,
                           hipStream_t s) {
  const Plan& p = ss.plan;
  DR_TRY(run_scan(fn, p, a, dtype, w, false, s));
  if (ss.dense) {
    if (!launch_threshold_dense(a.tmax, a.tmax_tiles, n_pos, a.n_users, ss.ks, ks1, thr, thr2, s))
      return plan_error(fn, "dense threshold rank");
    return launch_status(fn);
  }
  const ThresholdArgs t{a.cand, a.cnt, buf_map(p), p.cap, a.n_users, ss.ks, ks1, thr, thr2};
  const int64_t head_end = std::min(p.head_users(), n_pos);
  auto range = [&](int64_t u0, int64_t u1, int keys) {
    if (u1 <= u0) return (int)DR_OK;
    if (!launch_threshold(t, u0, u1, keys, s)) return plan_error(fn, "candidate sort");
    return launch_status(fn);
  };
  DR_TRY(range(0, head_end, head_keys(p, w, ss.ks)));
  return range(head_end, n_pos, tail_keys(p, w, ss.ks));
}

// Tile-transposed copy of S sample rows (rows j * stride of `table`).
int copy_sample_rows(const char* fn, const void* table, int64_t stride, int64_t S, int w,
                     char* out, hipStream_t s) {
  const int cpr = w / 8;  // 16-B chunks per row
  hipLaunchKernelGGL(sample_rows_kernel, dim3((unsigned)dr::ceil_div(S * cpr, 256)), dim3(256), 0,
                     s, (const uint4*)table, stride, S, cpr, (uint4*)out);
  return launch_status(fn);
}

// ------------------------------------------------------------------ streaming merge
// Merge of more than 2048 partial entries per user (e.g. 8 shards x top-1000):
// one wave per user keeps the running best keys in elements [0, 1024) of a
// 2048-key register array; every round loads the next <= 1024 input entries
// into elements [1024, 2048) and re-sorts. Needs k_out <= 1024.
__global__ __launch_bounds__(256) void topk_merge_stream_kernel(
    const float* __restrict__ in_s, const int32_t* __restrict__ in_i, int parts, int64_t n_users,
    int k_in, int k_out, float* __restrict__ out_s, int32_t* __restrict__ out_i) {
  constexpr int P = 32;
  const int lane = dr::lane_id();
  const int64_t u = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 6;
  if (u >= n_users) return;  // wave-uniform
  const int64_t total = (int64_t)parts * k_in;
  auto entry = [&](int64_t e) -> uint64_t {
    if (e >= total) return 0ull;
    const int64_t p = e / k_in, j = e % k_in;
    const size_t o = ((size_t)p * n_users + u) * k_in + j;
    const int32_t it = in_i[o];
    return it < 0 ? 0ull : dr::make_key(in_s[o], (uint32_t)it);
  };
  uint64_t key[P];
  stream_best_1024(key, total, [&](int64_t x0, int lane0) {
    if (lane < lane0) return;
#pragma unroll
    for (int i = 0; i < P; ++i) key[i] = entry(x0 + (int64_t)(lane - lane0) * P + i);
  });
  write_best<P>(key, k_out, out_s, out_i, u);
}

}  // namespace

extern "C" size_t dr_score_topk_workspace(int64_t n_users, int64_t n_items, int dtype, int d,
                                          int k) {
  if (n_users <= 0 || n_items <= 0 || k <= 0) return 0;
  const int w = width_for(dtype, d);
  if (w < 0 || cap_for(w, k) < 0) return 0;
  return make_layout(n_users, n_items, w, k).total() + 256;
}

// The launch plan dr_score_topk would use for these arguments on the current
// device (planner knobs included), for tests that must prove which plan they
// ran. out[0..11] = users per workgroup, user blocks, head blocks, tail chunks,
// chunk items, grid, candidate capacity, sample stride (0 = no guess), sample
// rows, sample rank ks (the safe, second-tier rank), main-scan finalize keys
// of a head user / a tail user; out[12] (n_out >= 13) the first-tier rank ks1
// the main scan starts from (= ks for a one-tier guess).
extern "C" int dr_score_topk_plan(int64_t n_users, int64_t n_items, int dtype, int d, int k,
                                  int64_t* out, int n_out) {
  DR_CHECK_ARG(n_users > 0 && n_items > 0, "sizes must be positive");
  DR_CHECK_ARG(k >= 1 && k <= 1024, "k must be in [1, 1024]");
  const int w = width_for(dtype, d);
  DR_CHECK_ARG(w > 0 && cap_for(w, k) > 0, "unsupported dtype / d / k");
  DR_CHECK_ARG(out && n_out >= 12, "out must hold 12 values");
  const Layout L = make_layout(n_users, n_items, w, k);
  const Plan& p = L.main;
  const int64_t v[13] = {p.users_per_wg, p.n_ublocks, p.n_head, p.tail_chunks, p.chunk_items,
                         p.grid, p.cap, L.g.stride, L.g.S, L.g.ks, head_keys(p, w, k),
                         tail_keys(p, w, k), L.g.ks1};
  const int n = n_out < 13 ? n_out : 13;
  for (int i = 0; i < n; ++i) out[i] = v[i];
  return DR_OK;
}

// The catalog chunks of a split tail block (tail_chunk_bounds): bounds[0..c],
// chunk j = rows [bounds[j], bounds[j + 1]).
extern "C" int dr_tail_chunk_bounds(int64_t n_items, int chunks, int stage_items,
                                    int64_t floor_items, int64_t* bounds) {
  DR_CHECK_ARG(n_items >= 1 && n_items < 0x7fffffffLL, "n_items must be in [1, 2^31)");
  DR_CHECK_ARG(chunks >= 1 && chunks <= kMaxTailChunks, "chunks must be in [1, 16]");
  DR_CHECK_ARG(stage_items >= kTileItems && stage_items % kTileItems == 0,
               "stage_items must be whole tiles");
  DR_CHECK_ARG(floor_items >= 1 && floor_items <= 0x7fffffffLL, "floor_items must be in [1, 2^31)");
  DR_CHECK_ARG(bounds, "null bounds");
  for (int j = 0; j < chunks; ++j) {
    const ChunkRange r = tail_chunk_bounds(n_items, chunks, stage_items, floor_items, j);
    bounds[j] = r.beg;
    bounds[j + 1] = r.end;
  }
  return DR_OK;
}

// The chunks the main scan of dr_score_topk gives a tail block for these
// arguments on the current device (planner knobs included): *n_chunks = c
// (1: no split tail) and bounds[0..c]; n_bounds >= 17 always suffices.
extern "C" int dr_score_topk_tail_chunks(int64_t n_users, int64_t n_items, int dtype, int d, int k,
                                         int64_t* bounds, int n_bounds, int* n_chunks) {
  DR_CHECK_ARG(n_users > 0 && n_items > 0, "sizes must be positive");
  DR_CHECK_ARG(k >= 1 && k <= 1024, "k must be in [1, 1024]");
  const int w = width_for(dtype, d);
  DR_CHECK_ARG(w > 0 && cap_for(w, k) > 0, "unsupported dtype / d / k");
  DR_CHECK_ARG(n_items < 0x7fffffffLL, "item ids must fit int32");
  const Plan p = make_layout(n_users, n_items, w, k).main;
  DR_CHECK_ARG(bounds && n_chunks && n_bounds > p.tail_chunks, "bounds must hold chunks + 1 values");
  *n_chunks = p.tail_chunks;
  return dr_tail_chunk_bounds(n_items, p.tail_chunks, stage_items(w, p.cap), p.chunk_floor, bounds);
}

// Users the guessed thresholds failed in the last dr_score_topk call that
// used this workspace with these arguments: out[0] first tier (rescanned from
// the safe threshold), out[1] second tier (rescanned from -inf). Host query:
// a synchronous copy of the device counters (no counters for plain scans: 0).
// Whether that call ran two tiers is read from the workspace (the call
// records it), not re-derived from the current planner knobs.
extern "C" int dr_score_topk_fail_counts(const void* workspace, int64_t n_users, int64_t n_items,
                                         int dtype, int d, int k, int32_t* out) {
  DR_CHECK_ARG(out, "null out");
  out[0] = out[1] = 0;
  const int w = width_for(dtype, d);
  DR_CHECK_ARG(w > 0 && k >= 1 && k <= 1024 && cap_for(w, k) > 0, "unsupported dtype / d / k");
  DR_CHECK_ARG(workspace && n_users > 0 && n_items > 0, "bad arguments");
  const Layout L = make_layout(n_users, n_items, w, k);
  if (L.g.S == 0) return DR_OK;
  const char* ws = (const char*)al256((uintptr_t)workspace);
  int32_t c[3] = {0, 0, 0};  // first tier, second tier, "ran two tiers"
  DR_CHECK_HIP(hipMemcpy(c, ws + L.off_fcnt(), sizeof(c), hipMemcpyDeviceToHost));
  out[0] = c[0];
  out[1] = c[2] ? c[1] : c[0];  // one tier: the first count went straight to the -inf rescan
  return DR_OK;
}

#ifdef DR_TOPK_DIAG
// Diag builds only: byte offset (from the 256-B aligned workspace base) of the
// [grid*8][16] u64 counter block of the main scan, and its grid size.
extern "C" size_t dr_score_topk_diag_offset(int64_t n_users, int64_t n_items, int dtype, int d,
                                            int k, int* grid) {
  Layout L = make_layout(n_users, n_items, width_for(dtype, d), k);
  *grid = L.main.grid;
  return L.off_diag();
}
#endif

// A guess's fail list: the users a finalize left with fewer than k keys
// (their table rows and output positions) and their count, on the device.
struct FailList {
  int64_t* rows;
  int64_t* pos;
  int32_t* cnt;
};

extern "C" int dr_score_topk(const void* user_table, const int64_t* user_ids, int64_t n_users,
                             const void* item_table, int64_t n_items, int64_t item_base,
                             int dtype, int d, int k, const int64_t* excl_rowptr,
                             const int32_t* excl_items, float* out_scores, int32_t* out_items,
                             void* workspace, size_t workspace_bytes, dr_stream_t stream) {
  const char* fn = __func__;
  int w = 0;
  DR_TRY(check_score_call(fn, user_table, n_users, item_table, n_items, item_base, dtype, d, k,
                          excl_rowptr, excl_items, out_scores, out_items, true, &w));
  if (n_users == 0) return DR_OK;
  hipStream_t s = (hipStream_t)stream;
  const Layout L = make_layout(n_users, n_items, w, k);
  char* ws = workspace_base(fn, workspace, workspace_bytes, L.total());
  if (!ws) return DR_EWORKSPACE;
  const Plan& p = L.main;
  TopkArgs a = args_for(p, user_table, user_ids, n_users, item_table, n_items, k, ws, L.cand);
  a.item_base = item_base;
  a.excl_rowptr = excl_rowptr;
  a.excl_items = excl_items;
  a.diag = (uint64_t*)(ws + L.off_diag());  // written only in DIAG builds
  const FinalizeArgs fin{a.cand, a.cnt, buf_map(p), p.cap, k, excl_rowptr, excl_items,
                         out_scores, out_items, user_ids};

  if (L.g.S == 0) {  // plain scan from -inf (keep_all plans included), finalize
    DR_TRY(run_scan(fn, p, a, dtype, w, false, s));
    return finalize_head_and_tail(fn, fin, p, w, n_users, s);
  }

  // ---- guessed thresholds: sample scan -> thresholds -> seeded scan -> verify
  const bool two_tier = L.g.ks1 < L.g.ks;
  float* thr = (float*)(ws + L.off_thr());
  float* thr2 = two_tier ? (float*)(ws + L.off_thr() + L.thr) : nullptr;
  char* samp = ws + L.off_samp();
  float* fthr = two_tier ? (float*)(ws + L.off_fthr()) : nullptr;
  // [0] first-tier failures, [1] second-tier, [2] 1 if this call ran two tiers,
  // [3] the main scan's unit queue
  int32_t* fcnt = (int32_t*)(ws + L.off_fcnt());
  const FailList fail1{(int64_t*)(ws + L.off_frows()), (int64_t*)(ws + L.off_fpos()), fcnt};
  const FailList fail2{(int64_t*)(ws + L.off_frows2()), (int64_t*)(ws + L.off_fpos2()), fcnt + 1};
  DR_CHECK_HIP(hipMemsetAsync(fcnt, 0, 4 * sizeof(int32_t), s));
  DR_CHECK_HIP(hipMemsetD32Async((hipDeviceptr_t)(fcnt + 2), two_tier ? 1 : 0, 1, s));
  DR_TRY(copy_sample_rows(fn, item_table, L.g.stride, L.g.S, w, samp, s));
  TopkArgs as = sample_args(L.sample, user_table, user_ids, n_users, samp, ws, L.cand);
  as.diag = a.diag;
  // every buffer position gets a threshold (padding: +inf, no key passes)
  DR_TRY(sample_scan_thresholds(fn, L.sample, as, dtype, w, L.g.ks1, p.n_users_pad, thr, thr2, s));

  // ---- first tier: the main scan from thr; the finalize lists the users left
  // with fewer than k keys (and their safe thresholds) in fail1
  a.init_thr = thr;
  a.unit_queue = L.queued ? (uint32_t*)(fcnt + 3) : nullptr;
  DR_TRY(run_scan(fn, p, a, dtype, w, true, s));
  a.unit_queue = nullptr;  // the rescans below run the static unit loop
  FinalizeArgs verify = fin;
  verify.fail_cnt = fail1.cnt;
  verify.fail_rows = fail1.rows;
  verify.fail_pos = fail1.pos;
  verify.fail_thr_src = thr2;
  verify.fail_thr = fthr;
  DR_TRY(finalize_head_and_tail(fn, verify, p, w, n_users, s));

  // ---- second tier (two-tier guesses): fail1's users rescanned from their
  // safe thresholds, every failing user block split over the CUs (plan on the
  // device: the count is there), any number of keys per user merged by the
  // streaming finalize; its own failures go to fail2
  if (two_tier) {
    TopkArgs a2 = a;
    a2.init_thr = fthr;
    a2.user_ids = fail1.rows;
    a2.pos_map = fail1.pos;
    a2.n_users_dev = fail1.cnt;
    a2.n_head = 0;
    a2.end_keep = 0;
    a2.keep_all = 0;
    a2.dev_split = kMaxRescanChunks;
    a2.buf_blocks = p.buf_rows / p.users_per_wg;
    a2.diag = nullptr;
    Plan p2 = p;
    p2.grid = scan_slots();
    DR_TRY(run_scan(fn, p2, a2, dtype, w, true, s));
    const DevSplitArgs dsa{p.users_per_wg, p2.grid, kMaxRescanChunks,
                           a2.buf_blocks,  n_items, stage_items(w, p.cap)};
    hipLaunchKernelGGL(topk_finalize_stream_kernel, dim3((unsigned)dr::ceil_div(n_users, 4)),
                       dim3(256), 0, s, a.cand, a.cnt, dsa, p.cap, n_users, k, excl_rowptr,
                       excl_items, out_scores, out_items, fail1.pos, fail1.cnt, fail1.rows,
                       fail2.cnt, fail2.rows, fail2.pos);
    DR_TRY(launch_status(fn));
  }

  // ---- third tier: the users every guess failed (usually none), rescanned
  // from -inf; whole-catalog units only, one buffer per listed user
  const FailList& last = two_tier ? fail2 : fail1;
  TopkArgs a3 = a;
  a3.init_thr = nullptr;
  a3.user_ids = last.rows;
  a3.pos_map = last.pos;
  a3.n_users_dev = last.cnt;
  a3.n_head = p.n_ublocks;
  a3.tail_chunks = 1;
  a3.chunk_items = n_items;
  a3.end_keep = 0;
  a3.keep_all = 0;
  a3.diag = nullptr;
  DR_TRY(run_scan(fn, p, a3, dtype, w, false, s));
  FinalizeArgs fin3 = fin;
  fin3.map = BufMap{p.n_users_pad, p.n_users_pad, 0, 1};
  fin3.user_ids = last.rows;
  fin3.pos_map = last.pos;
  fin3.n_users_dev = last.cnt;
  return finalize_range(fn, fin3, 0, n_users, head_keys(p, w, k), s);
}

// ------------------------------------------------------------------ caller-seeded scan
// dr_score_topk_seeded: the top-k, in the key order, of the items scoring
// strictly above the caller's per-user threshold (the item-sharded multi-GPU
// top-k passes thresholds guessed from a sample of the WHOLE catalog, so a
// shard keeps only items that can reach the global top-k; divrec.distributed).
// One seeded scan (split tail allowed) and one finalize; no guess, no verify.
Plan seeded_plan(int64_t n_users, int64_t n_items, int w, int k) {
  return make_plan(n_users, n_items, w, k, true);
}

extern "C" size_t dr_score_topk_seeded_workspace(int64_t n_users, int64_t n_items, int dtype,
                                                 int d, int k) {
  if (n_users <= 0 || n_items <= 0 || k <= 0) return 0;
  const int w = width_for(dtype, d);
  if (w < 0 || cap_for(w, k) < 0) return 0;
  const Plan p = seeded_plan(n_users, n_items, w, k);
  return p.cand_bytes + p.cnt_bytes + diag_bytes() + 256;
}

extern "C" int dr_score_topk_seeded(const void* user_table, const int64_t* user_ids,
                                    int64_t n_users, const void* item_table, int64_t n_items,
                                    int64_t item_base, int dtype, int d, int k,
                                    const float* init_thr, const int64_t* excl_rowptr,
                                    const int32_t* excl_items, float* out_scores,
                                    int32_t* out_items, void* workspace, size_t workspace_bytes,
                                    dr_stream_t stream) {
  const char* fn = __func__;
  int w = 0;
  DR_TRY(check_score_call(fn, user_table, n_users, item_table, n_items, item_base, dtype, d, k,
                          excl_rowptr, excl_items, out_scores, out_items, init_thr != nullptr,
                          &w));
  if (n_users == 0) return DR_OK;
  hipStream_t s = (hipStream_t)stream;
  const Plan p = seeded_plan(n_users, n_items, w, k);
  char* ws = workspace_base(fn, workspace, workspace_bytes,
                            p.cand_bytes + p.cnt_bytes + diag_bytes());
  if (!ws) return DR_EWORKSPACE;
  TopkArgs a = args_for(p, user_table, user_ids, n_users, item_table, n_items, k, ws,
                        p.cand_bytes);
  a.item_base = item_base;
  a.excl_rowptr = excl_rowptr;
  a.excl_items = excl_items;
  a.init_thr = init_thr;
  a.diag = (uint64_t*)(ws + p.cand_bytes + p.cnt_bytes);
  DR_TRY(run_scan(fn, p, a, dtype, w, true, s));
  const FinalizeArgs fin{a.cand, a.cnt, buf_map(p), p.cap, k, excl_rowptr, excl_items,
                         out_scores, out_items, user_ids};
  return finalize_head_and_tail(fn, fin, p, w, n_users, s);
}

// ------------------------------------------------------------------ sample thresholds
// dr_sample_thresholds: the guess of dr_score_topk on a caller-gathered sample
// (divrec.distributed.global_thresholds): tile-transposed copy of the whole
// tiles of the sample, the GMAX sample scan (k = ks), thresholds at ranks ks1
// and ks. Workspace: [cand | cnt | transposed sample].
SampleScan sample_thr_scan(int64_t n_users, int64_t n_sample, int w, int ks) {
  return sample_scan_for(n_users, n_sample / kTileItems * kTileItems, w, ks);
}
size_t sample_thr_bytes(const SampleScan& ss, int w) {
  return ss.cand_bytes + ss.plan.cnt_bytes + al256((size_t)ss.S * w * 2);
}

__global__ __launch_bounds__(256) void fill_f32_kernel(float* __restrict__ a, float* __restrict__ b,
                                                       int64_t n, float v) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t < n) {
    a[t] = v;
    b[t] = v;
  }
}

extern "C" size_t dr_sample_thresholds_workspace(int64_t n_users, int64_t n_sample, int dtype,
                                                 int d, int ks) {
  if (n_users <= 0 || n_sample < 0 || ks <= 0 || ks > 256) return 0;
  const int w = width_for(dtype, d);
  if (w < 0 || cap_for(w, ks) < 0) return 0;
  return sample_thr_bytes(sample_thr_scan(n_users, n_sample, w, ks), w) + 256;
}

extern "C" int dr_sample_thresholds(const void* user_table, const int64_t* user_ids,
                                    int64_t n_users, const void* sample_rows, int64_t n_sample,
                                    int dtype, int d, int ks1, int ks, float* thr1, float* thr2,
                                    void* workspace, size_t workspace_bytes, dr_stream_t stream) {
  const char* fn = __func__;
  DR_CHECK_ARG(n_users >= 0 && n_sample >= 0, "negative size");
  DR_CHECK_ARG(ks >= 1 && ks <= 256 && ks1 >= 1 && ks1 <= ks, "need 1 <= ks1 <= ks <= 256");
  DR_CHECK_ARG(dtype == DR_BF16 || dtype == DR_F32, "tables must be DR_BF16 or DR_F32");
  const int w = width_for(dtype, d);
  DR_CHECK_ARG(w > 0 && cap_for(w, ks) > 0, "unsupported dtype / d");
  if (n_users == 0) return DR_OK;
  DR_CHECK_ARG(user_table && thr1 && thr2, "null pointer");
  hipStream_t s = (hipStream_t)stream;
  const SampleScan ss = sample_thr_scan(n_users, n_sample, w, ks);
  if (ss.S == 0) {  // no whole tile of sample rows: no guess
    hipLaunchKernelGGL(fill_f32_kernel, dim3((unsigned)dr::ceil_div(n_users, 256)), dim3(256), 0, s,
                       thr1, thr2, n_users, -INFINITY);
    return launch_status(fn);
  }
  DR_CHECK_ARG(sample_rows, "null sample_rows");
  char* ws = workspace_base(fn, workspace, workspace_bytes, sample_thr_bytes(ss, w));
  if (!ws) return DR_EWORKSPACE;
  char* samp = ws + ss.cand_bytes + ss.plan.cnt_bytes;
  DR_TRY(copy_sample_rows(fn, sample_rows, 1, ss.S, w, samp, s));
  const TopkArgs a = sample_args(ss, user_table, user_ids, n_users, samp, ws, ss.cand_bytes);
  // the caller's arrays hold n_users thresholds: no padding positions
  return sample_scan_thresholds(fn, ss, a, dtype, w, ks1, n_users, thr1, thr2, s);
}

extern "C" int dr_topk_merge(const float* in_scores, const int32_t* in_items, int parts,
                             int64_t n_users, int k_in, int k_out, float* out_scores,
                             int32_t* out_items, dr_stream_t stream) {
  DR_CHECK_ARG(parts >= 1 && k_in >= 1 && k_out >= 1, "parts, k_in, k_out must be >= 1");
  DR_CHECK_ARG((int64_t)k_out <= (int64_t)parts * k_in, "k_out must be <= parts * k_in");
  const int64_t total = (int64_t)parts * k_in;
  DR_CHECK_ARG(total <= 2048 || k_out <= 1024,
               "k_out must be <= 1024 when parts * k_in > 2048");
  if (n_users == 0) return DR_OK;
  DR_CHECK_ARG(in_scores && in_items && out_scores && out_items, "null pointer");
  hipStream_t s = (hipStream_t)stream;
  const int grid = (int)dr::ceil_div(n_users, 4);
  if (total > 2048) {
    hipLaunchKernelGGL(topk_merge_stream_kernel, dim3(grid), dim3(256), 0, s, in_scores, in_items,
                       parts, n_users, k_in, k_out, out_scores, out_items);
    DR_CHECK_LAUNCH();
    return DR_OK;
  }
  auto go = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(256), 0, s, in_scores, in_items, parts, n_users,
                       k_in, k_out, out_scores, out_items);
  };
  switch (p_for((int)total)) {
    case 2: go(topk_merge_kernel<2>); break;
    case 4: go(topk_merge_kernel<4>); break;
    case 8: go(topk_merge_kernel<8>); break;
    case 16: go(topk_merge_kernel<16>); break;
    default: go(topk_merge_kernel<32>); break;
  }
  DR_CHECK_LAUNCH();
  return DR_OK;
}
