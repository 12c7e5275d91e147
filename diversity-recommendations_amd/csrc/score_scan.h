// The streaming score scan of dr_score_topk (csrc/score_topk.hip), shared by
// the per-dtype translation units score_scan_bf16.hip and score_scan_f32.hip.
//
// score_scan_kernel<W, CAP, SEEDED, F32> — one 512-thread workgroup (8 waves,
//   two per SIMD) owns UPWG = 8*NU_T*32 users and streams one chunk of the item
//   catalog, so every item byte staged in LDS feeds UPWG products.
//   * W is the row width in bf16 units (row bytes / 2): a bf16 table of width d
//     has W = d, an fp32 table W = 2d. Geometry (stages, user tiles, LDS
//     swizzle, 16-B fragments) depends only on the row bytes, so both dtypes
//     share it; only the MFMA differs (kstep1).
//   * Each wave keeps the rows of its NU_T*32 users resident in registers as
//     MFMA B fragments for the whole scan.
//   * Item rows go HBM -> LDS by LDS-DMA (global_load_lds_dwordx4) into a ring
//     of stages (W = 128: two 72-KB slots, one stage ahead; W <= 64: two
//     56-KB slots; W >= 256: three 32-KB slots, two ahead), one s_barrier per
//     stage; the LDS image is
//     XOR-swizzled through the per-lane source address so the A-fragment
//     ds_read_b128s are bank-conflict-free. All 8 waves share every stage.
//     In the bf16 d = 128 scans with 72-KB stages waves 0-3 issue the whole
//     refill (18 instructions each) and waves 4-7 none: the younger wave of
//     each SIMD is the stage's critical path (half_issue, boundary()).
//     A fragments are read two k-steps ahead of the MFMAs that use them.
//   * The 32x32 MFMAs put items on M and users on N, so a lane holds 16 scores
//     of ONE user: the hot epilogue is a 16-way max and one compare with that
//     user's running threshold. Scores never leave registers. The two waves of
//     a SIMD cover each other's epilogues.
//     The bf16 d = 128 direct-store scans (mfma16_scan) run the same wave tile
//     on 16x16x32 MFMAs: user tiles of 16, a lane holds 8 scores of one user.
//   * Survivors are stored straight into per-user candidate buffers in HBM
//     (slot from a per-user LDS counter), or for W <= 64 staged in LDS and
//     resolved per stage. Once a buffer holds more than k + kSlack + kFlushGap
//     keys the wave compacts it with an in-register radix select, keeping only
//     keys that can still reach the top k, and raises the user's threshold to
//     the selected bound.
//   * Guessed thresholds (SEEDED = true): a scan of a strided sample sets each
//     user's starting threshold; users the guess failed are rescanned.
//   * All VMEM traffic inside the scan (LDS-DMA and candidate stores) is
//     issued from inline asm and counted by the wave, so each stage wait is an
//     exact s_waitcnt vmcnt(N): no drain of the ring.
#pragma once

#include "score_scan_plan.h"

namespace dr_topk {


using dr::bf16x8;
using dr::f32x16;
using dr::sorted_contains;
using dr::wait_vmcnt;
using dr::wait_vmcnt_dyn;
using dr::wave_lds_sync;

// Diagnostic build (-DDR_TOPK_DIAG, libdivrec_hip_diag.so only): per-wave
// s_memtime cycle counters of each phase of the scan, written to the tail of
// the workspace. Never compiled into the product library.
#ifdef DR_TOPK_DIAG
#define DG_T0(v) const uint64_t v = __builtin_amdgcn_s_memtime()
#define DG_ADD(slot, t0) dg[slot] += __builtin_amdgcn_s_memtime() - (t0)
#define DG_CNT(slot) dg[slot] += 1
#define DG_MARK(mark) dg[mark] = __builtin_amdgcn_s_memtime()
#define DG_SINCE(slot, mark) dg[slot] += __builtin_amdgcn_s_memtime() - dg[mark]
#else
#define DG_T0(v) ((void)0)
#define DG_ADD(slot, t0) ((void)0)
#define DG_CNT(slot) ((void)0)
#define DG_MARK(mark) ((void)0)
#define DG_SINCE(slot, mark) ((void)0)
#endif
template <int V>
struct IC {
  static constexpr int value = V;
};
// f(IC<I>{}), f(IC<I + 1>{}), ..., f(IC<N - 1>{}): compile-time indices for
// register arrays (a runtime index would put them in scratch)
template <int I, int N, class F>
__device__ __forceinline__ void static_for(F&& f) {
  if constexpr (I < N) {
    f(IC<I>{});
    static_for<I + 1, N>(f);
  }
}

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// ------------------------------------------------------------------ asm VMEM
// The scan issues its VMEM traffic from inline asm so that hipcc does not put
// its own conservative s_waitcnt vmcnt(0) in front of the MFMAs (it cannot
// prove a C++ ds_read does not alias an in-flight LDS-DMA); the wave counts
// every instruction it issues and waits with exact counts. M0 is used by no
// other code in the kernel.
__device__ __forceinline__ void st64(uint64_t* p, uint64_t v) {
  asm volatile("global_store_dwordx2 %0, %1, off" : : "v"(p), "v"(v) : "memory");
}
__device__ __forceinline__ u32x4 ds_read_b128_asm(uint32_t lds_addr) {
  u32x4 v;
  asm volatile("ds_read_b128 %0, %1" : "=v"(v) : "v"(lds_addr));
  return v;
}
template <int OFF>
__device__ __forceinline__ u32x4 ds_read_b128_asm_off(uint32_t lds_addr) {
  static_assert(OFF >= 0 && OFF < 65536 && OFF % 16 == 0, "ds offset field");
  u32x4 v;
  asm volatile("ds_read_b128 %0, %1 offset:%c2" : "=v"(v) : "v"(lds_addr), "i"(OFF));
  return v;
}
// LDS waits that name the fragment they retire ("+v"): no consumer of it can
// be scheduled above the wait. lgkmcnt(1) = every LDS read but the youngest
// has returned (LDS reads return in order; extra younger reads only make the
// wait stricter).
__device__ __forceinline__ void lds_wait1(u32x4& v) {
  asm volatile("s_waitcnt lgkmcnt(1)" : "+v"(v) : : "memory");
}
__device__ __forceinline__ void lds_wait0(u32x4& v) {
  asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(v) : : "memory");
}
template <int N>
__device__ __forceinline__ void lds_waitn(u32x4& v) {
  static_assert(N >= 0 && N < 16, "lgkmcnt range");
  asm volatile("s_waitcnt lgkmcnt(%c1)" : "+v"(v) : "i"(N) : "memory");
}

// Wave-uniform 64-bit value, forced into SGPRs.
__device__ __forceinline__ int64_t uni64(int64_t v) {
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v);
  const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)((uint64_t)v >> 32));
  return (int64_t)(((uint64_t)hi << 32) | lo);
}

// Issue the LDS-DMA of one stage: rows [row0, row0 + SR*32) of the slice into
// the ring slot at LDS byte address `lds_stage`. The image is lane-linear
// (glds writes base + lane*16); the swizzle is on the SOURCE address
// (cdna_hip_programming.md §5.4 rule 21). Rows past the slice end are
// clamped to its last row; their scores are masked in the epilogue.
// Addressing is SGPR base (the stage's first row) + a 32-bit per-lane offset
// recomputed at every stage from the thread id: the empty asm makes the id
// opaque, so hipcc cannot hoist 64-bit per-lane addresses out of the tile loop
// (they cost registers the loop does not have, and their spill reloads wait
// vmcnt(0), draining the ring).
// The stage's 16-B chunks are dealt in rounds of one instruction per issuing
// wave: instruction j of wave w moves chunks j * ISSUERS * 64 + w * 64 + lane
// (1 KB, lane-linear in LDS at 16 * that index). Only waves < ISSUERS call.
// LANE_ONCE (the bf16 d = 128 scans): an instruction moves 4 rows of 256 B
// and a round ISSUERS * 64 / CPR rows (32 with eight issuers; 16 with four:
// rows 16 j + 4 w + lane / 16), a multiple of the swizzle's period, so a
// lane's 16-B chunk and the swizzle of its row are the same in every
// instruction of the stage. They are computed once per stage and three VALU
// per instruction are left (row, clamp, offset) of the general form's nine:
// the refill sits at the stage boundary (DESIGN.md §3.1 "The stage boundary").
template <int D, int CAP, bool LANE_ONCE, bool HALF>
__device__ __forceinline__ void issue_stage(const char* __restrict__ I, int64_t n_items,
                                            int64_t row0, uint32_t lds_stage) {
  using G = TileGeom<D, CAP, HALF>;
  constexpr int ROWS = G::SR * kTileItems;
  constexpr int ROUND = G::ISSUERS * 64;  // chunks per instruction round
  static_assert(!LANE_ONCE || (64 % G::CPR == 0 && (ROUND / G::CPR) % (G::RPB * (G::SWM + 1)) == 0),
                "a round's rows are a multiple of the swizzle period");
  uint32_t tid = threadIdx.x;
  asm volatile("" : "+v"(tid));
  const int lane = (int)(tid & 63u);
  const int wave = (int)(__builtin_amdgcn_readfirstlane(threadIdx.x) >> 6);  // < ISSUERS
  // readfirstlane: the base is wave-uniform; the asm takes it as an SGPR pair
  const char* base = reinterpret_cast<const char*>(uni64((int64_t)(I + row0 * (2 * D))));
  const int64_t left = n_items - 1 - row0;  // >= 0: a stage starts inside the slice
  const int rmax = left < ROWS - 1 ? (int)left : ROWS - 1;
  // LANE_ONCE: this lane's row in instruction 0 and its swizzled chunk's byte offset
  const uint32_t r0 = ((uint32_t)wave * 64u + (uint32_t)lane) / (uint32_t)G::CPR;
  const uint32_t lcb = (((uint32_t)lane % (uint32_t)G::CPR) ^ (uint32_t)G::swz((int)(r0 & 31u))) * 16u;
#pragma unroll
  for (int j = 0; j < G::LPT; ++j) {
    const int wave_first = j * ROUND + wave * 64;  // wave-uniform chunk index
    uint32_t off;
    if constexpr (LANE_ONCE) {
      const uint32_t r = r0 + (uint32_t)(j * (ROUND / G::CPR));
      const uint32_t rr = r < (uint32_t)rmax ? r : (uint32_t)rmax;
      off = rr * (uint32_t)(2 * D) + lcb;
    } else {
      const int idx = wave_first + lane;
      const int r = idx / G::CPR;
      const int lc = (idx % G::CPR) ^ G::swz(r & 31);
      const int rr = r < rmax ? r : rmax;
      off = (uint32_t)(rr * (2 * D) + lc * 16);
    }
    const uint32_t m0 = __builtin_amdgcn_readfirstlane(lds_stage + wave_first * 16);
    dr::lds_dma_b128(base, off, m0);
  }
}

__device__ __forceinline__ int lane_prefix(uint64_t bal) {  // set bits of bal below this lane
  return (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32),
                                        __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0u));
}

// Max of a lane's 16 scores of one user tile, as a VALUE (stored in keys):
// IEEE maxNum, NaN scores ignored; hipcc forms v_max3_f32 from the chain, with
// canonicalising copies of the MFMA results in front (10 VALU per tile).
__device__ __forceinline__ float max16(const f32x16& a) {
  float m = a[0];
#pragma unroll
  for (int r = 1; r < 16; ++r) m = fmaxf(m, a[r]);
  return m;
}

// A user's max of a tile's 32 scores (the tile-max sample scans): the two
// half-waves' 16-score maxima merged by v_permlane32_swap.
__device__ __forceinline__ float max32(const f32x16& a) {
  const float mh = max16(a);  // a value (stored): maxNum, NaN scores skipped
  const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(mh), __float_as_uint(mh),
                                                   false, false);
  return fmaxf(__uint_as_float(sw[0]), __uint_as_float(sw[1]));
}

// The hot test's max: IEEE-754-2019 maximum (gfx950 v_maximum3_f32: NaN
// propagates, no operand canonicalisation), 8 VALU per tile instead of 10.
// Only ever compared through hot(): a NaN max counts as a hit, so the exact
// per-score tests behind it see the tile (NaN scores are never admitted there,
// as with maxNum, where they were skipped by the max).
__device__ __forceinline__ float hot_max16(const f32x16& a) {
  float m = __builtin_elementwise_maximum(a[0], a[1]);
#pragma unroll
  for (int r = 2; r < 16; ++r) m = __builtin_elementwise_maximum(m, a[r]);
  return m;
}
// "some score of the tile may beat thr": a superset of `max > thr` (NaN = hit)
__device__ __forceinline__ bool hot(float m, float thr) { return !(m <= thr); }

// Item row (within its tile) of score register r of a lane of half-wave h.
__host__ __device__ constexpr int score_row(int r, int h) { return dr::tile_row(r, h); }
// The partial-tile rule: bit r is set iff score register r is a row of the
// slice, `left` rows of which remain from the tile's first (all 16 but in the
// slice's last tile, whose rows past the end repeat the last row).
__device__ __forceinline__ uint32_t valid_rows(int64_t left, int h) {
  uint32_t vmask = 0xffffu;
  if (left < kTileItems) {
    vmask = 0u;
#pragma unroll
    for (int r = 0; r < 16; ++r) vmask |= (score_row(r, h) < (int)left ? 1u : 0u) << r;
  }
  return vmask;
}

// The 16x16x32 scans (mfma16_scan): a lane of lane group q = lane / 16 holds 8
// scores of one user, registers j = 0..3 of the tile's two 16-row halves:
// rows 16 * half + 4 q + j. Score register b = 4 * half + j.
__device__ __forceinline__ float hot_max8(const dr::f32x4& a0, const dr::f32x4& a1) {
  float m = __builtin_elementwise_maximum(a0[0], a0[1]);
#pragma unroll
  for (int j = 2; j < 4; ++j) m = __builtin_elementwise_maximum(m, a0[j]);
#pragma unroll
  for (int j = 0; j < 4; ++j) m = __builtin_elementwise_maximum(m, a1[j]);
  return m;
}
__host__ __device__ constexpr int score_row16(int b, int q) { return 16 * (b >> 2) + (b & 3) + 4 * q; }
// valid_rows for that layout: bit b is set iff score register b is a row of the slice
__device__ __forceinline__ uint32_t valid_rows16(int64_t left, int q) {
  uint32_t vmask = 0xffu;
  if (left < kTileItems) {
    vmask = 0u;
#pragma unroll
    for (int b = 0; b < 8; ++b) vmask |= (score_row16(b, q) < (int)left ? 1u : 0u) << b;
  }
  return vmask;
}

struct CompactResult {
  int kept;
  float thr;
};

// Compaction of one candidate buffer (cold path, out of line so its registers
// do not raise the pressure of the MFMA loop). Keeps only the keys that can
// still be in the top k: radix select (8 bits per level, wave-wide LDS
// histogram) down to the bucket holding the k-th largest key, until at most
// k + kSlack keys remain at or above the bucket's lower bound. The bound's
// score is the new threshold: >= k kept keys rank above any later item of
// equal or lower score. Excluded items are dropped first.
//
// The buffer is streamed in chunks of 64 * P keys (P per lane) at every level
// instead of being held in registers, so the function's register footprint is
// the same for every capacity: a register-resident 2048-key buffer (CAP =
// 2048, k up to 1024) made the callee clobber so many registers that the
// caller spilled its B fragments inside the MFMA loop (5x slower tiles).
template <int P>
__device__ __noinline__ CompactResult compact_buffer_chunked(uint64_t* __restrict__ buf, int n_in, int k,
                                                     int slack, const int32_t* __restrict__ ex,
                                                     int exn, uint32_t* __restrict__ hist) {
  constexpr int CH = 64 * P;
  const int lane = dr::lane_id();
  const int nch = (n_in + CH - 1) / CH;
  wait_vmcnt<0>();  // this wave's candidate stores have landed
  auto load = [&](int c, uint64_t (&key)[P]) {
#pragma unroll
    for (int i = 0; i < P; ++i) {
      const int e = c * CH + lane * P + i;
      key[i] = e < n_in ? __hip_atomic_load(buf + e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
                        : 0ull;
    }
  };
  // pass 0: drop excluded items (zeroed in place) and count the live keys
  int total = 0;
#pragma unroll 1
  for (int c = 0; c < nch; ++c) {
    uint64_t key[P];
    load(c, key);
    if (exn > 0) {
#pragma unroll
      for (int i = 0; i < P; ++i)
        if (key[i] != 0ull && sorted_contains(ex, exn, (int32_t)dr::key_item(key[i]))) {
          key[i] = 0ull;
          buf[c * CH + lane * P + i] = 0ull;
        }
    }
#pragma unroll
    for (int i = 0; i < P; ++i) total += __popcll(__ballot(key[i] != 0ull));
  }
  if (exn > 0) wait_vmcnt<0>();  // the zeroed slots are visible to the passes below
  uint64_t lo = 1ull;  // keep keys >= lo (key 0 = empty slot)
  CompactResult res{total, -INFINITY};
  if (total > k + slack) {
    uint64_t pfx = 0ull;
    int need = k, above = 0, inb = total;
    for (int shift = 56; shift >= 0; shift -= 8) {
#pragma unroll
      for (int j = 0; j < 4; ++j) hist[lane * 4 + j] = 0u;
      wave_lds_sync();
#pragma unroll 1
      for (int c = 0; c < nch; ++c) {
        uint64_t key[P];
        load(c, key);
#pragma unroll
        for (int i = 0; i < P; ++i) {
          const bool in = key[i] != 0ull &&
                          (shift == 56 || (key[i] >> (shift + 8)) == (pfx >> (shift + 8)));
          if (in) atomicAdd(&hist[(uint32_t)(key[i] >> shift) & 255u], 1u);
        }
      }
      wave_lds_sync();
      uint32_t hv[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) hv[j] = hist[lane * 4 + j];
      const uint32_t s4 = hv[0] + hv[1] + hv[2] + hv[3];
      uint32_t sfx = s4;  // inclusive suffix sum over lanes >= this lane
#pragma unroll
      for (int m = 1; m < 64; m <<= 1) {
        const uint32_t o = __shfl_down(sfx, m);
        sfx += (lane + m < 64) ? o : 0u;
      }
      // this lane's bins from the top (4l+3 .. 4l): the one holding rank `need`
      uint32_t cum = sfx - s4;  // keys in bins above 4l+3
      int fb = -1;
      uint32_t fexcl = 0, fcnt = 0;
#pragma unroll
      for (int j = 3; j >= 0; --j) {
        const uint32_t nx = cum + hv[j];
        if (fb < 0 && cum < (uint32_t)need && (uint32_t)need <= nx) {
          fb = lane * 4 + j;
          fexcl = cum;
          fcnt = hv[j];
        }
        cum = nx;
      }
      const int src = __builtin_ctzll(__ballot(fb >= 0));
      const int b = __builtin_amdgcn_readlane(fb, src);
      const int excl = __builtin_amdgcn_readlane((int)fexcl, src);
      inb = __builtin_amdgcn_readlane((int)fcnt, src);
      pfx |= (uint64_t)b << shift;
      need -= excl;
      above += excl;
      wave_lds_sync();  // hist is re-zeroed by the next level
      if (above + inb <= k + slack) break;
    }
    lo = pfx;
    res.kept = above + inb;
    res.thr = dr::key_score(pfx);                // smallest score with the kept prefix
    if (res.thr != res.thr) res.thr = -INFINITY;  // prefix below -FLT_MAX decodes to NaN
  }
  // write the kept keys back densely (order is irrelevant), chunk by chunk: a
  // chunk is in registers before any of its slots is overwritten, and the
  // write cursor never passes the start of the next chunk
  int base = 0;
#pragma unroll 1
  for (int c = 0; c < nch; ++c) {
    uint64_t key[P];
    load(c, key);
#pragma unroll
    for (int i = 0; i < P; ++i) {
      const bool keep = key[i] >= lo;  // lo >= 1 also drops empty keys
      const uint64_t bal = __ballot(keep);
      if (keep) buf[base + lane_prefix(bal)] = key[i];
      base += __popcll(bal);
    }
  }
  wait_vmcnt<0>();
  return res;
}

// The same with the whole buffer (<= 64 * P keys) resident in registers:
// the CAP = 512 scans (k <= 224), whose footprint this exact code fixes
// (the chunked form measured slower at d = 64, and letting it keep chunk 0
// in registers spilled the d = 64 tile loop).
// Its radix levels repeat the chunked form's on purpose: with the level loop
// (or only its bucket pick) in a shared inline helper, the d = 128 CAP 2048
// scan (k = 1000) measured +0.2 to +0.3 % (profiles/scan_dedupe/).
template <int P>
__device__ __noinline__ CompactResult compact_buffer_resident(uint64_t* __restrict__ buf, int n_in, int k,
                                                     int slack, const int32_t* __restrict__ ex,
                                                     int exn, uint32_t* __restrict__ hist) {
  const int lane = dr::lane_id();
  wait_vmcnt<0>();  // this wave's candidate stores have landed
  uint64_t key[P];
#pragma unroll
  for (int i = 0; i < P; ++i) {
    const int e = lane * P + i;
    key[i] = e < n_in ? __hip_atomic_load(buf + e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
                      : 0ull;
  }
  if (exn > 0) {
#pragma unroll
    for (int i = 0; i < P; ++i)
      if (key[i] != 0ull && sorted_contains(ex, exn, (int32_t)dr::key_item(key[i])))
        key[i] = 0ull;
  }
  int total = 0;
#pragma unroll
  for (int i = 0; i < P; ++i) total += __popcll(__ballot(key[i] != 0ull));
  uint64_t lo = 1ull;  // keep keys >= lo (key 0 = empty slot)
  CompactResult res{total, -INFINITY};
  if (total > k + slack) {
    uint64_t pfx = 0ull;
    int need = k, above = 0, inb = total;
    for (int shift = 56; shift >= 0; shift -= 8) {
#pragma unroll
      for (int j = 0; j < 4; ++j) hist[lane * 4 + j] = 0u;
      wave_lds_sync();
#pragma unroll
      for (int i = 0; i < P; ++i) {
        const bool in = key[i] != 0ull &&
                        (shift == 56 || (key[i] >> (shift + 8)) == (pfx >> (shift + 8)));
        if (in) atomicAdd(&hist[(uint32_t)(key[i] >> shift) & 255u], 1u);
      }
      wave_lds_sync();
      uint32_t hv[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) hv[j] = hist[lane * 4 + j];
      const uint32_t s4 = hv[0] + hv[1] + hv[2] + hv[3];
      uint32_t sfx = s4;  // inclusive suffix sum over lanes >= this lane
#pragma unroll
      for (int m = 1; m < 64; m <<= 1) {
        const uint32_t o = __shfl_down(sfx, m);
        sfx += (lane + m < 64) ? o : 0u;
      }
      // this lane's bins from the top (4l+3 .. 4l): the one holding rank `need`
      uint32_t cum = sfx - s4;  // keys in bins above 4l+3
      int fb = -1;
      uint32_t fexcl = 0, fcnt = 0;
#pragma unroll
      for (int j = 3; j >= 0; --j) {
        const uint32_t nx = cum + hv[j];
        if (fb < 0 && cum < (uint32_t)need && (uint32_t)need <= nx) {
          fb = lane * 4 + j;
          fexcl = cum;
          fcnt = hv[j];
        }
        cum = nx;
      }
      const int src = __builtin_ctzll(__ballot(fb >= 0));
      const int b = __builtin_amdgcn_readlane(fb, src);
      const int excl = __builtin_amdgcn_readlane((int)fexcl, src);
      inb = __builtin_amdgcn_readlane((int)fcnt, src);
      pfx |= (uint64_t)b << shift;
      need -= excl;
      above += excl;
      wave_lds_sync();  // hist is re-zeroed by the next level
      if (above + inb <= k + slack) break;
    }
    lo = pfx;
    res.kept = above + inb;
    res.thr = dr::key_score(pfx);                // smallest score with the kept prefix
    if (res.thr != res.thr) res.thr = -INFINITY;  // prefix below -FLT_MAX decodes to NaN
  }
  // write the kept keys back densely (order is irrelevant)
  int base = 0;
#pragma unroll
  for (int i = 0; i < P; ++i) {
    const bool keep = key[i] >= lo;  // lo >= 1 also drops empty keys
    const uint64_t bal = __ballot(keep);
    if (keep) buf[base + lane_prefix(bal)] = key[i];
    base += __popcll(bal);
  }
  wait_vmcnt<0>();
  return res;
}

// One k-step (one 16-B A fragment per lane) against one user tile.
//   bf16: one v_mfma_f32_32x32x16_bf16 (lane (col, h) holds row col,
//         k = 16s + 8h .. +7).
//   fp32: the same 16 B are four floats k = 8s + 4h + j, j = 0..3; four
//         v_mfma_f32_32x32x2_f32, MFMA j summing k = 8s + j and 8s + 4 + j
//         over the two lane halves. The user fragment holds the same k, so
//         every product of the row pair is taken once. The result is an
//         exact fp32 fmaf chain (cdna_hip_programming.md, FP32-input MFMA).
template <bool F32>
__device__ __forceinline__ f32x16 kstep1(const u32x4& av, const u32x4& bv, f32x16 acc) {
  if constexpr (F32) {
    const dr::f32x4 a4 = __builtin_bit_cast(dr::f32x4, av), b4 = __builtin_bit_cast(dr::f32x4, bv);
#pragma unroll
    for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4[j], b4[j], acc, 0, 0, 0);
    return acc;
  } else {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, av),
                                                   __builtin_bit_cast(bf16x8, bv), acc, 0, 0, 0);
  }
}

// One 32-wide k-step of the 16x16x32 scans against one user tile of 16: lane
// (row r, group q) holds A[row r][k = 32s + 8q .. +7] and the same k of user r.
__device__ __forceinline__ dr::f32x4 kstep16(const u32x4& av, const u32x4& bv, dr::f32x4 acc) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, av),
                                                 __builtin_bit_cast(bf16x8, bv), acc, 0, 0, 0);
}

template <int W, int CAP, bool SEEDED, bool F32, bool GMAX = false>
__global__ __launch_bounds__(kWavesScan * 64, kWavesScan / 4) void score_scan_kernel(TopkArgs a) {
  // the instantiation's compile-time shape (score_scan_plan.h), by its short names
  using S = ScanShape<W, CAP, SEEDED, F32, GMAX>;
  using G = typename S::G;
  constexpr int D = S::D, NU_T = S::NU_T, NG = S::NG, NGRP = S::NGRP, KS = S::KS, TU = S::TU;
  constexpr int NT = S::NT, KQ = S::KQ, KF = S::KF, SR = S::SR, UPW = S::UPW, UPWG = S::UPWG;
  constexpr int P = S::P, kWaves = S::kWaves, kRing = S::kRing, kStageBytes = S::kStageBytes;
  constexpr int kLpt = S::kLpt, RING_BYTES = S::RING_BYTES, SB = S::SB, WAVE_BYTES = S::WAVE_BYTES;
  constexpr bool kHalf = S::kHalf, M16 = S::M16, kLaneOnce = S::kLaneOnce, STAGED = S::STAGED;
  constexpr bool UTP = S::UTP;
  // the ring and the waves' areas, then the claimed unit id (unit loop)
  __shared__ __attribute__((aligned(16))) char smem[S::LDS_BYTES + 16];
  static_assert(S::LDS_BYTES + 16 <= 163840, "LDS budget");

  // A buffer is compacted once it holds more than flush_at keys; a stage adds
  // at most MARGIN keys per user, so flush_at + MARGIN <= CAP. A small gap
  // above k + kSlack keeps the thresholds close to the running k-th score.
  // Unseeded scans start at -inf: every score of the first stages is a
  // survivor until the first compaction sets a real threshold.
  int flush_at = a.k + a.slack + a.gap;
  flush_at = flush_at < CAP - G::MARGIN ? flush_at : CAP - G::MARGIN;
  if (a.keep_all) flush_at = 0x7fffffff;  // at most n_items <= CAP keys per buffer

  const int wave = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  // wave-uniform, kept scalar: this wave issues (and counts, and waits for) ring refills
  const bool issuer = !kHalf || (int)(__builtin_amdgcn_readfirstlane(threadIdx.x) >> 6) < G::ISSUERS;
  const int h = lane >> 5;
  const int col = lane & 31;
  char* wbase = smem + RING_BYTES + wave * WAVE_BYTES;
  uint32_t* ucnt = reinterpret_cast<uint32_t*>(wbase);
  uint32_t* hist = reinterpret_cast<uint32_t*>(wbase + UPW * 4);
  float* blk_val = reinterpret_cast<float*>(wbase + UPW * 4);  // [SB][16], 16-B aligned
  // [SB] {tile within the stage | slot << 8 | h << 16, threshold bits}: one
  // ds_write_b64 per staged lane. A stage's blocks are always resolved before
  // the next stage begins (stage end, or an overflow inside the stage), so
  // the tile is named relative to the stage's first tile (stage_t0; SR <= 255
  // tiles): no bound on the catalog length
  uint2* blk_meta = reinterpret_cast<uint2*>(blk_val + SB * 16);
  const uint32_t lds_ring = dr::lds_addr(smem);
  // This lane's A-fragment byte offset for k-step s in a tile is
  // col*2D + ((2s + h) ^ swz(col)) * 16 = a_row + ((2s) ^ a_sw) * 16: two VALU
  // per read instead of KS resident offsets (registers are the budget here).
  const uint32_t a_row = (uint32_t)(col * (2 * D));
  const uint32_t a_sw = (uint32_t)(h ^ G::swz(col));
  auto a_off = [&](int s) -> uint32_t { return a_row + ((((uint32_t)(2 * s)) ^ a_sw) << 4); };
  // M16: the lane's user (and item row within a half tile) and its 16-B chunk
  // within a k-step. Row 16 * half + ucol swizzles by ucol, so the offset of
  // k-step s is a_row16 + half * 16 rows + ((4s + kq) ^ ucol) * 16, and 4s + kq
  // = 4s ^ kq: the same two VALU per read, the half an instruction offset.
  const int ucol = M16 ? (lane & 15) : col;
  const int kq = M16 ? (lane >> 4) : h;
  const uint32_t a_row16 = (uint32_t)(ucol * (2 * D));
  const uint32_t a_sw16 = (uint32_t)(kq ^ G::swz(ucol));
  auto a_off16 = [&](int s) -> uint32_t { return a_row16 + ((((uint32_t)(4 * s)) ^ a_sw16) << 4); };

#ifdef DR_TOPK_DIAG
  uint64_t dg[kDgSlots] = {};
  DG_T0(t_kernel);
  const uint64_t rt_kernel = __builtin_amdgcn_s_memrealtime();  // 100 MHz: clock = cycles / time
#endif
  int64_t n_users = a.n_users, n_ublocks = a.n_ublocks;
  if (a.n_users_dev) {  // fallback rescan: only the users the guess failed
    const int64_t n = __builtin_amdgcn_readfirstlane(*a.n_users_dev);
    n_users = n < n_users ? n : n_users;
    n_ublocks = (n_users + UPWG - 1) / UPWG;
  }
  int64_t n_head = a.n_head < n_ublocks ? a.n_head : n_ublocks;
  int tail_chunks = a.tail_chunks;
  int64_t chunk_items = 0, pad_rows = a.n_users_pad;  // chunk_items: the device-side plan's
  if (a.dev_split > 0) {  // second-tier rescan: every failing block split over the grid
    const DevSplit ds = dev_split_plan(n_ublocks, gridDim.x, a.dev_split, a.buf_blocks, a.n_items,
                                       (int64_t)SR * kTileItems);
    n_head = 0;
    tail_chunks = ds.chunks;
    chunk_items = ds.chunk_items;
    pad_rows = n_ublocks * UPWG;
  }
  const int64_t n_tail = n_ublocks - n_head;
  const int64_t n_units = n_head + n_tail * tail_chunks;
  // Units in id order: head blocks, then the tail chunks, chunk index major
  // (the longest chunks first). Without a queue workgroup b runs units b,
  // b + grid, ... With one (TopkArgs::unit_queue) lane 0 claims the next id and
  // publishes it through unit_word; every wave reads it behind the workgroup
  // barrier and takes the same branch on it, so the waves leave the loop
  // together and none is left at a barrier. The word is written again only
  // after the __syncthreads() that ends the unit, which every wave reaches
  // after its read.
  // thread 0, by a scalar and `lane` (live anyway): no VGPR kept for the test
  const bool wave0 = SEEDED && __builtin_amdgcn_readfirstlane(threadIdx.x) < 64u;
  for (int64_t unit = blockIdx.x;; unit += gridDim.x) {
    if constexpr (SEEDED) {  // only the seeded main scan is given a queue
      if (a.unit_queue != nullptr) {
        // a zero made here: the word's and the queue's address registers are
        // then built per claim, not hoisted into VGPRs held across the tile
        // loop (which has none to spare: a B fragment went to scratch)
        uint32_t z;
        asm volatile("v_mov_b32 %0, 0" : "=v"(z));
        volatile uint32_t* unit_word =
            reinterpret_cast<volatile uint32_t*>(smem + S::LDS_BYTES + z);
        if (wave0 && lane == 0) *unit_word = atomicAdd(a.unit_queue + z, 1u);
        __syncthreads();
        unit = __builtin_amdgcn_readfirstlane(*unit_word);
      }
    }
    if (unit >= n_units) break;
    DG_T0(t_pro);
    int64_t ub, i_beg = 0, i_end = a.n_items, brow;
    bool chunked = false;  // a tail chunk unit: compacted down to end_keep at its end
    if (unit < n_head) {
      ub = unit;
      brow = ub * UPWG;
    } else {
      const int64_t idx = unit - n_head;
      const int64_t j = idx / n_tail, tb = idx % n_tail;
      ub = n_head + tb;
      if (a.dev_split > 0) {  // the device-side plan's equal chunks
        i_beg = j * chunk_items;
        i_end = i_beg + chunk_items < a.n_items ? i_beg + chunk_items : a.n_items;
      } else {
        // The catalog length goes through a VGPR, so the whole rule is computed
        // in VGPRs (free here: the B fragments are not loaded yet) and only its
        // result comes back to SGPRs, which the tile loop has none to spare of.
        uint32_t nv = (uint32_t)a.n_items;  // < 2^31 (check_score_call)
        asm volatile("" : "+v"(nv));
        const ChunkRange r = tail_chunk_bounds((int64_t)nv, tail_chunks, SR * kTileItems,
                                               a.chunk_floor, (int)j);
        i_beg = uni64(r.beg);
        i_end = uni64(r.end);
      }
      brow = j == 0 ? ub * UPWG : pad_rows + ((j - 1) * n_tail + tb) * UPWG;
      chunked = tail_chunks > 1;
    }
    const int ntiles = i_end > i_beg ? (int)((i_end - i_beg + kTileItems - 1) / kTileItems) : 0;
    const int nst = (ntiles + SR - 1) / SR;
    const int64_t upos0 = ub * UPWG + (int64_t)wave * UPW;  // first user position of the wave
    const int64_t brow0 = brow + (int64_t)wave * UPW;      // its first buffer row
    // the unit's last compaction test: a chunk of a split tail block keeps at
    // most end_keep keys per user, so the finalize gathers a bounded count
    const int keep = chunked ? a.end_keep : a.head_keep;
    const int last_lim = (keep > 0 && keep < flush_at) ? keep : flush_at;
    uint64_t* cbase = a.cand + (size_t)brow0 * CAP;
    // dense tile maxima (gmax == 2): the 32 floats of user tile u, tile t of
    // the unit (unit slices start on tile boundaries; a partial tile's rows
    // past the slice end repeat its last row, so its max is still one of its
    // own items' scores)
    auto dense_tmax = [&](int u, int t) -> float* {
      return a.tmax + ((size_t)((upos0 >> 5) + u) * (size_t)a.tmax_tiles +
                       (size_t)((i_beg >> 5) + t)) * 32;
    };

    // Resident B fragments: lane holds user (ut*32+col), k = 16s + 8h .. +7
    // (M16: user ut*16 + ucol, k = 32s + 8 kq .. +7).
    u32x4 bfr[NT][KF];  // bf16x8 (bf16 tables) or f32x4 (fp32 tables) per k-step
    float thr[NT];
#pragma unroll
    for (int ut = 0; ut < NT; ++ut) {
      const int64_t pos = upos0 + ut * TU + ucol;
      int64_t row = 0;
      if (pos < n_users) row = a.user_ids ? a.user_ids[pos] : pos;
      const uint4* src = reinterpret_cast<const uint4*>(a.U + row * (2 * D) + 16 * kq);
#pragma unroll
      for (int s = 0; s < KF; ++s) bfr[ut][s] = __builtin_bit_cast(u32x4, src[KQ * s]);
      thr[ut] = SEEDED ? (pos < n_users ? a.init_thr[pos] : INFINITY) : -INFINITY;
    }
    // Retire those loads where the compiler can see it (else it waits for them
    // inside the loop, draining the ring).
    wait_vmcnt<0>();
    for (int s = lane; s < UPW; s += 64) ucnt[s] = 0;
    int stage_t0 = 0;   // first tile of the stage being scanned (staged blocks are relative to it)
    int vmc = 0;        // VMEM instructions issued by this wave in this unit
    int vm_done = 0;    // every op issued before this count has completed
    int vs[kRing - 1];  // vmc right after each outstanding stage's DMA
#pragma unroll
    for (int i = 0; i < kRing - 1; ++i) vs[i] = 0;
    DG_ADD(kDgPrologue, t_pro);

    // -------------------------------------------------------------- MFMA tile
    // LDS byte address of item tile t of the unit in the ring
    auto tile_lds = [&](int t) -> uint32_t {
      return lds_ring + ((t / SR) % kRing) * kStageBytes + (t % SR) * G::TILE_BYTES;
    };
    auto mma_tile = [&](int t, f32x16 (&acc)[NG], auto GI) {
      constexpr int g0 = decltype(GI)::value * NG;
      const uint32_t tb = tile_lds(t);
#pragma unroll
      for (int ut = 0; ut < NG; ++ut) acc[ut] = f32x16{};
      // Fragment s is read two k-steps before its MFMAs; each wait retires
      // exactly the fragment the next MFMAs consume.
      u32x4 af[KS];
      af[0] = ds_read_b128_asm(tb + a_off(0));
      if constexpr (KS > 1) af[1] = ds_read_b128_asm(tb + a_off(1));
#pragma unroll
      for (int s = 0; s < KS; ++s) {
        if (s + 1 < KS) lds_wait1(af[s]);
        else lds_wait0(af[s]);
        if (s + 2 < KS) af[s + 2] = ds_read_b128_asm(tb + a_off(s + 2));
        if (s == 0 && t == stage_t0 && g0 == 0) DG_SINCE(kDgBFirst, kDgBMark);
#pragma unroll
        for (int ut = 0; ut < NG; ++ut) acc[ut] = kstep1<F32>(af[s], bfr[g0 + ut][s], acc[ut]);
      }
    };

    // -------------------------------------------------------------- cold paths
    auto compact = [&](int ut, int c, int n_in, int slack) {
      DG_T0(t_f);
      const int slot = ut * TU + c;
      const int64_t upos = upos0 + slot;
      const int32_t* ex = nullptr;
      int exn = 0;
      if (a.excl_rowptr && upos < n_users) {
        const int64_t er = a.pos_map ? a.pos_map[upos] : upos;
        const int64_t e0 = a.excl_rowptr[er], e1 = a.excl_rowptr[er + 1];
        ex = a.excl_items + e0;
        exn = (int)(e1 - e0);
      }
      CompactResult r;
      if constexpr (CAP <= 64 * P)
        r = compact_buffer_resident<CAP / 64>(cbase + (size_t)slot * CAP, n_in, a.k, slack, ex,
                                              exn, hist);
      else
        r = compact_buffer_chunked<P>(cbase + (size_t)slot * CAP, n_in, a.k, slack, ex, exn,
                                      hist);
      vm_done = vmc;
      if (lane == 0) ucnt[slot] = (uint32_t)r.kept;
      wave_lds_sync();
#pragma unroll
      for (int u2 = 0; u2 < NT; ++u2)  // every lane of the user (2; M16: 4)
        if (u2 == ut && ucol == c) thr[u2] = fmaxf(thr[u2], r.thr);  // both bounds are valid
      DG_ADD(kDgFlush, t_f);
      DG_CNT(kDgNFlush);
    };

    // buffers above lim are compacted down to k + slack keys
    auto check_compact = [&](int lim, int slack) {
#pragma unroll
      for (int ut = 0; ut < NT; ++ut) {
        const uint32_t c_cnt = ucnt[ut * TU + ucol];
        uint64_t need = __ballot(c_cnt > (uint32_t)lim) & ((1ull << TU) - 1ull);
        while (need) {
          const int c = __builtin_ctzll(need);
          need &= need - 1;
          compact(ut, c, __builtin_amdgcn_readlane((int)c_cnt, c), slack);
        }
      }
    };

    // -------------------------------------------------------------- epilogues
    // Hot test (branch-free): per user tile, a 16-way max against the threshold.
    // The per-tile ballots are the v_cmp results themselves (SGPR pairs); their
    // OR is the one uniform branch of the common no-hit case.
    auto any_hits = [&](f32x16 (&acc)[NG], uint64_t (&hb)[NG], auto GI) -> uint64_t {
      constexpr int g0 = decltype(GI)::value * NG;
      uint64_t any = 0ull;
#pragma unroll
      for (int ut = 0; ut < NG; ++ut) {
        hb[ut] = __ballot(hot(hot_max16(acc[ut]), thr[g0 + ut]));
        any |= hb[ut];
      }
      return any;
    };

    // Append survivors straight to their users' candidate buffers in HBM, each
    // key's slot from the user's LDS key counter. No call and no queue in the
    // hot loop, so nothing forces the accumulators and B fragments out of
    // registers. A stage adds at most MARGIN keys per user, so a buffer
    // compacted at the stage end never overflows.
    // enqueue_ut is one user tile u of the group: one block per score register
    // r. m[r], the ballot of `score r > threshold`, is the v_cmp's own SGPR
    // pair; with only its lanes active the block takes the slot, builds the key
    // of the compile-time row score_row(r, h) and stores it. A lane with
    // several survivors takes part in several blocks; no per-lane mask, no
    // 16-way value select, no second max. Almost always ONE block of the 16
    // has a lane (a hit every 6th tile at the headline, one key), so what this
    // costs is the scalar branches that skip the empty ones: a binary tree
    // over the ORs of m[] reaches the block in 8 tests, 4 of them taken.
    // Measured at 1M x 10M, k = 100 against the per-lane mask and loop this
    // replaced (profiles/survivor_regs/): sixteen blocks each behind its own
    // test 0.0 %, skipped in groups of four -0.6 %, the tree -0.9 % (-3.9 %
    // at 1.25M rows).
    // vmc is bumped under wave-uniform branches only and stays in an SGPR.
    // gbase_h (the item id of the lane's score register 0) belongs to the item
    // tile and is passed in, as the partial-tile rule is applied there.
    // M16: the same with 8 score registers b = 4 * half + j of the user tile's
    // two accumulators, rows score_row16(b, kq), and a tree over 8 ballots. The
    // lanes of one block may be up to four of one user (rows 4 apart); the LDS
    // atomic gives each its own slot.
    auto enqueue_ut = [&](const auto& ac, auto UI, uint32_t gbase_h) {
      constexpr int u = decltype(UI)::value;
      constexpr int NR = M16 ? 8 : 16;
      // M16 has 8 user tiles: their buffer addresses hoisted out of the tile
      // loop would take 16 registers it does not have (a B fragment spilled),
      // so the lane's column is made opaque here, as in issue_stage
      uint32_t uc = (uint32_t)ucol;
      if constexpr (M16) asm volatile("" : "+v"(uc));
      const int slot = u * TU + (int)uc;
      uint64_t* ubuf = cbase + (size_t)slot * CAP;  // this lane's user buffer
      float sc[NR];  // the score registers, by name
#pragma unroll
      for (int r = 0; r < NR; ++r) {
        if constexpr (M16) sc[r] = ac[r >> 2][u][r & 3];
        else sc[r] = ac[r];
      }
      uint64_t m[NR];
#pragma unroll
      for (int r = 0; r < NR; ++r) m[r] = __ballot(sc[r] > thr[u]);  // strict: never a NaN score
      auto block = [&](auto RI) {
        constexpr int r = decltype(RI)::value;
        constexpr int row = M16 ? score_row16(r, 0) : score_row(r, 0);
        if (m[r] == 0ull) return;
        if (__builtin_amdgcn_inverse_ballot_w64(m[r])) {
          const uint32_t pos = atomicAdd(&ucnt[slot], 1u);
          if (pos < (uint32_t)CAP)  // always true (flush_at + MARGIN <= CAP): a guard only
            st64(ubuf + pos, dr::make_key(sc[r], gbase_h + (uint32_t)row));
        }
        vmc += 1;  // the store above issued once (some lane had a key)
      };
      // blocks [r0, r0 + n): skipped together when none of them has a lane
      auto blocks = [&](auto& self, auto R0, auto N) {
        constexpr int r0 = decltype(R0)::value, n = decltype(N)::value;
        if constexpr (n == 1) {
          block(R0);
        } else {
          uint64_t any = 0ull;
#pragma unroll
          for (int r = r0; r < r0 + n; ++r) any |= m[r];
          if (any != 0ull) {
            self(self, IC<r0>{}, IC<n / 2>{});
            self(self, IC<r0 + n / 2>{}, IC<n / 2>{});
          }
        }
      };
      blocks(blocks, IC<0>{}, IC<8>{});
      if constexpr (!M16) blocks(blocks, IC<8>{}, IC<8>{});
    };
    auto enqueue = [&](int t, f32x16 (&acc)[NG], const uint64_t (&hb)[NG], auto GI) {
      constexpr int g0 = decltype(GI)::value * NG;
      DG_T0(t_e);
      const int64_t tile0 = i_beg + (int64_t)t * kTileItems;
      // score_row(r, h) = score_row(r, 0) + 4 h
      const uint32_t gbase_h = (uint32_t)(a.item_base + tile0) + 4u * (uint32_t)h;
      // The slice's last tile (a wave-uniform test, true once per unit): the
      // scores of rows past the slice end become -inf, which no threshold
      // admits. A full tile pays the scalar branch; the blocks pay nothing
      // (the validity bit ANDed into m[r] behind a test in each block put 16
      // more taken branches on every hit: +3.7 % at the headline).
      if (i_end - tile0 < kTileItems) {
        const uint32_t vmask = valid_rows(i_end - tile0, h);
#pragma unroll
        for (int j = 0; j < NG; ++j)
#pragma unroll
          for (int r = 0; r < 16; ++r) acc[j][r] = ((vmask >> r) & 1u) ? acc[j][r] : -INFINITY;
      }
      static_for<0, NG>([&](auto J) {
        constexpr int j = decltype(J)::value;
        if (hb[j] != 0ull) enqueue_ut(acc[j], IC<g0 + j>{}, gbase_h);
      });
      DG_ADD(kDgEnqueue, t_e);
      DG_CNT(kDgNEnqueue);
    };

    // ------------------------------------------------- the 16x16x32 tile (M16)
    // The same output tile per wave (128 users x 32 items), the same 8
    // ds_read_b128, 64 accumulator registers and 1024 MFMA cycles: fragment
    // f = 4 * half + s (rows 16 * half .., k-step s of 32) is read two fragments
    // before its 8 MFMAs, one per user tile of 16, into acc[half][ut]. (k-step
    // major, f = 2 s + half, spilled three B fragments in the loop.)
    auto mma_tile16 = [&](int t, auto& acc) {  // acc: f32x4[2][NT]
      const uint32_t tb = tile_lds(t);
#pragma unroll
      for (int hf = 0; hf < 2; ++hf)
#pragma unroll
        for (int ut = 0; ut < NT; ++ut) acc[hf][ut] = dr::f32x4{};
      u32x4 af[8];
      auto read = [&](auto FI) {
        constexpr int f = decltype(FI)::value;
        af[f] = ds_read_b128_asm_off<(f / 4) * 16 * 2 * D>(tb + a_off16(f % 4));
      };
      read(IC<0>{});
      read(IC<1>{});
      static_for<0, 8>([&](auto FI) {
        constexpr int f = decltype(FI)::value;
        if constexpr (f + 1 < 8) lds_wait1(af[f]);
        else lds_wait0(af[f]);
        if constexpr (f + 2 < 8) read(IC<f + 2>{});
        // The read stays in front of its group: there every result of the
        // previous group is still live, so the registers it may be given were
        // last written by an MFMA at least a whole group earlier (hipcc puts
        // no wait states between an MFMA's write and an asm's: asm_audit.py).
        __builtin_amdgcn_sched_barrier(0);
        if (f == 0 && t == stage_t0) DG_SINCE(kDgBFirst, kDgBMark);
#pragma unroll
        for (int ut = 0; ut < NT; ++ut) acc[f / 4][ut] = kstep16(af[f], bfr[ut][f % 4], acc[f / 4][ut]);
        // a fragment's MFMAs stay together: moved across the waits, they keep
        // all 8 fragments live, and a B fragment spills (a vmcnt(0) per tile)
        __builtin_amdgcn_sched_barrier(0);
      });
    };
    // Hot test: a user's 32 scores of the tile sit in 8 registers of each of
    // its 4 lanes; each lane tests its own 8 against the user's threshold and
    // the ballot spans the lanes.
    auto any_hits16 = [&](const auto& acc, uint64_t (&hb)[NT]) -> uint64_t {
      uint64_t any = 0ull;
#pragma unroll
      for (int ut = 0; ut < NT; ++ut) {
        hb[ut] = __ballot(hot(hot_max8(acc[0][ut], acc[1][ut]), thr[ut]));
        any |= hb[ut];
      }
      return any;
    };
    auto enqueue16 = [&](int t, auto& acc, const uint64_t (&hb)[NT]) {
      DG_T0(t_e);
      const int64_t tile0 = i_beg + (int64_t)t * kTileItems;
      // score_row16(b, kq) = score_row16(b, 0) + 4 kq
      const uint32_t gbase_q = (uint32_t)(a.item_base + tile0) + 4u * (uint32_t)kq;
      if (i_end - tile0 < kTileItems) {  // the slice's last tile: as in enqueue()
        const uint32_t vmask = valid_rows16(i_end - tile0, kq);
#pragma unroll
        for (int b = 0; b < 8; ++b)
#pragma unroll
          for (int ut = 0; ut < NT; ++ut)
            acc[b >> 2][ut][b & 3] = ((vmask >> b) & 1u) ? acc[b >> 2][ut][b & 3] : -INFINITY;
      }
      static_for<0, NT>([&](auto J) {
        constexpr int j = decltype(J)::value;
        if (hb[j] != 0ull) enqueue_ut(acc, J, gbase_q);
      });
      DG_ADD(kDgEnqueue, t_e);
      DG_CNT(kDgNEnqueue);
    };

    // -------------------------------------------------------------- tile scan
    // Stage boundary s: wait (exact count) for this wave's DMA of stage s, a
    // raw barrier publishes the whole stage, then stage s+kRing-1 is issued
    // into the slot of stage s-1, which every wave finished reading.
    // kHalf: only waves 0-3 (`issuer`) issue the refill, count it (vmc, vs[])
    // and wait for it; waves 4-7, the younger wave of each SIMD and the last
    // to reach every barrier, keep vs[] = 0, so they wait for no VMEM here and
    // leave the barrier straight into the first tile's ds_reads and MFMAs
    // while their SIMD partners issue the DMA. Still correct:
    //   RAW  a wave always relied on the barrier for the other waves' pieces
    //        of the stage; waves 4-7 now rely on it for all pieces. An
    //        issuer's vmcnt wait for its DMA still precedes its arrival.
    //   WAR  the refill into the slot of stage s-1 is still issued only after
    //        the barrier every wave reaches after its last read of that slot
    //        (at the unit end: wait_vmcnt<0> and __syncthreads before the
    //        next unit's prologue refill).
    auto boundary = [&](int st) {
      DG_T0(t_b);
      stage_t0 = st * SR;
      if (vs[0] > vm_done) wait_vmcnt_dyn(vmc - vs[0]);
      if (issuer) DG_ADD(kDgBWait, t_b);
      DG_T0(t_bb);
      __builtin_amdgcn_s_barrier();
      DG_ADD(kDgBBarrier, t_bb);
#pragma unroll
      for (int i = 0; i + 1 < kRing - 1; ++i) vs[i] = vs[i + 1];
      if (issuer && st + kRing - 1 < nst) {
        DG_T0(t_i);
        issue_stage<D, CAP, kLaneOnce, kHalf>(a.I, a.n_items,
                                       i_beg + (int64_t)(st + kRing - 1) * SR * kTileItems,
                                       lds_ring + ((st + kRing - 1) % kRing) * kStageBytes);
        vmc += kLpt;
        DG_ADD(kDgBIssue, t_i);
      }
      if (issuer) vs[kRing - 2] = vmc;
      DG_ADD(kDgBoundary, t_b);
      DG_CNT(kDgNStages);
      DG_MARK(kDgBMark);
    };
    for (int st = 0; issuer && st < kRing - 1 && st < nst; ++st) {
      issue_stage<D, CAP, kLaneOnce, kHalf>(a.I, a.n_items, i_beg + (int64_t)st * SR * kTileItems,
                                     lds_ring + st * kStageBytes);
      vmc += kLpt;
#pragma unroll
      for (int i = 0; i < kRing - 1; ++i)
        if (i == st) vs[i] = vmc;
    }
    // Staged survivors. In the tile loop a lane whose 16 scores of a user tile
    // beat the user's threshold only copies them to an LDS block (four
    // ds_write_b128 + its item base, slot and threshold); resolve() later
    // turns the staged blocks into candidate keys with one lane per block, so
    // the per-score tests, value selects and LDS counter atomics run in
    // parallel across blocks, off the MFMA loop. A block's threshold is the one
    // at staging time: thresholds only rise, so it admits a superset.
    int nblk = 0;  // staged blocks (wave-uniform)
    // BATCHED: the stage-end form (accumulators dead there); the in-loop
    // overflow call keeps the light per-score form, whose few registers fit
    // beside the live accumulators
    auto resolve = [&](auto BATCHED) {
      DG_T0(t_d);
      wave_lds_sync();
#pragma unroll 1
      for (int b0 = 0; b0 < nblk; b0 += 64) {
        const int i = b0 + lane;
        const bool live = i < nblk;
        const int ii = live ? i : 0;
        const uint2 meta = blk_meta[ii];
        const uint32_t tl = (uint32_t)stage_t0 + (meta.x & 0xffu);  // tile of the unit
        const uint32_t slot = (meta.x >> 8) & 0xffu;
        const int hh = (int)((meta.x >> 16) & 1u);
        const float th = __uint_as_float(meta.y);
        const int64_t row0 = i_beg + (int64_t)tl * kTileItems;
        const uint32_t gb = (uint32_t)(a.item_base + row0);
        const int64_t left = i_end - row0;  // rows past the slice end are not scores
        const int vld = live ? (left < kTileItems ? (int)left : kTileItems) : 0;
        uint64_t* ubuf = cbase + (size_t)slot * CAP;
        const float4* src = reinterpret_cast<const float4*>(blk_val + ii * 16);
        if constexpr (decltype(BATCHED)::value != 0) {
        // One pass over the block's 16 scores builds the survivor mask and
        // keeps the survivor's value and row (the common case is one); ONE
        // LDS atomic per block then reserves all its slots. The per-score
        // atomics this replaces were a serial chain of LDS round trips.
        uint32_t mask = 0u;
        float hv = 0.f;
        int hr = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const float4 v4 = src[q];
          const float vq[4] = {v4.x, v4.y, v4.z, v4.w};
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int row = j + 8 * q + 4 * hh;  // score register r = 4q + j
            const bool hit = row < vld && vq[j] > th;
            mask |= (hit ? 1u : 0u) << (4 * q + j);
            hv = hit ? vq[j] : hv;
            hr = hit ? row : hr;
          }
        }
        const uint32_t n = (uint32_t)__popc(mask);
        uint32_t pos = 0u;
        if (n) pos = atomicAdd(&ucnt[slot], n);
        // pos + n <= CAP always holds (flush_at + MARGIN <= CAP); the tests
        // keep a broken invariant from ever writing past the buffer
        if (n == 1u && pos < (uint32_t)CAP) st64(ubuf + pos, dr::make_key(hv, gb + (uint32_t)hr));
        if (__ballot(n == 1u) != 0ull) vmc += 1;
        // blocks with several survivors (rare): one store per survivor
        uint32_t rest = n > 1u ? mask : 0u;
        while (__ballot(rest != 0u) != 0ull) {
          if (rest != 0u) {
            const int r = __builtin_ctz(rest);
            rest &= rest - 1u;
            const float v = blk_val[ii * 16 + r];
            const int row = (r & 3) + 8 * (r >> 2) + 4 * hh;
            if (pos < (uint32_t)CAP) st64(ubuf + pos, dr::make_key(v, gb + (uint32_t)row));
            ++pos;
          }
          vmc += 1;  // one store instruction (some lane had a key)
        }
        } else {
        // four registers (one float4) at a time: few VGPRs, so this also runs
        // inside stage_ut with the accumulators live
#pragma unroll 1
        for (int q = 0; q < 4; ++q) {
          const float4 v4 = src[q];
          const float vq[4] = {v4.x, v4.y, v4.z, v4.w};
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int row = j + 8 * q + 4 * hh;  // score register r = 4q + j
            const bool hit = row < vld && vq[j] > th;
            if (__ballot(hit) != 0ull) {
              if (hit) {
                const uint32_t pos = atomicAdd(&ucnt[slot], 1u);
                // pos < CAP always holds (flush_at + MARGIN <= CAP); the test
                // keeps a broken invariant from ever writing past the buffer
                if (pos < (uint32_t)CAP) st64(ubuf + pos, dr::make_key(vq[j], gb + (uint32_t)row));
              }
              vmc += 1;  // one store instruction (some lane had a key)
            }
          }
        }
        }
      }
      nblk = 0;
      wave_lds_sync();
      DG_ADD(kDgDrain, t_d);
      DG_CNT(kDgNDrain);
    };
    // stage_ut stages one user tile u: a block for every lane of `bal`.
    auto stage_ut = [&](int t, const f32x16& ac, uint64_t bal, auto UI) {
      constexpr int u = decltype(UI)::value;
      // the lane's hit bit straight from the ballot's SGPR pair (s_and_saveexec
      // on it; no VALU re-materialisation of the compare)
      const bool hit = __builtin_amdgcn_inverse_ballot_w64(bal);
      const int n = __popcll(bal);
      if (nblk + n > SB) resolve(IC<0>{});  // rare (a scan's first stages): few registers
      if (hit) {
        const int i = nblk + lane_prefix(bal);
        float4* dst = reinterpret_cast<float4*>(blk_val + i * 16);
#pragma unroll
        for (int q = 0; q < 4; ++q)
          dst[q] = make_float4(ac[4 * q], ac[4 * q + 1], ac[4 * q + 2], ac[4 * q + 3]);
        blk_meta[i] = make_uint2((uint32_t)(t - stage_t0) | ((uint32_t)(u * 32 + col) << 8) |
                                     ((uint32_t)h << 16),
                                 __float_as_uint(thr[u]));
      }
      nblk += n;
    };
    auto stage_hits = [&](int t, f32x16 (&acc)[NG], const uint64_t (&hb)[NG], auto GI) {
      constexpr int g0 = decltype(GI)::value * NG;
      DG_T0(t_e);
      static_for<0, NG>([&](auto J) {
        constexpr int j = decltype(J)::value;
        if (hb[j] != 0ull) stage_ut(t, acc[j], hb[j], IC<g0 + j>{});
      });
      DG_ADD(kDgEnqueue, t_e);
      DG_CNT(kDgNEnqueue);
    };
    // Group-max enqueue (GMAX sample scans): one key per user and tile, the
    // max of the tile's 32 scores of the user (max32). It is the whole
    // epilogue of such a scan (the max is its hot test too). Lane h = 0 of a
    // user appends its key; each user's LDS counter has that one writer, so
    // its slot is a plain read and write (no atomic: one LDS round trip per
    // user-tile group instead of one atomic per hitting half-wave, which also
    // conflicted between the two halves of a user). A partial last tile (rows
    // past the slice end repeat the last row) is skipped: leaving sample rows
    // out only lowers the sample's order statistics, so the guess stays a
    // lower bound.
    auto enqueue_gmax = [&](int t, f32x16 (&acc)[NG], auto GI) {
      constexpr int g0 = decltype(GI)::value * NG;
      DG_T0(t_e);
      const int64_t tile0 = i_beg + (int64_t)t * kTileItems;
      if (a.gmax != 2 && i_end - tile0 < kTileItems) return;
      float m[NG];
      uint64_t bal[NG];
      uint64_t any = 0ull;
#pragma unroll
      for (int ut = 0; ut < NG; ++ut) {
        m[ut] = max32(acc[ut]);
        if (a.gmax == 2) {  // dense tile maxima
          if (h == 0) dense_tmax(g0 + ut, t)[col] = m[ut];
          vmc += 1;
          continue;
        }
        bal[ut] = __ballot(h == 0 && m[ut] > thr[g0 + ut]);
        any |= bal[ut];
      }
      if (a.gmax == 2) return;
      if (any == 0ull) return;
      uint32_t pos[NG];
#pragma unroll
      for (int ut = 0; ut < NG; ++ut) pos[ut] = bal[ut] ? ucnt[(g0 + ut) * 32 + col] : 0u;
      const uint32_t gkey = (uint32_t)(a.item_base + tile0);
#pragma unroll
      for (int ut = 0; ut < NG; ++ut) {
        if (bal[ut] == 0ull) continue;
        if ((bal[ut] >> lane) & 1ull) {
          const int slot = (g0 + ut) * 32 + col;
          ucnt[slot] = pos[ut] + 1u;
          if (pos[ut] < (uint32_t)CAP) st64(cbase + (size_t)slot * CAP + pos[ut], dr::make_key(m[ut], gkey));
        }
        vmc += 1;  // the store above issued once (some lane had a key)
      }
      DG_ADD(kDgEnqueue, t_e);
      DG_CNT(kDgNEnqueue);
    };
    // The same rule for one job of the per-user-tile pipeline. Kept beside the
    // group form: folded into it (one form over N tiles, N = 1 here) the
    // d <= 32 / 64 sample scans reload a spilled buffer address, with a
    // vmcnt(0), at every store in the tile loop (none in this form), and the
    // group form's batched counter read is part of the wide sample scans'
    // instruction stream.
    auto gmax_ut = [&](int t, const f32x16& ac, auto UI) {
      constexpr int u = decltype(UI)::value;
      const int64_t tile0 = i_beg + (int64_t)t * kTileItems;
      const float m = max32(ac);
      if (a.gmax == 2) {  // dense tile maxima: one 128-B store, no test
        if (h == 0) dense_tmax(u, t)[col] = m;
        vmc += 1;
        return;
      }
      const uint64_t bal = __ballot(h == 0 && m > thr[u]);
      if (bal == 0ull || i_end - tile0 < kTileItems) return;  // a partial last tile is skipped
      DG_T0(t_e);
      if (__builtin_amdgcn_inverse_ballot_w64(bal)) {
        const int slot = u * 32 + col;
        const uint32_t pos = ucnt[slot];  // one writer per user counter
        ucnt[slot] = pos + 1u;
        if (pos < (uint32_t)CAP)
          st64(cbase + (size_t)slot * CAP + pos, dr::make_key(m, (uint32_t)(a.item_base + tile0)));
      }
      vmc += 1;  // the store above issued once (some lane had a key)
      DG_ADD(kDgEnqueue, t_e);
      DG_CNT(kDgNEnqueue);
    };
    auto epilogue = [&](int t, f32x16 (&acc)[NG], auto GI) {
      // the stage-end work runs after the last group of the tile
      constexpr bool last_group = decltype(GI)::value == NGRP - 1;
      if constexpr (GMAX) {  // sample scan: tile maxima only
        enqueue_gmax(t, acc, GI);
        if (a.gmax != 2 && last_group && ((t + 1) % SR == 0 || t + 1 == ntiles))
          check_compact(flush_at, a.slack);
        return;
      }
      DG_T0(t_h);
      uint64_t hb[NG];
      const uint64_t any = any_hits(acc, hb, GI);
      DG_ADD(kDgHits, t_h);
      if constexpr (STAGED) {
        if (any != 0ull) stage_hits(t, acc, hb, GI);
        // end of a stage: resolve the staged blocks, compact full buffers
        if (last_group && ((t + 1) % SR == 0 || t + 1 == ntiles)) {
          if (nblk > 0) resolve(IC<1>{});
          check_compact(flush_at, a.slack);
        }
      } else {
        if (any != 0ull) enqueue(t, acc, hb, GI);
        // end of a stage: compact the buffers that passed flush_at
        if (last_group && ((t + 1) % SR == 0 || t + 1 == ntiles))
          check_compact(flush_at, a.slack);
      }
    };
    // -------------------------------------------------- per-user-tile pipeline
    // (rows of <= 128 bytes: the main scans and the narrow GMAX sample scans,
    // whose job test is gmax_ut): a job is one (item tile t, user tile u)
    // pair, KS k-steps into ONE accumulator (a single accumulation chain of
    // v_mfma_f32_32x32x16_bf16 issues at full rate). Jobs run t-major; job
    // (t, u) writes accumulator u % 2, and its hot test runs right after job
    // (t, u + 1)'s chain is issued, so the test's max3 chain, compare and
    // ballot issue while this wave's own next MFMAs execute (an MFMA holds the
    // SIMD's vector issue for 8 of its 32 cycles) instead of after the whole
    // group's chain has drained. A hit stages the job (stage_ut) before its
    // accumulator is reused two jobs later. The tile's A fragments are read
    // once (KS ds_read_b128 at the tile start) for all its NU_T jobs; the first
    // chain retires them one k-step at a time.
    auto read_a = [&](int t, u32x4 (&af)[KS]) {
      const uint32_t tb = tile_lds(t);
#pragma unroll
      for (int s2 = 0; s2 < KS; ++s2) af[s2] = ds_read_b128_asm(tb + a_off(s2));
    };
    // the tile's first chain: fragment s retired (lgkmcnt(KS - 1 - s), the
    // fragment named "+v") right before its k-step
    auto chain_first = [&](u32x4 (&af)[KS], auto UI) -> f32x16 {
      constexpr int u = decltype(UI)::value;
      f32x16 acc = f32x16{};
      static_for<0, KS>([&](auto SI) {
        constexpr int s2 = decltype(SI)::value;
        lds_waitn<KS - 1 - s2>(af[s2]);
        acc = kstep1<F32>(af[s2], bfr[u][s2], acc);
        // keep each wait right before its k-step (hipcc would hoist the waits
        // together and wait for all but one fragment before the first MFMA)
        __builtin_amdgcn_sched_barrier(0);
      });
      return acc;
    };
    auto chain = [&](const u32x4 (&af)[KS], auto UI) -> f32x16 {
      constexpr int u = decltype(UI)::value;
      f32x16 acc = f32x16{};
#pragma unroll
      for (int s2 = 0; s2 < KS; ++s2) acc = kstep1<F32>(af[s2], bfr[u][s2], acc);
      return acc;
    };
    auto test_job = [&](int t, const f32x16& ac, auto UI) {
      constexpr int u = decltype(UI)::value;
      if constexpr (GMAX) {  // sample scan: the user tile's maxima only
        gmax_ut(t, ac, UI);
        return;
      }
      DG_T0(t_h);
      const uint64_t bal = __ballot(hot(hot_max16(ac), thr[u]));
      DG_ADD(kDgHits, t_h);
      if (bal == 0ull) return;
      DG_T0(t_e);
      stage_ut(t, ac, bal, UI);
      DG_ADD(kDgEnqueue, t_e);
      DG_CNT(kDgNEnqueue);
    };
    auto stage_end_utp = [&]() {
      if constexpr (STAGED) {
        if (nblk > 0) resolve(IC<1>{});
      }
      if (GMAX && a.gmax == 2) return;  // dense tile maxima: no buffers
      check_compact(flush_at, a.slack);
    };
    if constexpr (UTP) {
      f32x16 acc0, acc1;  // job (t, u) -> acc(u % 2)
      for (int t = 0; t < ntiles; ++t) {
        DG_CNT(kDgNTiles);
        if (t % SR == 0) {
          // the previous stage's last job, then its stage-end work (every
          // job of the stage tested: at most MARGIN keys per user since the
          // last compaction), then the ring boundary
          if (t > 0) {
            test_job(t - 1, acc1, IC<NU_T - 1>{});
            stage_end_utp();
          }
          boundary(t / SR);
        }
        u32x4 af[KS];
        read_a(t, af);
        DG_T0(t_m);
        acc0 = chain_first(af, IC<0>{});
        DG_ADD(kDgMma, t_m);
        if (t % SR != 0) test_job(t - 1, acc1, IC<NU_T - 1>{});
        static_for<1, NU_T>([&](auto UI) {
          constexpr int u = decltype(UI)::value;
          DG_T0(t_m2);
          if constexpr (u % 2 == 0) acc0 = chain(af, UI);
          else acc1 = chain(af, UI);
          DG_ADD(kDgMma, t_m2);
          if constexpr (u % 2 == 0) test_job(t, acc1, IC<u - 1>{});
          else test_job(t, acc0, IC<u - 1>{});
        });
      }
      if (ntiles > 0) {
        test_job(ntiles - 1, acc1, IC<NU_T - 1>{});
        stage_end_utp();
      }
    } else if constexpr (M16) {
      // the loop below on the 16x16x32 tile: one accumulator set, direct stores
      dr::f32x4 acc[2][NT];
      for (int t = 0; t < ntiles; ++t) {
        DG_CNT(kDgNTiles);
        if (t % SR == 0) boundary(t / SR);
        DG_T0(t_m);
        mma_tile16(t, acc);
        DG_ADD(kDgMma, t_m);
        DG_T0(t_h);
        uint64_t hb[NT];
        const uint64_t any = any_hits16(acc, hb);
        DG_ADD(kDgHits, t_h);
        if (any != 0ull) enqueue16(t, acc, hb);
        // end of a stage: compact the buffers that passed flush_at
        if ((t + 1) % SR == 0 || t + 1 == ntiles) check_compact(flush_at, a.slack);
      }
    } else {
    // One accumulator set: the partner wave on the same SIMD issues its MFMAs
    // while this wave runs the epilogue (two waves per SIMD by design).
    f32x16 acc[NG];
    for (int t = 0; t < ntiles; ++t) {
      DG_CNT(kDgNTiles);
      if (t % SR == 0) boundary(t / SR);
      DG_T0(t_m);
      mma_tile(t, acc, IC<0>{});
      DG_ADD(kDgMma, t_m);
      epilogue(t, acc, IC<0>{});
      if constexpr (NGRP > 1) {
        DG_T0(t_m2);
        mma_tile(t, acc, IC<1>{});
        DG_ADD(kDgMma, t_m2);
        epilogue(t, acc, IC<1>{});
      }
    }
    }
    // a chunk of a split tail block ends with at most end_keep keys per user,
    // a whole-catalog unit of a long-list plan with at most head_keep
    if (last_lim < flush_at && ntiles > 0) check_compact(last_lim, last_lim - a.k);
    wait_vmcnt<0>();
    wave_lds_sync();
    for (int s = lane; s < UPW; s += 64) a.cnt[(size_t)brow0 + s] = (int32_t)ucnt[s];
    __syncthreads();  // the ring is refilled by the next unit
  }
#ifdef DR_TOPK_DIAG
  DG_ADD(kDgTotal, t_kernel);
  dg[kDgRealtime] = __builtin_amdgcn_s_memrealtime() - rt_kernel;
  if (lane == 0 && a.diag) {  // the rescan (usually empty) leaves the main scan's record
    uint64_t* o = a.diag + ((size_t)blockIdx.x * kWaves + wave) * kDgSlots;
#pragma unroll
    for (int i = 0; i < kDgSlots; ++i) o[i] = dg[i];
  }
#endif
}

// Instantiate and launch one dtype's scan over the supported widths.
template <bool F32, int... Ws>
bool launch_scan_widths(const Plan& p, const TopkArgs& a, int w, bool seeded, hipStream_t s) {
  bool done = false;
  auto one = [&](auto WC) {
    constexpr int WW = decltype(WC)::value;
    if (done || w != WW) return;
    done = true;
#define DR_SCAN(CC, SD) \
  hipLaunchKernelGGL((score_scan_kernel<WW, CC, SD, F32>), dim3(p.grid), dim3(kWavesScan * 64), \
                     0, s, a)
#define DR_SCAN_GMAX(CC) \
  hipLaunchKernelGGL((score_scan_kernel<WW, CC, false, F32, true>), dim3(p.grid),               \
                     dim3(kWavesScan * 64), 0, s, a)
    if (a.gmax && !seeded) {  // sample scans (ks <= ~70 keys: CAP 512, or 1024 at narrow rows)
      if (p.cap == 512) DR_SCAN_GMAX(512);
      else if (p.cap == 1024) DR_SCAN_GMAX(1024);
      else done = false;
    } else if (p.cap == 512) {
      if (seeded) DR_SCAN(512, true); else DR_SCAN(512, false);
    } else if (p.cap == 1024) {
      if (seeded) DR_SCAN(1024, true); else DR_SCAN(1024, false);
    } else if (p.cap == 2048) {
      if (seeded) DR_SCAN(2048, true); else DR_SCAN(2048, false);
    } else {
      done = false;
    }
#undef DR_SCAN
#undef DR_SCAN_GMAX
  };
  (one(IC<Ws>{}), ...);
  return done;
}

}  // namespace dr_topk
