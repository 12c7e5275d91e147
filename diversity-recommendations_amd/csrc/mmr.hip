// MMR (maximal marginal relevance) diversity re-rank, config 5 of BASELINE.json: top-C candidates
// -> k_out picks per user. There is no reference symbol; the spec is the
// build's own:
//   pick_t = argmax_{i not picked} lambda * s_i - (1 - lambda) * max_{j picked} cos(e_i, e_j)
// (the max term is 0 before the first pick; ties -> lowest candidate position). A live candidate's
// score is max(s, -FLT_MAX), NaN counting as -FLT_MAX; a row whose sum of squares is 0 has cosine 0
// with every row and stays eligible on its score.
//
// Probe-batch design, one 512-thread workgroup per CU looping over users
// (persistent grid). MFMA work is proportional to the picks, not to the probes:
//   * A user's C <= 1024 candidate rows stay in registers as MFMA B fragments (wave w owns
//     positions w, w+8, ..., 4 tiles of 32): half the register file, so a CU holds one user; the
//     next user's ids, scores and tile-0 rows arrive by LDS-DMA while this one runs.
//   * The first pick has no max term: the best live candidate by lambda * s, one wave max per wave
//     and a combine; no probes, no rounds.
//   * A batch takes 64 PROBES (the 8 best live candidates of every wave by the current MMR value)
//     and BOUND, the best key outside them.
//   * Fast rounds run the greedy over the probes only, on wave 0, with the probes' 64 x 64 Gram (4
//     MFMA tiles of the staged probe rows, on waves 0-3); wave 0 holds its lane's Gram row in
//     registers (an SGPR-indexed register read per round, no LDS round trip). A pick is valid while
//     it beats BOUND. Values only fall once a pick exists (the max term grows), so no non-probe can
//     overtake a probe that beats BOUND: the picks are exactly the eager greedy's.
//   * When no probe beats BOUND the batch ends: one MFMA pass of the batch's picks (<= 32 rows per
//     pass) against every candidate folds their cosines into the max terms.
// Exactness: the fold computes acc(pick p, candidate c) * inv|c| * inv|p| from the same bf16 rows
// with the same operand roles (A = probe/pick rows from LDS, B = candidate row) as the Gram, so the
// values the rounds see for a probe are bit-identical to what the fold leaves in its max term: the
// picks are exactly the eager greedy's on these fp32 cosines.
//
// mmr_pick_kernel, at the end of the namespace, is the skeleton; each phase is a function above it:
//   per user:  load_candidates, prefetch_ids, first_pick, prefetch_rows
//   per batch: select_probes, stage_probes, gram_tile, fast_rounds, fold (forced pick: stage_pick0, fold)

#include <float.h>

#include "common.h"
#include "rerank_args.h"

namespace {

constexpr int kThreads = 512;
constexpr int kWaves = kThreads / 64;
constexpr int kTiles = 4;                          // candidate tiles of 32 per wave
constexpr int kMaxC = kWaves * kTiles * 32;        // 1024
constexpr int kPP = 64;                            // probes per batch
constexpr int kPPW = kPP / kWaves;                 // per wave
constexpr int kGS = kPP + 4;  // s_g row stride in floats (16-B rows, 4 banks apart)

typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x32 __attribute__((ext_vector_type(32)));
using dr::bf16x8;
using dr::f32x16;

// a[lane] max a[lane ^ 32]
__device__ __forceinline__ float half_swap_max(float x) {
  const dr::F32Pair r = dr::swap32_f32(x);
  return fmaxf(r.a, r.b);
}

using dr::lds_barrier;
// not dr::wait_vmcnt<0>(): hipcc merges the builtin's wait into its own and moves an s_barrier
__device__ __forceinline__ void wait_dma() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }

// Diagnostic build (-DDR_MMR_DIAG, a measurement variant library only): per-wave s_memtime cycles
// of each phase, summed over users into a device array that dr_mmr_diag_read copies out. Never in
// the product library.
#ifdef DR_MMR_DIAG
__device__ unsigned long long g_mmr_diag[kWaves][16];
#define MG_T0(v) uint64_t v = __builtin_amdgcn_s_memtime()
#define MG_ADD(slot, t0) dg[slot] += __builtin_amdgcn_s_memtime() - (t0)
#define MG_COUNT(slot) dg[slot] += 1
#else
#define MG_T0(v) ((void)0)
#define MG_ADD(slot, t0) ((void)0)
#define MG_COUNT(slot) ((void)0)
#endif
// the statements, timed into `slot`
#define MG_TIMED(slot, ...) { MG_T0(t_##slot); __VA_ARGS__; MG_ADD(slot, t_##slot); }
enum { kMgLoad, kMgSelect, kMgStage, kMgMma, kMgSync1, kMgRounds, kMgSync2, kMgFold, kMgBatches,
       kMgTotal, kMgStageBar, kMgGt, kMgSlots = 16 };

// A thread's coordinates: wave w (uniform), half-wave h, lane q of the half. Lane (q, h) of wave w
// holds, in tile j, half h of the row of the candidate at list position cpos(j); the wave-local
// index cidx(j) addresses s_cscore / s_cinv.
struct Lane {
  int w, tid, lane, h, q;
  __device__ __forceinline__ int cpos(int j) const { return kWaves * (32 * j + q) + w; }
  __device__ __forceinline__ int cidx(int j) const { return w * 128 + 32 * j + q; }
};
// Lane coordinates from an opaque copy of the thread id, taken anew at every user and every batch:
// from a plain threadIdx.x hipcc hoists the per-lane addresses and LDS offsets out of those loops
// and spills them.
__device__ __forceinline__ Lane opaque_lane(int w) {
  uint32_t tl = threadIdx.x;
  asm volatile("" : "+v"(tl));
  const int tid = (int)tl, lane = tid & 63;
  return Lane{w, tid, lane, lane >> 5, lane & 31};
}

template <int D> constexpr int kKS = D / 16;  // MFMA k-steps per row
template <int D> constexpr int kCPR = D / 8;  // 16-B chunks per row
template <int D> constexpr int kSWM = (kCPR<D> < 16 ? kCPR<D> : 16) - 1;
// Where half h (0 or 1) of k-step k of row r, its 16-B chunk 2k + h, sits in an LDS image of rows:
// r * CPR + ((2k + h) ^ (r & SWM)). The part of the xor that does not depend on k is written first:
// hipcc takes it out of the k loops then, which it does not do from (2k + h) inside a function.
template <int D>
__device__ __forceinline__ constexpr int frag_at(int r, int k, int h) {
  return r * kCPR<D> + ((2 * k) ^ (h ^ (r & kSWM<D>)));
}
template <int D> using Rows = bf16x8[kTiles][kKS<D>];  // a lane's candidate rows: B fragments [j][k]
using Pens = float[kTiles];                            // their max terms

// The workgroup's LDS, shared by the phases below.
template <int D> __shared__ uint4 s_prow[kPP * kCPR<D>];  // probe rows, slot p at frag_at<D>(p, ..)
// s_g[a*kGS + p] = cos(probe a, probe p) rounded as a's fold would round it
__shared__ __attribute__((aligned(16))) float s_g[kPP * kGS];
__shared__ float s_pinv[kPP], s_pscore[kPP], s_ppen[kPP];  // per probe slot: 1/|e|, score, max term
__shared__ int s_pcand[kPP], s_pitem[kPP];  // candidate position (-1 = empty slot) and item id
__shared__ int s_plist[kPP];                // this batch's picks: probe slots in pick order
__shared__ __attribute__((aligned(16))) float s_lpinv[kPP];  // 1/|e| of pick i
__shared__ int s_citem[kMaxC];                    // item id by candidate position
__shared__ float s_cscore[kMaxC], s_cinv[kMaxC];  // score and 1/|e|, wave-local index cidx
__shared__ uint64_t s_wbound[kWaves];             // per wave: its first-pick key, then its bound
__shared__ int s_state[5];  // rounds done, picks this batch, picked mask lo / hi, forced pick
__shared__ int s_out[kMaxC];  // the user's list
// the next user's ids and scores, and the rows of candidate tile 0 of every wave (256, at frag_at<D>)
__shared__ int s_nitem[kMaxC];
__shared__ float s_nscore[kMaxC];
template <int D> __shared__ uint4 s_pf[kWaves * 32 * kCPR<D>];

// ---- prefetch of the workgroup's next user, by LDS-DMA while this one runs: ids and scores of
// user un -> s_nitem / s_nscore: 2 x 16 LDS-DMA blocks of 64 words, 2 + 2 per wave (entries past C
// repeat entry C - 1: never read)
__device__ __forceinline__ void prefetch_ids(const Lane& l, const int32_t* cand_items,
                                             const float* cand_scores, int C, int64_t un) {
#pragma unroll
  for (int b = 0; b < 2; ++b) {
    const int e = (2 * l.w + b) * 64 + l.lane;
    const int64_t src = un * C + (e < C ? e : C - 1);
    const uint32_t m0i = dr::lds_addr(s_nitem) + (uint32_t)(2 * l.w + b) * 256u;
    const uint32_t m0s = dr::lds_addr(s_nscore) + (uint32_t)(2 * l.w + b) * 256u;
    dr::lds_dma_b32(cand_items + src, m0i);
    dr::lds_dma_b32(cand_scores + src, m0s);
  }
}
// tile-0 rows of the next user (its ids in s_nitem) -> s_pf: 256 * CPR 16-B chunks, 64 per DMA
// instruction; an empty or out-of-range id loads row 0 (never used)
template <int D>
__device__ __forceinline__ void prefetch_rows(const Lane& l, const __bf16* E, int64_t n_items) {
  constexpr int PER = 32 * kCPR<D> / 64;  // instructions per wave
#pragma unroll
  for (int k = 0; k < PER; ++k) {
    const int blk = l.w * PER + k;
    const uint32_t i = (uint32_t)(blk * 64 + l.lane);
    const uint32_t r = i / kCPR<D>, c = (i % kCPR<D>) ^ (r & kSWM<D>);
    const int32_t it = s_nitem[kWaves * (r & 31) + (r >> 5)];
    const int64_t row = (it >= 0 && (int64_t)it < n_items) ? it : 0;
    const __bf16* src = E + row * D + c * 8;
    const uint32_t m0 = dr::lds_addr(s_pf<D>) + (uint32_t)blk * 1024u;
    dr::lds_dma_b128(src, m0);
  }
}

// ---- candidate rows of user u -> B fragments brow (tile 0 from the prefetch, if any), pen = -inf;
// ids -> s_citem, scores (clamped to -FLT_MAX) -> s_cscore, 1/|e| (0 for a zero row) -> s_cinv;
// out-of-range ids counted into *err and treated as empty. Returns the lane's live mask (bit j:
// tile j holds a candidate).
template <int D>
__device__ __forceinline__ uint32_t load_candidates(
    const Lane& l, const int32_t* cand_items, const float* cand_scores, const __bf16* E, int C,
    int64_t n_items, int64_t u, bool pre, int32_t* err, Rows<D>& brow, Pens& pen) {
  uint32_t live = 0;
  int nbad = 0;
#pragma unroll
  for (int j = 0; j < kTiles; ++j) {
    const int c = l.cpos(j);
    int32_t item = c < C ? (pre ? s_nitem[c] : cand_items[u * C + c]) : -1;
    if (item >= 0 && (int64_t)item >= n_items) {
      nbad += l.h == 0 ? 1 : 0;
      item = -1;
    }
    const bool ok = item >= 0;
    live |= (ok ? 1u : 0u) << j;
    const float sc = ok ? (pre ? s_nscore[c] : cand_scores[u * C + c]) : 0.f;
    if (l.h == 0) {
      s_citem[c] = item;
      // a live candidate's value stays above -inf, the key of a dead slot (kDead): -inf and NaN
      // scores count as -FLT_MAX. Clamped here and not at the load: around the load hipcc merges
      // the two sources (prefetch image, global) into one flat load
      s_cscore[l.cidx(j)] = fmaxf(sc, -FLT_MAX);
    }
    pen[j] = -INFINITY;
    if (j == 0 && pre) {
      const int r = l.w * 32 + l.q;
#pragma unroll
      for (int k = 0; k < kKS<D>; ++k)
        brow[0][k] = __builtin_bit_cast(bf16x8, s_pf<D>[frag_at<D>(r, k, l.h)]);
    } else {
      const uint4* src = reinterpret_cast<const uint4*>(E + (int64_t)(ok ? item : 0) * D) + l.h;
#pragma unroll
      for (int k = 0; k < kKS<D>; ++k) brow[j][k] = __builtin_bit_cast(bf16x8, src[2 * k]);
    }
  }
  if (nbad && err) atomicAdd(err, nbad);
#pragma unroll
  for (int j = 0; j < kTiles; ++j) {
    float nsq = 0.f;
#pragma unroll
    for (int k = 0; k < kKS<D>; ++k) {
      const uint4 v = __builtin_bit_cast(uint4, brow[j][k]);
      const uint32_t pr[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const bf16x2 a = __builtin_bit_cast(bf16x2, pr[e]);
        nsq = __builtin_amdgcn_fdot2_f32_bf16(a, a, nsq, false);
      }
    }
    nsq += __shfl_xor(nsq, 32);
    // a zero row: 1/|e| = 0, as for an empty probe slot, so its cosine with every row is 0 (not
    // 0 * inf = NaN, which the fold's max would drop and leave the max term at -inf)
    if (l.h == 0) s_cinv[l.cidx(j)] = nsq > 0.f ? 1.f / sqrtf(nsq) : 0.f;
  }
  return live;
}

// max of mx and cos = (acc * 1/|c|) * 1/|p| over registers R0 .. R0 + 7 of one tile: the Gram's
// operand order, two scores per v_pk_mul_f32
template <int R0>
__device__ __forceinline__ float fold_max8(const f32x16& acc, f32x2 c2, const f32x2 (&pv2)[8], float mx) {
#pragma unroll
  for (int r = R0; r < R0 + 8; r += 2) {
    const f32x2 cs = (f32x2{acc[r], acc[r + 1]} * c2) * pv2[r / 2];
    mx = fmaxf(mx, fmaxf(cs.x, cs.y));
  }
  return mx;
}
// ---- fold: the np picks of s_plist (their rows staged in s_prow, 1/|e| in s_lpinv) into every
// candidate's max term pen: rows of A = the picks in pick order, 32 per pass; register r of tile j
// holds pick i = 8 (r / 4) + 4 h + r % 4.
template <int D>
__device__ __forceinline__ void fold(const Lane& l, int np, const Rows<D>& brow, Pens& pen) {
  for (int i0 = 0; i0 < np; i0 += 32) {
    const int nrow = np - i0 < 32 ? np - i0 : 32;
    const int sq = l.q < nrow ? s_plist[i0 + l.q] : -1;
    f32x16 acc[kTiles];
#pragma unroll
    for (int j = 0; j < kTiles; ++j) acc[j] = f32x16{};
#pragma unroll
    for (int k = 0; k < kKS<D>; ++k) {
      const uint4 av = sq >= 0 ? s_prow<D>[frag_at<D>(sq, k, l.h)] : uint4{0, 0, 0, 0};
      const bf16x8 a = __builtin_bit_cast(bf16x8, av);
#pragma unroll
      for (int j = 0; j < kTiles; ++j)
        acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, brow[j][k], acc[j], 0, 0, 0);
    }
    // 1/|pick| per register pair; NaN for rows past the picks, whose products (NaN) the max
    // ignores: no per-score select. Registers 8-15 (rows 16-31) are skipped when the pass has at
    // most 16 picks (the common case: ~15 picks per batch).
    const bool upper = nrow > 16;
    f32x2 pv2[8];
#pragma unroll
    for (int gg = 0; gg < 4; ++gg) {
      const float4 v = *reinterpret_cast<const float4*>(&s_lpinv[i0 + 8 * gg + 4 * l.h]);
      const int r0 = 8 * gg + 4 * l.h;
      const float nan = __builtin_nanf("");
      pv2[2 * gg] = f32x2{r0 < nrow ? v.x : nan, r0 + 1 < nrow ? v.y : nan};
      pv2[2 * gg + 1] = f32x2{r0 + 2 < nrow ? v.z : nan, r0 + 3 < nrow ? v.w : nan};
    }
#pragma unroll
    for (int j = 0; j < kTiles; ++j) {
      const float ci = s_cinv[l.cidx(j)];
      const f32x2 c2 = {ci, ci};
      float mx = fold_max8<0>(acc[j], c2, pv2, -INFINITY);
      if (upper) mx = fold_max8<8>(acc[j], c2, pv2, mx);
      pen[j] = fmaxf(pen[j], half_swap_max(mx));
    }
  }
}

// A single candidate, at list position pos, becomes output `slot` of the user and pick 0 of a
// one-pick fold: its owner lanes (both halves) stage its row as probe slot 0 and drop it from their
// live mask.
template <int D>
__device__ __forceinline__ void stage_pick0(const Lane& l, int pos, int slot, const Rows<D>& brow,
                                            uint32_t& live) {
  const int pj = (pos >> 3) >> 5, pq = (pos >> 3) & 31;  // pos = cpos(pj) of lane pq, wave pos & 7
  if (l.w == (pos & 7) && l.q == pq) {
#pragma unroll
    for (int j = 0; j < kTiles; ++j) {
      if (j == pj) {
#pragma unroll
        for (int k = 0; k < kKS<D>; ++k) s_prow<D>[2 * k + l.h] = __builtin_bit_cast(uint4, brow[j][k]);
        // ends the branch: else hipcc merges the four branches' stores into one set that reads brow
        // at a computed address, which puts brow in scratch
        asm volatile("");
      }
    }
    if (l.h == 0) {
      s_plist[0] = 0;
      s_lpinv[0] = s_cinv[l.cidx(pj)];
      s_out[slot] = s_citem[pos];
    }
    live &= ~(1u << pj);
  }
}

// ---- first pick: the best live candidate by lambda * score (no max term yet), found by one wave
// max per wave (s_wbound) + a combine; no probes, no rounds. Folds it into pen and returns the
// number of picks made: 1, or 0 when the user has no live candidate.
template <int D>
__device__ __forceinline__ int first_pick(const Lane& l, float lambda, const Rows<D>& brow,
                                          Pens& pen, uint32_t& live) {
  uint64_t lk = 0ull;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int j = 2 * l.h + i;
    if ((live >> j) & 1u) {
      const float sc = s_cscore[l.cidx(j)];
      lk = dr::umax64(lk, dr::make_key(lambda * sc, (uint32_t)l.cpos(j)));
    }
  }
  const uint64_t wb = dr::wave_max_u64(lk);
  if (l.lane == 0) s_wbound[l.w] = wb;
  lds_barrier();
  uint64_t best = 0ull;
#pragma unroll
  for (int i = 0; i < kWaves; ++i) best = dr::umax64(best, s_wbound[i]);
  if (best != 0ull) {
    stage_pick0<D>(l, (int)dr::key_item(best), 0, brow, live);
    lds_barrier();
    fold<D>(l, 1, brow, pen);
  }
  lds_barrier();  // s_wbound / s_prow are rewritten by the first batch
  return best != 0ull ? 1 : 0;
}

// One bit of the radix select: p | bit if more than 8 of the wave's values v0, v1 are >= p | bit,
// else p. Both ballots of a step go into their own SGPR pairs (hipcc serialises them through VCC).
__device__ __forceinline__ uint32_t radix_step(uint32_t p, uint32_t bit, uint32_t v0, uint32_t v1) {
  static_assert(kPPW + 1 == 9, "the asm below counts against 8");
  uint64_t ba_, bb_;
  uint32_t c_, na_, nb_;
  asm volatile(
      "s_or_b32 %[c], %[p], %[bit]\n\t"
      "v_cmp_le_u32_e64 %[ba], %[c], %[v0]\n\t"
      "v_cmp_le_u32_e64 %[bb], %[c], %[v1]\n\t"
      "s_bcnt1_i32_b64 %[na], %[ba]\n\t"
      "s_bcnt1_i32_b64 %[nb], %[bb]\n\t"
      "s_add_u32 %[na], %[na], %[nb]\n\t"
      "s_cmp_gt_u32 %[na], 8\n\t"
      "s_cselect_b32 %[p], %[c], %[p]"
      : [p] "+s"(p), [ba] "=&s"(ba_), [bb] "=&s"(bb_), [c] "=&s"(c_), [na] "=&s"(na_),
        [nb] "=&s"(nb_)
      : [bit] "s"(bit), [v0] "v"(v0), [v1] "v"(v1)
      : "scc");
  return p;
}
// ---- probes of this wave and its bound. Any probe set is exact as long as the bound is the best
// key outside it, so the wave takes every live candidate whose value beats the 9th-best value p of
// its 128 (at most kPPW of them), found by a radix select over the 32-bit value order: one ballot
// pair per bit, no serial argmax chain. The bound is (p, the lowest position holding p). Lane (q,
// h) ranks tiles 2h and 2h+1 (both half-waves hold the same candidates; this way each counts once).
// Reads pen, live and s_cscore / s_cinv / s_citem; writes the wave's kPPW probe slots of s_pcand,
// s_pitem, s_pinv, s_pscore, s_ppen and its bound s_wbound[w]. t = picks so far. myslot, per tile
// j: probe slot + 1 of this lane's candidate (bits 8j..), 0 when it is no probe; nprobe: the wave's
// probe count.
__device__ __forceinline__ void select_probes(const Lane& l, const Pens& pen, uint32_t live, int t,
                                              float lambda, float mu, uint32_t& myslot, int& nprobe) {
  uint32_t v2[2];
  float r_sc[2], r_pen[2];  // the ranked candidates' score and max term (probe state)
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const float sc = s_cscore[l.cidx(2 * l.h + i)];
    uint32_t o = 0u;
    float pn = 0.f;
#pragma unroll
    for (int j = 0; j < kTiles; ++j) {
      if (j == 2 * l.h + i) {
        pn = pen[j];
        if ((live >> j) & 1u) {
          const float val = t == 0 ? lambda * sc : fmaf(-mu, pen[j], lambda * sc);
          o = dr::f32_to_ord(val);
        }
      }
    }
    v2[i] = o;
    r_sc[i] = sc;
    r_pen[i] = pn;
  }
  // Probe threshold p9: the wave's probes are its live values > p9 (at most kPPW of them), p9 the
  // (kPPW + 1)-th largest value: the largest p with at least kPPW + 1 values >= p (0: fewer live),
  // found bit by bit. The selection is SALU-bound (the eight waves share the CU's scalar unit);
  // skipping the live values' common prefix and stopping 8 bits short measured slower (64.3 -> 65.7
  // ms), and so did counting on the VALU (v_bcnt of the ballot halves) on waves 0-3 or on every
  // wave, which balances the waves but lengthens each step (65.6 / 66.5 against 64.4 ms).
  uint32_t p9 = 0u;
#pragma unroll
  for (int bit = 31; bit >= 0; --bit) p9 = radix_step(p9, 1u << bit, v2[0], v2[1]);
  const uint64_t b0 = __ballot(v2[0] > p9), b1 = __ballot(v2[1] > p9);
  const int n0 = __popcll(b0);
  nprobe = n0 + __popcll(b1);
  myslot = 0u;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const uint64_t bm = i == 0 ? b0 : b1;
    if ((bm >> l.lane) & 1ull) {
      const int rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(bm >> 32),
                                                __builtin_amdgcn_mbcnt_lo((uint32_t)bm, 0));
      const int slot = l.w * kPPW + (i == 0 ? 0 : n0) + rank;
      const int j = 2 * l.h + i;
      const int pos = l.cpos(j);
      // the probe's state, written by the lane that ranked it (its row is staged by the two lanes
      // that hold its halves)
      s_pcand[slot] = pos;
      s_pitem[slot] = s_citem[pos];
      s_pinv[slot] = s_cinv[l.cidx(j)];
      s_pscore[slot] = r_sc[i];
      s_ppen[slot] = r_pen[i];
      myslot |= (uint32_t)(slot + 1) << (8 * j);
    }
  }
  myslot |= (uint32_t)__shfl_xor((int)myslot, 32);  // the other half-wave holds the same rows
  if (l.lane < kPPW && l.lane >= nprobe) {
    // an empty slot: 1/|e| = 0 (and a zero row, written at staging), so its Gram entries are 0
    // (finite) and the rounds' max terms stay finite without a select
    const int sl = l.w * kPPW + l.lane;
    s_pcand[sl] = -1;
    s_pinv[sl] = 0.f;
    s_ppen[sl] = 0.f;
  }
  // the wave's bound: the best value <= p9, at its lowest position; p9 itself is a value (0: fewer
  // than kPPW + 1 live)
  uint64_t wb = 0ull;
  if (p9 != 0u) {
    uint32_t mp = 0xffffffffu;
#pragma unroll
    for (int i = 0; i < 2; ++i)
      if (v2[i] == p9) {
        const uint32_t pos = (uint32_t)l.cpos(2 * l.h + i);
        mp = pos < mp ? pos : mp;
      }
    mp = dr::wave_min_u32_64(mp);
    wb = ((uint64_t)p9 << 32) | (uint32_t)~mp;
  }
  if (l.lane == 0) s_wbound[l.w] = wb;
}

// ---- staging: this wave's probe rows (brow of the lanes myslot names) and the zero rows of its
// empty slots -> s_prow. It runs after every wave's fold of the previous batch (each wave folds
// before it selects, and the barrier after staging waits for all), so the rows are written here and
// not during the selection: there is no barrier between a wave's fold and its next selection.
template <int D>
__device__ __forceinline__ void stage_probes(const Lane& l, const Rows<D>& brow, uint32_t myslot,
                                             int nprobe) {
  if (l.lane < kPPW && l.lane >= nprobe) {
    const int sl = l.w * kPPW + l.lane;
#pragma unroll
    for (int c = 0; c < kCPR<D>; ++c) s_prow<D>[sl * kCPR<D> + c] = uint4{0u, 0u, 0u, 0u};
  }
#pragma unroll
  for (int j = 0; j < kTiles; ++j) {
    const int sl = (int)((myslot >> (8 * j)) & 255u) - 1;
    if (sl >= 0) {
#pragma unroll
      for (int k = 0; k < kKS<D>; ++k)
        s_prow<D>[frag_at<D>(sl, k, l.h)] = __builtin_bit_cast(uint4, brow[j][k]);
    }
  }
}

// ---- Gram tile of wave w < 4, s_prow and s_pinv -> s_g: B columns = probes a = 32 ab + q, A rows
// = probes p = 32 pb + 8 (r / 4) + 4 h + r % 4 (register r)
template <int D>
__device__ __forceinline__ void gram_tile(const Lane& l) {
  const int pb = l.w & 1, ab = l.w >> 1;
  const int ra = 32 * pb + l.q, rb = 32 * ab + l.q;
  f32x16 g = f32x16{};
#pragma unroll
  for (int k = 0; k < kKS<D>; ++k) {
    const bf16x8 a = __builtin_bit_cast(bf16x8, s_prow<D>[frag_at<D>(ra, k, l.h)]);
    const bf16x8 b = __builtin_bit_cast(bf16x8, s_prow<D>[frag_at<D>(rb, k, l.h)]);
    g = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, g, 0, 0, 0);
  }
  const float ci = s_pinv[rb];
  float* row = &s_g[rb * kGS + 32 * pb + 4 * l.h];
#pragma unroll
  for (int gg = 0; gg < 4; ++gg) {
    const float4 v = *reinterpret_cast<const float4*>(&s_pinv[32 * pb + 8 * gg + 4 * l.h]);
    const float pv[4] = {v.x, v.y, v.z, v.w};
    float4 o;
    o.x = g[4 * gg + 0] * ci * pv[0];
    o.y = g[4 * gg + 1] * ci * pv[1];
    o.z = g[4 * gg + 2] * ci * pv[2];
    o.w = g[4 * gg + 3] * ci * pv[3];
    *reinterpret_cast<float4*>(&row[8 * gg]) = o;
  }
}

// a value in the key order's high word
__device__ __forceinline__ uint32_t ordv(float v) {
  return __float_as_uint(v) ^ ((uint32_t)((int32_t)__float_as_uint(v) >> 31) | 0x80000000u);
}
constexpr uint32_t kDead = 0x007fffffu;  // ordv(-inf)

// Common rounds in one asm loop: no tie, no stop test passed, list not full. Returns 1: the list is
// full (np == nr); 2: the caller's slow path (m <= bcut, or equal values) with m and bal =
// ballot(cur == m). The stop tests and the tie resolution sit off the common path (one scalar
// compare). The Gram row sits in v[2:65] (g0 then g1, contiguous by the operand constraints), read
// by one SGPR-indexed v_mov (s_set_gpr_idx_on); the pick's and the record's lane masks come from
// SALU shifts. Wait states as hipcc schedules these pairs: 2 between a DPP source write and the
// DPP.
__device__ __forceinline__ int common_rounds(
    uint32_t& cur, float& pna, float& lsa, int& rec_slot, int& np, uint64_t& picked, uint32_t& m,
    uint64_t& bal, const f32x32& g0, const f32x32& g1, uint32_t bcut, int nr, float nmu, float ninf) {
  uint64_t vm_, sh_;
  int status, sc_, spk_;
  float vt_, vga_, vpk_;
  asm volatile(
      "L_rt_%=:\n\t"
      "s_nop 1\n\t"
      "v_max_u32_dpp %[t], %[cur], %[cur] quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
      "s_nop 1\n\t"
      "v_max_u32_dpp %[t], %[t], %[t] quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
      "s_nop 1\n\t"
      "v_max_u32_dpp %[t], %[t], %[t] row_half_mirror row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
      "s_nop 1\n\t"
      "v_max_u32_dpp %[t], %[t], %[t] row_mirror row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
      "s_nop 1\n\t"
      "v_max_u32_dpp %[t], %[t], %[t] row_bcast:15 row_mask:0xa bank_mask:0xf\n\t"
      "s_nop 1\n\t"
      "v_max_u32_dpp %[t], %[t], %[t] row_bcast:31 row_mask:0xc bank_mask:0xf\n\t"
      "s_nop 1\n\t"
      "v_readlane_b32 %[m], %[t], 63\n\t"
      "s_cmp_le_u32 %[m], %[bcut]\n\t"
      "s_nop 0\n\t"
      "v_cmp_eq_u32_e64 %[bal], %[m], %[cur]\n\t"
      "s_cbranch_scc1 L_rs_%=\n\t"
      "s_bcnt1_i32_b64 %[c], %[bal]\n\t"
      "s_cmp_gt_u32 %[c], 1\n\t"
      "s_cbranch_scc1 L_rs_%=\n\t"
      "s_ff1_i32_b64 %[pk], %[bal]\n\t"
      "s_set_gpr_idx_on %[pk], gpr_idx(SRC0)\n\t"
      "v_mov_b32 %[ga], v2\n\t"
      "s_set_gpr_idx_off\n\t"
      "s_lshl_b64 %[sh], 1, %[pk]\n\t"
      "s_lshl_b64 %[vm], 1, %[np]\n\t"
      "v_mov_b32 %[pkv], %[pk]\n\t"
      "v_max_f32 %[pna], %[ga], %[pna]\n\t"
      "v_cndmask_b32_e64 %[lsa], %[lsa], %[ninf], %[sh]\n\t"
      "v_fma_f32 %[t], %[nmu], %[pna], %[lsa]\n\t"
      "v_ashrrev_i32 %[ga], 31, %[t]\n\t"
      "v_bitop3_b32 %[cur], %[ga], %[t], %[c80] bitop3:0x36\n\t"
      "s_or_b64 %[pkd], %[pkd], %[sh]\n\t"
      "v_cndmask_b32_e64 %[rec], %[rec], %[pkv], %[vm]\n\t"
      "s_add_u32 %[np], %[np], 1\n\t"
      "s_cmp_lt_u32 %[np], %[nr]\n\t"
      "s_cbranch_scc1 L_rt_%=\n\t"
      "s_mov_b32 %[st], 1\n\t"
      "s_branch L_re_%=\n"
      "L_rs_%=:\n\t"
      "s_mov_b32 %[st], 2\n"
      "L_re_%=:"
      : [cur] "+v"(cur), [pna] "+v"(pna), [lsa] "+v"(lsa), [rec] "+v"(rec_slot),
        [np] "+s"(np), [pkd] "+s"(picked), [st] "=s"(status), [m] "=s"(m), [bal] "=s"(bal),
        [t] "=&v"(vt_), [ga] "=&v"(vga_), [pkv] "=&v"(vpk_), [c] "=&s"(sc_),
        [pk] "=&s"(spk_), [vm] "=&s"(vm_), [sh] "=&s"(sh_)
      : [g0] "{v[2:33]}"(g0), [g1] "{v[34:65]}"(g1), [bcut] "s"(bcut), [nr] "s"(nr),
        [nmu] "v"(nmu), [ninf] "v"(ninf), [c80] "s"(0x80000000u)
      : "scc");
  return status;
}

// ---- fast rounds over the 64 probes on wave 0 (lane a = probe slot a). The chain of a round:
// value -> wave max (fused v_max_u32_dpp) -> ballot -> pick -> Gram entry (SGPR-indexed register
// read) -> max term -> key. The round's outputs are kept in registers (lane i: output i of this
// batch) and written to LDS once after the rounds, so no LDS access, and no wait on one, sits in
// the chain.
// Wave 0 only. Reads the probes' state (s_pcand, s_pscore, s_ppen, s_pitem, s_pinv), their Gram s_g
// and the waves' bounds s_wbound; t = picks so far. Writes the batch's picks: items -> s_out[t ..],
// probe slots -> s_plist, 1/|e| -> s_lpinv, and s_state = {picks so far, picks this batch, picked
// slot mask lo, hi, forced pick position or -1}.
__device__ __forceinline__ void fast_rounds(int lane, int t, int k_out, float lambda, float mu) {
  uint64_t bound = 0ull;  // the best key outside the probes
#pragma unroll
  for (int i = 0; i < kWaves; ++i) bound = dr::umax64(bound, s_wbound[i]);
  const int pa = s_pcand[lane];
  // +0: lambda * s is never -0, so no value below is -0 either (an fma with a nonzero or +0
  // addend), and the key order needs no -0 fix-up in the chain. An empty or picked slot has lsa =
  // -inf: its value is -inf, key kDead, below every live value.
  float lsa = pa >= 0 ? lambda * s_pscore[lane] + 0.0f : -INFINITY;
  float pna = s_ppen[lane];
  f32x32 g0, g1;  // this probe's Gram row, indexed by the (uniform) pick slot
  const float4* grow = reinterpret_cast<const float4*>(&s_g[lane * kGS]);
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const float4 a = grow[i], b = grow[8 + i];
    g0[4 * i + 0] = a.x; g0[4 * i + 1] = a.y; g0[4 * i + 2] = a.z; g0[4 * i + 3] = a.w;
    g1[4 * i + 0] = b.x; g1[4 * i + 1] = b.y; g1[4 * i + 2] = b.z; g1[4 * i + 3] = b.w;
  }
  const uint32_t bhi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(bound >> 32));
  const uint32_t blo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)bound);
  // a real bound's value is finite (bhi > kDead); bhi = 0: no candidate outside the probes. A round
  // stops at m <= bcut, except a tie with a real bound that the probe wins by a lower position.
  const uint32_t bcut = bhi > kDead ? bhi : kDead;
  // t >= 1 here whenever a live candidate exists (the first pick is made before the batches: values
  // only fall from then on, which the bound needs), so every live max term is finite
  uint32_t cur = ordv(fmaf(-mu, pna, lsa));
  int rec_slot = -1;  // lane i: probe slot of pick i of this batch
  const int t0 = t, nr = k_out - t;
  int np = 0;
  uint64_t picked = 0;
  uint32_t m = 0u;
  const float nmu = -mu, ninf = -INFINITY;
  for (;;) {
    uint64_t bal;
    if (common_rounds(cur, pna, lsa, rec_slot, np, picked, m, bal, g0, g1, bcut, nr, nmu, ninf) == 1)
      break;  // the list is full
    // slow path (rare): a stop test, or equal values at the top
    if (m <= bcut) {
      if (m != bhi) break;  // below a real bound, or no live probe (m = kDead)
      const uint32_t mp = dr::wave_min_u32_64(cur == m ? (uint32_t)pa : 0xffffffffu);
      if (mp >= ~blo) break;  // the bound's candidate has the lower position
      bal = __ballot(cur == m && (uint32_t)pa == mp);
    } else {  // equal values: lowest candidate position wins
      const uint32_t mp = dr::wave_min_u32_64(cur == m ? (uint32_t)pa : 0xffffffffu);
      bal = __ballot(cur == m && (uint32_t)pa == mp);
    }
    const int pk = __builtin_amdgcn_readfirstlane(__builtin_ctzll(bal));
    const float ga = g0[pk & 31], gb = g1[pk & 31];
    const float g = pk < 32 ? ga : gb;
    lsa = lane == pk ? -INFINITY : lsa;
    rec_slot = lane == np ? pk : rec_slot;
    picked |= 1ull << pk;
    float nx;  // max(pna, g): one v_max_f32 (no canonicalizing copies; no NaN here)
    asm("v_max_f32 %0, %1, %2" : "=v"(nx) : "v"(g), "v"(pna));
    pna = nx;
    cur = ordv(fmaf(-mu, pna, lsa));
    if (++np == nr) break;  // the list is full
  }
  t += np;
  if (lane < np) {
    s_out[t0 + lane] = s_pitem[rec_slot];
    s_plist[lane] = rec_slot;
    s_lpinv[lane] = s_pinv[rec_slot];
  }
  if (m == kDead && bhi == 0u) {  // no live candidate left: the rest are -1
    for (int i = t + lane; i < k_out; i += 64) s_out[i] = -1;
    t = k_out;
  }
  // No probe beats the bound (>= kPPW + 1 equal values at the top of every wave that has one): the
  // bound's candidate, the best key outside the probes, is the next pick.
  const int forced = (np == 0 && t < k_out && (bhi | blo) != 0u) ? (int)~blo : -1;
  if (lane == 0) {
    s_state[0] = t;
    s_state[1] = np;
    s_state[2] = (int)(uint32_t)picked;
    s_state[3] = (int)(uint32_t)(picked >> 32);
    s_state[4] = forced;
  }
}

// picked probes of this wave leave the live set
__device__ __forceinline__ void drop_picked(uint32_t myslot, uint64_t picked, uint32_t& live) {
#pragma unroll
  for (int j = 0; j < kTiles; ++j) {
    const int sl = (int)((myslot >> (8 * j)) & 255u) - 1;
    if (sl >= 0 && ((picked >> sl) & 1ull)) live &= ~(1u << j);
  }
}

template <int D>
__global__ __launch_bounds__(kThreads) void mmr_pick_kernel(
    const int32_t* __restrict__ cand_items, const float* __restrict__ cand_scores, int C,
    const __bf16* __restrict__ E, int64_t n_items, int64_t n_users, int k_out, float lambda,
    int32_t* __restrict__ out_items, int32_t* __restrict__ err) {
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const float mu = 1.f - lambda;
#ifdef DR_MMR_DIAG
  uint64_t dg[kMgSlots] = {};
#endif
  MG_T0(t_kernel);

  const int64_t G = gridDim.x;
  for (int64_t u = blockIdx.x; u < n_users; u += G) {
    const Lane lu = opaque_lane(w);
    const bool pre = u != (int64_t)blockIdx.x;  // ids, scores and tile-0 rows prefetched
    if (pre) {
      wait_dma();
      __syncthreads();
    }
    MG_T0(t_user);
    Rows<D> brow;
    Pens pen;
    uint32_t live = load_candidates<D>(lu, cand_items, cand_scores, E, C, n_items, u, pre, err,
                                       brow, pen);
    __syncthreads();
    MG_ADD(kMgLoad, t_user);
    const bool more = u + G < n_users;
    // s_nitem / s_nscore are free from here
    if (more) prefetch_ids(lu, cand_items, cand_scores, C, u + G);
    int t = first_pick<D>(lu, lambda, brow, pen, live);  // picks so far
    if (more) {  // the next user's ids are in (every wave's DMA + a barrier): its tile-0 rows
      wait_dma();
      __syncthreads();
      prefetch_rows<D>(lu, E, n_items);
    }
    for (int batch = 0; t < k_out && batch <= k_out; ++batch) {
      const Lane lb = opaque_lane(w);
      uint32_t myslot;  // per tile: this lane's probe slot + 1
      int nprobe;       // the wave's probe count
      MG_TIMED(kMgSelect, select_probes(lb, pen, live, t, lambda, mu, myslot, nprobe));
      MG_TIMED(kMgStage, stage_probes<D>(lb, brow, myslot, nprobe);
               MG_TIMED(kMgStageBar, lds_barrier()));
      MG_TIMED(kMgGt, if (w < 4) gram_tile<D>(lb));
      MG_TIMED(kMgSync1, lds_barrier());
      MG_TIMED(kMgRounds, if (w == 0) fast_rounds(lb.lane, t, k_out, lambda, mu));
      MG_T0(t_sync2);
      lds_barrier();
      t = s_state[0];
      const int np = s_state[1];
      const uint64_t picked = (uint64_t)(uint32_t)s_state[2] | ((uint64_t)(uint32_t)s_state[3] << 32);
      const int forced = s_state[4];
      MG_ADD(kMgSync2, t_sync2);
      MG_T0(t_fold);
      if (t >= k_out) break;  // the list is full: no fold, no further batch
      if (forced >= 0) {
        stage_pick0<D>(lb, forced, t, brow, live);
        t += 1;
        lds_barrier();
        if (t >= k_out) break;
        fold<D>(lb, 1, brow, pen);
      } else {
        fold<D>(lb, np, brow, pen);
        drop_picked(myslot, picked, live);
      }
      MG_ADD(kMgFold, t_fold);
      MG_COUNT(kMgBatches);
    }
    __syncthreads();
    for (int i = lu.tid; i < k_out; i += kThreads) out_items[u * k_out + i] = s_out[i];
  }
#ifdef DR_MMR_DIAG
  MG_ADD(kMgTotal, t_kernel);
  if ((threadIdx.x & 63) == 0)
    for (int i = 0; i < kMgSlots; ++i) atomicAdd(&g_mmr_diag[w][i], (unsigned long long)dg[i]);
#endif
}

}  // namespace

#ifdef DR_MMR_DIAG
// host: copy (and optionally reset) the per-wave phase totals, [8][16] u64
extern "C" int dr_mmr_diag_read(unsigned long long* out, int reset) {
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_mmr_diag), sizeof(g_mmr_diag)) != hipSuccess) return -1;
  if (reset) {
    static unsigned long long zero[kWaves][16] = {};
    if (hipMemcpyToSymbol(HIP_SYMBOL(g_mmr_diag), zero, sizeof(zero)) != hipSuccess) return -1;
  }
  return 0;
}
#endif

extern "C" int dr_mmr_rerank(const int32_t* cand_items, const float* cand_scores, int64_t n_users,
                             int C, const void* item_table, int64_t n_items, int d, int k_out,
                             float lambda, int32_t* out_items, int32_t* err, dr_stream_t stream) {
  // n_users is not looked at, and d only after the pointers (rerank_args.h)
  static_assert(kMaxC == dr::kRerankMaxC, "the shared check's bound");
  DR_CHECK_RC(dr::check_candidates(__func__, n_users, C, k_out, lambda, dr::kMmrArgs));
  DR_CHECK_RC(dr::check_item_rows(__func__, n_items));
  if (n_users == 0) return DR_OK;
  DR_CHECK_RC(dr::check_item_table_filled(__func__, n_items));
  DR_CHECK_ARG(cand_items && cand_scores && item_table && out_items, "null pointer");
  DR_CHECK_RC(dr::check_item_width(__func__, d));
  hipStream_t s = (hipStream_t)stream;
  // persistent grid: one workgroup per CU (a user's rows take half the register file), each looping
  // over users and prefetching the next one
  const int cus = dr::persistent_cus();
  const dim3 grid((unsigned)(n_users < cus ? n_users : cus));
#define DR_MMR(DD)                                                                            \
  hipLaunchKernelGGL(mmr_pick_kernel<DD>, grid, dim3(kThreads), 0, s, cand_items, cand_scores,  \
                     C, (const __bf16*)item_table, n_items, n_users, k_out, lambda, out_items, err)
  if (d == 64) DR_MMR(64); else DR_MMR(128);
#undef DR_MMR
  DR_CHECK_LAUNCH();
  return DR_OK;
}
