// What the host side of dr_score_topk (csrc/score_topk.hip) needs of the
// streaming score scan (csrc/score_scan.h), and the one place its shapes are
// computed: geometry constants, the kernel's compile-time shape (ScanShape),
// its arguments and launch plan. No device code.
#pragma once

#include "common.h"

namespace dr_topk {

// The diagnostic build's counter slots (DR_TOPK_DIAG, score_scan.h).
// The stage boundary is split in four: the exact-count vmcnt wait, the
// barrier wait, the refill's DMA issue, and the stretch from the end of
// boundary() to the first MFMA of the stage (kDgBFirst, also part of kDgMma;
// kDgBMark holds its start stamp).
enum {
  kDgTotal, kDgPrologue, kDgBoundary, kDgMma, kDgHits, kDgEnqueue, kDgDrain, kDgFlush,
  kDgNTiles, kDgNEnqueue, kDgNDrain, kDgNFlush, kDgNStages, kDgRealtime,
  kDgBWait, kDgBBarrier, kDgBIssue, kDgBFirst, kDgBMark, kDgSlots = 24
};

// Geometry. Every alternative measured against these values lost and was
// removed (DESIGN.md §3.1, A/B records under profiles/): one wave per SIMD
// (rounds 2 and 5), 12 / 16 waves at d <= 64, SIMD-pair priorities, two
// accumulator sets in ping-pong, the A fragments read per half chain, other
// stage sizes, slacks and flush gaps; in the direct survivor path
// (enqueue_ut, profiles/survivor_regs/) per-user key counts in registers
// instead of the LDS atomic, and v_xad_u32 for the A-fragment addresses.
// The one -D knob kept is the d = 128
// stage size (DR_STAGE_BYTES_WIDE, tools/build_variants.sh), re-measured in
// round 6 with PMC FETCH beside the time at the headline (1M x 10M, k = 100;
// profiles/r06/stage_fetch/): 72 KB 1770 ms, main-scan FETCH 227.6 GB;
// 64 KB 1776 ms, 243.0 GB. 72 KB wins both.
// Units (profiles/scan_units/): XCDs differ in speed persistently (1M x 10M:
// their mean workgroup lifetimes span 1604-1643 ms), so under the static unit
// loop the mean workgroup idled 27 ms (1.6 %) at the end of the seeded main
// scan. Its workgroups now claim units from a device queue
// (TopkArgs::unit_queue) and the tail chunks are graded, longest first
// (tail_chunk_bounds): idle 6.7 ms; one-process A/B 1535.6 -> 1499.0 ms at the
// headline (-2.4 %; the queue alone, on equal chunks, 1527.6), 220.8 -> 217.4
// at 1M x 1.25M, 1974.0 -> 1965.8 at k = 1000, lists identical.
#ifndef DR_STAGE_BYTES_WIDE
#define DR_STAGE_BYTES_WIDE 73728  // ring slot for d = 128 (9 tiles: 72 KB)
#endif
constexpr int kStageBytesOther = 32768;  // ring slot for d = 256 / 512 (three slots)
constexpr int kRingOther = 3;
constexpr int kNutWide = 4;           // user tiles of 32 per wave for d = 128
constexpr int kNutNarrow = 8;         // for d <= 64 (+14 % at d = 64, 1M x 1M, against 4)
constexpr int kFlushGap = 96;         // new keys a buffer takes past k + kSlack before compaction
// Survivors are staged in LDS and resolved per stage for d <= 64 (twice as
// dense per MFMA there: 4 % faster) and for d = 128 long lists (below),
// stored directly for other d >= 128 (4 % faster there at k = 100).
constexpr int kStageBlocks = 64;  // staged lane blocks per wave (>= 64: one user tile always fits)

// Waves per workgroup of a scan (one workgroup per CU): two per SIMD, 256
// VGPRs each.
constexpr int kWavesScan = 8;
constexpr int kTileItems = 32;
constexpr int kSlack = 32;  // keys kept beyond k by a compaction

// Stage geometry per row width. d = 128: two 72-KB slots (one barrier per
// 9 tiles; measured against three 32-KB slots: +2 % at 10M items, +6 % at
// 1.25M, where the survivor stream makes per-stage wave imbalance larger;
// round 5: against two 64-KB slots -0.4 to -0.8 % at 10M, -0.35 to -0.65 % at
// k = 1000, +0.1 % at 1.25M; three 48-KB slots +1 to +2.6 %). d <= 64 (its
// LDS survivor staging needs room): two 56-KB slots, a barrier every 14 tiles
// at d = 64 (round 5, two 48-KB slots against three 32-KB: -0.4 to -0.9 % at
// config 2, -1.6 % at d = 32; four 24-KB slots +3.5 %; 56 KB, with the
// compaction histogram moved into the staging area, against 48 KB: -0.7 to
// -1.7 % at config 2, -0.25 % at d = 32; the stage margin of 448 keys puts
// k = 100 on CAP 1024 there). d = 256 spills with 64-KB stages.
constexpr int kStageBytesNarrow = 57344;  // ring slot for d <= 64
// Long lists at d = 128 (CAP 2048, k > ~670): survivors are dense enough
// (k = 1000: direct stores were 16 % of wave time) that the d <= 64 staging
// pays there too (round 6: 2046 -> 2009 ms at 1M x 10M, k = 1000, lists
// identical, profiles/r06/long_staged/); its LDS area (8 waves x 4.6 KB) fits
// beside two 56-KB slots (7 tiles) instead of 72-KB ones.
constexpr bool long_staged(int w, int cap) { return w == 128 && cap == 2048; }
constexpr int kStageBytesLong = 57344;
constexpr int stage_bytes_for(int w, int cap) {
  return long_staged(w, cap) ? kStageBytesLong
       : w == 128 ? DR_STAGE_BYTES_WIDE : (w <= 64 ? kStageBytesNarrow : kStageBytesOther);
}
// item rows per stage (whole tiles): the most new keys a user gets per stage
constexpr int stage_items(int w, int cap) {
  return stage_bytes_for(w, cap) / (kTileItems * w * 2) * kTileItems;
}
// ring slots: two (one stage ahead) for d <= 128, three for wider rows
constexpr int ring_for(int w) { return w <= 128 ? 2 : kRingOther; }

// Which scans leave the ring refill to waves 0-3 (TileGeom::ISSUERS = 4; the
// comment at the kernel's boundary() has the why): the bf16 d = 128 main
// scans and rescans with 72-KB stages. One-process A/B against eight issuers
// (profiles/refill_half/): -1.4 to -2.2 % at 1M x 10M, k = 100, -0.9 % at
// 1M x 1.25M; the mirror image (waves 4-7 issue) +0.35 % at the headline.
// Kept on eight issuers: the staged long-list instance (k = 1000: -0.9 % on
// one machine, +0.3 to +0.7 % in three records on another), d <= 64 (config 2:
// inside the parent arm's spread), the sample scans (1 % of the headline
// step: no A/B resolves them), fp32 and d >= 256 (not measured).
constexpr bool half_issue(int w, int cap, bool f32, bool gmax) {
  return w == 128 && !f32 && !gmax && !long_staged(w, cap);
}

// Which scans run on v_mfma_f32_16x16x32_bf16 instead of 32x32x16: the same
// set, which holds every scan that stores keys of a k <= ~670 list at d = 128
// (main scan and both rescan tiers), so all keys of one list come from one
// MFMA shape (the two may round their fp32 sums differently). Cycles per flop
// are equal; the chip holds a higher clock on the 16x16x32 stream. One-process
// A/B against the 32x32x16 form of the same scans (profiles/mfma16/): -10.5 %
// at 1M x 10M, k = 100, -6.5 % at 1M x 1.25M (DESIGN.md §3.1 "The other MFMA
// shape"). The sample scans, the staged long-list instance, other widths and
// fp32 keep 32x32 shapes (not measured).
constexpr bool mfma16_scan(int w, int cap, bool f32, bool gmax) {
  return half_issue(w, cap, f32, gmax);
}

// D = W, the row's width in bf16 units (row bytes / 2); HALF: half_issue()
template <int D, int CAP, bool HALF = false>
struct TileGeom : dr::RowSwizzle<D> {  // CPR, swz(row): the stage's XOR swizzle
  static constexpr int WAVES = kWavesScan;
  static constexpr int THREADS = WAVES * 64;
  static constexpr int ISSUERS = HALF ? 4 : WAVES;       // waves that issue the ring refill
  static constexpr int STAGE_BYTES = stage_bytes_for(D, CAP);  // one LDS ring slot
  static constexpr int RING = ring_for(D);                // slots (RING - 1 stages in flight)
  // LDS-DMA instructions per issuing wave per stage (one moves 64 * 16 B)
  static constexpr int LPT = STAGE_BYTES / 16 / (ISSUERS * 64);
  static constexpr int KSTEPS = D / 16;                 // MFMA k-steps per row
  static constexpr int TILE_BYTES = kTileItems * D * 2;
  static constexpr int MARGIN = stage_items(D, CAP);    // max new keys per user per stage
  static constexpr int SR = MARGIN / kTileItems;        // row tiles per stage
  static_assert(LPT >= 1 && STAGE_BYTES % (16 * ISSUERS * 64) == 0, "stage geometry");
  static_assert(RING >= 2, "ring depth");
  static_assert(SR >= 1, "a stage holds at least one tile");
};

// User tiles (of 32) per wave. The B fragments take NU_T*KSTEPS*4 VGPRs (128 at
// d=128, NU_T=4; 128 at d=64, NU_T=8). The tiles are scored in groups of at
// most four against each item tile, one accumulator set (4*16 VGPRs) reused
// by the groups, so narrow rows can hold more users per wave.
constexpr int nut_for(int w) {
  return w >= 512 ? 1 : (w >= 256 ? 2 : (w <= 64 ? kNutNarrow : kNutWide));
}
constexpr int ngroup_for(int w) { return nut_for(w) > 4 ? nut_for(w) / 2 : nut_for(w); }
// users of one workgroup (one unit's user block): 32 per user tile of each wave
constexpr int users_per_wg(int w) { return nut_for(w) * 32 * kWavesScan; }

// Every compile-time quantity of score_scan_kernel<W, CAP, SEEDED, F32, GMAX>.
template <int W, int CAP, bool SEEDED, bool F32, bool GMAX>
struct ScanShape {
  static_assert(!(GMAX && SEEDED), "tile-max scans are the (unseeded) sample scans");
  static constexpr int D = W;  // geometry is by row bytes: an fp32 row of d is a bf16 row of 2d
  static constexpr bool kHalf = half_issue(W, CAP, F32, GMAX);  // waves 0-3 issue the whole ring refill
  using G = TileGeom<D, CAP, kHalf>;
  static constexpr int NU_T = nut_for(D);
  static constexpr int NG = ngroup_for(D);  // user tiles per accumulator group
  static constexpr int NGRP = NU_T / NG;    // groups scored against each item tile
  static_assert(NGRP * NG == NU_T && NGRP <= 2, "user tile groups");
  static constexpr int KS = G::KSTEPS;
  // The MFMA shape. 32x32x16 (and the fp32 form): user tiles of 32, a lane's
  // 16-B chunk of a k-step is its half-wave's (2 per k-step of 16). 16x16x32
  // (M16): user tiles of 16, k-steps of 32, the chunk is the lane group's
  // (lane / 16; 4 per k-step). The wave's users, its B-fragment registers and
  // its LDS counters are the same either way.
  static constexpr bool M16 = mfma16_scan(W, CAP, F32, GMAX);
  static constexpr int TU = M16 ? 16 : 32;          // users per MFMA user tile
  static constexpr int NT = NU_T * 32 / TU;         // user tiles (thresholds) per lane
  static constexpr int KQ = M16 ? 4 : 2;            // 16-B chunks per k-step
  static constexpr int KF = KS * 2 / KQ;            // k-steps (B fragments) per user tile
  static_assert(!M16 || (NGRP == 1 && D == 128), "the 16x16x32 form is the d = 128 direct-store scan");
  static constexpr int SR = G::SR;
  static_assert(SR <= 255, "stage-relative tile field is 8 bits");
  static constexpr int kWaves = G::WAVES;
  static constexpr int UPWG = users_per_wg(D);  // users per workgroup
  static constexpr int UPW = UPWG / kWaves;     // users per wave
  static constexpr int P = 8;                   // keys per lane per compaction chunk (any CAP)
  static constexpr int kRing = G::RING;
  static constexpr int kStageBytes = G::STAGE_BYTES;
  static constexpr int kLpt = G::LPT;
  static constexpr bool kLaneOnce = W == 128 && !F32;  // issue_stage's per-stage lane addressing
  static constexpr int RING_BYTES = kRing * kStageBytes;
  // per wave: per-user key counts, radix histogram, staged survivor blocks
  // (16 scores + one 8-B record: tile | slot | h, threshold)
  static constexpr bool STAGED = D <= 64 || long_staged(D, CAP);
  static constexpr int SB = STAGED ? kStageBlocks : 0;
  // stage_ut resolves a full stage area, then stages up to 64 lanes of one
  // user tile: the area must hold a whole wave's worth of blocks
  static_assert(!STAGED || SB >= 64, "staging area smaller than a wave");
  static_assert(!STAGED || NU_T * 32 <= 256, "staged slot field is 8 bits");
  // The compaction's radix histogram (1 KB) shares the staging area: it is
  // used only by check_compact, which runs after resolve() has emptied the
  // staged blocks (stage ends, unit end).
  static constexpr int STAGE_AREA = SB * (64 + 8);
  static constexpr int WAVE_BYTES = UPW * 4 + (STAGE_AREA > 1024 ? STAGE_AREA : 1024);
  static constexpr int LDS_BYTES = RING_BYTES + kWaves * WAVE_BYTES;
  static_assert(LDS_BYTES <= 163840, "LDS budget");
  // The per-user-tile pipeline (score_scan.h) serves rows of <= 128 bytes
  // only: at d = 128 (the headline) it measured +0.4 % (a chain of 8 k-steps
  // already covers the group's hot test), and the fp32 d = 128 / bf16 d = 256
  // instances spill in the loop with it.
  static constexpr bool UTP = NU_T % 2 == 0 && W <= 64;
  static_assert(!UTP || STAGED, "the per-user-tile jobs stage their survivors");
};

// The c catalog chunks of a split tail block: rows [beg, end) of chunk j.
// Lengths are whole stages (the last chunk ends at n_items), never increase
// with j, and cover [0, n_items) once. A chunk takes half of what is left
// while that is more than an equal share and leaves every later chunk at
// least floor_items rows; from there on the rest is shared equally, as
// ceil(rest / chunks left) stages each, a chunk giving way only so that every
// later one keeps a stage (none is empty unless the catalog has fewer than c
// stages). c = 6, a floor far below n_items / 32: 1/2, 1/4, 1/8, 1/16, 1/32,
// 1/32 of the catalog. floor_items >= n_items / c never halves: c equal
// chunks of ceil(ceil(n_items / c) / stage) stages, Plan::chunk_items, the
// plan before units were claimed from a queue (DESIGN.md §3.1 "Grid tail").
// n_items < 2^31 (check_score_call), floor_items <= 2^31.
struct ChunkRange {
  int64_t beg, end;
};
__host__ __device__ inline ChunkRange tail_chunk_bounds(int64_t n_items, int c, int stage_items,
                                                        int64_t floor_items, int j) {
  const uint32_t st = (uint32_t)stage_items;
  const int S = (int)(((uint32_t)n_items + st - 1) / st);  // stages in the catalog
  const int F = (int)(((uint32_t)(floor_items < n_items ? floor_items : n_items) + st - 1) / st);
  int rem = S, pos = 0, len = 0, per = 0;
  bool spare = false;  // the equal part has a stage for every chunk
  for (int i = 0; i <= j; ++i) {
    pos += len;
    rem -= len;
    const int left = c - i;
    if (per == 0) {
      const int half = rem >> 1;
      if ((half - 1) * left >= rem) {  // half > ceil(rem / left)
        // the shortest chunk if the rest were shared equally from here
        const int rest = rem - half, later = left - 1;
        const int share = (int)(((uint32_t)rest + (uint32_t)later - 1) / (uint32_t)later);
        if (rest - (later - 1) * share >= F) {
          len = half;
          continue;
        }
      }
      per = (int)(((uint32_t)rem + (uint32_t)left - 1) / (uint32_t)left);
      per = per > 0 ? per : 1;
      spare = rem >= left;
    }
    const int most = spare ? rem - (left - 1) : rem;
    len = per < most ? per : most;
  }
  ChunkRange r;
  r.beg = (int64_t)pos * stage_items;
  r.end = (int64_t)(pos + len) * stage_items;
  r.beg = r.beg < n_items ? r.beg : n_items;
  r.end = r.end < n_items ? r.end : n_items;
  return r;
}

struct TopkArgs {
  const char* U;  // user table rows: W * 2 bytes each
  const int64_t* user_ids;
  int64_t n_users;
  int64_t n_users_pad;  // n_ublocks * UPWG: candidate buffers exist for padded users too
  const char* I;  // item slice rows: W * 2 bytes each
  int64_t n_items;
  int64_t item_base;
  int k;
  const int64_t* excl_rowptr;
  const int32_t* excl_items;
  // Units (one workgroup pass each; DESIGN.md §3.1 "grid tail"): the first
  // n_head user blocks scan the whole catalog in one unit; each of the other
  // n_ublocks - n_head ("tail") blocks is split into tail_chunks catalog chunks
  // of chunk_items rows, so the last round of a grid of whole-catalog units
  // does not leave CUs idle. Chunk 0 of every block uses the user's buffer
  // row = its position; chunk j >= 1 of tail block b uses row n_users_pad +
  // ((j - 1) * n_tail + b - n_head) * UPWG + (position within the block).
  // The chunks of a tail block are tail_chunk_bounds(n_items, tail_chunks,
  // stage items, chunk_floor): graded (longest first) where units are claimed
  // from the queue below, equal (chunk_floor = n_items) everywhere else.
  int64_t n_ublocks;
  int64_t n_head;
  int tail_chunks;
  int64_t chunk_items;  // nominal (equal) chunk length: multiple of the stage's item count
  int64_t chunk_floor;  // no graded chunk is shorter than this many rows
  // Unit queue (the seeded main scan of dr_score_topk): a zeroed device word
  // the workgroups claim their unit ids from, in id order, whenever they are
  // free (atomicAdd), so a CU that runs ahead takes more of the short last
  // units instead of idling. NULL: workgroup b runs units b, b + grid, ...
  // Buffers go by unit id either way, so the lists do not depend on it.
  uint32_t* unit_queue;
  int end_keep;         // tail chunk units compact buffers above this count at their end
  int head_keep;        // whole-catalog units compact buffers above this count at their end (0: none)
  int slack;            // keys a compaction keeps beyond k (kSlack; smaller for sample scans)
  int gap;              // new keys a buffer takes past k + slack before it is compacted
  const float* init_thr;  // [n_users_pad] starting thresholds (SEEDED scans only)
  // Second-tier rescan only (dev_split > 0): the user count is on the device,
  // so the grid's units are planned there: every user block is split into up
  // to dev_split catalog chunks (dev_split_plan), chunk buffers past the
  // blocks' chunk-0 rows, bounded by buf_blocks user blocks of buffer rows.
  int dev_split;
  int64_t buf_blocks;
  // Sample scans of the guessed thresholds (the GMAX instantiation): a user
  // keeps only the MAX of its 32 scores of a tile (one key per tile) instead of
  // every score above the threshold. The k-th best tile max is a lower bound
  // of the k-th best score (the best k tiles' maxima are k distinct items), so
  // the guessed threshold stays a valid lower bound — it only drops below the
  // exact sample rank when two of the best k sample items share a tile
  // (~k^2 / (2 S / 32) of users; the tile-transposed sample puts samples T
  // apart in a tile) — while the survivor stream of a scan from -inf shrinks
  // up to 32-fold. Keys name the tile (its row base), not an item: only their
  // scores are read.
  //   gmax == 2 (dense tile maxima, ks <= kDenseMaxKs): no keys, no
  //   counters, no compaction: every (user, tile) maximum is stored to
  //   tmax[(user / 32) * tmax_tiles + tile][user % 32] (one 128-B line per
  //   job), and topk_threshold_dense_kernel ranks each user's column. The
  //   compaction path paid one serialized buffer round trip per user when
  //   every user's buffer filled in the same stage (the whole workgroup
  //   waits at the next ring barrier).
  int gmax;
  float* tmax;
  int64_t tmax_tiles;
  // Small catalogs (round 6): the plan made CAP >= n_items, so every key of
  // the unit fits its buffer and nothing is ever compacted (keep_all = 1):
  // the finalize sorts all of them. An unseeded scan of a short catalog
  // otherwise compacted each user's buffer several times from -inf, serially
  // per wave, while the catalog's few tiles left the MFMA idle.
  int keep_all;
  // Fallback rescan only: the user count lives on the device (n_users and
  // n_ublocks above are its upper bounds), and pos_map[p] is the caller's
  // position of list entry p (its exclusion row). NULL otherwise.
  const int32_t* n_users_dev;
  const int64_t* pos_map;
  uint64_t* cand;  // [buffer rows][CAP] keys (unsorted)
  int32_t* cnt;    // [buffer rows] valid keys per buffer
  uint64_t* diag;  // [gridDim.x * waves][kDgSlots] in DR_TOPK_DIAG builds
};

// Chunking of a second-tier rescan, computed where the failing-user count is
// (on the device; the scan and its finalize compute the same plan): nb user
// blocks share `grid` workgroups, so each block's catalog is split into
// c ~ grid / nb chunks (at most max_c, at least min_chunk rows each, and no
// more chunk buffers than buf_blocks blocks of rows hold); chunk length is a
// whole number of stages.
struct DevSplit {
  int chunks;
  int64_t chunk_items;
};
__host__ __device__ inline DevSplit dev_split_plan(int64_t nb, int64_t grid, int max_c,
                                                   int64_t buf_blocks, int64_t n_items,
                                                   int64_t stage_items) {
  constexpr int64_t kMinChunk = 16384;
  int64_t c = nb > 0 ? grid / nb : 1;
  c = c < max_c ? c : max_c;
  const int64_t by_buf = nb > 0 ? buf_blocks / nb : 1;
  c = c < by_buf ? c : by_buf;
  const int64_t by_len = n_items / kMinChunk;
  c = c < by_len ? c : by_len;
  if (c < 1) c = 1;
  int64_t per = (n_items + c - 1) / c;
  per = (per + stage_items - 1) / stage_items * stage_items;
  DevSplit d;
  d.chunk_items = per;
  d.chunks = (int)((n_items + per - 1) / per);
  return d;
}

// ------------------------------------------------------------------ launch plan
struct Plan {
  int cap;
  int users_per_wg;
  int64_t n_ublocks;
  int64_t n_users_pad;
  int64_t n_head;       // user blocks scanned whole (one unit each)
  int tail_chunks;      // catalog chunks per tail block (1 = no split)
  int64_t chunk_items;  // tail chunk length (nominal: the equal chunks' length)
  int64_t chunk_floor;  // shortest graded chunk (tail_chunk_bounds); n_items: equal chunks
  int end_keep;         // keys a tail chunk buffer keeps at its end (0: no end compaction)
  int head_keep;        // keys a whole-catalog buffer keeps at its end (0: no end compaction)
  int slack, gap;       // compaction slack and flush gap (TopkArgs)
  int64_t buf_rows;     // candidate buffers: n_users_pad + the tail's extra chunks
  int keep_all;         // TopkArgs::keep_all: CAP >= n_items, no compaction
  int64_t all_keys;     // keep_all: the keys a buffer ends with (n_items)
  int grid;
  size_t cand_bytes;
  size_t cnt_bytes;
  int64_t head_users() const { return n_head * users_per_wg; }
};

// Launch the scan for rows of width W (bf16 units) on stream s; defined per
// dtype in score_scan_bf16.hip / score_scan_f32.hip. Returns false for a
// (W, cap) pair that has no instantiation.
bool launch_scan_bf16(const Plan& p, const TopkArgs& a, int w, bool seeded, hipStream_t s);
bool launch_scan_f32(const Plan& p, const TopkArgs& a, int w, bool seeded, hipStream_t s);

}  // namespace dr_topk
