// Shared device/host helpers for libdivrec_hip (gfx950 / CDNA4 only).
//
// Everything here is written for 64-lane wavefronts: lane = threadIdx.x & 63,
// ballots are 64-bit, cross-lane moves go through ds_bpermute (__shfl_xor).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>

#include "../../include/divrec_hip.h"

namespace dr {

// ---------------------------------------------------------------- errors
// Thread-local last-error string behind dr_last_error() (include/divrec_hip.h).
void set_error(const std::string& msg);

// Planner knobs (dr_set_plan_knob, include/divrec_hip.h): true and *v set when
// knob `id` holds a value (not NaN).
bool plan_knob(int id, double* v);

// Compute units of the current device (cached per device ordinal; 256 if the
// query fails): the grid of the persistent kernels.
int device_cus();

// device_cus() CAPPED by the DR_KNOB_SCAN_SLOTS test knob (applied when it is
// below the count): the grid of the re-rank kernels, so that tests reach many
// users per workgroup with few users. The score scan's planner reads the same
// knob as an OVERRIDE (score_topk.hip, scan_slots()): a value above the device's
// count is honoured there too, which is how plans for a larger device are tested.
int persistent_cus();

#define DR_CHECK_ARG(cond, msg)                                   \
  do {                                                            \
    if (!(cond)) {                                                \
      ::dr::set_error(std::string(__func__) + ": " + (msg));      \
      return DR_EINVAL;                                           \
    }                                                             \
  } while (0)

#define DR_CHECK_HIP(expr)                                                        \
  do {                                                                            \
    hipError_t e_ = (expr);                                                       \
    if (e_ != hipSuccess) {                                                       \
      ::dr::set_error(std::string(__func__) + ": " #expr " -> " +                 \
                      hipGetErrorString(e_));                                     \
      return DR_EHIP;                                                             \
    }                                                                             \
  } while (0)

#define DR_CHECK_LAUNCH() DR_CHECK_HIP(hipGetLastError())

// ---------------------------------------------------------------- types
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kWave = 64;

__device__ __forceinline__ int lane_id() { return threadIdx.x & 63; }

// The two bf16 values of a packed word as fp32: element 0 (low half), element 1.
__device__ __forceinline__ float bf16_lo(uint32_t u) { return __uint_as_float(u << 16); }
__device__ __forceinline__ float bf16_hi(uint32_t u) { return __uint_as_float(u & 0xffff0000u); }

// Is `item` in the ascending list[0, n)? N is the count's type and T the type
// the comparison is made in (an int64 id is searched without narrowing).
template <typename N, typename T>
__device__ __forceinline__ bool sorted_contains(const int32_t* __restrict__ list, N n, T item) {
  N lo = 0, hi = n;
  while (lo < hi) {
    const N mid = (lo + hi) >> 1;
    if ((T)list[mid] < item) lo = mid + 1; else hi = mid;
  }
  return lo < n && (T)list[lo] == item;
}

// Counter-based draws (sampler.hip, warp.hip): 64 bits from a hash of (seed,
// position, draw, attempt), the same on the host and on the device, so a draw
// depends on no launch geometry.
__host__ __device__ __forceinline__ uint64_t mix64(uint64_t z) {  // splitmix64 finaliser
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}

__host__ __device__ __forceinline__ uint64_t draw_bits(uint64_t seed, int64_t pos, int64_t draw,
                                                       int64_t attempt) {
  uint64_t z = mix64(seed + 0x9e3779b97f4a7c15ull * (uint64_t)(pos + 1));
  z = mix64(z ^ (0xd1b54a32d192ed03ull * (uint64_t)(draw + 1)));
  return mix64(z + 0x8cb92ba72f3d8dd7ull * (uint64_t)(attempt + 1));
}

// LDS written by the lanes of a wave is visible to its other lanes after this
// (one wave's private LDS area: no workgroup barrier).
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Workgroup barrier that orders LDS traffic only: the wave's LDS operations
// are waited for (lgkmcnt), its global loads and stores stay in flight.
// __syncthreads() also waits for those (vmcnt(0)), which puts a store's whole
// round trip into every step of a loop that stores a result per step.
__device__ __forceinline__ void lds_barrier() {
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

// v_mfma_f32_32x32x16: accumulator register q of a lane of half-wave h
// (lane >> 5) holds row tile_row(q, h) of column (lane & 31).
__host__ __device__ constexpr int tile_row(int q, int h) { return (q & 3) + 8 * (q >> 2) + 4 * h; }

// LDS image of rows of D bf16: the 16-B chunk c of row r sits at chunk
// c ^ swz(r), which spreads the 32 rows that one A-fragment ds_read_b128
// touches over distinct 16-B bank slots.
template <int D>
struct RowSwizzle {
  static constexpr int CPR = D / 8;                               // 16-B chunks per row
  static constexpr int RPB = (2 * D >= 256) ? 1 : 256 / (2 * D);  // rows per 256-B bank row
  static constexpr int SWM = (CPR < 16 ? CPR : 16) - 1;
  __host__ __device__ static constexpr int swz(int r) { return (r / RPB) & SWM; }
};

// ---------------------------------------------------------------- top-K keys
// A (score, item) pair is packed into one 64-bit key whose unsigned order is
// the ranking order of the reference path with its tie-break made explicit:
// score descending, then item id ascending (divrec/train/utils.py:73 ranks with
// an unstable argsort; SURVEY.md §8 quirk 3 fixes ties to "id asc").
//   key = ord(score) << 32 | ~item
// ord() maps fp32 to an order-preserving uint32 after canonicalising -0 to +0
// (so -0 and +0 tie, as they do under float comparison). Key 0 = empty slot.
__device__ __forceinline__ uint32_t f32_to_ord(float f) {
  f = f + 0.0f;  // -0.0 -> +0.0 (round-to-nearest); not folded without fast-math
  uint32_t u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float ord_to_f32(uint32_t o) {
  uint32_t u = (o & 0x80000000u) ? (o & 0x7fffffffu) : ~o;
  return __uint_as_float(u);
}
__device__ __forceinline__ uint64_t make_key(float score, uint32_t item) {
  return ((uint64_t)f32_to_ord(score) << 32) | (uint64_t)(~item);
}
__device__ __forceinline__ uint32_t key_item(uint64_t key) { return ~(uint32_t)key; }
__device__ __forceinline__ float key_score(uint64_t key) {
  return ord_to_f32((uint32_t)(key >> 32));
}

__device__ __forceinline__ uint64_t shfl_xor_u64(uint64_t v, int mask) {
  uint32_t lo = (uint32_t)v, hi = (uint32_t)(v >> 32);
  lo = __shfl_xor(lo, mask);
  hi = __shfl_xor(hi, mask);
  return ((uint64_t)hi << 32) | lo;
}

__device__ __forceinline__ uint64_t umax64(uint64_t a, uint64_t b) { return a > b ? a : b; }
__device__ __forceinline__ uint64_t umin64(uint64_t a, uint64_t b) { return a < b ? a : b; }

// Wave-wide bitonic sort, DESCENDING, of N = 64*P keys held in registers.
// Element e lives in lane e / P, register e % P. Every loop bound is a
// compile-time constant, so the network unrolls and all register indices are
// static (no scratch). Strides < P are register swaps inside a lane; strides
// >= P exchange with lane ^ (stride / P).
template <int P>
__device__ __forceinline__ void wave_sort_desc(uint64_t (&key)[P]) {
  constexpr int N = 64 * P;
  const int lane = lane_id();
#pragma unroll
  for (int k = 2; k <= N; k <<= 1) {
#pragma unroll
    for (int j = k >> 1; j > 0; j >>= 1) {
      if (j < P) {
#pragma unroll
        for (int i = 0; i < P; ++i) {
          if ((i & j) == 0) {
            const int e = lane * P + i;
            const bool desc = (e & k) == 0;
            uint64_t a = key[i], b = key[i | j];
            uint64_t mx = umax64(a, b), mn = umin64(a, b);
            key[i] = desc ? mx : mn;
            key[i | j] = desc ? mn : mx;
          }
        }
      } else {
        const int lm = j / P;
        const bool lower = (lane & lm) == 0;
#pragma unroll
        for (int i = 0; i < P; ++i) {
          const int e = lane * P + i;
          const bool desc = (e & k) == 0;
          uint64_t o = shfl_xor_u64(key[i], lm);
          const bool keep_max = (lower == desc);
          key[i] = keep_max ? umax64(key[i], o) : umin64(key[i], o);
        }
      }
    }
  }
}

// Select register i of a lane-local array with a runtime index without
// dynamic register indexing (which would spill to scratch).
template <int P, typename T>
__device__ __forceinline__ T select_reg(const T (&v)[P], int idx) {
  T r = v[0];
#pragma unroll
  for (int i = 1; i < P; ++i) r = (idx == i) ? v[i] : r;
  return r;
}
// The same for 64-bit keys as a masked OR: at P >= 16 hipcc turns the select
// chain above back into an indexed access of a stack copy (scratch).
template <int P>
__device__ __forceinline__ uint64_t select_key(const uint64_t (&v)[P], int idx) {
  uint64_t r = 0ull;
#pragma unroll
  for (int i = 0; i < P; ++i) r |= v[i] & (0ull - (uint64_t)(idx == i));
  return r;
}

__device__ __forceinline__ uint64_t readlane_u64(uint64_t v, int lane) {
  uint32_t lo = __builtin_amdgcn_readlane((int)(uint32_t)v, lane);
  uint32_t hi = __builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), lane);
  return ((uint64_t)hi << 32) | lo;
}

// Three wave sums, three summation orders (their results may differ in the
// last bit, so one does not stand in for another):
//   wave_sum_f32      the shuffle sum: six ds_bpermute round trips, every lane
//                     gets the sum;
//   wave_sum_dpp_f32  the uniform DPP sum (below): row_bcast steps carry the
//                     result into lane 63, which is read back wave-uniform;
//   wave_allsum_f32   the all-lanes sum (below): DPP rotations and
//                     v_permlane16/32_swap, VALU only, every lane gets the sum;
//                     half_sum_f32 is its 32-lane part.
__device__ __forceinline__ float wave_sum_f32(float v) {
#pragma unroll
  for (int m = 32; m > 0; m >>= 1) v += __shfl_xor(v, m);
  return v;
}

// ---------------------------------------------------------------- DPP reductions
// Wave reductions on DPP lane moves (VALU, no LDS round trip), for the serial
// chains of the re-rank kernels: quad swaps, half-row and row mirrors, then
// row_bcast15 / 31 carry the running result into lane 63, which is read back
// as a wave-uniform value.
template <int CTRL, int ROW_MASK = 0xF>
__device__ __forceinline__ uint64_t dpp_u64(uint64_t v) {  // v itself in masked-out rows
  const int lo = (int)(uint32_t)v, hi = (int)(uint32_t)(v >> 32);
  const int nlo = __builtin_amdgcn_update_dpp(lo, lo, CTRL, ROW_MASK, 0xF, false);
  const int nhi = __builtin_amdgcn_update_dpp(hi, hi, CTRL, ROW_MASK, 0xF, false);
  return ((uint64_t)(uint32_t)nhi << 32) | (uint32_t)nlo;
}
__device__ __forceinline__ uint64_t wave_max_u64(uint64_t v) {
  v = umax64(v, dpp_u64<0xB1>(v));        // quad_perm [1,0,3,2]
  v = umax64(v, dpp_u64<0x4E>(v));        // quad_perm [2,3,0,1]
  v = umax64(v, dpp_u64<0x141>(v));       // row_half_mirror
  v = umax64(v, dpp_u64<0x140>(v));       // row_mirror: every lane holds its row's max
  v = umax64(v, dpp_u64<0x142, 0xA>(v));  // row_bcast15 into rows 1 and 3
  v = umax64(v, dpp_u64<0x143, 0xC>(v));  // row_bcast31 into rows 2 and 3
  return readlane_u64(v, 63);
}
__device__ __forceinline__ uint32_t wave_min_u32_64(uint32_t v) {
  v = min(v, (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0xB1, 0xF, 0xF, false));
  v = min(v, (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x4E, 0xF, 0xF, false));
  v = min(v, (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x141, 0xF, 0xF, false));
  v = min(v, (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x140, 0xF, 0xF, false));
  v = min(v, (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x142, 0xA, 0xF, false));
  v = min(v, (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x143, 0xC, 0xF, false));
  return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}
// Max over the wave's 64 lanes (lanes = 64) or over lanes 0..31 (lanes = 32)
// by fused v_max_u32_dpp steps (one VALU each: the reduction is the latency
// of the serial chains below); the result is read from the last lane.
template <int LANES>
__device__ __forceinline__ uint32_t wmax_u32(uint32_t v) {
  v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xF, 0xF, true));
  v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xF, 0xF, true));
  v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x141, 0xF, 0xF, true));
  v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x140, 0xF, 0xF, true));
  v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xA, 0xF, true));
  if constexpr (LANES == 64) {
    v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xC, 0xF, true));
    return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
  } else {
    return (uint32_t)__builtin_amdgcn_readlane((int)v, 31);
  }
}
template <int CTRL, int ROW_MASK = 0xF>
__device__ __forceinline__ float dpp_f32(float v) {  // 0 in masked-out rows
  return __int_as_float(
      __builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, ROW_MASK, 0xF, false));
}
__device__ __forceinline__ float quad_sum_f32(float v) {  // every lane: its quad's sum
  v += dpp_f32<0xB1>(v);
  v += dpp_f32<0x4E>(v);
  return v;
}
__device__ __forceinline__ float wave_sum_dpp_f32(float v) {  // uniform: the wave's sum
  v = quad_sum_f32(v);
  v += dpp_f32<0x141>(v);
  v += dpp_f32<0x140>(v);
  v += dpp_f32<0x142, 0xA>(v);
  v += dpp_f32<0x143, 0xC>(v);
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63));
}
// Lane g's entry of a normalised profile row (the calibrated and the xQuAD
// re-rank and their metrics): max(w_g, 0) / sum (NaN counts as 0; 0 everywhere
// for a row without positive weight). G <= 64; lanes >= G get 0.
__device__ __forceinline__ float profile_entry(const float* __restrict__ row, int G, int lane) {
  const float w = fmaxf(lane < G ? row[lane] : 0.f, 0.f);
  const float sum = wave_sum_dpp_f32(w);
  return sum > 0.f ? w / sum : 0.f;
}
// v[lane] and v[lane ^ 16] / v[lane ^ 32], in an order that depends on the
// lane's half (v_permlane16/32_swap: one VALU, no LDS round trip): for
// commutative merges.
struct F32Pair { float a, b; };
__device__ __forceinline__ F32Pair swap16_f32(float v) {
  const auto p = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  return {__uint_as_float(p[0]), __uint_as_float(p[1])};
}
__device__ __forceinline__ F32Pair swap32_f32(float v) {
  const auto p = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  return {__uint_as_float(p[0]), __uint_as_float(p[1])};
}
// The two 16-lane rows of a 32-lane group added.
__device__ __forceinline__ float add_rows_f32(float v) {
  const F32Pair p = swap16_f32(v);
  return p.a + p.b;
}
// Sum over a 32-lane group in VALU only; every lane of the group gets it. Both
// groups of a wave may call it under different exec masks: no step crosses
// the group.
__device__ __forceinline__ float half_sum_f32(float v) {
  v = quad_sum_f32(v);
  v += dpp_f32<0x124>(v);  // row_ror:4
  v += dpp_f32<0x128>(v);  // row_ror:8
  return add_rows_f32(v);
}
__device__ __forceinline__ float wave_allsum_f32(float v) {  // every lane: the wave's sum
  const F32Pair p = swap32_f32(half_sum_f32(v));
  return p.a + p.b;
}

// ---------------------------------------------------------------- VMEM waits
// s_waitcnt vmcnt(N) only (expcnt / lgkmcnt left at their maxima): what every
// user of the LDS-DMA below waits with.
template <int N>
__device__ __forceinline__ void wait_vmcnt() {
  static_assert(N >= 0 && N < 64, "vmcnt range");
  __builtin_amdgcn_s_waitcnt((N & 0xF) | ((N >> 4) << 14) | (0x7 << 4) | (0xF << 8));
}
// Two waits for a wave-uniform run-time count n. wait_vmcnt_dyn rounds n down
// to a power of two (waits for a little more than required, always correct):
// six scalar compares, for a wait at every stage of a long loop.
// wait_vm_exact<LO, HI> waits for exactly n in [LO, HI] (a binary search over
// the immediates, six scalar branches), for a pipeline whose younger loads
// must stay in flight.
__device__ __forceinline__ void wait_vmcnt_dyn(int n) {
  if (n >= 32) wait_vmcnt<32>();
  else if (n >= 16) wait_vmcnt<16>();
  else if (n >= 8) wait_vmcnt<8>();
  else if (n >= 4) wait_vmcnt<4>();
  else if (n >= 2) wait_vmcnt<2>();
  else if (n >= 1) wait_vmcnt<1>();
  else wait_vmcnt<0>();
}
template <int LO, int HI>
__device__ __forceinline__ void wait_vm_exact(int n) {
  if constexpr (LO == HI) {
    asm volatile("s_waitcnt vmcnt(%c0)" : : "i"(LO) : "memory");
  } else {
    constexpr int MID = (LO + HI) / 2;
    if (n <= MID) wait_vm_exact<LO, MID>(n);
    else wait_vm_exact<MID + 1, HI>(n);
  }
}

// ---------------------------------------------------------------- LDS-DMA
// global_load_lds_*: a wave's 64 dwords (or 16-B chunks) go from global memory
// straight into LDS, lane l's at M0 + l * 4 (or 16), with no VGPR in between;
// the load counts in vmcnt like any other. lds_base is the wave-uniform LDS
// byte address for M0: the caller makes it uniform (readfirstlane) where it
// computes it. The s_nop 0 separates the M0 write from the DMA that reads it.

// LDS byte address of a __shared__ object
__device__ __forceinline__ uint32_t lds_addr(const void* p) {
  return (uint32_t)(uintptr_t)((const __attribute__((address_space(3))) char*)p);
}

#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Winline-asm"
// one dword / one 16-B chunk per lane from the lane's own 64-bit address
__device__ __forceinline__ void lds_dma_b32(const void* src, uint32_t lds_base) {
  asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dword %0, off"
               : : "v"(src), "s"(lds_base) : "memory", "m0");
}
__device__ __forceinline__ void lds_dma_b128(const void* src, uint32_t lds_base) {
  asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, off"
               : : "v"(src), "s"(lds_base) : "memory", "m0");
}
// one 16-B chunk per lane from a wave-uniform base (an SGPR pair) plus the
// lane's 32-bit byte offset
__device__ __forceinline__ void lds_dma_b128(const char* base, uint32_t off, uint32_t lds_base) {
  asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1"
               :
               : "v"(off), "s"(base), "s"(lds_base)
               : "memory", "m0");
}
#pragma clang diagnostic pop

inline int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

// Grid of a persistent kernel whose workgroups loop over the work: as many
// workgroups per CU as are resident at once (the kernel's own occupancy;
// fallback_per_cu if the query fails) over persistent_cus() CUs, and no more
// than the work needs. The DR_KNOB_SCAN_SLOTS cap applies through
// persistent_cus(), so tests reach many units per workgroup with little work.
template <typename Kernel>
dim3 persistent_grid(Kernel kernel, int threads, int64_t blocks_needed, int fallback_per_cu) {
  int per_cu = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, threads, 0) != hipSuccess ||
      per_cu < 1)
    per_cu = fallback_per_cu;
  const int64_t cap = (int64_t)persistent_cus() * per_cu;
  return dim3((unsigned)(blocks_needed < cap ? blocks_needed : cap));
}

}  // namespace dr
