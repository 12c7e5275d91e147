// DPP (determinantal point process) greedy MAP diversity re-rank (Chen, Zhang,
// Zhou, NeurIPS 2018): top-C candidates -> k_out picks per user. There is no
// reference symbol, as for MMR; the spec is the build's own (include/divrec_hip.h):
//   pick_t = argmax_{i live, r_i > DR_DPP_EPS} lambda * s_i + (1 - lambda) * logf(r_i)
// with r_i = det S_{Y+i} / det S_Y the residual of candidate i given the picked
// set Y under the cosine Gram S (r_i starts at exactly 1; ties -> lowest
// candidate position).
//
// Basis form, one 512-thread workgroup per user, persistent
// over users:
//   * a user's C <= 1024 candidate rows stay in registers as bf16 MFMA B
//     fragments (wave w: positions 128 w .. 128 w + 127, 8 tiles of 16; the
//     four lanes of a column hold a quarter of its row each), and each lane
//     keeps r, 1/|e|, the score and the id of two of its column's tiles;
//   * the picked rows' Gram-Schmidt basis b_0 .. b_{t-1} (fp32, <= 128 x D)
//     sits in LDS. A step takes the workgroup argmax of the 64-bit (value
//     order, ~position) key, orthogonalises the picked unit row against the
//     basis twice (CGS2, so fp32 keeps the basis orthonormal), and runs one
//     pass of the new direction v against every candidate row on the MFMA
//     (v as three bf16 rows hi + mid + lo = v exactly, so the sums are fp32
//     product sums): e_i = <v, x_i> / |v|, r_i -= e_i^2. No per-candidate
//     Cholesky vector exists anywhere.
// A step is a serial chain (argmax -> stage -> 2 x project -> pass), so its
// reductions run on DPP lane moves, not LDS round trips.
#include "common.h"
#include "rerank_args.h"

namespace {

constexpr int kThreads = 512;
constexpr int kWaves = kThreads / 64;
constexpr int kTiles = 8;                // candidate tiles of 16 per wave
constexpr int kPer = kTiles / 4;         // tiles whose state a lane keeps (2 kg, 2 kg + 1)
constexpr int kMaxC = kWaves * kTiles * 16;  // 1024
constexpr int kMaxK = 128;               // picks (basis rows) per user

using dr::bf16x8;
using dr::f32x4;

// the bf16 unpacking and the DPP wave reductions of common.h
using dr::bf16_hi;
using dr::bf16_lo;
using dr::quad_sum_f32;
using dr::wave_max_u64;

// sum of squares of 8 bf16 (one 16-B chunk of a row), even and odd elements apart
__device__ __forceinline__ void sumsq8(const uint4 u, float& even, float& odd) {
  const uint32_t pr[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    even = fmaf(bf16_lo(pr[e]), bf16_lo(pr[e]), even);
    odd = fmaf(bf16_hi(pr[e]), bf16_hi(pr[e]), odd);
  }
}

template <int D>
__global__ __launch_bounds__(kThreads) void dpp_pick_kernel(
    const int32_t* __restrict__ cand_items, const float* __restrict__ cand_scores, int C,
    const __bf16* __restrict__ E, int64_t n_items, int64_t n_users, int k_out, float lambda,
    int32_t* __restrict__ out_items, float* __restrict__ out_resid, int32_t* __restrict__ err) {
  constexpr int CPR = D / 8;          // 16-B chunks per row
  constexpr int KS = D / 32;          // MFMA k-steps per row (four chunks each)
  constexpr int BS = D + 16;         // basis row stride in floats: the 8 lanes of a
                                      // ds_read_b128 group (2 rows x 4 parts) hit 32 distinct banks
  constexpr int QC = D / 4;           // float4 columns of a row
  constexpr int NG = kThreads / QC;   // row groups of the projection sum
  __shared__ __attribute__((aligned(16))) float s_basis[kMaxK * BS];
  __shared__ __attribute__((aligned(16))) uint4 s_raw[CPR];    // the picked row as stored (bf16)
  __shared__ __attribute__((aligned(16))) uint4 s_split[3 * CPR];  // v as bf16 rows hi, mid, lo
  __shared__ __attribute__((aligned(16))) float s_v[D];        // the picked unit row, orthogonalised
  __shared__ __attribute__((aligned(16))) float4 s_part[kThreads];  // [NG][QC] partial projections
  __shared__ float s_g[kMaxK];        // <b_t', v>
  __shared__ float s_xinv;            // 1/|e| of the picked row
  __shared__ float s_nsq[2];          // |v|^2 per wave of the D threads that finish v
  __shared__ uint64_t s_wkey[kWaves];
  __shared__ int s_oitem[kMaxK];
  __shared__ float s_oresid[kMaxK];

  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int col = lane & 15, kg = lane >> 4;  // MFMA column and 16-B chunk group of this lane
  auto cpos = [&](int j) { return w * (kTiles * 16) + j * 16 + col; };  // position of (tile j, col)
  const float mu = 1.f - lambda;
  const float4* v4 = reinterpret_cast<const float4*>(s_v);

  for (int64_t u = blockIdx.x; u < n_users; u += gridDim.x) {
    // ---- the wave's 128 candidates as MFMA B fragments (tile j, column col:
    // position cpos(j)); this lane's chunks of every row, and the state (1/|e|,
    // r = 1, score, id) of its own two tiles 2 kg and 2 kg + 1
    bf16x8 brow[kTiles][KS];
    float inv[kPer] = {}, sc[kPer] = {}, r[kPer] = {};
    int32_t item[kPer] = {-1, -1};
    uint32_t alive = 0;
    int nbad = 0;
#pragma unroll
    for (int j = 0; j < kTiles; ++j) {
      const int pos = cpos(j);
      int32_t it = pos < C ? cand_items[u * C + pos] : -1;
      if (it >= 0 && (int64_t)it >= n_items) {
        nbad += kg == 0 ? 1 : 0;  // the four lanes of a column see the same id
        it = -1;
      }
      const bool ok = it >= 0;
      const uint4* src = reinterpret_cast<const uint4*>(E + (int64_t)(ok ? it : 0) * D);
      float n0 = 0.f, n1 = 0.f;
#pragma unroll
      for (int s = 0; s < KS; ++s) {
        const uint4 x = src[4 * s + kg];
        brow[j][s] = __builtin_bit_cast(bf16x8, x);
        sumsq8(x, n0, n1);
      }
      float nsq = n0 + n1;  // this lane's quarter of the row; the same sum in all four lanes
      nsq += __shfl_xor(nsq, 16);
      nsq += __shfl_xor(nsq, 32);
      if ((j >> 1) == kg) {
        const bool unit = ok && nsq > 0.f && nsq < INFINITY;  // a zero-norm row is never eligible
        item[j & 1] = it;
        sc[j & 1] = ok ? cand_scores[u * C + pos] : 0.f;
        inv[j & 1] = unit ? 1.f / sqrtf(nsq) : 0.f;
        r[j & 1] = 1.0f;
        alive |= (unit ? 1u : 0u) << (j & 1);
      }
    }
    if (nbad && err) atomicAdd(err, nbad);

    for (int t = 0; t < k_out; ++t) {
      // ---- workgroup argmax of (value, ~position) over the eligible candidates
      uint64_t key = 0ull;
#pragma unroll
      for (int m = 0; m < kPer; ++m) {
        if (((alive >> m) & 1u) && r[m] > DR_DPP_EPS) {
          const float val = fmaf(mu, logf(r[m]), lambda * sc[m]);
          key = dr::umax64(key, dr::make_key(val, (uint32_t)cpos(2 * kg + m)));
        }
      }
      key = wave_max_u64(key);
      if (lane == 0) s_wkey[w] = key;
      __syncthreads();
      uint64_t best = 0ull;
#pragma unroll
      for (int i = 0; i < kWaves; ++i) best = dr::umax64(best, s_wkey[i]);
      if (best == 0ull) {  // nobody eligible: the list ends here
        for (int i = t + tid; i < k_out; i += kThreads) {
          s_oitem[i] = -1;
          s_oresid[i] = 0.f;
        }
        break;
      }
      const int pc = (int)dr::key_item(best);
      const int pj = (pc >> 4) & (kTiles - 1);
      if (w == (pc >> 7) && col == (pc & 15)) {
        // the four lanes that hold the pick's row stage their chunks; the one
        // that holds its state records the pick
#pragma unroll
        for (int j = 0; j < kTiles; ++j) {
          if (j == pj) {
#pragma unroll
            for (int s = 0; s < KS; ++s) s_raw[4 * s + kg] = __builtin_bit_cast(uint4, brow[j][s]);
          }
        }
        if (kg == (pj >> 1)) {
#pragma unroll
          for (int m = 0; m < kPer; ++m) {
            if (m == (pj & 1)) {
              s_xinv = inv[m];
              s_oitem[t] = item[m];
              s_oresid[t] = r[m];
              alive &= ~(1u << m);
            }
          }
        }
      }
      __syncthreads();
      if (t + 1 == k_out) break;  // the list is full: no further residual is needed

      // ---- v = the picked unit row, minus (CGS2: twice) its projection on the basis
      // g_t' = <b_t', v>: row t' = tid / 4, a quarter of the columns per lane
      auto dots = [&](bool raw) {
        const int tt = tid >> 2, p = tid & 3;
        float acc = 0.f;
        if (tt < t) {
          const float4* b4 = reinterpret_cast<const float4*>(&s_basis[tt * BS]);
          const float xi = s_xinv;
#pragma unroll
          for (int i = 0; i < D / 16; ++i) {
            float4 x;
            if (raw) {
              const uint2 q = reinterpret_cast<const uint2*>(s_raw)[4 * i + p];
              x = float4{bf16_lo(q.x) * xi, bf16_hi(q.x) * xi, bf16_lo(q.y) * xi, bf16_hi(q.y) * xi};
            } else {
              x = v4[4 * i + p];
            }
            const float4 b = b4[4 * i + p];
            acc = fmaf(b.x, x.x, acc);
            acc = fmaf(b.y, x.y, acc);
            acc = fmaf(b.z, x.z, acc);
            acc = fmaf(b.w, x.w, acc);
          }
        }
        acc = quad_sum_f32(acc);
        if (p == 0 && tt < t) s_g[tt] = acc;
      };
      // four columns of sum_t' g_t' b_t' over the rows t' = grp, grp + NG, ...
      auto project = [&]() {
        const int c4 = tid % QC, grp = tid / QC;
        float4 acc = {0.f, 0.f, 0.f, 0.f};
        for (int tt = grp; tt < t; tt += NG) {
          const float g = s_g[tt];
          const float4 b = reinterpret_cast<const float4*>(&s_basis[tt * BS])[c4];
          acc.x = fmaf(g, b.x, acc.x);
          acc.y = fmaf(g, b.y, acc.y);
          acc.z = fmaf(g, b.z, acc.z);
          acc.w = fmaf(g, b.w, acc.w);
        }
        s_part[tid] = acc;
      };
      // column tid of v (from the staged row or from v) minus the projection,
      // and |v|^2 of this wave's columns
      auto finish = [&](bool raw, bool projected) {
        if (tid < D) {
          float x = raw ? bf16_lo((uint32_t)reinterpret_cast<const uint16_t*>(s_raw)[tid]) * s_xinv
                        : s_v[tid];
          if (projected) {
            const float* part = reinterpret_cast<const float*>(s_part);
            float sum = 0.f;
#pragma unroll
            for (int g = 0; g < NG; ++g) sum += part[g * D + tid];
            x -= sum;
          }
          s_v[tid] = x;
          // x = hi + mid + lo exactly, each a bf16 (8 mantissa bits a piece, by
          // truncation): the three A rows of the candidate pass
          const uint32_t hi = __float_as_uint(x) & 0xffff0000u;
          const float x1 = x - __uint_as_float(hi);
          const uint32_t mid = __float_as_uint(x1) & 0xffff0000u;
          const float x2 = x1 - __uint_as_float(mid);
          uint16_t* split = reinterpret_cast<uint16_t*>(s_split);
          split[tid] = (uint16_t)(hi >> 16);
          split[D + tid] = (uint16_t)(mid >> 16);
          split[2 * D + tid] = (uint16_t)(__float_as_uint(x2) >> 16);
          const float sq = dr::wave_sum_dpp_f32(x * x);
          if (lane == 0) s_nsq[w] = sq;
        }
        __syncthreads();
      };
      if (t == 0) {
        finish(true, false);
      } else {
        dots(true);
        __syncthreads();
        project();
        __syncthreads();
        finish(true, true);
        dots(false);
        __syncthreads();
        project();
        __syncthreads();
        finish(false, true);
      }

      // ---- b_t = v / |v| joins the basis; e_i = <b_t, x_i>, r_i -= e_i^2
      const float nsq = D > 64 ? s_nsq[0] + s_nsq[1] : s_nsq[0];
      const float invn = nsq > 0.f ? 1.f / sqrtf(nsq) : 0.f;
      if (tid < D) s_basis[t * BS + tid] = s_v[tid] * invn;
      // <v, row> of every candidate on the MFMA: A rows 4 g + (0, 1, 2) = the
      // hi, mid and lo parts of v (bf16 x bf16 products are exact in fp32, so
      // the three sums add up to the fp32 product sum), row 4 g + 3 = 0; the
      // candidate rows are the B columns. Accumulator register i of a lane is
      // A row 4 kg + i of column col: part i of that candidate, in all four lanes.
      f32x4 acc[kTiles];
#pragma unroll
      for (int j = 0; j < kTiles; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int s = 0; s < KS; ++s) {
        const uint4 av = (col & 3) < 3 ? s_split[(col & 3) * CPR + 4 * s + kg] : uint4{0u, 0u, 0u, 0u};
        const bf16x8 a = __builtin_bit_cast(bf16x8, av);
#pragma unroll
        for (int j = 0; j < kTiles; ++j)
          acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, brow[j][s], acc[j], 0, 0, 0);
      }
      float dot[kPer] = {0.f, 0.f};
#pragma unroll
      for (int j = 0; j < kTiles; ++j) {
        if ((j >> 1) == kg) dot[j & 1] = (acc[j][2] + acc[j][1]) + acc[j][0];
      }
#pragma unroll
      for (int m = 0; m < kPer; ++m) {
        const float e = dot[m] * inv[m] * invn;
        r[m] = fmaf(-e, e, r[m]);
      }
    }
    __syncthreads();
    for (int i = tid; i < k_out; i += kThreads) {
      out_items[u * k_out + i] = s_oitem[i];
      if (out_resid) out_resid[u * k_out + i] = s_oresid[i];
    }
    __syncthreads();
  }
}

}  // namespace

extern "C" int dr_dpp_rerank(const int32_t* cand_items, const float* cand_scores, int64_t n_users,
                             int C, const void* item_table, int64_t n_items, int d, int k_out,
                             float lambda, int32_t* out_items, float* out_resid, int32_t* err,
                             dr_stream_t stream) {
  static_assert(kMaxC == dr::kRerankMaxC && kMaxK == dr::kDppArgs.max_k,
                "the shared check's bounds");
  DR_CHECK_RC(dr::check_candidates(__func__, n_users, C, k_out, lambda, dr::kDppArgs));
  DR_CHECK_RC(dr::check_item_rows(__func__, n_items));
  DR_CHECK_RC(dr::check_item_width(__func__, d));  // before the n_users == 0 exit, unlike MMR
  if (n_users == 0) return DR_OK;
  DR_CHECK_RC(dr::check_item_table_filled(__func__, n_items));
  DR_CHECK_ARG(cand_items && cand_scores && item_table && out_items, "null pointer");
  hipStream_t s = (hipStream_t)stream;
  // persistent grid: one workgroup per CU (a user's rows take half the register
  // file), each looping over users
  const int cus = dr::persistent_cus();
  const dim3 grid((unsigned)(n_users < cus ? n_users : cus));
#define DR_DPP(DD)                                                                             \
  hipLaunchKernelGGL(dpp_pick_kernel<DD>, grid, dim3(kThreads), 0, s, cand_items, cand_scores,  \
                     C, (const __bf16*)item_table, n_items, n_users, k_out, lambda, out_items,  \
                     out_resid, err)
  if (d == 64) DR_DPP(64); else DR_DPP(128);
#undef DR_DPP
  DR_CHECK_LAUNCH();
  return DR_OK;
}
