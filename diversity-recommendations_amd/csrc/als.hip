// Implicit-feedback ALS row solve (Hu, Koren, Volinsky, ICDM 2008): for every
// row r of a CSR over the fixed table Y,
//   A_r = G + alpha sum_i w_i y_i y_i^T + reg I,  b_r = sum_i (1 + alpha w_i) y_i,
//   x_r = A_r^-1 b_r.
// There is no reference symbol; the spec is the build's own (include/divrec_hip.h).
//
// Layout: one 256-thread workgroup solves one row at a time,
// persistent over rows. The threads form a 16 x 16 grid; thread (ty, tx) keeps
// the T x T tile (T = D / 16) of A at rows ty T .. and columns tx T .. in
// registers from the first FMA to the last elimination step, and the threads
// ty = 0 keep b beside it.
//   * accumulate: the row's item rows are gathered in chunks of 32 through LDS
//     (global -> registers under the previous chunk's FMAs -> the other of two
//     buffers, one barrier per chunk); per item a thread reads its T row and T
//     column values and does T^2 FMAs;
//   * factor: right-looking Cholesky, one barrier per column, the trailing
//     matrix never leaving the registers. Step s = 16 b + jj eliminates index
//     jj T + b (the order that keeps every thread busy until its slot b is
//     done: a symmetric permutation of A, which changes nothing for an SPD
//     matrix): the 16 threads tx = jj write their column, unscaled, as row s
//     of the LDS image; after the barrier everybody reads its T + T values of
//     it, scales them by 1 / sqrt(pivot) and updates its tile. b rides along
//     as one more row, which is the forward substitution;
//   * back substitution by wave 0 over the image's rows (lane = step), then
//     D / 4 threads store x as float4.
#include "common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kChunk = 32;  // item rows per LDS buffer

// T consecutive floats at a T * 4-byte aligned address
template <int T>
__device__ __forceinline__ void read_vec(const float* p, float (&v)[T]) {
  if constexpr (T == 2) {
    const float2 x = *reinterpret_cast<const float2*>(p);
    v[0] = x.x, v[1] = x.y;
  } else {
#pragma unroll
    for (int q = 0; q < T / 4; ++q) {
      const float4 x = reinterpret_cast<const float4*>(p)[q];
      v[4 * q] = x.x, v[4 * q + 1] = x.y, v[4 * q + 2] = x.z, v[4 * q + 3] = x.w;
    }
  }
}
template <int T>
__device__ __forceinline__ void write_vec(float* p, const float (&v)[T]) {
  if constexpr (T == 2) {
    *reinterpret_cast<float2*>(p) = float2{v[0], v[1]};
  } else {
#pragma unroll
    for (int q = 0; q < T / 4; ++q)
      reinterpret_cast<float4*>(p)[q] = float4{v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]};
  }
}

template <int D>
__global__ __launch_bounds__(kThreads) void als_solve_kernel(
    const float* __restrict__ Y, int64_t m, const float* __restrict__ G,
    const int64_t* __restrict__ rowptr, const int32_t* __restrict__ cols,
    const float* __restrict__ weights, int64_t n_rows, float alpha, float reg,
    float* __restrict__ out, uint32_t* __restrict__ err) {
  constexpr int T = D / 16;          // tile edge of a thread
  constexpr int S = D + 4;           // row stride of the factor's image (rows 16-B aligned)
  constexpr int Q = D / 4;           // float4 per item row
  constexpr int RPP = kThreads / Q;  // item rows the workgroup loads per pass
  constexpr int NP = kChunk / RPP;   // passes per chunk
  constexpr int kStage = 2 * kChunk * D;
  constexpr int kLds = D * S > kStage ? D * S : kStage;
  // the two gather buffers, then (the gather done) the factor's image
  __shared__ __attribute__((aligned(16))) float s_mem[kLds];
  __shared__ float s_cf[2][kChunk];  // alpha * w of a buffer's rows
  __shared__ float s_z[D];           // b as it stood when step s took its entry
  __shared__ float s_inv[D];         // 1 / sqrt(pivot) of step s
  __shared__ __attribute__((aligned(16))) float s_x[D];

  const int tid = threadIdx.x, lane = tid & 63;
  const int ty = tid >> 4, tx = tid & 15;
  const int lr = tid / Q, lq = tid % Q;  // the gather: row of a pass, float4 of the row
  const float4* Y4 = reinterpret_cast<const float4*>(Y);
  float4* out4 = reinterpret_cast<float4*>(out);
  unsigned nbad = 0;

  for (int64_t r = blockIdx.x; r < n_rows; r += gridDim.x) {
    const int64_t beg = rowptr[r], len = rowptr[r + 1] - beg;
    if (len <= 0 || !cols) {  // empty row: exactly 0 (uniform: no barrier is skipped by a part)
      if (tid < Q) out4[r * Q + tid] = float4{0.f, 0.f, 0.f, 0.f};
      continue;
    }
    float acc[T][T], bv[T];
#pragma unroll
    for (int a = 0; a < T; ++a) {
      bv[a] = 0.f;
#pragma unroll
      for (int c = 0; c < T; ++c) acc[a][c] = 0.f;
    }

    // ---- accumulate: sum_i (alpha w_i) y_i y_i^T and sum_i (1 + alpha w_i) y_i
    float4 v[NP];
    float cf[NP];
    auto load = [&](int64_t base, int cnt) {  // an invalid or absent entry: a zero row, weight 0
#pragma unroll
      for (int p = 0; p < NP; ++p) {
        const int row = p * RPP + lr;
        v[p] = float4{0.f, 0.f, 0.f, 0.f};
        cf[p] = 0.f;
        if (row < cnt) {
          const int32_t c = cols[base + row];
          if (c >= 0 && (int64_t)c < m) {
            v[p] = Y4[(int64_t)c * Q + lq];
            cf[p] = alpha * (weights ? weights[base + row] : 1.f);
          } else if (lq == 0) {
            ++nbad;
          }
        }
      }
    };
    auto store = [&](int buf) {
#pragma unroll
      for (int p = 0; p < NP; ++p) {
        const int row = p * RPP + lr;
        reinterpret_cast<float4*>(s_mem + buf * (kChunk * D) + row * D)[lq] = v[p];
        if (lq == 0) s_cf[buf][row] = cf[p];
      }
    };
    const int64_t n_chunks = (len + kChunk - 1) / kChunk;
    load(beg, len < kChunk ? (int)len : kChunk);
    store(0);
    __syncthreads();
    for (int64_t ch = 0; ch < n_chunks; ++ch) {
      const int64_t left = len - ch * kChunk;
      const int cnt = left < kChunk ? (int)left : kChunk;
      const int buf = (int)(ch & 1);
      const bool more = ch + 1 < n_chunks;
      if (more) load(beg + (ch + 1) * kChunk, left - kChunk < kChunk ? (int)(left - kChunk) : kChunk);
      const float* img = s_mem + buf * (kChunk * D);
#pragma unroll 4
      for (int j = 0; j < cnt; ++j) {
        const float w = s_cf[buf][j];
        float yr[T], yc[T];
        read_vec<T>(img + j * D + ty * T, yr);
        read_vec<T>(img + j * D + tx * T, yc);
#pragma unroll
        for (int a = 0; a < T; ++a) {
          const float s = w * yr[a];
#pragma unroll
          for (int c = 0; c < T; ++c) acc[a][c] = fmaf(s, yc[c], acc[a][c]);
        }
        if (ty == 0) {
          const float wb = 1.f + w;
#pragma unroll
          for (int c = 0; c < T; ++c) bv[c] = fmaf(wb, yc[c], bv[c]);
        }
      }
      if (more) store(buf ^ 1);
      __syncthreads();
    }


    // ---- + G + reg I (G read here, not ahead of the sum: started from G the
    // D = 128 instance needs all 256 VGPRs, and its one run was slower)
#pragma unroll
    for (int a = 0; a < T; ++a) {
      float g[T];
      read_vec<T>(G + (ty * T + a) * D + tx * T, g);
#pragma unroll
      for (int c = 0; c < T; ++c) acc[a][c] += g[c] + ((ty == tx && a == c) ? reg : 0.f);
    }

    // ---- Cholesky in the registers, one column (image row) and one barrier per step
    bool bad = false;
#pragma unroll
    for (int b = 0; b < T; ++b) {
      if (bad) break;
      for (int jj = 0; jj < 16; ++jj) {
        const int s = 16 * b + jj;  // eliminates index jj * T + b
        float* rowp = s_mem + s * S;
        if (tx == jj) {
          float col[T];
#pragma unroll
          for (int a = 0; a < T; ++a) col[a] = acc[a][b];
          write_vec<T>(rowp + ty * T, col);
          if (ty == 0) s_z[s] = bv[b];
        }
        __syncthreads();
        // every read of the step is issued before the pivot's arithmetic
        const float piv = rowp[jj * T + b], zs = s_z[s];
        float li[T], lk[T];
        read_vec<T>(rowp + ty * T, li);
        read_vec<T>(rowp + tx * T, lk);
        if (!(piv > 0.f && piv < INFINITY)) {  // the same value in every thread
          bad = true;
          break;
        }
        // 1 / sqrt(pivot): v_rsq_f32 and one Newton step (the step waits for
        // this chain; the IEEE sqrt and divide are 35 dependent instructions)
        float inv = __builtin_amdgcn_rsqf(piv);
        inv *= fmaf(-0.5f * piv * inv, inv, 1.5f);
        const float inv2 = inv * inv;  // l_a l_c = (column_a / pivot) column_c
        // slots below b are eliminated already: nothing reads them again
#pragma unroll
        for (int a = b; a < T; ++a) {
          const float l = li[a] * inv2;
#pragma unroll
          for (int c = b; c < T; ++c) acc[a][c] = fmaf(-l, lk[c], acc[a][c]);
        }
        if (ty == 0) {
          const float z = zs * inv2;
#pragma unroll
          for (int c = b; c < T; ++c) bv[c] = fmaf(-lk[c], z, bv[c]);
        }
        if (tid == 0) s_inv[s] = inv;
      }
    }
    __syncthreads();

    // ---- L^T x = z by wave 0: lane = step (two steps per lane at D = 128)
    if (!bad && tid < 64) {
      constexpr int NPL = (D + 63) / 64;
      float z[NPL], iv[NPL], xr[NPL];  // xr: x of the lane's own steps
      int rowof[NPL];
#pragma unroll
      for (int e = 0; e < NPL; ++e) {
        const int st = lane + 64 * e, stc = st < D ? st : D - 1;
        iv[e] = s_inv[stc];
        z[e] = s_z[stc] * iv[e];
        rowof[e] = stc * S;
        xr[e] = 0.f;
      }
#pragma unroll
      for (int e = NPL - 1; e >= 0; --e) {
        constexpr int kTop = D < 64 ? D : 64;
#pragma unroll 8
        for (int l = kTop - 1; l >= 0; --l) {
          const int s = 64 * e + l, idx = (s & 15) * T + (s >> 4);
          const float x = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(z[e] * iv[e]), l));
          xr[e] = lane == l ? x : xr[e];
          // no LDS store and no branch in the chain: the image reads of the
          // unrolled steps do not wait for x
#pragma unroll
          for (int f = 0; f <= e; ++f) {
            const float lv = s_mem[rowof[f] + idx] * iv[f];
            z[f] = lane + 64 * f < s ? fmaf(-lv, x, z[f]) : z[f];
          }
        }
      }
#pragma unroll
      for (int e = 0; e < NPL; ++e) {
        const int st = lane + 64 * e;
        if (st < D) s_x[(st & 15) * T + (st >> 4)] = xr[e];
      }
    }
    __syncthreads();
    if (tid < Q) {
      const float nan = __int_as_float(0x7fc00000);
      out4[r * Q + tid] = bad ? float4{nan, nan, nan, nan} : reinterpret_cast<const float4*>(s_x)[tid];
    }
    // the next row's gather overwrites the image: wave 0 is past it (the barrier above)
  }
  if (nbad && err) atomicAdd(err, nbad);
}

}  // namespace

extern "C" int dr_als_solve(const float* fixed_table, int64_t n_fixed_rows, int d,
                            const float* gram, const int64_t* rowptr, const int32_t* cols,
                            const float* weights, int64_t n_rows, float alpha, float reg,
                            float* out, uint32_t* err, dr_stream_t stream) {
  DR_CHECK_ARG(d == 32 || d == 64 || d == 128, "d must be 32, 64 or 128");
  DR_CHECK_ARG(reg > 0.f && reg < INFINITY, "reg must be > 0 and finite");  // NaN fails
  DR_CHECK_ARG(alpha >= 0.f && alpha < INFINITY, "alpha must be >= 0 and finite");
  DR_CHECK_ARG(n_rows >= 0, "n_rows must be >= 0");
  DR_CHECK_ARG(n_fixed_rows >= 0 && n_fixed_rows < 0x7fffffffLL, "n_fixed_rows must be in [0, 2^31)");
  if (n_rows == 0) return DR_OK;
  // cols may be NULL (every row empty), fixed_table when it has no rows
  DR_CHECK_ARG((fixed_table || n_fixed_rows == 0) && gram && rowptr && out, "null pointer");
  hipStream_t s = (hipStream_t)stream;
#define DR_ALS(DD)                                                                              \
  hipLaunchKernelGGL(als_solve_kernel<DD>,                                                      \
                     dr::persistent_grid(als_solve_kernel<DD>, kThreads, n_rows, 1),             \
                     dim3(kThreads), 0, s, fixed_table, n_fixed_rows, gram, rowptr, cols,        \
                     weights, n_rows, alpha, reg, out, err)
  if (d == 32) DR_ALS(32); else if (d == 64) DR_ALS(64); else DR_ALS(128);
#undef DR_ALS
  DR_CHECK_LAUNCH();
  return DR_OK;
}
