// Gradient of the embedding ILD (dr_ild_embedding, ild.hip) with respect to
// the item table: dr_ild_embedding_backward (include/divrec_hip.h states the
// closed forms). For every list u and position p it adds to grad_item[r[u,p]]
// the derivative of scale * grad_out[u] * ILD_u, read from the fp32 master
// table (the forward's value comes from its bf16 copy).
//
// Bytes per list: k ids, k rows of d fp32 read once (k*d*4 B, gathered), and
// k rows of fp32 atomics (k*d*4 B). The atomics are the budget: they run at
// ~1.3 TB/s of added bytes chip-wide whatever else the kernel does
// (MI355X_MICROARCH.md, Global float atomics): 39 ms for 1M lists of 100 at
// d = 128. The gather of the same bytes runs on a path several times as wide.
//
// Layout: one 256-thread workgroup per list at a time (persistent grid, lists
// u = block, block + grid, ...). The list's rows are staged once in LDS as
// fp32 (k*d*4 <= 128 KB; three LDS classes so that short lists keep several
// workgroups per CU), which serves all three kinds:
//   * dot / cosine need S = sum_q e_q (cosine: of the unit rows) and then one
//     pass over the rows; the column sums come from the staged rows, so no
//     Gram matrix and no second trip to L2;
//   * euclidean is O(k^2 d) in fp32 VALU: the 32-lane group that owns row p
//     sweeps the k staged rows four at a time, forms |e_p - e_q|^2 from the
//     differences (n_p + n_q - 2g cancels for near rows) and sums the unit
//     differences in registers.
// As in bpr.hip / mse.hip a group of 32 lanes owns a row and lane l takes
// elements l, l + 32, ...: every no-return atomic wave-instruction is two
// contiguous 128-B row segments, the full-rate shape. Each position is added
// on its own; a destination shared between lists (the head items of top-k
// lists) is not summed on chip: uniform and top-k lists measured the same
// (DESIGN.md §3.3a).
#include "common.h"

namespace {

constexpr int kBlock = 256;
constexpr int kGroups = kBlock / 32;
constexpr int kGradMaxK = 128;
constexpr int kGradMaxD = 256;

using dr::dpp_f32;  // CTRL 0x00-0xFF quad_perm, 0x121-0x12F row_ror: inside the 16-lane row

// dr::half_sum_f32 for four sums at once: lane l of the group gets the group's
// sum of v[l & 3].
// Inside the quad each exchange halves the values a lane carries (after the
// lane ^ 1 step it keeps j = b and b + 2, b = l & 1; after the lane ^ 2 step
// j = l & 3); the rotations by 4 and 8 and the row swap keep l & 3.
__device__ __forceinline__ float group_sum4(const float (&v)[4], int gl) {
  const bool b = gl & 1, c = gl & 2;
  const float t0 = v[0] + dpp_f32<0xB1>(v[0]), t1 = v[1] + dpp_f32<0xB1>(v[1]);
  const float t2 = v[2] + dpp_f32<0xB1>(v[2]), t3 = v[3] + dpp_f32<0xB1>(v[3]);
  const float a0 = b ? t1 : t0, a1 = b ? t3 : t2;
  const float u0 = a0 + dpp_f32<0x4E>(a0), u1 = a1 + dpp_f32<0x4E>(a1);
  float r = c ? u1 : u0;
  r += dpp_f32<0x124>(r);
  r += dpp_f32<0x128>(r);
  return dr::add_rows_f32(r);
}

// 1 / sqrt(s) for s > 0 (v_rsq_f32, <= 1 ulp; denormal s is scaled into
// range first), 0 for s == 0: a zero norm or a zero distance adds nothing.
__device__ __forceinline__ float rsqrt_or_zero(float s) {
  const bool tiny = s < 0x1p-96f;
  const float r = __builtin_amdgcn_rsqf(s * (tiny ? 0x1p64f : 1.f)) * (tiny ? 0x1p32f : 1.f);
  return s > 0.f ? r : 0.f;
}

// The call's arguments as the kernel takes them (names of include/divrec_hip.h;
// T = item_table, G = grad_item).
struct GradArgs {
  const void* recs;
  int rec_i64;  // ids are int64 (else int32)
  int64_t n_users;
  int k;
  const float* T;
  int64_t n_items;
  int d;
  int vec;  // rows are whole, 16-B aligned float4 pieces
  const float* grad_out;
  float scale;
  float* G;
  int32_t* err;
};

// E: row elements per lane (>= ceil(d / 32)); ROWF: floats of the row stage.
template <int E, int KIND, int ROWF>
__global__ __launch_bounds__(kBlock) void ild_grad_kernel(const GradArgs a) {
  const void* __restrict__ recs = a.recs;
  const float* __restrict__ T = a.T;
  const float* __restrict__ grad_out = a.grad_out;
  float* __restrict__ G = a.G;
  int32_t* __restrict__ err = a.err;
  const int rec_i64 = a.rec_i64, k = a.k, d = a.d, vec = a.vec;
  const int64_t n_users = a.n_users, n_items = a.n_items;
  const float scale = a.scale;
  __shared__ __attribute__((aligned(16))) float s_row[ROWF];  // the list's rows, [k][d]
  __shared__ int64_t s_id[kGradMaxK];    // its ids
  __shared__ float s_inv[kGradMaxK];     // cosine: 1/|e_p| (0 for a zero row)
  __shared__ float s_sum[kGradMaxD];     // dot: sum_q e_q; cosine: sum_q e_q/|e_q|
  const int tid = threadIdx.x, gl = tid & 31, grp = tid >> 5;
  const float norm = scale / (float)(k * (k - 1));
  for (int64_t u = blockIdx.x; u < n_users; u += gridDim.x) {
    // the list, range-checked before any table access
    bool bad = false;
    if (tid < k) {
      const int64_t v = rec_i64 ? reinterpret_cast<const int64_t*>(recs)[u * k + tid]
                                : (int64_t)reinterpret_cast<const int32_t*>(recs)[u * k + tid];
      s_id[tid] = v;
      bad = v < 0 || v >= n_items;
    }
    if (KIND != DR_ILD_EUCLIDEAN && tid < d) s_sum[tid] = 0.f;
    if (__syncthreads_or(bad)) {  // uniform: the list adds nothing and counts once
      if (tid == 0 && err) atomicAdd(err, 1);
      continue;  // nothing below the barrier read LDS
    }
    // stage the rows: thread-linear over the list's 16-B pieces (4-B without
    // vec), four independent loads in flight per thread before the LDS writes
    // (a piece past the list's end loads the last piece again and stores nothing)
    auto stage = [&](auto piece, int per_row) {
      using P = decltype(piece);
      constexpr int W = sizeof(P) / 4;  // floats per piece
      const int np = k * per_row;
      auto src = [&](int f) {
        const int fc = f < np ? f : np - 1, p = fc / per_row;
        return *reinterpret_cast<const P*>(T + s_id[p] * d + W * (fc - p * per_row));
      };
      for (int f = tid; f < np; f += 4 * kBlock) {
        const P v0 = src(f), v1 = src(f + kBlock), v2 = src(f + 2 * kBlock),
                v3 = src(f + 3 * kBlock);
        P* dst = reinterpret_cast<P*>(s_row) + f;
        dst[0] = v0;
        if (f + kBlock < np) dst[kBlock] = v1;
        if (f + 2 * kBlock < np) dst[2 * kBlock] = v2;
        if (f + 3 * kBlock < np) dst[3 * kBlock] = v3;
      }
    };
    if (vec) stage(float4{}, d >> 2);
    else stage(0.f, d);
    __syncthreads();
    if constexpr (KIND == DR_ILD_COSINE) {  // 1/|e_p|, a group per row
      // the group's rows grp, grp + 8, ... four at a time: one reduction and
      // one rsqrt serve all four (lane l ends with row j = l & 3 of the batch)
      for (int p0 = grp; p0 < k; p0 += 4 * kGroups) {
        float ss[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int p = p0 + j * kGroups;
          ss[j] = 0.f;
#pragma unroll
          for (int e = 0; e < E; ++e) {
            const int x = e * 32 + gl;
            const float v = (p < k && x < d) ? s_row[p * d + x] : 0.f;
            ss[j] = fmaf(v, v, ss[j]);
          }
        }
        const float inv = rsqrt_or_zero(group_sum4(ss, gl));
        const int p = p0 + gl * kGroups;
        if (gl < 4 && p < k) s_inv[p] = inv;
      }
      __syncthreads();
    }
    if constexpr (KIND != DR_ILD_EUCLIDEAN) {
      // column sums of the staged rows: thread (part, x) sums column x over
      // rows part, part + parts, ...; the parts meet in s_sum (zeroed above)
      const int parts = d <= kBlock / 2 ? kBlock / d : 1;
      const int part = tid / d, x = tid - part * d;
      if (part < parts) {
        float s = 0.f;
#pragma unroll 4
        for (int q = part; q < k; q += parts)
          s = fmaf(s_row[q * d + x], KIND == DR_ILD_COSINE ? s_inv[q] : 1.f, s);
        atomicAdd(&s_sum[x], s);
      }
      __syncthreads();
    }
    const float w = norm * (grad_out ? grad_out[u] : 1.f);
    if constexpr (KIND == DR_ILD_COSINE) {
      // four of the group's rows at a time, as above: the four u_p . t_p share
      // one reduction and come back to the quad by DPP broadcasts
      float S[E];
#pragma unroll
      for (int e = 0; e < E; ++e) S[e] = e * 32 + gl < d ? s_sum[e * 32 + gl] : 0.f;
      for (int p0 = grp; p0 < k; p0 += 4 * kGroups) {
        float un[4][E], t[4][E], c[4], inv[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int p = p0 + j * kGroups;
          inv[j] = p < k ? s_inv[p] : 0.f;  // 0: a zero row, or no row
          c[j] = 0.f;
#pragma unroll
          for (int e = 0; e < E; ++e) {
            const int x = e * 32 + gl;
            const bool in = p < k && x < d;
            un[j][e] = in ? s_row[p * d + x] * inv[j] : 0.f;  // the unit row
            t[j][e] = in ? S[e] - un[j][e] : 0.f;
            c[j] = fmaf(un[j][e], t[j][e], c[j]);
          }
        }
        const float c4 = group_sum4(c, gl);
        const float cq[4] = {dpp_f32<0x00>(c4), dpp_f32<0x55>(c4), dpp_f32<0xAA>(c4),
                             dpp_f32<0xFF>(c4)};  // quad_perm broadcasts of lanes 0..3
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if (inv[j] == 0.f) continue;  // no gradient for a zero row (uniform in the group)
          float* dst = G + s_id[p0 + j * kGroups] * d;
          const float f = -w * inv[j];
#pragma unroll
          for (int e = 0; e < E; ++e) {
            const int x = e * 32 + gl;
            if (x < d) atomicAdd(dst + x, f * fmaf(-cq[j], un[j][e], t[j][e]));
          }
        }
      }
    } else for (int p = grp; p < k; p += kGroups) {  // dot, euclidean: row by row
      float ep[E], g[E];
#pragma unroll
      for (int e = 0; e < E; ++e) {
        const int x = e * 32 + gl;
        ep[e] = x < d ? s_row[p * d + x] : 0.f;
      }
      if constexpr (KIND == DR_ILD_DOT) {
#pragma unroll
        for (int e = 0; e < E; ++e) {
          const int x = e * 32 + gl;
          g[e] = x < d ? w * (s_sum[x] - ep[e]) : 0.f;
        }
      } else {
#pragma unroll
        for (int e = 0; e < E; ++e) g[e] = 0.f;
        // Four rows q at a time: one group-wide reduction and one rsqrt serve
        // all four (group_sum4 leaves |e_p - e_q|^2 of row q0 + (l & 3) on lane
        // l; its 1/sqrt goes back to the quad by DPP broadcasts). q == p has
        // all differences 0 and is skipped like any zero distance; rows past
        // the list stand in as row p itself.
        for (int q0 = 0; q0 < k; q0 += 4) {
          float df[4][E], ss[4];
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int q = q0 + j < k ? q0 + j : p;
            ss[j] = 0.f;
#pragma unroll
            for (int e = 0; e < E; ++e) {
              const int x = e * 32 + gl;
              df[j][e] = ep[e] - (x < d ? s_row[q * d + x] : 0.f);
              ss[j] = fmaf(df[j][e], df[j][e], ss[j]);
            }
          }
          const float r = rsqrt_or_zero(group_sum4(ss, gl));
          const float rq[4] = {dpp_f32<0x00>(r), dpp_f32<0x55>(r), dpp_f32<0xAA>(r),
                               dpp_f32<0xFF>(r)};  // quad_perm broadcasts of lanes 0..3
#pragma unroll
          for (int j = 0; j < 4; ++j) {
#pragma unroll
            for (int e = 0; e < E; ++e) g[e] = fmaf(df[j][e], rq[j], g[e]);
          }
        }
#pragma unroll
        for (int e = 0; e < E; ++e) g[e] *= w;
      }
      float* dst = G + s_id[p] * d;
#pragma unroll
      for (int e = 0; e < E; ++e) {
        const int x = e * 32 + gl;
        if (x < d) atomicAdd(dst + x, g[e]);
      }
    }
    __syncthreads();  // the stage is rewritten by the next list
  }
}

template <int E, int KIND>
void launch_rows(const GradArgs& a, hipStream_t s) {
  // LDS classes of the row stage and the workgroups per CU each leaves room
  // for (160 KB; ids, norms and sums take 2.6 KB more): 16 KB x 8, 50 KB x 3
  // (k = 100 at d = 128 exactly), 128 KB x 1
  const int need = a.k * a.d;
  const int per_cu = need <= 4096 ? 8 : need <= 12800 ? 3 : 1;
  const int64_t cap = (int64_t)dr::device_cus() * per_cu;
  const dim3 grid((unsigned)(a.n_users < cap ? a.n_users : cap));
  if (need <= 4096) hipLaunchKernelGGL((ild_grad_kernel<E, KIND, 4096>), grid, dim3(kBlock), 0, s, a);
  else if (need <= 12800) hipLaunchKernelGGL((ild_grad_kernel<E, KIND, 12800>), grid, dim3(kBlock), 0, s, a);
  else hipLaunchKernelGGL((ild_grad_kernel<E, KIND, kGradMaxK * kGradMaxD>), grid, dim3(kBlock), 0, s, a);
}

template <int KIND>
void launch_kind(const GradArgs& a, hipStream_t s) {
  const int e = (a.d + 31) / 32;  // 1..8 elements per lane, instances at 1, 2, 4, 8
  if (e <= 1) launch_rows<1, KIND>(a, s);
  else if (e <= 2) launch_rows<2, KIND>(a, s);
  else if (e <= 4) launch_rows<4, KIND>(a, s);
  else launch_rows<8, KIND>(a, s);
}

}  // namespace

extern "C" int dr_ild_embedding_backward(const void* recs, int rec_dtype, int64_t n_users, int k,
                                         const float* item_table, int64_t n_items, int d, int kind,
                                         const float* grad_out, float scale, float* grad_item,
                                         int32_t* err, dr_stream_t stream) {
  DR_CHECK_ARG(k >= 1 && k <= kGradMaxK, "k must be in [1, 128]");
  DR_CHECK_ARG(d >= 1 && d <= kGradMaxD, "d must be in [1, 256]");
  DR_CHECK_ARG(kind == DR_ILD_COSINE || kind == DR_ILD_DOT || kind == DR_ILD_EUCLIDEAN,
               "unknown distance kind");
  DR_CHECK_ARG(rec_dtype == DR_I32 || rec_dtype == DR_I64, "rec_dtype must be DR_I32/DR_I64");
  DR_CHECK_ARG(n_users >= 0 && n_items >= 0, "sizes must be >= 0");
  if (n_users == 0) return DR_OK;
  DR_CHECK_ARG(recs && item_table && grad_item, "null pointer");
  if (k == 1) return DR_OK;  // no pairs: nothing to add
  // rows of whole, aligned 16-B pieces are staged with dwordx4 loads
  const int vec = d % 4 == 0 && (reinterpret_cast<uintptr_t>(item_table) & 15) == 0;
  const GradArgs a{recs, rec_dtype == DR_I64, n_users, k, item_table, n_items, d, vec,
                   grad_out, scale, grad_item, err};
  hipStream_t s = (hipStream_t)stream;
  if (kind == DR_ILD_COSINE) launch_kind<DR_ILD_COSINE>(a, s);
  else if (kind == DR_ILD_DOT) launch_kind<DR_ILD_DOT>(a, s);
  else launch_kind<DR_ILD_EUCLIDEAN>(a, s);
  DR_CHECK_LAUNCH();
  return DR_OK;
}
