// Weighted CSR row sum over an embedding table (an SpMM with a d-wide dense
// side): for every row r of a CSR over the fp32 table,
//   out[r, :] = sum_{e in [rowptr[r], rowptr[r + 1])} w[e] * table[cols[e], :].
// Over the row -> feature CSR it composes a table from feature embeddings;
// over the transposed CSR it is the exact gradient with respect to the feature
// table. There is no reference symbol; the spec is the build's own
// (include/divrec_hip.h).
//
// Layout: a GROUP of G lanes (G = 4 .. 64, the power of two
// that covers d / 4) owns one work item at a time, 16 B of the row per lane
// (two float4 per lane above d = 256). When d is no multiple of 4 or a
// pointer is not 16-B aligned a lane holds single floats instead: groups of
// 32 lanes up to d = 128, whole waves above, up to 8 floats of a row per lane. A wave holds
// 64 / G groups, and a group keeps U entries' table rows in flight, so a wave
// has U * 64 / G rows of loads outstanding.
//   * a work item is a CHUNK: at most L = DR_ROW_SUM_CHUNK consecutive entries
//     of one row, summed from 0 in entry order by fp32 FMAs (weights NULL: by
//     adds). A row of at most L entries is one chunk, written to out. A longer
//     row is cut into L-entry chunks: separate groups sum them into fp32
//     partial rows, and a second kernel adds a row's partials in chunk order,
//     p0 + p1 + p2 + ..., and writes out;
//   * the plan (made once per CSR) lists every item of a CSR that has long
//     rows, longest first; the groups take them in serpentine order, so that
//     no group, and no wave, ends far behind the others however skewed the
//     rows are;
//   * without a plan, or with the plan of a CSR without long rows, the groups
//     stride over the rows, and a group sums a long row's chunks itself, in
//     the same order with the same roundings: the plan changes who sums, never
//     what.
// So a row's result depends, bitwise, on its entry list and on L alone: not on
// the grid, the CU count, U, the row's place in the CSR or its neighbours.
// No atomics.
#include "common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kL = DR_ROW_SUM_CHUNK;

// Measurement variants (tools/feature_time.py); neither
// changes a result bit. U: entries whose rows a group loads before it adds the
// first (halved where a lane holds 8 values of a row). SCALAR: the
// one-float-per-lane layout for every width.
#ifndef DR_ROW_SUM_U
#define DR_ROW_SUM_U 4
#endif
#ifndef DR_ROW_SUM_SCALAR
#define DR_ROW_SUM_SCALAR 0
#endif

__device__ __forceinline__ void set_zero(float& a) { a = 0.f; }
__device__ __forceinline__ void set_zero(float4& a) { a = float4{0.f, 0.f, 0.f, 0.f}; }
__device__ __forceinline__ void fma_into(float& a, float w, const float& v) { a = fmaf(w, v, a); }
__device__ __forceinline__ void fma_into(float4& a, float w, const float4& v) {
  a.x = fmaf(w, v.x, a.x), a.y = fmaf(w, v.y, a.y), a.z = fmaf(w, v.z, a.z), a.w = fmaf(w, v.w, a.w);
}
__device__ __forceinline__ void add_into(float& a, const float& v) { a += v; }
__device__ __forceinline__ void add_into(float4& a, const float4& v) {
  a.x += v.x, a.y += v.y, a.z += v.z, a.w += v.w;
}

// fp32 -> bf16, round to nearest even (NaN -> the quiet NaN 0x7fc0)
__device__ __forceinline__ uint16_t bf16_rne(float f) {
  const uint32_t u = __float_as_uint(f);
  if ((u & 0x7fffffffu) > 0x7f800000u) return 0x7fc0;
  return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}
__device__ __forceinline__ void store_bf16(uint16_t* p, const float& v) { *p = bf16_rne(v); }
__device__ __forceinline__ void store_bf16(uint16_t* p, const float4& v) {  // p 8-B aligned
  const uint32_t lo = bf16_rne(v.x) | ((uint32_t)bf16_rne(v.y) << 16);
  const uint32_t hi = bf16_rne(v.z) | ((uint32_t)bf16_rne(v.w) << 16);
  *reinterpret_cast<uint2*>(p) = uint2{lo, hi};
}

// One finished row: element col (in units of V) of row r of out, fp32 or bf16.
template <typename V>
__device__ __forceinline__ void store_out(void* out, bool bf16, int64_t r, int dv, int col,
                                          const V& v) {
  constexpr int kPer = sizeof(V) / 4;
  if (bf16)
    store_bf16(reinterpret_cast<uint16_t*>(out) + (r * dv + col) * kPer, v);
  else
    reinterpret_cast<V*>(out)[r * dv + col] = v;
}

// acc = sum over the entries [beg, end) in entry order, from 0. U entries'
// rows are loaded before the first of them is added; the adds stay in order.
// A column outside the table is a zero row of weight 0 (acc + 0 * 0 = acc).
template <int G, int NV, typename V, int U>
__device__ __forceinline__ void sum_entries(const V* __restrict__ table, int64_t n_table_rows,
                                            int dv, const int32_t* __restrict__ cols,
                                            const float* __restrict__ weights, int64_t beg,
                                            int64_t end, int gl, V (&acc)[NV], unsigned& nbad) {
#pragma unroll
  for (int j = 0; j < NV; ++j) set_zero(acc[j]);
  if (!cols) end = beg;  // cols NULL: every row is empty, whatever rowptr says
  for (int64_t e = beg; e < end; e += U) {
    V v[U][NV];
    float w[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      w[u] = 0.f;
#pragma unroll
      for (int j = 0; j < NV; ++j) set_zero(v[u][j]);
      if (e + u < end) {
        const int32_t c = cols[e + u];
        if (c >= 0 && (int64_t)c < n_table_rows) {
          w[u] = weights ? weights[e + u] : 1.f;
#pragma unroll
          for (int j = 0; j < NV; ++j) {
            const int col = gl + j * G;
            if (col < dv) v[u][j] = table[(int64_t)c * dv + col];
          }
        } else if (gl == 0) {
          ++nbad;
        }
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
#pragma unroll
      for (int j = 0; j < NV; ++j) fma_into(acc[j], w[u], v[u][j]);
    }
  }
}

struct RowSumPlan {  // the plan's five lists (device), NULL without a plan
  const int64_t* item_row;    // [n_items] the row a work item belongs to
  const int64_t* item_beg;    // [n_items] its first entry (an index into cols)
  const int64_t* item_slot;   // [n_items] its partial row in the workspace, -1: a whole row -> out
  const int64_t* long_row;    // [n_long] the rows cut into chunks
  const int64_t* long_first;  // [n_long + 1] a long row's first partial row
};

template <int NV, int G, typename V>
__device__ __forceinline__ void store_row(void* out, bool bf16, int64_t r, int dv, int gl,
                                          const V (&v)[NV]) {
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    const int col = gl + j * G;
    if (col < dv) store_out<V>(out, bf16, r, dv, col, v[j]);
  }
}

template <int G, int NV, typename V, int U>
__global__ __launch_bounds__(kThreads) void row_sum_kernel(
    const V* __restrict__ table, int64_t n_table_rows, int dv, const int64_t* __restrict__ rowptr,
    const int32_t* __restrict__ cols, const float* __restrict__ weights, int64_t n_rows,
    RowSumPlan plan, int64_t n_items, int64_t n_chunks, V* __restrict__ partials,
    void* __restrict__ out, bool out_bf16, uint32_t* __restrict__ err) {
  constexpr int kGroups = kThreads / G;
  const int gl = threadIdx.x % G;
  const int64_t group = (int64_t)blockIdx.x * kGroups + threadIdx.x / G;
  const int64_t n_groups = (int64_t)gridDim.x * kGroups;
  unsigned nbad = 0;
  V acc[NV];
  if (n_items) {
    // The plan's items, longest first, dealt to the groups in serpentine order
    // (round 0 forwards, round 1 backwards, ...): the groups' loads stay equal,
    // and the groups of one wave hold items of about one length.
    for (int64_t round = 0; round * n_groups < n_items; ++round) {
      const int64_t item = round * n_groups + ((round & 1) ? n_groups - 1 - group : group);
      if (item >= n_items) continue;
      const int64_t row = plan.item_row[item], slot = plan.item_slot[item];
      if (row < 0 || row >= n_rows || slot < -1 || slot >= n_chunks) continue;  // never followed
      const int64_t rb = rowptr[row], re = rowptr[row + 1];
      int64_t beg = plan.item_beg[item];
      if (beg < rb || beg > re) beg = re;  // an item outside its row: empty
      sum_entries<G, NV, V, U>(table, n_table_rows, dv, cols, weights, beg,
                               beg + kL < re ? beg + kL : re, gl, acc, nbad);
      if (slot < 0) {
        store_row<NV, G, V>(out, out_bf16, row, dv, gl, acc);
      } else {
#pragma unroll
        for (int j = 0; j < NV; ++j) {
          const int col = gl + j * G;
          if (col < dv) partials[slot * dv + col] = acc[j];
        }
      }
    }
  } else {
    // No item list: the rows in order, each whole; a row longer than L chunk by chunk.
    for (int64_t r = group; r < n_rows; r += n_groups) {
      const int64_t rb = rowptr[r], re = rowptr[r + 1];
      V total[NV];
      sum_entries<G, NV, V, U>(table, n_table_rows, dv, cols, weights, rb,
                               rb + kL < re ? rb + kL : re, gl, total, nbad);
      for (int64_t b = rb + kL; b < re; b += kL) {
        sum_entries<G, NV, V, U>(table, n_table_rows, dv, cols, weights, b,
                                 b + kL < re ? b + kL : re, gl, acc, nbad);
#pragma unroll
        for (int j = 0; j < NV; ++j) add_into(total[j], acc[j]);
      }
      store_row<NV, G, V>(out, out_bf16, r, dv, gl, total);
    }
  }
  if (nbad && err) atomicAdd(err, nbad);  // the error counter, not the result
}

// out[long_row[j]] = p[c0] + p[c0 + 1] + ... in chunk order. One workgroup per
// long row at a time: a row's partial rows are adjacent in the workspace, so
// the workgroup streams them as one contiguous array, kTile elements (of V) a
// step: all 256 threads load the next tile into registers while the threads
// that own a column add the current one's rows, in order, out of LDS.
constexpr int kTile = 2048;  // V per tile: 32 KiB of float4
constexpr int kTilePer = kTile / kThreads;

template <typename V>
__global__ __launch_bounds__(kThreads) void row_sum_combine_kernel(
    const V* __restrict__ partials, int dv, RowSumPlan plan, int64_t n_long, int64_t n_chunks,
    int64_t n_rows, void* __restrict__ out, bool out_bf16) {
  __shared__ V s_tile[kTile];
  const int tid = threadIdx.x;
  const int rows_per_tile = kTile / dv;  // >= 4: dv <= 512
  constexpr int kCols = DR_ROW_SUM_MAX_D / kThreads;  // columns a thread may own (float, d = 512)
  for (int64_t j = blockIdx.x; j < n_long; j += gridDim.x) {
    const int64_t row = plan.long_row[j];
    int64_t c0 = plan.long_first[j], c1 = plan.long_first[j + 1];
    if (row < 0 || row >= n_rows) continue;              // uniform over the workgroup
    if (c0 < 0 || c1 > n_chunks || c0 > c1) c0 = c1 = 0;
    V total[kCols], regs[kTilePer];
#pragma unroll
    for (int q = 0; q < kCols; ++q) set_zero(total[q]);
    auto load = [&](int64_t c) {  // the tile that starts at partial row c
      const int64_t left = (c1 - c) * dv;
      const int n = left < (int64_t)rows_per_tile * dv ? (int)left : rows_per_tile * dv;
#pragma unroll
      for (int i = 0; i < kTilePer; ++i) {
        const int at = tid + i * kThreads;
        V v;
        set_zero(v);
        if (at < n) v = partials[c * dv + at];
        regs[i] = v;
      }
    };
    if (c0 < c1) load(c0);
    for (int64_t c = c0; c < c1; c += rows_per_tile) {
      const int rows = c1 - c < rows_per_tile ? (int)(c1 - c) : rows_per_tile;
      __syncthreads();  // the previous tile's adds are done
#pragma unroll
      for (int i = 0; i < kTilePer; ++i) {
        const int at = tid + i * kThreads;
        if (at < rows * dv) s_tile[at] = regs[i];
      }
      __syncthreads();
      if (c + rows_per_tile < c1) load(c + rows_per_tile);  // in flight under the adds
#pragma unroll
      for (int q = 0; q < kCols; ++q) {
        const int col = tid + q * kThreads;
        if (col < dv) {
          for (int r = 0; r < rows; ++r) {
            // the first partial is taken as it is: 0 + p would turn a -0 into +0,
            // which the unsplit order (total = p0) does not
            if (c == c0 && r == 0) total[q] = s_tile[col]; else add_into(total[q], s_tile[r * dv + col]);
          }
        }
      }
    }
#pragma unroll
    for (int q = 0; q < kCols; ++q) {
      const int col = tid + q * kThreads;
      if (col < dv) store_out<V>(out, out_bf16, row, dv, col, total[q]);
    }
    __syncthreads();  // the next row's first tile overwrites s_tile
  }
}

template <int G, int NV, typename V, int U>
int launch(const float* table, int64_t n_table_rows, int dv, const int64_t* rowptr,
           const int32_t* cols, const float* weights, int64_t n_rows, const RowSumPlan& plan,
           int64_t n_items, int64_t n_chunks, int64_t n_long, void* workspace, void* out,
           bool out_bf16, uint32_t* err, hipStream_t s) {
  auto sum = row_sum_kernel<G, NV, V, U>;
  const int64_t blocks = dr::ceil_div(n_items ? n_items : n_rows, kThreads / G);
  hipLaunchKernelGGL(sum, dr::persistent_grid(sum, kThreads, blocks, 1), dim3(kThreads), 0, s,
                     reinterpret_cast<const V*>(table), n_table_rows, dv, rowptr, cols, weights,
                     n_rows, plan, n_items, n_chunks, reinterpret_cast<V*>(workspace), out,
                     out_bf16, err);
  DR_CHECK_LAUNCH();
  if (n_long) {
    auto combine = row_sum_combine_kernel<V>;
    hipLaunchKernelGGL(combine, dr::persistent_grid(combine, kThreads, n_long, 1), dim3(kThreads),
                       0, s, reinterpret_cast<const V*>(workspace), dv, plan, n_long, n_chunks,
                       n_rows, out, out_bf16);
    DR_CHECK_LAUNCH();
  }
  return DR_OK;
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

extern "C" int dr_csr_row_sum_chunk(void) { return kL; }

extern "C" size_t dr_csr_row_sum_workspace(int64_t n_chunks, int d) {
  if (n_chunks <= 0 || d < 1 || d > DR_ROW_SUM_MAX_D) return 0;
  return (size_t)n_chunks * (size_t)d * sizeof(float);
}

extern "C" int dr_csr_row_sum(const float* table, int64_t n_table_rows, int d,
                              const int64_t* rowptr, const int32_t* cols, const float* weights,
                              int64_t n_rows, const int64_t* plan, int64_t n_chunks,
                              int64_t n_long, void* out, int out_dtype, void* workspace,
                              size_t workspace_bytes, uint32_t* err, dr_stream_t stream) {
  DR_CHECK_ARG(d >= 1 && d <= DR_ROW_SUM_MAX_D, "d must be in [1, 512]");
  DR_CHECK_ARG(n_rows >= 0, "n_rows must be >= 0");
  DR_CHECK_ARG(n_table_rows >= 0 && n_table_rows < 0x7fffffffLL,
               "n_table_rows must be in [0, 2^31)");
  DR_CHECK_ARG(n_chunks >= 0 && n_long >= 0 && 2 * n_long <= n_chunks && n_long <= n_rows,
               "need 0 <= 2 n_long <= n_chunks and n_long <= n_rows");
  DR_CHECK_ARG(out_dtype == DR_F32 || out_dtype == DR_BF16, "out must be DR_F32 or DR_BF16");
  if (n_rows == 0) return DR_OK;
  // cols may be NULL (every row empty), table when it has no rows
  DR_CHECK_ARG((table || n_table_rows == 0) && rowptr && out, "null pointer");
  DR_CHECK_ARG(n_chunks == 0 || (plan && workspace), "null pointer (a plan with chunks)");
  DR_CHECK_ARG(workspace_bytes >= dr_csr_row_sum_workspace(n_chunks, d),
               "workspace smaller than dr_csr_row_sum_workspace");
  DR_CHECK_ARG(cols || !weights, "weights without cols");
  // a plan without long rows holds nothing the kernel needs: the rows in order
  const int64_t n_items = n_long ? n_rows - n_long + n_chunks : 0;
  RowSumPlan p{nullptr, nullptr, nullptr, nullptr, nullptr};
  if (n_items) {
    p.item_row = plan;
    p.item_beg = plan + n_items;
    p.item_slot = plan + 2 * n_items;
    p.long_row = plan + 3 * n_items;
    p.long_first = plan + 3 * n_items + n_long;
  }
  const bool bf16 = out_dtype == DR_BF16;
  hipStream_t s = (hipStream_t)stream;
#define DR_ROW_SUM(G, NV, V, U, DV)                                                            \
  return launch<G, NV, V, U>(table, n_table_rows, DV, rowptr, cols, weights, n_rows, p,        \
                             n_items, n_chunks, n_long, workspace, out, bf16, err, s)
  if (!DR_ROW_SUM_SCALAR && d % 4 == 0 && aligned16(table) && aligned16(out) &&
      aligned16(workspace)) {
    const int dv = d / 4;
    if (dv <= 4) DR_ROW_SUM(4, 1, float4, DR_ROW_SUM_U, dv);
    if (dv <= 8) DR_ROW_SUM(8, 1, float4, DR_ROW_SUM_U, dv);
    if (dv <= 16) DR_ROW_SUM(16, 1, float4, DR_ROW_SUM_U, dv);
    if (dv <= 32) DR_ROW_SUM(32, 1, float4, DR_ROW_SUM_U, dv);
    if (dv <= 64) DR_ROW_SUM(64, 1, float4, DR_ROW_SUM_U, dv);
    DR_ROW_SUM(64, 2, float4, DR_ROW_SUM_U / 2, dv);
  }
  // one float per lane: row_runs.h's 32-lane groups up to d = 128, whole waves above
  if (d <= 32) DR_ROW_SUM(32, 1, float, DR_ROW_SUM_U, d);
  if (d <= 64) DR_ROW_SUM(32, 2, float, DR_ROW_SUM_U, d);
  if (d <= 128) DR_ROW_SUM(32, 4, float, DR_ROW_SUM_U, d);
  if (d <= 256) DR_ROW_SUM(64, 4, float, DR_ROW_SUM_U, d);
  DR_ROW_SUM(64, 8, float, DR_ROW_SUM_U / 2, d);
#undef DR_ROW_SUM
}
