// MFMA shape probe (measurement tooling, not product code): bf16 MFMA loops on
// random operands, 512-thread workgroups (two waves per SIMD, the score scan's
// occupancy), one workgroup per CU, for v_mfma_f32_32x32x16_bf16 and
// v_mfma_f32_16x16x32_bf16 at equal flops per iteration. Under sustained
// full-chip load the clock the chip holds depends on the instruction mix
// (MI355X_MICROARCH.md reports ~1.15x the FLOP/s for the 16x16x32 loop); this
// probe measures it on this box for the scan's next-step decision.
//
// Two arm pairs:
//   reg  both operands stay in registers (4 or 8 independent MFMAs a turn);
//   lds  the scan's d = 128 tile step: a wave holds 128 users x 128 k as B in
//        128 VGPRs, reads a 32-item x 128-k A tile from a swizzled LDS image
//        with 8 ds_read_b128 and issues 1024 MFMA cycles on 64 accumulators.
// Every kernel stamps s_memtime and s_memrealtime around its loop into a
// buffer of its own (one record per workgroup), so the caller can read the
// in-kernel clock: d(memtime) / d(memrealtime) x 100 MHz.
#include <hip/hip_runtime.h>
#include <stdint.h>

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

// stamps[4 * workgroup + {0, 1, 2, 3}] = memtime, memrealtime before the loop, then after it
__device__ __forceinline__ void stamp(uint64_t* __restrict__ stamps, int which) {
  const uint64_t t = __builtin_amdgcn_s_memtime();
  const uint64_t r = __builtin_amdgcn_s_memrealtime();
  if (threadIdx.x == 0) {
    stamps[4 * (int64_t)blockIdx.x + 2 * which] = t;
    stamps[4 * (int64_t)blockIdx.x + 2 * which + 1] = r;
  }
}

__global__ __launch_bounds__(512, 1) void mfma32_kernel(const uint4* __restrict__ src, int iters,
                                                       float* __restrict__ out,
                                                       uint64_t* __restrict__ stamps) {
  const int64_t t = (int64_t)blockIdx.x * 512 + threadIdx.x;
  bf16x8 a[4], b[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    a[i] = __builtin_bit_cast(bf16x8, src[(t * 8 + i) & 0xFFFFF]);
    b[i] = __builtin_bit_cast(bf16x8, src[(t * 8 + 4 + i) & 0xFFFFF]);
  }
  f32x16 acc[4] = {f32x16{}, f32x16{}, f32x16{}, f32x16{}};
  stamp(stamps, 0);
  for (int it = 0; it < iters; ++it) {
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[i], b[i], acc[i], 0, 0, 0);
  }
  stamp(stamps, 1);
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) s += acc[i][r];
  out[t] = s;
}

// 16x16x32: half the flops per instruction, so 8 per iteration (same flops
// per iteration as the 4 above), 8 independent accumulators.
__global__ __launch_bounds__(512, 1) void mfma16_kernel(const uint4* __restrict__ src, int iters,
                                                       float* __restrict__ out,
                                                       uint64_t* __restrict__ stamps) {
  const int64_t t = (int64_t)blockIdx.x * 512 + threadIdx.x;
  bf16x8 a[8], b[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    a[i] = __builtin_bit_cast(bf16x8, src[(t * 16 + i) & 0xFFFFF]);
    b[i] = __builtin_bit_cast(bf16x8, src[(t * 16 + 8 + i) & 0xFFFFF]);
  }
  f32x4 acc[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) acc[i] = f32x4{};
  stamp(stamps, 0);
  for (int it = 0; it < iters; ++it) {
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[i], b[i], acc[i], 0, 0, 0);
  }
  stamp(stamps, 1);
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int r = 0; r < 4; ++r) s += acc[i][r];
  out[t] = s;
}

// The LDS arms. The image is a ring of LDS_TILES tiles of 32 rows x 256 bytes
// (128 bf16), 16-byte chunks swizzled as the scan's stage is: physical chunk =
// logical chunk ^ (row & 15). Iteration `it` reads tile it % LDS_TILES.
constexpr int LDS_TILES = 8;

__device__ __forceinline__ void fill_image(uint4* img, const uint4* __restrict__ src) {
  // 8 tiles x 32 rows x 16 chunks = 4096 chunks, 8 per thread; random data, so
  // which chunk lands where does not matter.
#pragma unroll
  for (int i = 0; i < LDS_TILES * 32 * 16 / 512; ++i)
    img[i * 512 + threadIdx.x] = src[((int64_t)blockIdx.x * 4096 + i * 512 + threadIdx.x) & 0xFFFFF];
  __syncthreads();
}

// 32x32x16: lane l reads row l % 32, logical chunk 2s + l / 32 for the k-step
// s = 0..7; B fragment (ut, s) is one of 4 user tiles of 32.
__global__ __launch_bounds__(512, 1) void lds32_kernel(const uint4* __restrict__ src, int iters,
                                                      float* __restrict__ out,
                                                      uint64_t* __restrict__ stamps) {
  __shared__ uint4 img[LDS_TILES * 32 * 16];
  const int64_t t = (int64_t)blockIdx.x * 512 + threadIdx.x;
  const int lane = threadIdx.x & 63;
  fill_image(img, src);
  bf16x8 b[4][8];
#pragma unroll
  for (int ut = 0; ut < 4; ++ut)
#pragma unroll
    for (int s = 0; s < 8; ++s) b[ut][s] = __builtin_bit_cast(bf16x8, src[(t * 32 + ut * 8 + s) & 0xFFFFF]);
  f32x16 acc[4] = {f32x16{}, f32x16{}, f32x16{}, f32x16{}};
  const int row = lane & 31, hi = lane >> 5;
  stamp(stamps, 0);
  for (int it = 0; it < iters; ++it) {
    const uint4* tile = img + (it & (LDS_TILES - 1)) * 32 * 16 + row * 16;
    bf16x8 a[8];
#pragma unroll
    for (int s = 0; s < 8; ++s) a[s] = __builtin_bit_cast(bf16x8, tile[(2 * s + hi) ^ (row & 15)]);
#pragma unroll
    for (int s = 0; s < 8; ++s)
#pragma unroll
      for (int ut = 0; ut < 4; ++ut)
        acc[ut] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[s], b[ut][s], acc[ut], 0, 0, 0);
    asm volatile("" ::: "memory");  // the reads stay inside the loop
  }
  stamp(stamps, 1);
  float sum = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) sum += acc[i][r];
  out[t] = sum;
}

// 16x16x32: lane l reads row 16 * half + l % 16, logical chunk 4s + l / 16 for
// the k-step s = 0..3; B fragment (ut, s) is one of 8 user tiles of 16.
__global__ __launch_bounds__(512, 1) void lds16_kernel(const uint4* __restrict__ src, int iters,
                                                      float* __restrict__ out,
                                                      uint64_t* __restrict__ stamps) {
  __shared__ uint4 img[LDS_TILES * 32 * 16];
  const int64_t t = (int64_t)blockIdx.x * 512 + threadIdx.x;
  const int lane = threadIdx.x & 63;
  fill_image(img, src);
  bf16x8 b[8][4];
#pragma unroll
  for (int ut = 0; ut < 8; ++ut)
#pragma unroll
    for (int s = 0; s < 4; ++s) b[ut][s] = __builtin_bit_cast(bf16x8, src[(t * 32 + ut * 4 + s) & 0xFFFFF]);
  f32x4 acc[2][8];
#pragma unroll
  for (int h = 0; h < 2; ++h)
#pragma unroll
    for (int ut = 0; ut < 8; ++ut) acc[h][ut] = f32x4{};
  const int r16 = lane & 15, q = lane >> 4;
  stamp(stamps, 0);
  for (int it = 0; it < iters; ++it) {
    const uint4* tile = img + (it & (LDS_TILES - 1)) * 32 * 16;
    bf16x8 a[2][4];
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int s = 0; s < 4; ++s)
        a[h][s] = __builtin_bit_cast(bf16x8, tile[(16 * h + r16) * 16 + ((4 * s + q) ^ r16)]);
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int ut = 0; ut < 8; ++ut)
          acc[h][ut] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[h][s], b[ut][s], acc[h][ut], 0, 0, 0);
    asm volatile("" ::: "memory");  // the reads stay inside the loop
  }
  stamp(stamps, 1);
  float sum = 0.f;
#pragma unroll
  for (int h = 0; h < 2; ++h)
#pragma unroll
    for (int ut = 0; ut < 8; ++ut)
#pragma unroll
      for (int r = 0; r < 4; ++r) sum += acc[h][ut][r];
  out[t] = sum;
}

// shape 32 or 16; lds 0 (operands in registers) or 1 (A from the LDS image).
// stamps holds 4 uint64 per workgroup.
extern "C" int probe_mfma(int shape, int lds, const void* src, int grid, int iters, float* out,
                          uint64_t* stamps, hipStream_t s) {
  auto k = lds ? (shape == 32 ? lds32_kernel : lds16_kernel) : (shape == 32 ? mfma32_kernel : mfma16_kernel);
  hipLaunchKernelGGL(k, dim3(grid), dim3(512), 0, s, (const uint4*)src, iters, out, stamps);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
