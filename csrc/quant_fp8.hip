// FP8 (OCP e4m3) activation quantisers for MI355X: bf16 rows to e4m3 codes
// plus f32 scales, one scale per row (the per-channel dense and grouped GEMMs)
// or one per row and group of 128 K elements (the block-scaled GEMMs). All of
// them apply the rule of fp8_gemm.h (fp8_quant_scale, fp8_quant8) and are
// bit-equal to their torch_ref statement.
#include "fp8_gemm.h"

// ---- row quantisation: bf16 [R, K] -> e4m3 [R, Kp] + f32 scale [R] ----
// The rule of fp8_gemm.h with one scale per row: torch_ref.quantize_rows_fp8,
// which this matches bit for bit. One wave per row, 16-byte loads; rows of up
// to 64 * 8 * QR_CACHE elements are held in registers between the amax
// reduction and the convert (one pass over memory), wider rows are read a
// second time. The tail [K, Kp) is zeroed.
// row_limit (optional, device side): rows >= row_limit[0] * limit_mul are
// skipped — the stage-2 input only needs the live padded total.
#define QR_CACHE 8

__global__ void __launch_bounds__(256) quant_rows_fp8_kernel(
    u8* __restrict__ out_q,        // [R, Kp] e4m3
    float* __restrict__ out_scale,  // [R]
    const u16* __restrict__ x,     // [R, K] bf16
    const int* __restrict__ row_limit, int limit_mul, long R, int K, int Kp) {
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= R) return;
  if (row_limit && row >= (long)row_limit[0] * limit_mul) return;
  const u16* xr = x + row * K;
  u8* qr = out_q + row * Kp;
  const int nch = K >> 3;        // 8-element chunks of input
  const int nchp = Kp >> 3;      // 8-byte chunks of output
  const bool cached = nch <= 64 * QR_CACHE;

  u16x8 v[QR_CACHE];
  float amax = 0.f;
  if (cached) {
#pragma unroll
    for (int i = 0; i < QR_CACHE; ++i) {
      const int c = i * 64 + lane;
      v[i] = u16x8{0, 0, 0, 0, 0, 0, 0, 0};
      if (c < nch) v[i] = *(const u16x8*)(xr + c * 8);
#pragma unroll
      for (int e = 0; e < 8; ++e) amax = fmaxf(amax, fabsf(bf2f(v[i][e])));
    }
  } else {
    for (int c = lane; c < nch; c += 64) {
      const u16x8 t = *(const u16x8*)(xr + c * 8);
#pragma unroll
      for (int e = 0; e < 8; ++e) amax = fmaxf(amax, fabsf(bf2f(t[e])));
    }
  }
  amax = wave_max_f32(amax);
  const float scale = fp8_quant_scale(amax);
  if (lane == 0) out_scale[row] = scale;

  if (cached) {
#pragma unroll
    for (int i = 0; i < QR_CACHE; ++i) {
      const int c = i * 64 + lane;
      if (c < nch) *(u32x2*)(qr + c * 8) = fp8_quant8(v[i], scale);
    }
  } else {
    for (int c = lane; c < nch; c += 64)
      *(u32x2*)(qr + c * 8) = fp8_quant8(*(const u16x8*)(xr + c * 8), scale);
  }
  for (int c = nch + lane; c < nchp; c += 64)
    *(u32x2*)(qr + c * 8) = u32x2{0u, 0u};
}

// Block-per-row variant for few, wide rows (the dense FP8 projections at
// decode batch sizes): one block of up to 1024 threads per row, each thread
// holding its QB_CACHE 8-element chunks in registers (rows of up to
// 1024 * 8 * QB_CACHE = 32768 elements, one pass over memory where the wave
// kernel above reads rows wider than 4096 twice). amax goes through the wave
// reduction and one LDS round; max is order-independent and the scale and
// convert expressions are the ones above, so the output is bit-identical.
#define QB_CACHE 4
#define QB_MAX_K (1024 * 8 * QB_CACHE)

__global__ void __launch_bounds__(1024) NO_PACKED_F32
quant_rows_fp8_block_kernel(
    u8* __restrict__ out_q, float* __restrict__ out_scale,
    const u16* __restrict__ x, const int* __restrict__ row_limit,
    int limit_mul, long R, int K, int Kp) {
  __shared__ float wmax[16];
  const long row = blockIdx.x;
  if (row_limit && row >= (long)row_limit[0] * limit_mul) return;
  const int tid = threadIdx.x, nthr = blockDim.x;
  const u16* xr = x + row * K;
  u8* qr = out_q + row * Kp;
  const int nch = K >> 3;
  const int nchp = Kp >> 3;

  u16x8 v[QB_CACHE];
  float amax = 0.f;
#pragma unroll
  for (int i = 0; i < QB_CACHE; ++i) {
    const int c = i * nthr + tid;
    v[i] = u16x8{0, 0, 0, 0, 0, 0, 0, 0};
    if (c < nch) v[i] = *(const u16x8*)(xr + c * 8);
#pragma unroll
    for (int e = 0; e < 8; ++e) amax = fmaxf(amax, fabsf(bf2f(v[i][e])));
  }
  amax = wave_max_f32(amax);
  if ((tid & 63) == 0) wmax[tid >> 6] = amax;
  __syncthreads();
  const int nw = nthr >> 6;
  amax = wmax[0];
  for (int i = 1; i < nw; ++i) amax = fmaxf(amax, wmax[i]);
  const float scale = fp8_quant_scale(amax);
  if (tid == 0) out_scale[row] = scale;

#pragma unroll
  for (int i = 0; i < QB_CACHE; ++i) {
    const int c = i * nthr + tid;
    if (c >= nch) continue;
    *(u32x2*)(qr + c * 8) = fp8_quant8(v[i], scale);
  }
  for (int c = nch + tid; c < nchp; c += nthr)
    *(u32x2*)(qr + c * 8) = u32x2{0u, 0u};
}

// The (R, K) range in which the block-per-row kernel runs when the caller
// leaves the choice open, from profiles/PROFILES.md capture D2 by the
// project's routing margin: it cleared the margin at every measured R
// (8 .. 256) for K = 8192 and 25600; at K = 5120 it missed it at R = 8, so
// that width stays on the wave kernel.
#define QB_AUTO_MAX_R 256
#define QB_AUTO_MIN_K 8192

// variant: -1 = the measured rule above, 0 = one wave per row, 1 = one block
// per row (K <= QB_MAX_K, else the wave kernel runs).
extern "C" void sutro_quant_rows_fp8(void* out_q, float* out_scale,
                                     const void* x, const int* row_limit,
                                     int limit_mul, long R, int K, int Kp,
                                     int variant, hipStream_t stream) {
  if (R == 0) return;
  // static grid, no host sync, no hipGetLastError: runs inside captured
  // decode steps
  const bool block_row =
      K <= QB_MAX_K && R < (1L << 31) &&
      (variant == 1 ||
       (variant < 0 && R <= QB_AUTO_MAX_R && K >= QB_AUTO_MIN_K));
  if (block_row) {
    // one 8-element chunk per thread up to 1024 threads, whole waves
    const int thr = min(1024, ((K >> 3) + 63) / 64 * 64);
    hipLaunchKernelGGL(quant_rows_fp8_block_kernel, dim3((unsigned)R),
                       dim3(thr), 0, stream, (u8*)out_q, out_scale,
                       (const u16*)x, row_limit, limit_mul, R, K, Kp);
    return;
  }
  hipLaunchKernelGGL(quant_rows_fp8_kernel, dim3((unsigned)((R + 3) / 4)),
                     dim3(256), 0, stream, (u8*)out_q, out_scale,
                     (const u16*)x, row_limit, limit_mul, R, K, Kp);
}

// ---- activation quantiser: bf16 [R, K] -> e4m3 [R, K] + f32 [K/128, R] ----
// Every group of 128 consecutive K elements of a row gets its own scale, by
// the rule of fp8_gemm.h — torch_ref.quantize_rows_fp8_block128, which this
// matches bit for bit. A group is 16 lanes of one 16-byte load each, so a
// wave takes 4 groups and the amax is a 16-lane reduction. The scale goes to
// out_scale[kb * lds + row] (K-block-major, row stride lds >= R).
__global__ void __launch_bounds__(256) quant_rows_fp8_block128_kernel(
    u8* __restrict__ out_q,         // [R, K] e4m3
    float* __restrict__ out_scale,  // [K/128, lds]
    const u16* __restrict__ x,      // [R, K] bf16
    long R, int KB, long lds) {
  const int lane = threadIdx.x & 63;
  const long g = ((long)blockIdx.x * 4 + (threadIdx.x >> 6)) * 4 + (lane >> 4);
  const bool live = g < R * KB;
  const long off = g * 128 + (lane & 15) * 8;  // group g starts at g * 128
  u16x8 v = u16x8{0, 0, 0, 0, 0, 0, 0, 0};
  if (live) v = *(const u16x8*)(x + off);
  float amax = 0.f;
#pragma unroll
  for (int e = 0; e < 8; ++e) amax = fmaxf(amax, fabsf(bf2f(v[e])));
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) amax = fmaxf(amax, __shfl_xor(amax, o, 64));
  if (!live) return;
  const float scale = fp8_quant_scale(amax);
  if ((lane & 15) == 0) out_scale[(g % KB) * lds + g / KB] = scale;
  *(u32x2*)(out_q + off) = fp8_quant8(v, scale);
}

// K % 128 == 0, lds >= R. Static grid, no host sync, no hipGetLastError: runs
// inside captured decode steps.
extern "C" void sutro_quant_rows_fp8_block128(void* out_q, float* out_scale,
                                              const void* x, long R, long K,
                                              long lds, hipStream_t stream) {
  if (R == 0) return;
  const long KB = K / 128;
  const long groups = R * KB;
  hipLaunchKernelGGL(quant_rows_fp8_block128_kernel,
                     dim3((unsigned)((groups + 15) / 16)), dim3(256), 0,
                     stream, (u8*)out_q, out_scale, (const u16*)x, R, (int)KB,
                     lds);
}
