// FP8 (OCP e4m3) GEMM primitives shared by the dense and grouped kernels: the
// block-scaled 16x16x128 MFMA, its operand fragment read, the sources of the
// dense 256x256 pipeline, and the activation quantise rule.
#pragma once

#include "lds_tile.h"

// e8m0 1.0 in every byte: the hardware block scale is a no-op
constexpr int SCALE_ONE = 0x7f7f7f7f;

// mfma_scale_f32_16x16x128_f8f6f4 — the block-scaled form is the only fp8
// MFMA that runs at twice the bf16 rate. Operand lane map (8-bit formats):
// lane l supplies row l & 15, k = 32 * (l >> 4) + j for byte j of its 32-byte
// operand. C/D layout is the 16x16 shape's: col = l & 15,
// row = (l >> 4) * 4 + reg. Verified with exact integer data by
// tests/test_gpu_moe_fp8.py.
// e4m3 x e4m3 (cbsz = blgp = 0), both hardware scales 1.0, accumulating
__device__ __forceinline__ f32x4 mfma128(i32x8 a, i32x8 b, f32x4 c) {
  return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(
      a, b, c, 0, 0, 0, SCALE_ONE, 0, SCALE_ONE);
}

// the same from a zero C: the unscaled partial products of one K-tile
__device__ __forceinline__ f32x4 mfma128z(i32x8 a, i32x8 b) {
  return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(
      a, b, f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0, SCALE_ONE, 0, SCALE_ONE);
}

// A e4m3 (cbsz 0) x B e2m1 (blgp 4); opsel 0 on both scale registers, the A
// scale 1.0 and the B scale the real one (lane maps: grouped_gemm_mxfp4.hip)
__device__ __forceinline__ f32x4 mfma128x(i32x8 a, i32x8 b, f32x4 c,
                                          int b_scale) {
  return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(
      a, b, c, 0, 4, 0, SCALE_ONE, 0, b_scale);
}

// 32 operand bytes of one lane: k-quarter q = lane >> 4 of a 128-byte row of
// a swizzled tile, i.e. the swizzled 16-byte chunks 2q and 2q+1
__device__ __forceinline__ i32x8 lds_frag_row(const u8* lds, int row, int q) {
  const u32 lb = (u32)row * 128u + (u32)q * 32u;
  const u32x4 lo = *(const u32x4*)(lds + swz2(lb));
  const u32x4 hi = *(const u32x4*)(lds + swz2(lb + 16u));
  return i32x8{(int)lo[0], (int)lo[1], (int)lo[2], (int)lo[3],
               (int)hi[0], (int)hi[1], (int)hi[2], (int)hi[3]};
}

// the same as two 16-byte ds_reads at the pre-swizzled offsets of chunks 2q
// and 2q+1
__device__ __forceinline__ i32x8 lds_frag(const char* smem, u32 off_lo,
                                          u32 off_hi) {
  const u32x4 lo = *(const u32x4*)(smem + off_lo);
  const u32x4 hi = *(const u32x4*)(smem + off_hi);
  return i32x8{(int)lo[0], (int)lo[1], (int)lo[2], (int)lo[3],
               (int)hi[0], (int)hi[1], (int)hi[2], (int)hi[3]};
}

// a half-tile's staging sources in the dense 256x256 FP8 pipelines: 128 rows
// from row0 of base, row stride Kb bytes, rows past rows_valid clamped
__device__ __forceinline__ Src make_src(const u8* base, long row0,
                                        long rows_valid, long Kb, int wave,
                                        int lane) {
  Src s;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const u32 b = (u32)(wave * 2 + j) * 1024u + (u32)lane * 16u;
    const u32 lb = swz2(b);  // pre-swizzled source, lane-linear LDS
    long row = (long)(lb >> 7);
    row = row < rows_valid ? row : rows_valid - 1;  // edge: dup rows
    s.p[j] = (const char*)base + (row0 + row) * Kb + (lb & 127u);
  }
  return s;
}

// ---- the activation quantise rule ----
// scale = amax / 448 (true f32 division; 1 for an all-zero row or group),
// code = e4m3_rne(clamp(x / scale, -448, 448)) — the formula of
// torch_ref.quantize_rows_fp8 and quantize_rows_fp8_block128, which every
// quantiser matches bit for bit.
__device__ __forceinline__ float fp8_quant_scale(float amax) {
  return amax > 0.f ? amax / 448.0f : 1.0f;
}

__device__ __forceinline__ float fp8_quant_clamp(float x, float scale) {
  return fminf(fmaxf(x / scale, -448.0f), 448.0f);
}

// 8 bf16 -> 8 e4m3 codes
__device__ __forceinline__ u32x2 fp8_quant8(const u16x8 t, float scale) {
  u32 w[2];
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    float f[4];
#pragma unroll
    for (int e = 0; e < 4; ++e)
      f[e] = fp8_quant_clamp(bf2f(t[p * 4 + e]), scale);
    w[p] = (u32)f2fp8x2(f[0], f[1]) | ((u32)f2fp8x2(f[2], f[3]) << 16);
  }
  return u32x2{w[0], w[1]};
}
