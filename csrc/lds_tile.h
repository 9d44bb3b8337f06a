// Tile staging shared by the GEMM kernels: direct global->LDS copies, the
// 128-byte-row LDS swizzle, the grouped (MoE) tile staging, and the slot
// layout of the dense 256x256 pipelines.
#pragma once

#include "common.h"

// Direct HBM->LDS copies (`global_load_lds`). lds is the wave-uniform base:
// the instruction takes it from lane 0 and lane l lands at lds + l*16
// (glds16) / lds + l*4 (glds4), so LDS stays lane-linear and any swizzle goes
// on the SOURCE address. (A lane-linear address base + l*16 is the same value
// in lane 0; grouped_stage below passes that form.)
__device__ __forceinline__ void glds16(const void* g, void* lds) {
  __builtin_amdgcn_global_load_lds(
      (const __attribute__((address_space(1))) u32*)g,
      (__attribute__((address_space(3))) u32*)lds, 16, 0, 0);
}

__device__ __forceinline__ void glds4(const void* g, void* lds) {
  __builtin_amdgcn_global_load_lds(
      (const __attribute__((address_space(1))) u32*)g,
      (__attribute__((address_space(3))) u32*)lds, 4, 0, 0);
}

// Swizzle mode 2 of a byte offset within a tile of 128-byte rows (an
// involution, bits >= 7 fixed): row bits 1..3 XOR'd into the 16B-chunk index
// — a ds_read_b128 quarter (16 consecutive rows, fixed k-chunk) hits all 16
// bank groups: group = 8*(row&1) + (chunk ^ ((row>>1)&7)), bijective over 16
// rows. Applied on the glds source address and on the ds_read address.
__device__ __forceinline__ u32 swz2(u32 byte) {
  return byte ^ (((byte >> 8) & 7u) << 4);
}

// ---- grouped (per-expert) GEMMs ----

// Stage a ROWS x 128-byte tile (64 bf16 or 128 e4m3 a row) with WAVES waves;
// each wave issues ROWS/(8*WAVES) x 1KB chunks. GATHER: source rows are
// tokens, indexed through row_tok[m0 + row]; rows past rows_valid and padding
// entries (-1) read token 0. Otherwise rows m0.. of gsrc, clamped to the last
// valid one. glds16 gets the lane-linear LDS address (lane 0's is the chunk
// base): with the wave index in a VGPR, as in the three grouped files that
// use this, the wave-uniform base compiles to different code.
template <int ROWS, int WAVES, bool GATHER>
__device__ __forceinline__ void grouped_stage(
    void* lds, const void* gsrc, long row_stride_b, const int* row_tok, int m0,
    int rows_valid, int wave, int lane) {
  constexpr int CH = ROWS / (8 * WAVES);
  static_assert(CH >= 1, "tile too small for wave count");
#pragma unroll
  for (int j = 0; j < CH; ++j) {
    const int c = wave * CH + j;
    const u32 b = (u32)c * 1024u + (u32)lane * 16u;  // lane-linear LDS byte
    const u32 lb = swz2(b);                          // pre-swizzled source
    const int row = (int)(lb >> 7);
    long grow;
    if (GATHER) {
      int tok = (row < rows_valid) ? row_tok[m0 + row] : 0;
      if (tok < 0) tok = 0;  // padding: deterministic garbage, discarded
      grow = (long)tok;
    } else {
      grow = (long)(m0 + min(row, rows_valid - 1));
    }
    glds16((const u8*)gsrc + grow * row_stride_b + (lb & 127u),
           (u8*)lds + b);
  }
}

// ---- dense 256x256 pipelines ----
// One dynamic LDS array: 2 K-tile buffers x 4 half-tiles of 128 rows x 128
// bytes (16 KiB), in staging order B0, A0, B1, A1.
constexpr int HT = 16384;       // half-tile bytes
constexpr int KTILE_B = 65536;  // one K-tile buffer: 4 half-tiles
constexpr int SLOT_B0 = 0, SLOT_A0 = 1, SLOT_B1 = 2, SLOT_A1 = 3;

// this thread's two staging sources of one half-tile (k = 0), rows clamped
struct Src {
  const char* p[2];
};

__device__ __forceinline__ void stage_half(char* slot_wave, const Src& s,
                                           long koff) {
  glds16(s.p[0] + koff, slot_wave);
  glds16(s.p[1] + koff, slot_wave + 1024);
}

// XCD-aware bijective remap (guide §5) of a block id, nwg = grid size:
// consecutive same-XCD blocks are m-neighbours of one n-column, recovering W
// reuse in each XCD's L2
__device__ __forceinline__ int xcd_remap(int bid, int nwg) {
  const int q = nwg >> 3, r = nwg & 7;
  const int xcd = bid & 7, seq = bid >> 3;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + seq;
}
