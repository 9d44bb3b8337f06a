// Shared-prefix decode attention, phase 1: one wave per (tile of rows, kv_head)
// walks the P KV pages the tile's rows have in common ONCE and leaves each
// (row, head)'s running softmax state in f32; the per-row kernel's CONT
// instantiation (attn_decode_mfma.hip) resumes from it at page P.
//
// The per-row kernel puts G = Hq/Hk <= 8 heads of one row in the 16 MFMA
// columns and zero-pads the rest. Here a 16-column block holds (row, head)
// pairs: G is padded to Gp in {1,2,4,8}, column j of a block is row j/Gp,
// head j%Gp, and a wave owns CB column blocks — R = CB*16/Gp rows per tile.
// Per shared page the K fragments are loaded once and V^T is staged once;
// the score MFMAs, the softmax update and the PV MFMAs then run per column
// block through mfma_page_update, the same function the per-row kernel runs,
// so every column sees the same floating-point operations on either route
// and the f32 state passes through memory losslessly: the result is
// bit-identical to the per-row kernel over the full table.
//
// Resource usage (gfx950, -Rpass-analysis=kernel-resource-usage) is recorded
// in docs/ENGINE.md, "Shared-prefix decode attention".
#include "attn_decode_mfma.h"

#define PREFIX_CB 4  // column blocks per wave (ops.PREFIX_CB mirrors this)

template <int D, int CB>
struct PrefixSmem {
  u16 qt[CB][16 * D];      // Q^T per column block, row-swizzled
  u16 vt[D * PV_PAD];      // V^T [dD][pos32+pad] of the current page
  u16 p[16 * PV_PAD];      // P of the column block being processed
  float alpha[16];
  int col_row[CB * 16];    // batch row of each column, -1 = empty
};

template <int D, bool KV8, int CB>
__global__ __launch_bounds__(256) void attn_prefix_partial_kernel(
    float* __restrict__ part_o,       // [n, Hq, D] unnormalised
    float* __restrict__ part_m,       // [n, Hq]
    float* __restrict__ part_l,       // [n, Hq]
    const u16* __restrict__ q,        // [n, Hq, D]
    const u8* __restrict__ k_cache,   // [nb, Hk, BS, D] bf16 or e4m3
    const u8* __restrict__ v_cache,
    const int* __restrict__ block_tables,     // [n, bt_stride]
    const int* __restrict__ row_prefix_pages, // [n]
    const int* __restrict__ tile_rows,        // [NT, R], -1 = empty slot
    int bt_stride, int n, int NT, int R, int Hq, int Hk, int gp_log2,
    float scale) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = threadIdx.x / WAVE;
  const long item = (long)blockIdx.x * (blockDim.x / WAVE) + wid;
  if (item >= (long)NT * Hk) return;
  const int tile = (int)(item / Hk);
  const int kh = (int)(item - (long)tile * Hk);
  const int G = Hq / Hk;
  const int* trow = tile_rows + (long)tile * R;

  // the tile's first valid row names the shared pages (wave-uniform scan)
  int first = -1;
  for (int i = 0; i < R; ++i) {
    const int r = trow[i];
    if (r >= 0 && r < n) { first = r; break; }
  }
  if (first < 0) return;  // a tile of all -1
  const int P = min(row_prefix_pages[first], bt_stride);
  if (P <= 0) return;
  const int* bt = block_tables + (long)first * bt_stride;

  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  PrefixSmem<D, CB>* sm = ((PrefixSmem<D, CB>*)smem_raw) + wid;

  const int lo16 = lane & 15;   // column in block / A row
  const int hi4 = lane >> 4;    // 0..3
  const int gmask = (1 << gp_log2) - 1;

  // ---- stage Q^T per column block: column lo16 = (row lo16>>gp_log2 of the
  // block, head lo16&gmask), scaled exactly as the per-row kernel scales it;
  // empty slots and heads >= G are zero columns.
#pragma unroll
  for (int c = 0; c < CB; ++c) {
    const int slot = (c << (4 - gp_log2)) + (lo16 >> gp_log2);
    const int head = lo16 & gmask;
    int row = trow[slot];
    if (row < 0 || row >= n || head >= G) row = -1;
    if (hi4 == 0) sm->col_row[c * 16 + lo16] = row;
#pragma unroll
    for (int t = 0; t < D / 32; ++t) {
      const int k0 = hi4 * 8 + t * 32;
      u16x8 val = {};
      if (row >= 0) {
        const u16* qrow = q + ((long)row * Hq + kh * G + head) * D;
#pragma unroll
        for (int j = 0; j < 8; ++j) val[j] = f2bf(bf2f(qrow[k0 + j]) * scale);
      }
      *(u16x8*)((char*)sm->qt[c] + qt_swz<D>(lo16, k0 * 2)) = val;
    }
  }

  wave_lds_sync();

  constexpr int DB = D / 16;
  float m_run[CB], l_run[CB];   // for column lo16 of block c
  f32x4 acc[CB][DB];            // O[column hi4*4+r][d lo16 + 16*b] of block c
#pragma unroll
  for (int c = 0; c < CB; ++c) {
    m_run[c] = -1e30f;
    l_run[c] = 0.f;
#pragma unroll
    for (int b = 0; b < DB; ++b) acc[c][b] = (f32x4)(0.f);
  }

  constexpr int ES = KV8 ? 1 : 2;  // bytes per cache element
  for (int pg = 0; pg < P; ++pg) {
    const long kv_base = (((long)bt[pg] * Hk + kh) * BS) * D * ES;
    mfma_stage_vt<D, KV8>(sm->vt, v_cache + kv_base, lane);
    bf16frag ka[2][D / 32];
    mfma_load_k<D, KV8>(ka, k_cache + kv_base, lo16, hi4);
    // a shared page is full: every row has positions beyond its prefix
#pragma unroll
    for (int c = 0; c < CB; ++c)
      mfma_page_update<D>(sm->qt[c], sm->vt, sm->p, sm->alpha, ka, BS, lo16,
                          hi4, m_run[c], l_run[c], acc[c]);
  }

  // ---- write the running state of every live column
#pragma unroll
  for (int c = 0; c < CB; ++c) {
    if (hi4 == 0) {
      const int row = sm->col_row[c * 16 + lo16];
      if (row >= 0) {
        const long hq = (long)row * Hq + kh * G + (lo16 & gmask);
        part_m[hq] = m_run[c];
        part_l[hq] = l_run[c];
      }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int col = hi4 * 4 + r;
      const int row = sm->col_row[c * 16 + col];
      if (row < 0) continue;
      float* orow = part_o + ((long)row * Hq + kh * G + (col & gmask)) * D;
#pragma unroll
      for (int b = 0; b < DB; ++b) orow[b * 16 + lo16] = acc[c][b][r];
    }
  }
}

extern "C" void sutro_attn_decode_mfma_cont(
    void*, const void*, const void*, const void*, const int*, const int*, int,
    int, int, int, float, int, int, const int*, const float*, const float*,
    const float*, hipStream_t);

extern "C" int sutro_attn_prefix_tile_rows(int Hq, int Hk) {
  const int G = Hq / Hk;
  int gp = 1;
  while (gp < G) gp <<= 1;
  return PREFIX_CB * 16 / gp;
}

// decode-only batch of n rows: phase 1 over the tiles, then the per-row
// kernel's CONT instantiation for every row
extern "C" void sutro_attn_decode_shared(
    void* out, const void* q, const void* k_cache, const void* v_cache,
    const int* block_tables, const int* seq_lens, int bt_stride, int n,
    int Hq, int Hk, float scale, int kv_fp8, int head_dim,
    const int* row_prefix_pages, const int* tile_rows, int NT, int R,
    float* part_o, float* part_m, float* part_l, hipStream_t s) {
  if (n == 0) return;
  const int G = Hq / Hk;
  int gp_log2 = 0;
  while ((1 << gp_log2) < G) ++gp_log2;
  if (NT > 0) {
    const int wpb = 2;  // D=128: 27.6 KB LDS per wave
    const long items = (long)NT * Hk;
    const long blocks = (items + wpb - 1) / wpb;
#define LAUNCH_PREFIX(D, KV8)                                                \
  if (head_dim == D && kv_fp8 == (KV8 ? 1 : 0)) {                            \
    hipLaunchKernelGGL((attn_prefix_partial_kernel<D, KV8, PREFIX_CB>),      \
                       dim3((unsigned)blocks), dim3(wpb * WAVE),             \
                       sizeof(PrefixSmem<D, PREFIX_CB>) * wpb, s, part_o,    \
                       part_m, part_l, (const u16*)q, (const u8*)k_cache,    \
                       (const u8*)v_cache, block_tables, row_prefix_pages,   \
                       tile_rows, bt_stride, n, NT, R, Hq, Hk, gp_log2,      \
                       scale);                                               \
  }
    LAUNCH_PREFIX(128, false)
    LAUNCH_PREFIX(128, true)
    LAUNCH_PREFIX(64, false)
    LAUNCH_PREFIX(64, true)
#undef LAUNCH_PREFIX
  }
  sutro_attn_decode_mfma_cont(out, q, k_cache, v_cache, block_tables,
                              seq_lens, bt_stride, n, Hq, Hk, scale, kv_fp8,
                              head_dim, row_prefix_pages, part_o, part_m,
                              part_l, s);
}
