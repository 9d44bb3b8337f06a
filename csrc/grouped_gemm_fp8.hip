// FP8 (OCP e4m3) expert weights for the dropless MoE grouped GEMM on MI355X.
//
// Same contract as csrc/grouped_gemm.hip (segments padded to the tile
// height, static grid that exits early on the device-side tile_off table,
// row_tok gather in stage 1, gate/up double stream with the SwiGLU fused into
// the epilogue, the same three tile configurations) with e4m3 operands:
//
//   A: e4m3 [., Kp] + f32 scale per row   (stage 1: indexed through row_tok)
//   W: e4m3 [E, N, Kp] + f32 scale per output channel [E, N]
//   out: bf16
//
// Kp = K rounded up to 128 with a zero tail, so one LDS row stays 128 bytes
// (= 128 K-elements): the dwordx4 HBM->LDS staging and the swizzle of the
// bf16 kernel (grouped_stage, swz2 of lds_tile.h) carry over byte for byte.
// One K-tile is ONE mfma_scale_f32_16x16x128_f8f6f4 per (i, j) fragment pair
// (mfma128 of fp8_gemm.h, which also states the operand lane map and the C/D
// layout). Both hardware block scales are e8m0 1.0; the real per-row /
// per-channel f32 scales are applied in the epilogue, before SwiGLU:
// acc * a_scale[row] * w_scale[e, n]. A lane's 32 operand bytes are two
// consecutive 16-byte chunks of the 128-byte LDS row (lds_frag_row).
#include "fp8_gemm.h"

// GATE_SILU=1: B has two streams (gate/up at N-offset 0 and n_cols), output
// n_cols wide with silu(g)*u. GATE_SILU=0: plain B, plain store.
// Waves arranged WROWS(M) x WCOLS(N); wave tile = (BM/WROWS) x (BN/WCOLS).
template <int GATE_SILU, int BM, int BN, int WROWS, int WCOLS>
__global__ __launch_bounds__(WROWS* WCOLS * 64) void grouped_gemm_fp8_kernel(
    u16* __restrict__ out,            // [rows_max, n_cols] bf16
    const u8* __restrict__ a,         // GATHER: [T, Kp]; else [rows_max, Kp]
    const float* __restrict__ a_scale,  // [T] / [rows_max]
    const u8* __restrict__ w,         // [E, N, Kp] (N = n_cols or 2*n_cols)
    const float* __restrict__ w_scale,  // [E, N]
    const int* __restrict__ row_tok,    // [rows_max] or nullptr
    const int* __restrict__ tile_off,   // [E+1] padded-offset / BM
    const int* __restrict__ counts,     // [E] live rows per expert
    int n_experts, int n_cols, long Kp) {
  constexpr int WAVES = WROWS * WCOLS;
  constexpr int WM = BM / WROWS;
  constexpr int WN = BN / WCOLS;
  constexpr int MF = WM / 16;
  constexpr int NF = WN / 16;
  constexpr int NB = GATE_SILU ? 2 : 1;
  const int t = blockIdx.x;
  const int n0 = blockIdx.y * BN;
  if (t >= tile_off[n_experts]) return;
  // binary search: expert e with tile_off[e] <= t < tile_off[e+1]
  int lo = 0, hi = n_experts - 1;
  while (lo < hi) {
    int mid = (lo + hi + 1) >> 1;
    if (tile_off[mid] <= t) lo = mid;
    else hi = mid - 1;
  }
  const int e = lo;
  const int m0 = (t - tile_off[e]) * BM;              // within-segment row
  const int seg0 = tile_off[e] * BM;                  // segment global base
  const int rows_valid = counts[e] - m0;              // live rows this tile

  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int wm = wave / WCOLS, wn = wave % WCOLS;

  __shared__ __attribute__((aligned(16))) u8 smem[2][(BM + NB * BN) * 128];
  const int b_off = BM * 128;
  const int b2_off = (BM + BN) * 128;

  const u8* wa = w + (long)e * NB * n_cols * Kp;
  const u8* wg = wa + (long)n0 * Kp;
  const u8* wu = wa + (long)(n_cols + n0) * Kp;       // up rows (stage 1)
  const u8* aa = GATE_SILU ? a : a + (long)seg0 * Kp;
  const int* rt = row_tok ? row_tok + seg0 : nullptr;

  f32x4 accg[MF][NF], accu[GATE_SILU ? MF : 1][GATE_SILU ? NF : 1];
#pragma unroll
  for (int i = 0; i < MF; ++i)
#pragma unroll
    for (int j = 0; j < NF; ++j) {
      accg[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (GATE_SILU) accu[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    }

  // prologue
  if (GATE_SILU)
    grouped_stage<BM, WAVES, true>(smem[0], aa, Kp, rt, m0, rows_valid, wave,
                                   lane);
  else
    grouped_stage<BM, WAVES, false>(smem[0], aa, Kp, nullptr, m0, BM, wave,
                                    lane);
  grouped_stage<BN, WAVES, false>(smem[0] + b_off, wg, Kp, nullptr, 0, BN,
                                  wave, lane);
  if (GATE_SILU)
    grouped_stage<BN, WAVES, false>(smem[0] + b2_off, wu, Kp, nullptr, 0, BN,
                                    wave, lane);
  __syncthreads();

  const int KT = (int)(Kp >> 7);
  const int q = lane >> 4;
  for (int kt = 0; kt < KT; ++kt) {
    const int p = kt & 1;
    const u8* aT = smem[p];
    const u8* bgT = smem[p] + b_off;
    const u8* buT = smem[p] + b2_off;
    if (kt + 1 < KT) {
      const long ko = (long)(kt + 1) * 128;
      if (GATE_SILU)
        grouped_stage<BM, WAVES, true>(smem[p ^ 1], aa + ko, Kp, rt, m0,
                                       rows_valid, wave, lane);
      else
        grouped_stage<BM, WAVES, false>(smem[p ^ 1], aa + ko, Kp, nullptr, m0,
                                        BM, wave, lane);
      grouped_stage<BN, WAVES, false>(smem[p ^ 1] + b_off, wg + ko, Kp,
                                      nullptr, 0, BN, wave, lane);
      if (GATE_SILU)
        grouped_stage<BN, WAVES, false>(smem[p ^ 1] + b2_off, wu + ko, Kp,
                                        nullptr, 0, BN, wave, lane);
    }
    i32x8 bg[NF], bu[GATE_SILU ? NF : 1];
#pragma unroll
    for (int j = 0; j < NF; ++j) {
      bg[j] = lds_frag_row(bgT, wn * WN + j * 16 + (lane & 15), q);
      if (GATE_SILU)
        bu[j] = lds_frag_row(buT, wn * WN + j * 16 + (lane & 15), q);
    }
#pragma unroll
    for (int i = 0; i < MF; ++i) {
      const i32x8 af = lds_frag_row(aT, wm * WM + i * 16 + (lane & 15), q);
#pragma unroll
      for (int j = 0; j < NF; ++j) {
        accg[i][j] = mfma128(af, bg[j], accg[i][j]);
        if (GATE_SILU) accu[i][j] = mfma128(af, bu[j], accu[i][j]);
      }
    }
    __syncthreads();
  }

  // epilogue: D[16,16] lane l holds rows (l/16)*4+r, col l%16
  const int drow = (lane >> 4) * 4;
  const int dcol = lane & 15;
  const float* ws = w_scale + (long)e * NB * n_cols;
#pragma unroll
  for (int i = 0; i < MF; ++i) {
    float as[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int grow = wm * WM + i * 16 + drow + r;
      if (GATE_SILU) {
        int tok = (grow < rows_valid) ? rt[m0 + grow] : 0;
        if (tok < 0) tok = 0;  // padding rows: same clamp as the staging
        as[r] = a_scale[tok];
      } else {
        as[r] = a_scale[seg0 + m0 + grow];
      }
    }
#pragma unroll
    for (int j = 0; j < NF; ++j) {
      const int gn = n0 + wn * WN + j * 16 + dcol;
      const float wsg = ws[gn];
      const float wsu = GATE_SILU ? ws[n_cols + gn] : 0.f;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int grow = wm * WM + i * 16 + drow + r;
        const long o = (long)(seg0 + m0 + grow) * n_cols + gn;
        float v = accg[i][j][r] * as[r] * wsg;
        if (GATE_SILU) {
          const float g = v;
          const float u = accu[i][j][r] * as[r] * wsu;
          v = g / (1.0f + __expf(-g)) * u;
        }
        out[o] = f2bf(v);
      }
    }
  }
}

extern "C" void sutro_grouped_gemm_fp8(
    void* out, const void* a, const float* a_scale, const void* w,
    const float* w_scale, const int* row_tok, const int* tile_off,
    const int* counts, int n_experts, int max_tiles, int n_cols, long Kp,
    int gate_silu, int bm, hipStream_t stream) {
  if (max_tiles == 0) return;
#define GQ_LAUNCH(GS, BM, BN, WR, WC)                                        \
  {                                                                          \
    dim3 grid((unsigned)max_tiles, (unsigned)(n_cols / BN)),                 \
        block(WR* WC * 64);                                                  \
    hipLaunchKernelGGL((grouped_gemm_fp8_kernel<GS, BM, BN, WR, WC>), grid,  \
                       block, 0, stream, (u16*)out, (const u8*)a, a_scale,   \
                       (const u8*)w, w_scale, row_tok, tile_off, counts,     \
                       n_experts, n_cols, Kp);                               \
    return;                                                                  \
  }
  /* no hipGetLastError in this launcher: error-state queries are rejected
     while a stream is capturing (decode steps replay under hipGraphs) */
  if (bm == 128 && n_cols % 128 == 0) {
    if (gate_silu) GQ_LAUNCH(1, 128, 128, 2, 4)
    else GQ_LAUNCH(0, 128, 128, 2, 4)
  }
  if (bm == 128) {
    if (gate_silu) GQ_LAUNCH(1, 128, 64, 4, 2)
    else GQ_LAUNCH(0, 128, 64, 4, 2)
  }
  if (gate_silu) GQ_LAUNCH(1, 64, 64, 2, 2)
  else GQ_LAUNCH(0, 64, 64, 2, 2)
#undef GQ_LAUNCH
}
