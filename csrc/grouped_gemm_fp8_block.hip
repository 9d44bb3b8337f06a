// Block-scaled FP8 (OCP e4m3) expert weights for the dropless MoE grouped
// GEMM on MI355X: the experts of the published block-FP8 checkpoints
// (`weight` e4m3 + `weight_scale_inv` f32, one scale per 128x128 block).
//
// The contract is csrc/grouped_gemm_fp8.hip's (segments padded to the tile
// height, static grid that exits early on the device-side tile_off table,
// expert lookup by bisection, row_tok gather in stage 1, gate/up double
// stream, no host sync and no error-state query: it runs inside captured
// decode steps). The operands are the dense block kernel's
// (csrc/gemm_tn_fp8_block_pipe.hip, torch_ref.fp8_block_linear):
//
//   A: e4m3 [., K] + f32 a_s [K/128, rows], K-block-major with row stride
//      lda_s (stage 1: codes AND scales indexed through row_tok)
//   W: e4m3 [E, N, K] + f32 w_s [E, N/128, K/128]
//   K % 128 == 0, n_cols % 128 == 0: a gate/up half starts on a scale-block
//   row and a 64- or 128-column tile lies inside one scale block.
//
// Arithmetic. One K-tile (128 bytes of an LDS row) is one scale group. Its
// MFMAs (mfma_scale_f32_16x16x128_f8f6f4, hardware scales e8m0 1.0) start
// from a zero C and give the unscaled partial products p, which are folded
// into the running accumulators by
//     acc[r] = fma(p[r], a_s[kb, row r] * w_s[e, n / 128, kb], acc[r])
// with the factor formed as one f32 product, kb ascending — the fold of the
// dense block kernel, so one expert with an identity row_tok reproduces that
// kernel bit for bit. The weight scale is uniform over the block for a
// (tile, kb) pair: one scalar load, fetched a K-tile ahead.
//
// Where the activation scales come from. D[16,16] lane l holds rows
// (l/16)*4 + r of column l%16, so a lane needs the 4 scales of rows
// (l/16)*4 .. +3 of each of its m-fragments.
//   stage 2 (plain): the rows of a tile are consecutive in a_s[kb, :], so
//     those 4 scales are one 16-byte global read per fragment; the reads of
//     K-tile t+1 are issued before the staging of that tile and are held in
//     registers over the barrier.
//   stage 1 (gather): the rows are tokens, scattered in a_s[kb, :]. The BM
//     scales of K-tile t+1 take the road of the tiles: `global_load_lds`,
//     4 bytes a lane, one load per row, by the first BM/64 waves into a
//     double-buffered [2][BM] f32 area beside the tile buffers; padding rows
//     are clamped to token 0 exactly as the code staging does. The fragment's
//     4 scales are then one 16-byte LDS read.
// The loop is the simple double-buffered one with a full barrier per K-tile.
//
// Stage 1 epilogue (GATE_Q): the block owns BM rows x 128 columns of the
// activation = whole 128-wide K groups of the stage-2 input, so it writes
// that input itself, quantised, and the bf16 round trip and the second
// quantiser pass disappear:
//   1. v = silu(g) * u in f32 (g / (1 + __expf(-g)) * u), rounded once to
//      bf16 — the value the separate path would have stored;
//   2. per row the amax of the 128 rounded values: over the lane's n-
//      fragments, a 16-lane shuffle reduction, then across the 4 N-waves
//      through LDS (the tile buffers are free after the last barrier);
//   3. the rule of quant_rows_fp8_block128 (fp8_quant_scale and
//      fp8_quant_clamp of fp8_gemm.h, then e4m3 round-to-nearest-even);
//   4. the codes are collected in LDS as a plain [BM][128] byte tile and
//      leave as full 128-byte rows in 16-byte stores to act_q [rows, I];
//      the scales go to act_s[n0 / 128, row] (row stride ldo_s).
// The result is bit-identical to writing bf16 and running the quantiser.
//
// Tiles (waves as WROWS(M) x WCOLS(N)): stage 1 always 128 columns wide,
// 128x128 and 64x128 with 8 waves as 2x4; stage 2 the per-channel kernel's
// configurations for n_cols % 128 == 0, 128x128 (2x4) and 64x64 (2x2).
// Operand lane map and C/D layout: see mfma128 in fp8_gemm.h.
#include "fp8_gemm.h"

// grouped_stage of lds_tile.h with the wave-uniform LDS base: here the wave
// index is in a scalar register (readfirstlane), and the lane-linear address
// the shared form passes costs a register and 8 to 17 instructions a kernel.
template <int ROWS, int WAVES, bool GATHER>
__device__ __forceinline__ void stage_tile(
    u8* lds, const u8* gsrc, long row_stride_b, const int* row_tok, int m0,
    int rows_valid, int wave, int lane) {
  constexpr int CH = ROWS / (8 * WAVES);
  static_assert(CH >= 1, "tile too small for wave count");
#pragma unroll
  for (int j = 0; j < CH; ++j) {
    const u32 cb = (u32)(wave * CH + j) * 1024u;     // wave-uniform LDS base
    const u32 lb = swz2(cb + (u32)lane * 16u);       // pre-swizzled source
    const int row = (int)(lb >> 7);
    long grow;
    if (GATHER) {
      int tok = (row < rows_valid) ? row_tok[m0 + row] : 0;
      if (tok < 0) tok = 0;  // padding: deterministic garbage, discarded
      grow = (long)tok;
    } else {
      grow = (long)(m0 + min(row, rows_valid - 1));
    }
    glds16(gsrc + grow * row_stride_b + (lb & 127u), lds + cb);
  }
}

// NO_PACKED_F32: the fold is scalar v_fma_f32 on purpose, as in the dense
// block kernel

// GATE_Q=1: B has two streams (gate/up at N-offset 0 and n_cols), SwiGLU and
// the group quantiser in the epilogue, out_q / out_s written (BN == 128).
// GATE_Q=0: plain B, bf16 store to out.
template <int GATE_Q, int BM, int BN, int WROWS, int WCOLS>
NO_PACKED_F32 __global__ __launch_bounds__(WROWS* WCOLS * 64) void
grouped_gemm_fp8_block_kernel(
    u16* __restrict__ out,            // GATE_Q=0: [rows_max, n_cols] bf16
    u8* __restrict__ out_q,           // GATE_Q=1: [rows_max, n_cols] e4m3
    float* __restrict__ out_s,        // GATE_Q=1: [n_cols/128, ldo_s]
    long ldo_s,
    const u8* __restrict__ a,         // GATHER: [T, K]; else [rows_max, K]
    const float* __restrict__ a_s,    // [K/128, lda_s]: tokens / padded rows
    long lda_s,
    const u8* __restrict__ w,         // [E, N, K] (N = n_cols or 2*n_cols)
    const float* __restrict__ w_s,    // [E, N/128, K/128]
    const int* __restrict__ row_tok,  // [rows_max] (GATE_Q=1)
    const int* __restrict__ tile_off,  // [E+1] padded-offset / BM
    const int* __restrict__ counts,    // [E] live rows per expert
    int n_experts, int n_cols, long K) {
  constexpr int WAVES = WROWS * WCOLS;
  constexpr int WM = BM / WROWS;
  constexpr int WN = BN / WCOLS;
  constexpr int MF = WM / 16;
  constexpr int NF = WN / 16;
  constexpr int NB = GATE_Q ? 2 : 1;
  static_assert(!GATE_Q || (BN == 128 && WCOLS == 4 && BM % 64 == 0),
                "the quantising epilogue owns whole 128-column groups");
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
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wm = wave / WCOLS, wn = wave % WCOLS;

  __shared__ __attribute__((aligned(1024))) u8 smem[2][(BM + NB * BN) * 128];
  // stage 1: the BM gathered activation scales of a K-tile, double-buffered
  __shared__ __attribute__((aligned(16))) float as_lds[GATE_Q ? 2 : 1]
                                                      [GATE_Q ? BM : 4];
  const int b_off = BM * 128;
  const int b2_off = (BM + BN) * 128;

  const int KT = (int)(K >> 7);
  const u8* wa = w + (long)e * NB * n_cols * K;
  const u8* wg = wa + (long)n0 * K;
  const u8* wu = wa + (long)(n_cols + n0) * K;        // up rows (stage 1)
  const u8* aa = GATE_Q ? a : a + (long)seg0 * K;
  const int* rt = GATE_Q ? row_tok + seg0 : nullptr;
  // scale-block rows of this tile's gate (or plain) and up columns
  const float* wsg = w_s + ((long)e * (NB * n_cols >> 7) + (n0 >> 7)) * KT;
  const float* wsu = wsg + (long)(n_cols >> 7) * KT;

  const int q = lane >> 4;
  const int drow = q * 4;
  const int dcol = lane & 15;

  // activation scales. Stage 1: lane l of wave v < BM/64 copies the scale of
  // tile row v*64 + l (its token's, padding clamped to token 0). Stage 2:
  // this lane's 4 rows of m-fragment i are 16 contiguous, aligned bytes.
  const float* asg = nullptr;
  if (GATE_Q) {
    if (wave < BM / 64) {
      const int row = wave * 64 + lane;
      int tok = (row < rows_valid) ? rt[m0 + row] : 0;
      if (tok < 0) tok = 0;
      asg = a_s + tok;
    }
  } else {
    asg = a_s + seg0 + m0 + wm * WM + drow;
  }

  f32x4 accg[MF][NF], accu[GATE_Q ? MF : 1][GATE_Q ? NF : 1];
#pragma unroll
  for (int i = 0; i < MF; ++i)
#pragma unroll
    for (int j = 0; j < NF; ++j) {
      accg[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (GATE_Q) accu[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    }

  f32x4 asn[MF];          // stage 2: the scales of the next K-tile
  float wsgn, wsun = 0.f;  // weight scales of the next K-tile

#define STAGE_KTILE(BUF_, KB_)                                               \
  {                                                                          \
    const long ko = (long)(KB_) * 128;                                       \
    if (GATE_Q) {                                                            \
      if (wave < BM / 64)                                                    \
        glds4(asg + (long)(KB_) * lda_s, &as_lds[BUF_][wave * 64]);          \
      stage_tile<BM, WAVES, true>(smem[BUF_], aa + ko, K, rt, m0,            \
                                  rows_valid, wave, lane);                   \
    } else {                                                                 \
      _Pragma("unroll") for (int i = 0; i < MF; ++i)                         \
          asn[i] = *(const f32x4*)(asg + (long)(KB_) * lda_s + i * 16);      \
      stage_tile<BM, WAVES, false>(smem[BUF_], aa + ko, K, nullptr, m0, BM,  \
                                   wave, lane);                              \
    }                                                                        \
    wsgn = wsg[KB_];                                                         \
    if (GATE_Q) wsun = wsu[KB_];                                             \
    stage_tile<BN, WAVES, false>(smem[BUF_] + b_off, wg + ko, K, nullptr, 0, \
                                 BN, wave, lane);                            \
    if (GATE_Q)                                                              \
      stage_tile<BN, WAVES, false>(smem[BUF_] + b2_off, wu + ko, K, nullptr, \
                                   0, BN, wave, lane);                       \
  }

  STAGE_KTILE(0, 0)
  __syncthreads();

  for (int kt = 0; kt < KT; ++kt) {
    const int p = kt & 1;
    const u8* aT = smem[p];
    const u8* bgT = smem[p] + b_off;
    const u8* buT = smem[p] + b2_off;
    // this K-tile's scales: fetched during the previous one
    const float wsgc = wsgn, wsuc = wsun;
    f32x4 asc[MF];
#pragma unroll
    for (int i = 0; i < MF; ++i) {
      if (GATE_Q)
        asc[i] = *(const f32x4*)&as_lds[p][wm * WM + i * 16 + drow];
      else
        asc[i] = asn[i];
    }
    if (kt + 1 < KT) STAGE_KTILE(p ^ 1, kt + 1)

    i32x8 bg[NF], bu[GATE_Q ? NF : 1];
#pragma unroll
    for (int j = 0; j < NF; ++j) {
      bg[j] = lds_frag_row(bgT, wn * WN + j * 16 + dcol, q);
      if (GATE_Q) bu[j] = lds_frag_row(buT, wn * WN + j * 16 + dcol, q);
    }
#pragma unroll
    for (int i = 0; i < MF; ++i) {
      const i32x8 af = lds_frag_row(aT, wm * WM + i * 16 + dcol, q);
      // one f32 product per (row, weight block) as the factor
      float fg[4], fu[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        fg[r] = asc[i][r] * wsgc;
        fu[r] = GATE_Q ? asc[i][r] * wsuc : 0.f;
      }
#pragma unroll
      for (int j = 0; j < NF; ++j) {
        const f32x4 pg = mfma128z(af, bg[j]);
#pragma unroll
        for (int r = 0; r < 4; ++r)
          accg[i][j][r] = __builtin_fmaf(pg[r], fg[r], accg[i][j][r]);
        if (GATE_Q) {
          const f32x4 pu = mfma128z(af, bu[j]);
#pragma unroll
          for (int r = 0; r < 4; ++r)
            accu[i][j][r] = __builtin_fmaf(pu[r], fu[r], accu[i][j][r]);
        }
      }
    }
    __syncthreads();
  }
#undef STAGE_KTILE

  // epilogue: D[16,16] lane l holds rows (l/16)*4+r, col l%16; the
  // accumulators already carry their scales
  if constexpr (!GATE_Q) {
#pragma unroll
    for (int i = 0; i < MF; ++i)
#pragma unroll
      for (int j = 0; j < NF; ++j) {
        const int gn = n0 + wn * WN + j * 16 + dcol;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int grow = wm * WM + i * 16 + drow + r;
          out[(long)(seg0 + m0 + grow) * n_cols + gn] = f2bf(accg[i][j][r]);
        }
      }
  } else {
  static_assert(NF % 2 == 0, "codes are converted in pairs");
  // the tile buffers are free after the loop's last barrier:
  //   red  [BM][WCOLS] f32  per-row amax of each N-wave
  //   code [BM][128]   u8   the quantised tile, plain row-major
  float* red = (float*)&smem[0][0];
  u8* code = &smem[0][0] + BM * WCOLS * 4;

  // SwiGLU in f32, one rounding to bf16, the rounded value back in f32
  float x[MF][NF][4];
#pragma unroll
  for (int i = 0; i < MF; ++i) {
    float am[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < NF; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float g = accg[i][j][r];
        const float u = accu[i][j][r];
        const float v = bf2f(f2bf(g / (1.0f + __expf(-g)) * u));
        x[i][j][r] = v;
        am[r] = fmaxf(am[r], fabsf(v));
      }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
#pragma unroll
      for (int o = 8; o > 0; o >>= 1)
        am[r] = fmaxf(am[r], __shfl_xor(am[r], o, 64));
      if (dcol == 0) red[(wm * WM + i * 16 + drow + r) * WCOLS + wn] = am[r];
    }
  }
  __syncthreads();

#pragma unroll
  for (int i = 0; i < MF; ++i)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = wm * WM + i * 16 + drow + r;
      const f32x4 a4 = *(const f32x4*)&red[row * WCOLS];
      const float amax = fmaxf(fmaxf(a4[0], a4[1]), fmaxf(a4[2], a4[3]));
      const float scale = fp8_quant_scale(amax);
      if (wn == 0 && dcol == 0)
        out_s[(long)(n0 >> 7) * ldo_s + seg0 + m0 + row] = scale;
#pragma unroll
      for (int j = 0; j < NF; j += 2) {
        const float f0 = fp8_quant_clamp(x[i][j][r], scale);
        const float f1 = fp8_quant_clamp(x[i][j + 1][r], scale);
        const u16 c2 = f2fp8x2(f0, f1);
        code[row * 128 + wn * WN + j * 16 + dcol] = (u8)(c2 & 0xff);
        code[row * 128 + wn * WN + (j + 1) * 16 + dcol] = (u8)(c2 >> 8);
      }
    }
  __syncthreads();

  // full 128-byte rows, 16 bytes a thread
#pragma unroll
  for (int c = threadIdx.x; c < BM * 8; c += WAVES * 64) {
    const int row = c >> 3, ch = c & 7;
    *(u32x4*)(out_q + (long)(seg0 + m0 + row) * n_cols + n0 + ch * 16) =
        *(const u32x4*)(code + row * 128 + ch * 16);
  }
  }  // GATE_Q
}

// Plain stage (down): out [rows, n_cols] bf16. K % 128 == 0,
// n_cols % 128 == 0, a_s 16-byte aligned with lda_s % 4 == 0 and at least
// max_tiles * bm rows. Static grid, no host sync, no hipGetLastError: runs
// inside captured decode steps.
extern "C" void sutro_grouped_gemm_fp8_block(
    void* out, const void* a, const float* a_s, long lda_s, const void* w,
    const float* w_s, const int* tile_off, const int* counts, int n_experts,
    int max_tiles, int n_cols, long K, int bm, hipStream_t stream) {
  if (max_tiles == 0) return;
#define GB_LAUNCH(BM, BN, WR, WC)                                            \
  {                                                                          \
    dim3 grid((unsigned)max_tiles, (unsigned)(n_cols / BN)),                 \
        block(WR* WC * 64);                                                  \
    hipLaunchKernelGGL((grouped_gemm_fp8_block_kernel<0, BM, BN, WR, WC>),   \
                       grid, block, 0, stream, (u16*)out, (u8*)nullptr,      \
                       (float*)nullptr, 0L, (const u8*)a, a_s, lda_s,        \
                       (const u8*)w, w_s, (const int*)nullptr, tile_off,     \
                       counts, n_experts, n_cols, K);                        \
    return;                                                                  \
  }
  if (bm == 128) GB_LAUNCH(128, 128, 2, 4)
  GB_LAUNCH(64, 64, 2, 2)
#undef GB_LAUNCH
}

// Stage 1 (gate/up through row_tok, SwiGLU, group quantiser): act_q
// [rows, n_cols] e4m3 + act_s [n_cols/128, ldo_s] f32. w is [E, 2*n_cols, K].
extern "C" void sutro_grouped_gemm_fp8_block_gate_q(
    void* act_q, float* act_s, long ldo_s, const void* a, const float* a_s,
    long lda_s, const void* w, const float* w_s, const int* row_tok,
    const int* tile_off, const int* counts, int n_experts, int max_tiles,
    int n_cols, long K, int bm, hipStream_t stream) {
  if (max_tiles == 0) return;
#define GB_LAUNCH(BM)                                                        \
  {                                                                          \
    dim3 grid((unsigned)max_tiles, (unsigned)(n_cols / 128)), block(512);    \
    hipLaunchKernelGGL((grouped_gemm_fp8_block_kernel<1, BM, 128, 2, 4>),    \
                       grid, block, 0, stream, (u16*)nullptr, (u8*)act_q,    \
                       act_s, ldo_s, (const u8*)a, a_s, lda_s, (const u8*)w, \
                       w_s, row_tok, tile_off, counts, n_experts, n_cols,    \
                       K);                                                   \
    return;                                                                  \
  }
  if (bm == 128) GB_LAUNCH(128)
  GB_LAUNCH(64)
#undef GB_LAUNCH
}
