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
// (= 128 K-elements): the global_load_lds dwordx4 staging and the gswz
// swizzle of the bf16 kernel carry over byte for byte. One K-tile is ONE
// mfma_scale_f32_16x16x128_f8f6f4 per (i, j) fragment pair (cbsz = blgp = 0:
// e4m3 x e4m3) — the block-scaled form is the only fp8 MFMA that runs at
// twice the bf16 rate. Both hardware block scales are e8m0 1.0; the real
// per-row / per-channel f32 scales are applied in the epilogue, before
// SwiGLU: acc * a_scale[row] * w_scale[e, n].
//
// Operand lane map (16x16x128, 8-bit formats): lane l supplies row l & 15,
// k = 32 * (l >> 4) + j for byte j of its 32-byte operand — two consecutive
// 16-byte chunks of the 128-byte LDS row. Verified with exact integer data
// by tests/test_gpu_moe_fp8.py. C/D layout is the 16x16 shape's:
// col = l & 15, row = (l >> 4) * 4 + reg.
#include "common.h"

typedef int i32x8 __attribute__((ext_vector_type(8)));

// e8m0 1.0 in every byte: the hardware block scale is a no-op
#define FP8_SCALE_ONE 0x7f7f7f7f

__device__ __forceinline__ f32x4 mfma128q(i32x8 a, i32x8 b, f32x4 c) {
  return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(
      a, b, c, 0, 0, 0, FP8_SCALE_ONE, 0, FP8_SCALE_ONE);
}

__device__ __forceinline__ void glds16q(const u32* g, u32* lds) {
  __builtin_amdgcn_global_load_lds(
      (const __attribute__((address_space(1))) u32*)g,
      (__attribute__((address_space(3))) u32*)lds, 16, 0, 0);
}

// swizzle mode 2 of gemm_tn.hip: row bits 1..3 XOR'd into the 16B chunk idx
__device__ __forceinline__ u32 qswz(u32 byte) {
  return byte ^ (((byte >> 8) & 7u) << 4);
}

// ---- row quantisation: bf16 [R, K] -> e4m3 [R, Kp] + f32 scale [R] ----
// scale = amax / 448 (true f32 division; 1 for an all-zero row),
// code = e4m3_rne(clamp(x / scale, -448, 448)) — the formula of
// torch_ref.quantize_rows_fp8, which this matches bit for bit. One wave per
// row, 16-byte loads; rows of up to 64 * 8 * QR_CACHE elements are held in
// registers between the amax reduction and the convert (one pass over
// memory), wider rows are read a second time. The tail [K, Kp) is zeroed.
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
  const float scale = amax > 0.f ? amax / 448.0f : 1.0f;
  if (lane == 0) out_scale[row] = scale;

  auto conv8 = [&](const u16x8 t) {
    u32 w[2];
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      float f[4];
#pragma unroll
      for (int e = 0; e < 4; ++e)
        f[e] = fminf(fmaxf(bf2f(t[p * 4 + e]) / scale, -448.0f), 448.0f);
      w[p] = (u32)f2fp8x2(f[0], f[1]) | ((u32)f2fp8x2(f[2], f[3]) << 16);
    }
    return u32x2{w[0], w[1]};
  };

  if (cached) {
#pragma unroll
    for (int i = 0; i < QR_CACHE; ++i) {
      const int c = i * 64 + lane;
      if (c < nch) *(u32x2*)(qr + c * 8) = conv8(v[i]);
    }
  } else {
    for (int c = lane; c < nch; c += 64)
      *(u32x2*)(qr + c * 8) = conv8(*(const u16x8*)(xr + c * 8));
  }
  for (int c = nch + lane; c < nchp; c += 64)
    *(u32x2*)(qr + c * 8) = u32x2{0u, 0u};
}

extern "C" void sutro_quant_rows_fp8(void* out_q, float* out_scale,
                                     const void* x, const int* row_limit,
                                     int limit_mul, long R, int K, int Kp,
                                     hipStream_t stream) {
  if (R == 0) return;
  // static grid, no host sync, no hipGetLastError: runs inside captured
  // decode steps
  hipLaunchKernelGGL(quant_rows_fp8_kernel, dim3((unsigned)((R + 3) / 4)),
                     dim3(256), 0, stream, (u8*)out_q, out_scale,
                     (const u16*)x, row_limit, limit_mul, R, K, Kp);
}

// ---- grouped GEMM ----

// Stage a ROWS x 128-byte tile with WAVES waves; each wave issues
// ROWS/(8*WAVES) x 1KB chunks (byte-identical to gg_stage of the bf16
// kernel: a 128-byte row is 128 e4m3 instead of 64 bf16).
template <int ROWS, int WAVES, bool GATHER>
__device__ __forceinline__ void gq_stage(
    u8* lds, const u8* gsrc, long row_stride_b, const int* row_tok,
    int m0, int rows_valid, int wave, int lane) {
  constexpr int CH = ROWS / (8 * WAVES);
  static_assert(CH >= 1, "tile too small for wave count");
#pragma unroll
  for (int j = 0; j < CH; ++j) {
    const int c = wave * CH + j;
    const u32 b = (u32)c * 1024u + (u32)lane * 16u;  // lane-linear LDS byte
    const u32 lb = qswz(b);                          // pre-swizzled source
    int row = (int)(lb >> 7);
    long grow;
    if (GATHER) {
      int r = m0 + row;
      int tok = (row < rows_valid) ? row_tok[r] : 0;
      if (tok < 0) tok = 0;  // padding: deterministic garbage, discarded
      grow = (long)tok;
    } else {
      grow = (long)(m0 + min(row, rows_valid - 1));
    }
    glds16q((const u32*)(gsrc + grow * row_stride_b + (lb & 127u)),
            (u32*)(lds + b));
  }
}

// 32 operand bytes of one lane: k-quarter q = lane >> 4 of a 128-byte row,
// i.e. the swizzled 16-byte chunks 2q and 2q+1
__device__ __forceinline__ i32x8 gq_frag(const u8* lds, int row, int q) {
  const u32 lb = (u32)row * 128u + (u32)q * 32u;
  const u32x4 lo = *(const u32x4*)(lds + qswz(lb));
  const u32x4 hi = *(const u32x4*)(lds + qswz(lb + 16u));
  return i32x8{(int)lo[0], (int)lo[1], (int)lo[2], (int)lo[3],
               (int)hi[0], (int)hi[1], (int)hi[2], (int)hi[3]};
}

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
    gq_stage<BM, WAVES, true>(smem[0], aa, Kp, rt, m0, rows_valid, wave, lane);
  else
    gq_stage<BM, WAVES, false>(smem[0], aa, Kp, nullptr, m0, BM, wave, lane);
  gq_stage<BN, WAVES, false>(smem[0] + b_off, wg, Kp, nullptr, 0, BN, wave,
                             lane);
  if (GATE_SILU)
    gq_stage<BN, WAVES, false>(smem[0] + b2_off, wu, Kp, nullptr, 0, BN, wave,
                               lane);
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
        gq_stage<BM, WAVES, true>(smem[p ^ 1], aa + ko, Kp, rt, m0,
                                  rows_valid, wave, lane);
      else
        gq_stage<BM, WAVES, false>(smem[p ^ 1], aa + ko, Kp, nullptr, m0, BM,
                                   wave, lane);
      gq_stage<BN, WAVES, false>(smem[p ^ 1] + b_off, wg + ko, Kp, nullptr, 0,
                                 BN, wave, lane);
      if (GATE_SILU)
        gq_stage<BN, WAVES, false>(smem[p ^ 1] + b2_off, wu + ko, Kp, nullptr,
                                   0, BN, wave, lane);
    }
    i32x8 bg[NF], bu[GATE_SILU ? NF : 1];
#pragma unroll
    for (int j = 0; j < NF; ++j) {
      bg[j] = gq_frag(bgT, wn * WN + j * 16 + (lane & 15), q);
      if (GATE_SILU) bu[j] = gq_frag(buT, wn * WN + j * 16 + (lane & 15), q);
    }
#pragma unroll
    for (int i = 0; i < MF; ++i) {
      const i32x8 af = gq_frag(aT, wm * WM + i * 16 + (lane & 15), q);
#pragma unroll
      for (int j = 0; j < NF; ++j) {
        accg[i][j] = mfma128q(af, bg[j], accg[i][j]);
        if (GATE_SILU) accu[i][j] = mfma128q(af, bu[j], accu[i][j]);
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
