// MXFP4 (OCP MX: e2m1 codes + e8m0 scale per 32 K-elements) expert weights
// for the dropless MoE grouped GEMM on MI355X. W4A8: activations keep the
// e4m3 + f32-per-row path of csrc/grouped_gemm_fp8.hip.
//
// Same contract as sutro_grouped_gemm_fp8 (segments padded to the tile
// height, static grid that exits early on the device-side tile_off table,
// row_tok gather in stage 1 with the -1 -> 0 clamp in staging and epilogue,
// gate/up double stream with the SwiGLU fused into the epilogue, the same
// three tile configurations) except for the weight format:
//
//   A:      e4m3 [., Kp] + f32 scale per row (stage 1: indexed by row_tok)
//   W:      u8 [E, N, Kp/2], two e2m1 codes per byte, element 2i in the low
//           nibble of byte i; codes in [K, Kp) are 0
//   scales: u8 [E, N, Kp/32] e8m0 (2^(b-127)), one per 32 consecutive K;
//           natural layout, no pre-arrangement
//   out:    bf16
//
// One K-tile (128 elements) is ONE mfma_scale_f32_16x16x128_f8f6f4 per
// (i, j) fragment pair with cbsz = 0 (A e4m3) and blgp = 4 (B e2m1). The A
// block scale is e8m0 1.0, the B block scale is the real one, so the
// dequantisation of W happens inside the instruction; the epilogue is
// acc * a_scale[row], then SwiGLU.
//
// Operand maps of the mixed e4m3 x e2m1 form, found with exact data on the
// hardware and pinned by
// tests/test_gpu_moe_mxfp4.py::test_lane_and_scale_maps_exact. q = l >> 4
// is the lane's k-group, j = 0..31 the element index inside a lane's operand.
//   B (e2m1, 16 bytes in the low four dwords of the i32x8): lane l supplies
//     weight row l & 15 and k = 32q + j, code j = nibble j & 1 of byte
//     j >> 1 (low nibble first) — 32 consecutive k, as expected.
//   B scale: with opsel = 0, byte 0 of lane l's scale register scales that
//     lane's own 32 elements, i.e. block q of row l & 15 — as expected.
//   A (e4m3, 32 bytes): lane l supplies row l & 15 and
//         k = 64 * (j >> 4) + 16 * q + (j & 15),
//     two 16-element runs 16q.. and 64+16q.. — NOT k = 32q + j: the low four
//     dwords of the four k-groups are the first 64 k of the tile, the high
//     four dwords the second 64, for 8-bit and 4-bit operands alike (a 4-bit
//     operand has only the low four, which then span all 128 k). The fp8
//     kernel's k = 32q + j on both operands is the same instruction seen
//     where A and B share the permutation and the scales are 1; with a 4-bit
//     B it would multiply the wrong pairs and apply the scales of blocks
//     0, 2, 0, 2, 1, 3, 1, 3 to the eight 16-element runs of a K-tile.
//   C/D: the 16x16 shape's, col = l & 15, row = (l >> 4) * 4 + reg.
//
// Scales are 1/16 of the weight bytes and skip LDS: each lane loads the one
// byte of its own (row, k-block) straight from global into the scale
// register — a zero-extended byte load puts it in byte 0, which is what
// opsel = 0 selects, so no shift is needed — one K-tile ahead, issued after
// the tile's global_load_lds so that the barrier that retires the staging
// retires the scales with it.
//
// LDS: the A tile is staged as in the fp8 kernel (128-byte rows, qswz); a
// lane reads the 16-byte chunks q and 4 + q of its row. A K-tile of W is 64
// bytes per row; one wave's 1 KiB global_load_lds piece covers 16 rows, and a
// lane reads one 16-byte chunk (row l & 15, chunk q). ds_read_b128 serves
// 16 lanes per LDS cycle from a 256-byte bank window (4 rows of W): chunk c
// of row r is stored at chunk c ^ g((r >> 2) & 3) with g = {0, 2, 3, 1},
// which makes every 16-lane group hit 16 distinct 16-byte bank groups.
// tools/sim_grouped_gemm_mxfp4.py proves the staging / read bijection and the
// conflict-freeness of the W and the A reads; the row-bit XOR of qswz would
// put rows 0, 2, 4, ... of W on the same banks.
#include "common.h"

typedef int i32x8 __attribute__((ext_vector_type(8)));

// e8m0 1.0 in every byte: the A-side hardware block scale is a no-op
#define MX_SCALE_ONE 0x7f7f7f7f

// A e4m3 (cbsz 0) x B e2m1 (blgp 4); opsel 0 on both scale registers
__device__ __forceinline__ f32x4 mfma128x(i32x8 a, i32x8 b, f32x4 c,
                                          int b_scale) {
  return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(
      a, b, c, 0, 4, 0, MX_SCALE_ONE, 0, b_scale);
}

__device__ __forceinline__ void glds16x(const u32* g, u32* lds) {
  __builtin_amdgcn_global_load_lds(
      (const __attribute__((address_space(1))) u32*)g,
      (__attribute__((address_space(3))) u32*)lds, 16, 0, 0);
}

// A tile, 128-byte rows: row bits 1..3 XOR'd into the 16B chunk index
__device__ __forceinline__ u32 aswz(u32 byte) {
  return byte ^ (((byte >> 8) & 7u) << 4);
}

// W tile, 64-byte rows: chunk ^= g(row >> 2), g = {0, 2, 3, 1} packed in 0x78
__device__ __forceinline__ u32 wswz(u32 byte) {
  return byte ^ (((0x78u >> (((byte >> 8) & 3u) << 1)) & 3u) << 4);
}

// ---- weight quantisation: bf16 [R, K] -> e2m1 codes + e8m0 block scales ----
// The rule of torch_ref.quantize_weight_mxfp4 (OCP MX v1.0), bit for bit:
//   amax = max |w| over the block (elements past K count as 0)
//   b    = clamp(floor(log2(amax)) - 2 + 127, 0, 254), 127 when amax == 0
//        = max(biased_exponent(amax) - 2, 0) for finite amax
//   x    = clamp(w * 2^(127-b), -6, 6)         (exact: a power of two)
//   code = e2m1_rne(x), ties to even; no negative zero
// One wave per row, one 32-element block per lane and step. Runs once per
// shard at start-up.
__device__ __forceinline__ u32 e2m1_rne(float x) {
  const float m = fminf(fabsf(x), 6.0f);
  // midpoints of the grid {0, .5, 1, 1.5, 2, 3, 4, 6}; a tie goes to the
  // code with an even mantissa bit (0, 1, 2, 4)
  const u32 c = (u32)(m > 0.25f) + (u32)(m >= 0.75f) + (u32)(m > 1.25f) +
                (u32)(m >= 1.75f) + (u32)(m > 2.5f) + (u32)(m >= 3.5f) +
                (u32)(m > 5.0f);
  return (x < 0.f && c != 0u) ? (c | 8u) : c;
}

__global__ void __launch_bounds__(256) quant_weight_mxfp4_kernel(
    u8* __restrict__ out_q,      // [R, Kp/2]
    u8* __restrict__ out_scale,  // [R, Kp/32]
    const u16* __restrict__ x,   // [R, K] bf16
    long R, int K, int Kp) {
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= R) return;
  const u16* xr = x + row * K;
  u8* qr = out_q + row * (Kp >> 1);
  u8* sr = out_scale + row * (Kp >> 5);
  const int nblk = Kp >> 5;
  for (int blk = lane; blk < nblk; blk += 64) {
    float f[32];
    float amax = 0.f;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int k = blk * 32 + c * 8;
      u16x8 t = u16x8{0, 0, 0, 0, 0, 0, 0, 0};
      if (k < K) t = *(const u16x8*)(xr + k);  // K % 8 == 0
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        f[c * 8 + e] = bf2f(t[e]);
        amax = fmaxf(amax, fabsf(f[c * 8 + e]));
      }
    }
    const int ef = (int)((__float_as_uint(amax) >> 23) & 0xffu);
    const int b = amax > 0.f ? max(ef - 2, 0) : 127;
    const float inv = __uint_as_float((u32)(254 - b) << 23);  // 2^(127-b)
    u32 wds[4];
#pragma unroll
    for (int d = 0; d < 4; ++d) {
      u32 wd = 0;
#pragma unroll
      for (int e = 0; e < 8; ++e)
        wd |= e2m1_rne(f[d * 8 + e] * inv) << (4 * e);
      wds[d] = wd;
    }
    *(u32x4*)(qr + blk * 16) = u32x4{wds[0], wds[1], wds[2], wds[3]};
    sr[blk] = (u8)b;
  }
}

extern "C" void sutro_quant_weight_mxfp4(void* out_q, void* out_scale,
                                         const void* x, long R, int K, int Kp,
                                         hipStream_t stream) {
  if (R == 0) return;
  hipLaunchKernelGGL(quant_weight_mxfp4_kernel, dim3((unsigned)((R + 3) / 4)),
                     dim3(256), 0, stream, (u8*)out_q, (u8*)out_scale,
                     (const u16*)x, R, K, Kp);
}

// ---- grouped GEMM ----

// Stage a ROWS x 128-byte A tile with WAVES waves (gq_stage of the fp8
// kernel): each wave issues ROWS/(8*WAVES) x 1KB pieces.
template <int ROWS, int WAVES, bool GATHER>
__device__ __forceinline__ void gx_stage_a(
    u8* lds, const u8* gsrc, long row_stride_b, const int* row_tok,
    int m0, int rows_valid, int wave, int lane) {
  constexpr int CH = ROWS / (8 * WAVES);
  static_assert(CH >= 1, "tile too small for wave count");
#pragma unroll
  for (int j = 0; j < CH; ++j) {
    const int c = wave * CH + j;
    const u32 b = (u32)c * 1024u + (u32)lane * 16u;  // lane-linear LDS byte
    const u32 lb = aswz(b);                          // pre-swizzled source
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
    glds16x((const u32*)(gsrc + grow * row_stride_b + (lb & 127u)),
            (u32*)(lds + b));
  }
}

// Stage the W tile: NB streams of BN rows x 64 bytes, contiguous in LDS
// (stream 1 = the up rows, n_cols further down in global). A 1KB piece is 16
// rows; pieces are dealt round-robin to the waves (a wave-uniform branch
// when there are fewer pieces than waves).
template <int BN, int NB, int WAVES>
__device__ __forceinline__ void gx_stage_w(
    u8* lds, const u8* gsrc, long row_stride_b, int n_cols, int wave,
    int lane) {
  constexpr int PIECES = NB * BN / 16;
  constexpr int CH = (PIECES + WAVES - 1) / WAVES;
#pragma unroll
  for (int j = 0; j < CH; ++j) {
    const int c = j * WAVES + wave;
    if (PIECES % WAVES != 0 && c >= PIECES) break;
    const u32 b = (u32)c * 1024u + (u32)lane * 16u;  // lane-linear LDS byte
    const u32 lb = wswz(b);                          // pre-swizzled source
    const int row = (int)(lb >> 6);
    const long grow = row < BN ? row : n_cols + row - BN;
    glds16x((const u32*)(gsrc + grow * row_stride_b + (lb & 63u)),
            (u32*)(lds + b));
  }
}

// 32 e4m3 operand bytes of one lane, k-group q of a 128-byte row:
// k = 16q .. 16q+15 and 64+16q .. 64+16q+15 (16-byte chunks q and 4 + q)
__device__ __forceinline__ i32x8 gx_frag_a(const u8* lds, int row, int q) {
  const u32 lb = (u32)row * 128u + (u32)q * 16u;
  const u32x4 lo = *(const u32x4*)(lds + aswz(lb));
  const u32x4 hi = *(const u32x4*)(lds + aswz(lb + 64u));
  return i32x8{(int)lo[0], (int)lo[1], (int)lo[2], (int)lo[3],
               (int)hi[0], (int)hi[1], (int)hi[2], (int)hi[3]};
}

// 16 operand bytes (32 e2m1 codes) of one lane: k = 32q .. 32q+31, chunk q of
// a 64-byte row, in the low four dwords
__device__ __forceinline__ i32x8 gx_frag_w(const u8* lds, int row, int q) {
  const u32 lb = (u32)row * 64u + (u32)q * 16u;
  const u32x4 v = *(const u32x4*)(lds + wswz(lb));
  return i32x8{(int)v[0], (int)v[1], (int)v[2], (int)v[3], 0, 0, 0, 0};
}

// GATE_SILU=1: B has two streams (gate/up at N-offset 0 and n_cols), output
// n_cols wide with silu(g)*u. GATE_SILU=0: plain B, plain store.
// Waves arranged WROWS(M) x WCOLS(N); wave tile = (BM/WROWS) x (BN/WCOLS).
template <int GATE_SILU, int BM, int BN, int WROWS, int WCOLS>
__global__ __launch_bounds__(WROWS* WCOLS * 64) void grouped_gemm_mxfp4_kernel(
    u16* __restrict__ out,              // [rows_max, n_cols] bf16
    const u8* __restrict__ a,           // GATHER: [T, Kp]; else [rows_max, Kp]
    const float* __restrict__ a_scale,  // [T] / [rows_max]
    const u8* __restrict__ w,           // [E, N, Kp/2] (N = n_cols or 2*n_cols)
    const u8* __restrict__ w_scale,     // [E, N, Kp/32] e8m0
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

  __shared__ __attribute__((aligned(16))) u8 smem[2][BM * 128 + NB * BN * 64];
  const int b_off = BM * 128;
  const int b2_off = BM * 128 + BN * 64;

  const long wrow_b = Kp >> 1;   // bytes per weight row
  const long srow_b = Kp >> 5;   // scale bytes per weight row
  const u8* wg = w + ((long)e * NB * n_cols + n0) * wrow_b;
  const u8* aa = GATE_SILU ? a : a + (long)seg0 * Kp;
  const int* rt = row_tok ? row_tok + seg0 : nullptr;

  const int q = lane >> 4;
  // this lane's scale byte per (stream, j): row n0 + wn*WN + j*16 + (l & 15),
  // k-block 4*kt + q
  const u8* sg = w_scale +
      ((long)e * NB * n_cols + n0 + wn * WN + (lane & 15)) * srow_b + q;
  const long su_off = (long)n_cols * srow_b;          // up rows (stage 1)

  f32x4 accg[MF][NF], accu[GATE_SILU ? MF : 1][GATE_SILU ? NF : 1];
#pragma unroll
  for (int i = 0; i < MF; ++i)
#pragma unroll
    for (int j = 0; j < NF; ++j) {
      accg[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (GATE_SILU) accu[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    }

  int scg[NF], scu[GATE_SILU ? NF : 1];
  int sng[NF], snu[GATE_SILU ? NF : 1];

  // prologue
  if (GATE_SILU)
    gx_stage_a<BM, WAVES, true>(smem[0], aa, Kp, rt, m0, rows_valid, wave,
                                lane);
  else
    gx_stage_a<BM, WAVES, false>(smem[0], aa, Kp, nullptr, m0, BM, wave, lane);
  gx_stage_w<BN, NB, WAVES>(smem[0] + b_off, wg, wrow_b, n_cols, wave, lane);
#pragma unroll
  for (int j = 0; j < NF; ++j) {
    scg[j] = (int)sg[(long)j * 16 * srow_b];
    if (GATE_SILU) scu[j] = (int)sg[su_off + (long)j * 16 * srow_b];
  }
  __syncthreads();

  const int KT = (int)(Kp >> 7);
  for (int kt = 0; kt < KT; ++kt) {
    const int p = kt & 1;
    const u8* aT = smem[p];
    const u8* bgT = smem[p] + b_off;
    const u8* buT = smem[p] + b2_off;
    if (kt + 1 < KT) {
      const long ko = (long)(kt + 1) * 128;
      if (GATE_SILU)
        gx_stage_a<BM, WAVES, true>(smem[p ^ 1], aa + ko, Kp, rt, m0,
                                    rows_valid, wave, lane);
      else
        gx_stage_a<BM, WAVES, false>(smem[p ^ 1], aa + ko, Kp, nullptr, m0,
                                     BM, wave, lane);
      gx_stage_w<BN, NB, WAVES>(smem[p ^ 1] + b_off, wg + (ko >> 1), wrow_b,
                                n_cols, wave, lane);
      // next tile's scales, behind the staging: first used after the barrier
      // below, which waits for both
#pragma unroll
      for (int j = 0; j < NF; ++j) {
        sng[j] = (int)sg[(long)j * 16 * srow_b + (kt + 1) * 4];
        if (GATE_SILU)
          snu[j] = (int)sg[su_off + (long)j * 16 * srow_b + (kt + 1) * 4];
      }
    }
    i32x8 bg[NF], bu[GATE_SILU ? NF : 1];
#pragma unroll
    for (int j = 0; j < NF; ++j) {
      bg[j] = gx_frag_w(bgT, wn * WN + j * 16 + (lane & 15), q);
      if (GATE_SILU) bu[j] = gx_frag_w(buT, wn * WN + j * 16 + (lane & 15), q);
    }
#pragma unroll
    for (int i = 0; i < MF; ++i) {
      const i32x8 af = gx_frag_a(aT, wm * WM + i * 16 + (lane & 15), q);
#pragma unroll
      for (int j = 0; j < NF; ++j) {
        accg[i][j] = mfma128x(af, bg[j], accg[i][j], scg[j]);
        if (GATE_SILU) accu[i][j] = mfma128x(af, bu[j], accu[i][j], scu[j]);
      }
    }
    __syncthreads();
    if (kt + 1 < KT) {
#pragma unroll
      for (int j = 0; j < NF; ++j) {
        scg[j] = sng[j];
        if (GATE_SILU) scu[j] = snu[j];
      }
    }
  }

  // epilogue: D[16,16] lane l holds rows (l/16)*4+r, col l%16
  const int drow = (lane >> 4) * 4;
  const int dcol = lane & 15;
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
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int grow = wm * WM + i * 16 + drow + r;
        const long o = (long)(seg0 + m0 + grow) * n_cols + gn;
        float v = accg[i][j][r] * as[r];
        if (GATE_SILU) {
          const float g = v;
          const float u = accu[i][j][r] * as[r];
          v = g / (1.0f + __expf(-g)) * u;
        }
        out[o] = f2bf(v);
      }
    }
  }
}

extern "C" void sutro_grouped_gemm_mxfp4(
    void* out, const void* a, const float* a_scale, const void* w,
    const void* w_scale, const int* row_tok, const int* tile_off,
    const int* counts, int n_experts, int max_tiles, int n_cols, long Kp,
    int gate_silu, int bm, hipStream_t stream) {
  if (max_tiles == 0) return;
#define GX_LAUNCH(GS, BM, BN, WR, WC)                                         \
  {                                                                           \
    dim3 grid((unsigned)max_tiles, (unsigned)(n_cols / BN)),                  \
        block(WR* WC * 64);                                                   \
    hipLaunchKernelGGL((grouped_gemm_mxfp4_kernel<GS, BM, BN, WR, WC>), grid, \
                       block, 0, stream, (u16*)out, (const u8*)a, a_scale,    \
                       (const u8*)w, (const u8*)w_scale, row_tok, tile_off,   \
                       counts, n_experts, n_cols, Kp);                        \
    return;                                                                   \
  }
  /* no hipGetLastError in this launcher: error-state queries are rejected
     while a stream is capturing (decode steps replay under hipGraphs) */
  if (bm == 128 && n_cols % 128 == 0) {
    if (gate_silu) GX_LAUNCH(1, 128, 128, 2, 4)
    else GX_LAUNCH(0, 128, 128, 2, 4)
  }
  if (bm == 128) {
    if (gate_silu) GX_LAUNCH(1, 128, 64, 4, 2)
    else GX_LAUNCH(0, 128, 64, 4, 2)
  }
  if (gate_silu) GX_LAUNCH(1, 64, 64, 2, 2)
  else GX_LAUNCH(0, 64, 64, 2, 2)
#undef GX_LAUNCH
}
