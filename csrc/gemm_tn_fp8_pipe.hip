// Pipelined FP8 (OCP e4m3, W8A8) TN GEMM for MI355X:
//
//   out[M, N] bf16 = (A_q[M, Kp] . W_q[N, Kp]^T) * a_scale[m] * w_scale[n]
//
// and the dense-MLP variant out[M, I] = silu(g) * u on the merged [2I, Kp]
// gate_up weight (gate rows 0..I-1, up rows I..2I-1, read in place), with
// g / u the scaled gate / up products. A_q and W_q hold e4m3 codes, a_scale
// [M] and w_scale [N] are f32 (the row quantiser of grouped_gemm_fp8.hip
// writes both), Kp is a multiple of 128 with a zero tail.
//
// The schedule is csrc/gemm_tn_pipe.hip's, byte for byte: 256x256 output
// tile, 8 waves as 2(M)x4(N), `global_load_lds` dwordx4 staging of 128-byte
// LDS rows (64 bf16 there, 128 e4m3 here), swizzle mode 2, bijective XCD
// remap, one dynamic LDS array of 128 KiB = 2 K-tile buffers x 4 half-tiles
// of 128 rows x 128 bytes (16 KiB), in staging order
//   0 = B0 (W rows nb0..nb0+127)   1 = A0 (A rows m0..m0+127)
//   2 = B1 (W rows nb1..nb1+127)   3 = A1 (A rows m0+128..m0+255)
// plain: nb0 = n0, nb1 = n0 + 128.  SwiGLU: nb0 = n0 (gate), nb1 = I + n0
// (the matching up rows), n0 a multiple of 128.
//
// The arithmetic is csrc/grouped_gemm_fp8.hip's: one K-tile is ONE
// mfma_scale_f32_16x16x128_f8f6f4 (cbsz = blgp = 0, both hardware block
// scales e8m0 1.0) per 16x16 fragment pair, K-tiles ascending into one
// accumulator per fragment, then acc * a_scale * w_scale in the epilogue. So
// the output is bit-identical to the grouped kernel's with one expert.
// Operand lane map as gq_frag there: lane l supplies row l & 15 and the
// swizzled 16-byte chunks 2q, 2q+1 of the 128-byte row, q = l >> 4.
//
// Wave (wm, wn) owns rows wm*64..+63 of A0 and of A1 and columns wn*32..+31
// of B0 and of B1: four 64x32 C quadrants, one per phase. In the SwiGLU
// variant a lane therefore holds gate (quadrants x0) and up (quadrants x1) of
// the same output element: the epilogue needs no shuffle and no LDS.
//
// Schedule per K-tile t (buffer P = t & 1), one half-tile staged per phase;
// counts are 16-byte ds_reads per wave (a fragment = 2 of them):
//   ph0: ds_read B0(2x2=4) A0(4x2=8) | stage (t+1).A1 | lgkmcnt(8) | C00
//   ph1: ds_read B1(2x2=4)           | stage (t+2).B0 |            | C01
//   ph2: ds_read A1(4x2=8)           | stage (t+2).A0 |            | C10
//   ph3:                             | stage (t+2).B1 | vmcnt(6)   | C11
// each phase: reads+stage, s_barrier, lgkmcnt(0), 8 MFMA (4 m x 2 n
// fragments, K = 128 each: the matrix-core time of the bf16 kernel's 16
// MFMAs of K = 32), s_barrier. Waves 4..7 (wm == 1, the SIMD partners of
// 0..3) run one barrier behind, so one partner's MFMA cluster overlaps the
// other's LDS reads.
//
// Ordering. The new fragment read issues the same number of ds_reads in the
// same slot order as the bf16 kernel (B before A in ph0), and a half-tile is
// still 2 staging loads per wave, so the counted waits hold unchanged:
//  RAW  ph3's vmcnt(6) leaves only (t+2).{B0,A0,B1} = 3 half-tiles x 2 loads
//       in flight, so tile t+1 has landed; it sits before ph3's first
//       barrier and tile t+1 is first read in the next phase.
//  WAR  a slot is restaged >= 2 phases after its last ds_read (A0: read ph0,
//       restaged ph2; B1: ph1 -> ph3; A1: ph2 -> next ph0), except B0 (read
//       ph0, restaged ph1), whose 4 reads are issued first (LDS reads retire
//       in order) and are retired by the lgkmcnt(8) — 12 issued, at most the
//       8 A0 reads outstanding — before ph0's first barrier.
// The tail keeps the counts uniform: tiles past the end are staged from the
// last K-tile into slots whose reads are over (never read again).
#include "common.h"

typedef int i32x8 __attribute__((ext_vector_type(8)));

namespace {

// e8m0 1.0 in every byte: the hardware block scale is a no-op
constexpr int SCALE_ONE = 0x7f7f7f7f;

__device__ __forceinline__ f32x4 mfma128(i32x8 a, i32x8 b, f32x4 c) {
  return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(
      a, b, c, 0, 0, 0, SCALE_ONE, 0, SCALE_ONE);
}

// direct HBM->LDS 16-byte copy; lds is the wave-uniform base, lane l lands at
// lds + l*16
__device__ __forceinline__ void glds16(const char* g, char* lds) {
  __builtin_amdgcn_global_load_lds(
      (const __attribute__((address_space(1))) u32*)g,
      (__attribute__((address_space(3))) u32*)lds, 16, 0, 0);
}

// swizzle mode 2 of gemm_tn.hip: row bits 1..3 XOR'd into the 16B chunk idx
__device__ __forceinline__ u32 swz(u32 byte) {
  return byte ^ (((byte >> 8) & 7u) << 4);
}

constexpr int HT = 16384;       // half-tile bytes
constexpr int KTILE_B = 65536;  // one K-tile buffer: 4 half-tiles
constexpr int SLOT_B0 = 0, SLOT_A0 = 1, SLOT_B1 = 2, SLOT_A1 = 3;

// this thread's two staging sources of one half-tile (k = 0), rows clamped
struct Src {
  const char* p[2];
};

__device__ __forceinline__ Src make_src(const u8* base, long row0,
                                        long rows_valid, long Kb, int wave,
                                        int lane) {
  Src s;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const u32 b = (u32)(wave * 2 + j) * 1024u + (u32)lane * 16u;
    const u32 lb = swz(b);  // pre-swizzled source, lane-linear LDS
    long row = (long)(lb >> 7);
    row = row < rows_valid ? row : rows_valid - 1;  // edge: dup rows
    s.p[j] = (const char*)base + (row0 + row) * Kb + (lb & 127u);
  }
  return s;
}

__device__ __forceinline__ void stage_half(char* slot_wave, const Src& s,
                                           long koff) {
  glds16(s.p[0] + koff, slot_wave);
  glds16(s.p[1] + koff, slot_wave + 1024);
}

// 32 operand bytes of one lane: two 16-byte ds_reads at the pre-swizzled
// offsets of chunks 2q and 2q+1
__device__ __forceinline__ i32x8 lds_frag(const char* smem, u32 off_lo,
                                          u32 off_hi) {
  const u32x4 lo = *(const u32x4*)(smem + off_lo);
  const u32x4 hi = *(const u32x4*)(smem + off_hi);
  return i32x8{(int)lo[0], (int)lo[1], (int)lo[2], (int)lo[3],
               (int)hi[0], (int)hi[1], (int)hi[2], (int)hi[3]};
}

}  // namespace

// EPI: 0 = plain store, 1 = residual add, 2 = SwiGLU (out is [M, N/2])
template <int EPI>
__global__ __launch_bounds__(512) void gemm_tn_fp8_pipe_kernel(
    u16* __restrict__ out, const u8* __restrict__ a,
    const float* __restrict__ a_scale, const u8* __restrict__ w,
    const float* __restrict__ w_scale, const u16* __restrict__ res, int M,
    int N, long Kp, int xcd_swz) {
  extern __shared__ __attribute__((aligned(1024))) char smem[];

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wm = wave >> 2;
  const int wn = wave & 3;

  int bid = blockIdx.x;
  if (xcd_swz) {
    const int nwg = gridDim.x;
    const int q = nwg >> 3, r = nwg & 7;
    const int xcd = bid & 7, seq = bid >> 3;
    bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + seq;
  }
  const int MT = (M + 255) >> 8;
  const int m0 = (bid % MT) * 256;
  // SwiGLU: N = 2I, a block covers 128 gate + the 128 matching up rows
  const int I = N >> 1;
  const int nt = bid / MT;
  const int nb0 = (EPI == 2) ? nt * 128 : nt * 256;
  const int nb1 = (EPI == 2) ? I + nt * 128 : nt * 256 + 128;
  const int nlim = (EPI == 2) ? I : N;  // rows of w valid for B0's range

  // rows valid per half-tile (>= 1 wherever the half is ever stored from; a
  // half that lies wholly past the edge is staged from its last valid row)
  const long a0v = min(128, M - m0);
  const long a1v = max(1, min(128, M - m0 - 128));
  const long b0v = min(128, nlim - nb0);
  const long b1v = (EPI == 2) ? 128 : max(1, min(128, N - nb1));
  const long a1r = (M - m0 - 128 >= 1) ? m0 + 128 : m0 + a0v - 1;
  const long b1r = (EPI == 2 || N - nb1 >= 1) ? nb1 : nb0 + b0v - 1;
  const Src sB0 = make_src(w, nb0, b0v, Kp, wave, lane);
  const Src sA0 = make_src(a, m0, a0v, Kp, wave, lane);
  const Src sB1 = make_src(w, b1r, b1v, Kp, wave, lane);
  const Src sA1 = make_src(a, a1r, a1v, Kp, wave, lane);

  char* const sw = smem + wave * 2048;  // this wave's 2 KiB of every slot

  // fragment read offsets inside a half-tile: row = w?*.. + f*16 + lane%16
  // (f*16 rows = f*2048 bytes, above the swizzled bits), chunks 2q and 2q+1
  u32 aoff[2], boff[2];
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    const u32 kc = (u32)((lane >> 4) * 2 + c) * 16u;
    aoff[c] = swz((u32)(wm * 64 + (lane & 15)) * 128u + kc);
    boff[c] = swz((u32)(wn * 32 + (lane & 15)) * 128u + kc);
  }

  f32x4 acc[2][2][4][2];  // [A half][B half][m frag][n frag]
#pragma unroll
  for (int x = 0; x < 2; ++x)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[x][b][i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int KT = (int)(Kp >> 7);
  const int klast = KT - 1;

  // prologue: tile 0 whole, tile 1's first three half-tiles; 14 loads, the
  // wait leaves the last 6 (tile 1) in flight
  {
    const long k1 = (long)min(1, klast) * 128;
    stage_half(sw + SLOT_B0 * HT, sB0, 0);
    stage_half(sw + SLOT_A0 * HT, sA0, 0);
    stage_half(sw + SLOT_B1 * HT, sB1, 0);
    stage_half(sw + SLOT_A1 * HT, sA1, 0);
    stage_half(sw + KTILE_B + SLOT_B0 * HT, sB0, k1);
    stage_half(sw + KTILE_B + SLOT_A0 * HT, sA0, k1);
    stage_half(sw + KTILE_B + SLOT_B1 * HT, sB1, k1);
    asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    if (wm == 1) __builtin_amdgcn_s_barrier();  // stagger waves 4..7
  }

  i32x8 fa[4], fb0[2], fb1[2];

#define PHASE_SYNC_MFMA(A_, B_, FB_)                                     \
  __builtin_amdgcn_sched_barrier(0);                                     \
  __builtin_amdgcn_s_barrier();                                          \
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                     \
  __builtin_amdgcn_sched_barrier(0);                                     \
  __builtin_amdgcn_s_setprio(1);                                         \
  _Pragma("unroll") for (int i = 0; i < 4; ++i)                          \
  _Pragma("unroll") for (int j = 0; j < 2; ++j)                          \
      acc[A_][B_][i][j] = mfma128(fa[i], FB_[j], acc[A_][B_][i][j]);     \
  __builtin_amdgcn_s_setprio(0);                                         \
  __builtin_amdgcn_sched_barrier(0);                                     \
  __builtin_amdgcn_s_barrier();                                          \
  __builtin_amdgcn_sched_barrier(0);

  // one K-tile out of buffer P; kn1/kn2 = byte offsets of tiles t+1, t+2
#define KTILE(P)                                                         \
  {                                                                      \
    const char* cur = smem + (P) * KTILE_B;                              \
    char* nxt = sw + ((P) ^ 1) * KTILE_B;                                \
    char* own = sw + (P) * KTILE_B;                                      \
    /* ph0 */                                                            \
    _Pragma("unroll") for (int j = 0; j < 2; ++j)                        \
        fb0[j] = lds_frag(cur + SLOT_B0 * HT + j * 2048, boff[0],        \
                          boff[1]);                                      \
    __builtin_amdgcn_sched_barrier(0);                                   \
    _Pragma("unroll") for (int i = 0; i < 4; ++i)                        \
        fa[i] = lds_frag(cur + SLOT_A0 * HT + i * 2048, aoff[0],         \
                         aoff[1]);                                       \
    __builtin_amdgcn_sched_barrier(0);                                   \
    stage_half(nxt + SLOT_A1 * HT, sA1, kn1);                            \
    __builtin_amdgcn_sched_barrier(0);                                   \
    asm volatile("s_waitcnt lgkmcnt(8)" ::: "memory");                   \
    PHASE_SYNC_MFMA(0, 0, fb0)                                           \
    /* ph1 */                                                            \
    _Pragma("unroll") for (int j = 0; j < 2; ++j)                        \
        fb1[j] = lds_frag(cur + SLOT_B1 * HT + j * 2048, boff[0],        \
                          boff[1]);                                      \
    __builtin_amdgcn_sched_barrier(0);                                   \
    stage_half(own + SLOT_B0 * HT, sB0, kn2);                            \
    PHASE_SYNC_MFMA(0, 1, fb1)                                           \
    /* ph2 */                                                            \
    _Pragma("unroll") for (int i = 0; i < 4; ++i)                        \
        fa[i] = lds_frag(cur + SLOT_A1 * HT + i * 2048, aoff[0],         \
                         aoff[1]);                                       \
    __builtin_amdgcn_sched_barrier(0);                                   \
    stage_half(own + SLOT_A0 * HT, sA0, kn2);                            \
    PHASE_SYNC_MFMA(1, 0, fb0)                                           \
    /* ph3 */                                                            \
    stage_half(own + SLOT_B1 * HT, sB1, kn2);                            \
    __builtin_amdgcn_sched_barrier(0);                                   \
    asm volatile("s_waitcnt vmcnt(6)" ::: "memory");                     \
    PHASE_SYNC_MFMA(1, 1, fb1)                                           \
  }

  for (int t = 0; t < KT; t += 2) {
    {
      const long kn1 = (long)min(t + 1, klast) * 128;
      const long kn2 = (long)min(t + 2, klast) * 128;
      KTILE(0)
    }
    if (t + 1 < KT) {
      const long kn1 = (long)min(t + 2, klast) * 128;
      const long kn2 = (long)min(t + 3, klast) * 128;
      KTILE(1)
    }
  }
#undef KTILE
#undef PHASE_SYNC_MFMA

  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  if (wm == 0) __builtin_amdgcn_s_barrier();  // balances the stagger

  // epilogue: D[16,16] lane l holds rows (l/16)*4+r, col l%16. The real
  // scales go on here, in the grouped kernel's order: acc * a_scale * w_scale
  const int drow = (lane >> 4) * 4;
  const int dcol = lane & 15;
#pragma unroll
  for (int x = 0; x < 2; ++x)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int gm = m0 + x * 128 + wm * 64 + i * 16 + drow;
      float as[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) as[r] = gm + r < M ? a_scale[gm + r] : 0.f;
      if (EPI == 2) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const int gn = nb0 + wn * 32 + j * 16 + dcol;  // < I (I % 128 == 0)
          const float wsg = w_scale[gn];
          const float wsu = w_scale[I + gn];
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            if (gm + r >= M) continue;
            // f32 SwiGLU on the scaled values, one rounding
            const float g = acc[x][0][i][j][r] * as[r] * wsg;
            const float u = acc[x][1][i][j][r] * as[r] * wsu;
            out[(long)(gm + r) * I + gn] = f2bf(g / (1.0f + __expf(-g)) * u);
          }
        }
      } else {
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
          for (int j = 0; j < 2; ++j) {
            const int gn = nb0 + b * 128 + wn * 32 + j * 16 + dcol;
            if (gn >= N) continue;
            const float ws = w_scale[gn];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              if (gm + r >= M) continue;
              const long o = (long)(gm + r) * N + gn;
              float v = acc[x][b][i][j][r] * as[r] * ws;
              // a separate f32 add (no contraction into the scale multiply),
              // then the one rounding to bf16
              if (EPI == 1) v = __fadd_rn(v, bf2f(res[o]));
              out[o] = f2bf(v);
            }
          }
      }
    }
}

// epi: 0 plain, 1 residual (res != nullptr), 2 SwiGLU (N = 2I rows of w,
// out [M, I], I % 128 == 0). 1 <= M <= 2^31 - 256 (the row-tile count is
// taken in int), N % 64 == 0 (epi 0/1; the binding enforces it and the tests
// cover nothing else, though columns are guarded one by one), Kp % 128 == 0.
// No hipGetLastError and no sync: it runs under hipGraph capture.
// Returns 0, or the hipError_t of the LDS-size attribute call.
extern "C" int sutro_gemm_tn_fp8_pipe_launch(
    void* out, const void* a, const float* a_scale, const void* w,
    const float* w_scale, const void* res, int M, int N, long Kp, int epi,
    int xcd_swz, hipStream_t stream) {
  constexpr int LDS_BYTES = 2 * KTILE_B;
  const int mt = (M + 255) / 256;
  const int ntl = (epi == 2) ? (N / 2) / 128 : (N + 255) / 256;
  dim3 grid(mt * ntl), block(512);
  // dynamic LDS above 64 KiB needs the attribute, which is per device and
  // per instantiation: set once each (setting it twice in a race is harmless)
  constexpr int MAX_DEV = 64;
  static bool attr_set[3][MAX_DEV];
  int dev = 0;
  const int ed = (int)hipGetDevice(&dev);
  if (ed != 0) return ed;
#define LAUNCH(EPI)                                                          \
  if (epi == EPI) {                                                          \
    if (dev < 0 || dev >= MAX_DEV || !attr_set[EPI][dev]) {                  \
      const int e = (int)hipFuncSetAttribute(                                \
          (const void*)gemm_tn_fp8_pipe_kernel<EPI>,                         \
          hipFuncAttributeMaxDynamicSharedMemorySize, LDS_BYTES);            \
      if (e != 0) return e;                                                  \
      if (dev >= 0 && dev < MAX_DEV) attr_set[EPI][dev] = true;              \
    }                                                                        \
    gemm_tn_fp8_pipe_kernel<EPI><<<grid, block, LDS_BYTES, stream>>>(        \
        (u16*)out, (const u8*)a, a_scale, (const u8*)w, w_scale,             \
        (const u16*)res, M, N, Kp, xcd_swz);                                 \
    return 0;                                                                \
  }
  LAUNCH(0)
  LAUNCH(1)
  LAUNCH(2)
#undef LAUNCH
  return -1;
}
