// Pipelined bf16 TN GEMM for MI355X: out[M,N] = x[M,K] @ W[N,K]^T, and the
// dense-MLP variant out[M,I] = silu(x @ Wg^T) * (x @ Wu^T) on the merged
// [2I, K] gate_up weight (gate rows 0..I-1, up rows I..2I-1, read in place).
//
// Same tile as csrc/gemm_tn.hip (256x256x64, 8 waves as 2(M)x4(N),
// `global_load_lds` dwordx4 staging, the three LDS swizzle modes, bijective
// XCD remap, mfma_f32_16x16x32_bf16 with K ascending in steps of 32 — so the
// plain output is bit-identical to gemm_tn_kernel's), but the K loop is the
// CDNA4 guide's 8-phase schedule: the staging loads stay in flight across
// raw s_barriers behind a counted vmcnt that is never 0 inside the loop.
//
// LDS: one dynamic array of 128 KiB = 2 K-tile buffers x 4 half-tiles of
// 128 rows x 64 k (16 KiB). Half-tile slots in staging order:
//   0 = B0 (W rows nb0..nb0+127)   1 = A0 (x rows m0..m0+127)
//   2 = B1 (W rows nb1..nb1+127)   3 = A1 (x rows m0+128..m0+255)
// plain: nb0 = n0, nb1 = n0 + 128.  SwiGLU: nb0 = n0 (gate), nb1 = I + n0
// (the matching up rows), n0 a multiple of 128.
//
// Wave (wm, wn) owns rows wm*64..+63 of A0 and of A1 and columns wn*32..+31
// of B0 and of B1: four 64x32 C quadrants, one per phase. In the SwiGLU
// variant a lane therefore holds gate (quadrants x0) and up (quadrants x1) of
// the same output element: the epilogue needs no shuffle and no LDS.
//
// Schedule per K-tile t (buffer P = t & 1), one half-tile staged per phase:
//   ph0: ds_read B0(4) A0(8) | stage (t+1).A1 | lgkmcnt(8) | C00 += A0 B0
//   ph1: ds_read B1(4)       | stage (t+2).B0 |            | C01 += A0 B1
//   ph2: ds_read A1(8)       | stage (t+2).A0 |            | C10 += A1 B0
//   ph3:                     | stage (t+2).B1 | vmcnt(6)   | C11 += A1 B1
// each phase: reads+stage, s_barrier, lgkmcnt(0), 16 MFMA, s_barrier. Waves
// 4..7 (wm == 1, the SIMD partners of 0..3) run one barrier behind, so one
// partner's MFMA cluster overlaps the other's LDS reads.
//
// Ordering (the guide's rules, with the one-barrier stagger counted in):
//  RAW  ph3's vmcnt(6) leaves only (t+2).{B0,A0,B1} = 3 half-tiles x 2 loads
//       in flight, so tile t+1 has landed; it sits before ph3's first
//       barrier and tile t+1 is first read in the next phase.
//  WAR  a slot is restaged >= 2 phases after its last ds_read (A0: read ph0,
//       restaged ph2; B1: ph1 -> ph3; A1: ph2 -> next ph0), except B0 (read
//       ph0, restaged ph1), whose 4 reads are issued first and retired by
//       the lgkmcnt(8) before ph0's first barrier.
// The tail keeps the counts uniform: tiles past the end are staged from the
// last K-tile into slots whose reads are over (never read again).
#include "common.h"

typedef s16x8 bf16x8;

namespace {

__device__ __forceinline__ f32x4 mfma16(bf16x8 a, bf16x8 b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}

// direct HBM->LDS 16-byte copy; lds is the wave-uniform base, lane l lands at
// lds + l*16
__device__ __forceinline__ void glds16(const char* g, char* lds) {
  __builtin_amdgcn_global_load_lds(
      (const __attribute__((address_space(1))) u32*)g,
      (__attribute__((address_space(3))) u32*)lds, 16, 0, 0);
}

// same involutions as gemm_tn.hip (bits >= 12 fixed, so they act inside a
// 16 KiB half-tile exactly as inside a whole tile)
template <int SWZ>
__device__ __forceinline__ u32 swz(u32 byte) {
  if (SWZ == 1) return byte ^ (((byte >> 9) & 1u) << 5);
  if (SWZ == 2) return byte ^ (((byte >> 8) & 7u) << 4);
  return byte;
}

constexpr int HT = 16384;       // half-tile bytes
constexpr int KTILE_B = 65536;  // one K-tile buffer: 4 half-tiles
constexpr int SLOT_B0 = 0, SLOT_A0 = 1, SLOT_B1 = 2, SLOT_A1 = 3;

// this thread's two staging sources of one half-tile (k = 0), rows clamped
struct Src {
  const char* p[2];
};

template <int SWZ>
__device__ __forceinline__ Src make_src(const u16* base, long row0,
                                        long rows_valid, long Kb, int wave,
                                        int lane) {
  Src s;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const u32 b = (u32)(wave * 2 + j) * 1024u + (u32)lane * 16u;
    const u32 lb = swz<SWZ>(b);  // pre-swizzled source, lane-linear LDS
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

__device__ __forceinline__ bf16x8 lds_frag(const char* smem, u32 off) {
  return *(const bf16x8*)(smem + off);
}

}  // namespace

// EPI: 0 = plain store, 1 = residual add, 2 = SwiGLU (out is [M, N/2])
template <int EPI, int SWZ>
__global__ __launch_bounds__(512) void gemm_tn_pipe_kernel(
    u16* __restrict__ out, const u16* __restrict__ x,
    const u16* __restrict__ w, const u16* __restrict__ res, int M, int N,
    long K, int xcd_swz) {
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

  const long Kb = K * 2;
  // rows valid per half-tile (>= 1 wherever the half is ever stored from; a
  // half that lies wholly past the edge is staged from its last valid row)
  const long a0v = min(128, M - m0);
  const long a1v = max(1, min(128, M - m0 - 128));
  const long b0v = min(128, nlim - nb0);
  const long b1v = (EPI == 2) ? 128 : max(1, min(128, N - nb1));
  const long a1r = (M - m0 - 128 >= 1) ? m0 + 128 : m0 + a0v - 1;
  const long b1r = (EPI == 2 || N - nb1 >= 1) ? nb1 : nb0 + b0v - 1;
  const Src sB0 = make_src<SWZ>(w, nb0, b0v, Kb, wave, lane);
  const Src sA0 = make_src<SWZ>(x, m0, a0v, Kb, wave, lane);
  const Src sB1 = make_src<SWZ>(w, b1r, b1v, Kb, wave, lane);
  const Src sA1 = make_src<SWZ>(x, a1r, a1v, Kb, wave, lane);

  char* const sw = smem + wave * 2048;  // this wave's 2 KiB of every slot

  // fragment read offsets inside a half-tile: row = w?*.. + f*16 + lane%16,
  // k chunk = kk*4 + lane/16
  u32 aoff[2], boff[2];
#pragma unroll
  for (int kk = 0; kk < 2; ++kk) {
    const u32 kc = (u32)(kk * 4 + (lane >> 4)) * 16u;
    aoff[kk] = swz<SWZ>((u32)(wm * 64 + (lane & 15)) * 128u + kc);
    boff[kk] = swz<SWZ>((u32)(wn * 32 + (lane & 15)) * 128u + kc);
  }

  f32x4 acc[2][2][4][2];  // [A half][B half][m frag][n frag]
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[a][b][i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int KT = (int)(K >> 6);
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

  bf16x8 fa[4][2], fb0[2][2], fb1[2][2];

#define PHASE_SYNC_MFMA(A_, B_, FB_)                                     \
  __builtin_amdgcn_sched_barrier(0);                                     \
  __builtin_amdgcn_s_barrier();                                          \
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                     \
  __builtin_amdgcn_sched_barrier(0);                                     \
  __builtin_amdgcn_s_setprio(1);                                         \
  _Pragma("unroll") for (int kk = 0; kk < 2; ++kk)                       \
  _Pragma("unroll") for (int i = 0; i < 4; ++i)                          \
  _Pragma("unroll") for (int j = 0; j < 2; ++j)                          \
      acc[A_][B_][i][j] = mfma16(fa[i][kk], FB_[j][kk], acc[A_][B_][i][j]); \
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
    _Pragma("unroll") for (int kk = 0; kk < 2; ++kk)                     \
        fb0[j][kk] = lds_frag(cur + SLOT_B0 * HT + j * 2048, boff[kk]);  \
    __builtin_amdgcn_sched_barrier(0);                                   \
    _Pragma("unroll") for (int i = 0; i < 4; ++i)                        \
    _Pragma("unroll") for (int kk = 0; kk < 2; ++kk)                     \
        fa[i][kk] = lds_frag(cur + SLOT_A0 * HT + i * 2048, aoff[kk]);   \
    __builtin_amdgcn_sched_barrier(0);                                   \
    stage_half(nxt + SLOT_A1 * HT, sA1, kn1);                            \
    __builtin_amdgcn_sched_barrier(0);                                   \
    asm volatile("s_waitcnt lgkmcnt(8)" ::: "memory");                   \
    PHASE_SYNC_MFMA(0, 0, fb0)                                           \
    /* ph1 */                                                            \
    _Pragma("unroll") for (int j = 0; j < 2; ++j)                        \
    _Pragma("unroll") for (int kk = 0; kk < 2; ++kk)                     \
        fb1[j][kk] = lds_frag(cur + SLOT_B1 * HT + j * 2048, boff[kk]);  \
    __builtin_amdgcn_sched_barrier(0);                                   \
    stage_half(own + SLOT_B0 * HT, sB0, kn2);                            \
    PHASE_SYNC_MFMA(0, 1, fb1)                                           \
    /* ph2 */                                                            \
    _Pragma("unroll") for (int i = 0; i < 4; ++i)                        \
    _Pragma("unroll") for (int kk = 0; kk < 2; ++kk)                     \
        fa[i][kk] = lds_frag(cur + SLOT_A1 * HT + i * 2048, aoff[kk]);   \
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

  // epilogue: D[16,16] lane l holds rows (l/16)*4+r, col l%16
  const int drow = (lane >> 4) * 4;
  const int dcol = lane & 15;
  if (EPI == 2) {
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const int gn = nb0 + wn * 32 + j * 16 + dcol;  // < I (I % 128 == 0)
          const int gm = m0 + a * 128 + wm * 64 + i * 16 + drow;
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            if (gm + r >= M) continue;
            // both halves rounded to bf16 first: the unfused pipeline's
            // arithmetic (GEMM output in bf16, then silu_mul_kernel)
            const float gf = bf2f(f2bf(acc[a][0][i][j][r]));
            const float uf = bf2f(f2bf(acc[a][1][i][j][r]));
            const float s = gf / (1.f + __expf(-gf));
            out[(long)(gm + r) * I + gn] = f2bf(s * uf);
          }
        }
  } else {
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j) {
            const int gn = nb0 + b * 128 + wn * 32 + j * 16 + dcol;
            if (gn >= N) continue;
            const int gm = m0 + a * 128 + wm * 64 + i * 16 + drow;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              if (gm + r >= M) continue;
              const long o = (long)(gm + r) * N + gn;
              float v = acc[a][b][i][j][r];
              if (EPI == 1) v += bf2f(res[o]);
              out[o] = f2bf(v);
            }
          }
  }
}

// epi: 0 plain, 1 residual (res != nullptr), 2 SwiGLU (N = 2I rows of w,
// out [M, I], I % 128 == 0). Any M >= 1, any N >= 1 (epi 0/1), K % 64 == 0.
// Returns 0, or the hipError_t of the LDS-size attribute call.
extern "C" int sutro_gemm_tn_pipe_launch(void* out, const void* x,
                                         const void* w, const void* res,
                                         int M, int N, long K, int epi,
                                         int swz_mode, int xcd_swz,
                                         hipStream_t stream) {
  constexpr int LDS_BYTES = 2 * KTILE_B;
  const int mt = (M + 255) / 256;
  const int ntl = (epi == 2) ? (N / 2) / 128 : (N + 255) / 256;
  dim3 grid(mt * ntl), block(512);
  // dynamic LDS above 64 KiB needs the attribute, which is per device and
  // per instantiation: set once each (setting it twice in a race is harmless)
  constexpr int MAX_DEV = 64;
  static bool attr_set[3][3][MAX_DEV];
  int dev = 0;
  const int ed = (int)hipGetDevice(&dev);
  if (ed != 0) return ed;
#define LAUNCH_1(EPI, SWZ)                                                   \
  if (epi == EPI && swz_mode == SWZ) {                                       \
    if (dev < 0 || dev >= MAX_DEV || !attr_set[EPI][SWZ][dev]) {             \
      const int e = (int)hipFuncSetAttribute(                                \
          (const void*)gemm_tn_pipe_kernel<EPI, SWZ>,                        \
          hipFuncAttributeMaxDynamicSharedMemorySize, LDS_BYTES);            \
      if (e != 0) return e;                                                  \
      if (dev >= 0 && dev < MAX_DEV) attr_set[EPI][SWZ][dev] = true;         \
    }                                                                        \
    gemm_tn_pipe_kernel<EPI, SWZ><<<grid, block, LDS_BYTES, stream>>>(       \
        (u16*)out, (const u16*)x, (const u16*)w, (const u16*)res, M, N, K,   \
        xcd_swz);                                                            \
    return 0;                                                                \
  }
#define LAUNCH(EPI) LAUNCH_1(EPI, 0) LAUNCH_1(EPI, 1) LAUNCH_1(EPI, 2)
  LAUNCH(0)
  LAUNCH(1)
  LAUNCH(2)
#undef LAUNCH
#undef LAUNCH_1
  return -1;
}
