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
//
// gemm_swiglu_persist_kernel (further down) runs the same loop over a list of
// tiles per block and fills those tail slots with the next tile instead; the
// RAW / WAR notes for that seam, and why the epilogue's stores cannot loosen
// a later vmcnt(6), stand at its definition. The tile orders (tile_mn,
// tile_mn_banded) are shared by both kernels and change no result.
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

// Tile number -> (M-tile, N-tile). Tiles are numbered in groups of group_m
// M-tiles: inside a group m runs fastest, then n; the last group takes the
// remainder. group_m <= 0 or >= MT is the plain order (m fastest over all MT).
__device__ __forceinline__ void tile_mn(int tile, int MT, int NT, int group_m,
                                        int& mt, int& nt) {
  if (group_m <= 0 || group_m >= MT) {
    mt = tile % MT;
    nt = tile / MT;
    return;
  }
  const int per = group_m * NT;
  const int g = tile / per;
  const int first = g * group_m;
  const int gsz = min(group_m, MT - first);
  const int local = tile - g * per;
  mt = first + local % gsz;
  nt = local / gsz;
}

// The banded order (group_m < 0, XCD remap on): label xl of nx (the XCD a
// block lands on) owns a band of a = MT / nx whole rows of M-tiles,
// [a*xl, a*xl + a), and walks it by tile_mn in groups of -group_m; its i-th
// tile is therefore at the same N-tile on every label, so the labels sweep W
// together and one fetch of a W panel from memory serves all of them. The
// MT % nx leftover rows come last, m fastest, split evenly over the labels.
// A label's tile count is that of the bijective split, whatever the order.
__device__ __forceinline__ void tile_mn_banded(int xl, int i, int nx, int MT,
                                               int NT, int group_m, int& mt,
                                               int& nt) {
  const int a = MT / nx, b = MT - a * nx;
  const int whole = a * NT;
  if (i < whole) {
    tile_mn(i, a, NT, -group_m, mt, nt);
    mt += a * xl;
    return;
  }
  const int left = b * NT;
  const int q = left / nx, r = left % nx;
  const int idx =
      (xl < r ? xl * (q + 1) : r * (q + 1) + (xl - r) * q) + (i - whole);
  mt = nx * a + idx % b;
  nt = idx / b;
}

// The persistent kernel's form of a staging source: a wave-uniform base (row
// and k offset folded in, kept in scalar registers) plus this thread's two
// 32-bit byte offsets inside the half-tile's 128 source rows. The offsets of
// an unclamped half are the same for every tile, so a tile change costs only
// scalar work and the two clamped A offsets pairs.
struct USrc {
  const char* base;
  u32 o0, o1;
};

template <int SWZ>
__device__ __forceinline__ void lane_offsets(u32& o0, u32& o1, int rows_valid,
                                             u32 Kb, int wave, int lane) {
  u32 o[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const u32 b = (u32)(wave * 2 + j) * 1024u + (u32)lane * 16u;
    const u32 lb = swz<SWZ>(b);  // pre-swizzled source, lane-linear LDS
    const u32 row = min(lb >> 7, (u32)(rows_valid - 1));  // edge: dup rows
    o[j] = row * Kb + (lb & 127u);
  }
  o0 = o[0];
  o1 = o[1];
}

__device__ __forceinline__ void stage_half(char* slot_wave, const USrc& s,
                                           long koff) {
  glds16(s.base + koff + s.o0, slot_wave);
  glds16(s.base + koff + s.o1, slot_wave + 1024);
}

// one SwiGLU tile's sources (m0 = 256 * M-tile, nb0 = 128 * N-tile;
// I % 128 == 0, so both B halves are whole and share the unclamped offsets)
struct TileSrc {
  const char *b0, *a0, *b1, *a1;  // wave-uniform row bases
  u32 a0o0, a0o1, a1o0, a1o1;     // A offsets, clamped at the M edge
};

template <int SWZ>
__device__ __forceinline__ TileSrc swiglu_tile_src(const u16* x, const u16* w,
                                                   int M, int I, u32 Kb,
                                                   int m0, int nb0, int wave,
                                                   int lane) {
  const int a0v = min(128, M - m0);
  const int a1v = max(1, min(128, M - m0 - 128));
  const long a1r = (M - m0 - 128 >= 1) ? m0 + 128 : m0 + a0v - 1;
  TileSrc t;
  t.b0 = (const char*)w + (long)nb0 * Kb;
  t.a0 = (const char*)x + (long)m0 * Kb;
  t.b1 = (const char*)w + ((long)I + nb0) * Kb;
  t.a1 = (const char*)x + a1r * Kb;
  lane_offsets<SWZ>(t.a0o0, t.a0o1, a0v, Kb, wave, lane);
  lane_offsets<SWZ>(t.a1o0, t.a1o1, a1v, Kb, wave, lane);
  return t;
}

}  // namespace

// One phase's barrier / wait / 16 MFMA / barrier, and one K-tile out of buffer
// P (the schedule in the header). KTILE_G names every staging source: SA1 at
// byte offset KA1 goes to the other buffer's A1 slot in ph0, SB0 / SA0 / SB1
// at K2 go to buffer P's own slots in ph1..ph3. Both expect smem, sw, acc,
// fa, fb0, fb1, aoff and boff in scope.
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

#define KTILE_G(P, SA1, KA1, SB0, SA0, SB1, K2)                          \
  {                                                                      \
    const char* kt_cur = smem + (P) * KTILE_B;                           \
    char* kt_nxt = sw + ((P) ^ 1) * KTILE_B;                             \
    char* kt_own = sw + (P) * KTILE_B;                                   \
    /* ph0 */                                                            \
    _Pragma("unroll") for (int j = 0; j < 2; ++j)                        \
    _Pragma("unroll") for (int kk = 0; kk < 2; ++kk)                     \
        fb0[j][kk] = lds_frag(kt_cur + SLOT_B0 * HT + j * 2048,       \
                              boff[kk]);                                 \
    __builtin_amdgcn_sched_barrier(0);                                   \
    _Pragma("unroll") for (int i = 0; i < 4; ++i)                        \
    _Pragma("unroll") for (int kk = 0; kk < 2; ++kk)                     \
        fa[i][kk] = lds_frag(kt_cur + SLOT_A0 * HT + i * 2048,        \
                             aoff[kk]);                                  \
    __builtin_amdgcn_sched_barrier(0);                                   \
    stage_half(kt_nxt + SLOT_A1 * HT, SA1, KA1);                         \
    __builtin_amdgcn_sched_barrier(0);                                   \
    asm volatile("s_waitcnt lgkmcnt(8)" ::: "memory");                   \
    PHASE_SYNC_MFMA(0, 0, fb0)                                           \
    /* ph1 */                                                            \
    _Pragma("unroll") for (int j = 0; j < 2; ++j)                        \
    _Pragma("unroll") for (int kk = 0; kk < 2; ++kk)                     \
        fb1[j][kk] = lds_frag(kt_cur + SLOT_B1 * HT + j * 2048,       \
                              boff[kk]);                                 \
    __builtin_amdgcn_sched_barrier(0);                                   \
    stage_half(kt_own + SLOT_B0 * HT, SB0, K2);                          \
    PHASE_SYNC_MFMA(0, 1, fb1)                                           \
    /* ph2 */                                                            \
    _Pragma("unroll") for (int i = 0; i < 4; ++i)                        \
    _Pragma("unroll") for (int kk = 0; kk < 2; ++kk)                     \
        fa[i][kk] = lds_frag(kt_cur + SLOT_A1 * HT + i * 2048,        \
                             aoff[kk]);                                  \
    __builtin_amdgcn_sched_barrier(0);                                   \
    stage_half(kt_own + SLOT_A0 * HT, SA0, K2);                          \
    PHASE_SYNC_MFMA(1, 0, fb0)                                           \
    /* ph3 */                                                            \
    stage_half(kt_own + SLOT_B1 * HT, SB1, K2);                          \
    __builtin_amdgcn_sched_barrier(0);                                   \
    asm volatile("s_waitcnt vmcnt(6)" ::: "memory");                     \
    PHASE_SYNC_MFMA(1, 1, fb1)                                           \
  }

// EPI: 0 = plain store, 1 = residual add, 2 = SwiGLU (out is [M, N/2])
template <int EPI, int SWZ>
__global__ __launch_bounds__(512) void gemm_tn_pipe_kernel(
    u16* __restrict__ out, const u16* __restrict__ x,
    const u16* __restrict__ w, const u16* __restrict__ res, int M, int N,
    long K, int xcd_swz, int group_m) {
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
  // SwiGLU: N = 2I, a block covers 128 gate + the 128 matching up rows
  const int I = N >> 1;
  int mt, nt;  // group_m = 0: mt = bid % MT, nt = bid / MT
  if (group_m < 0)  // launched with xcd_swz only
    tile_mn_banded(blockIdx.x & 7, blockIdx.x >> 3, 8, MT,
                   (int)gridDim.x / MT, group_m, mt, nt);
  else
    tile_mn(bid, MT, (int)gridDim.x / MT, group_m, mt, nt);
  const int m0 = mt * 256;
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

  // one K-tile out of buffer P; kn1/kn2 = byte offsets of tiles t+1, t+2
#define KTILE(P) KTILE_G(P, sA1, kn1, sB0, sA0, sB1, kn2)

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

// Persistent form of the SwiGLU instantiation: gridDim.x blocks, each walking
// a list of tiles through the same 8-phase loop. K % 128 == 0 (KT even), so
// every tile starts in buffer 0 and the KTILE(0) / KTILE(1) pairing, the
// counts and the barriers are those of gemm_tn_pipe_kernel; every output
// element is the same accumulator summed in the same order, rounded and
// activated by the same expression: results are bit-identical to it.
//
// Tile list. XCD label xl = bid % nx, slot s = bid / nx (nx = 8, or the grid
// if smaller; 1 without xcd_swz). Label xl owns one contiguous, balanced span
// of tile numbers (the bijective split of the one-tile-per-block kernel) and
// its slots walk it together: span0 + slots*r + s. Tile numbers map to
// (m, n) by tile_mn; group_m < 0 is the banded order, where the label's
// slots*r + s -th tile comes from tile_mn_banded instead. A block with no
// tile returns before its first barrier.
//
// Seam. In a tile's last two K-tiles the stage slots that the one-tile kernel
// fills with clamped dummies fetch the NEXT tile: K-tile KT-2 stages
// next.K0.{B0,A0,B1} (ph1..3, buffer 0), K-tile KT-1 stages next.K0.A1 (ph0,
// buffer 0) and next.K1.{B0,A0,B1} (ph1..3, buffer 1) — the slots, order and
// counts of the loop's own (t+1).A1 / (t+2).{B0,A0,B1}, so after the last ph3
// the block is where the prologue would have left it. Only the block's first
// tile runs the prologue; only its last stages dummies and drains.
//  RAW  next.K0's last two loads (A1) are issued in ph0 of K-tile KT-1; that
//       K-tile's ph3 vmcnt(6) leaves only next.K1.{B0,A0,B1} in flight, so
//       next.K0 has landed in this thread; the two barriers of that ph3 (one
//       of them after every staggered partner's own vmcnt(6)) come before the
//       first ds_read of next.K0 in the next tile's ph0 — the in-loop
//       argument with t+1 = next.K0.
//  WAR  the seam stages into exactly the slots the loop would restage at the
//       same phases, so no slot is restaged within two phases of its last
//       ds_read (B0 by the lgkmcnt(8) rule); the next tile's ph0 restages
//       buffer 1's A1, last read in ph2 of K-tile KT-1, two phases earlier.
//  Epilogue  runs between the last phase of tile n and ph0 of tile n+1, with
//       next.K1's 6 loads in flight, and has no barrier: the one-barrier
//       stagger carries across tiles and is balanced once at the block's end.
//       Its global stores count in vmcnt but are OLDER than every load issued
//       after them, and loads retire in order among loads: a later vmcnt(6)
//       with stores still counted waits for more loads, never for fewer. The
//       first one (next tile, K-tile 0, ph3) has 8 younger loads behind the
//       stores, so it also retires them all.
//  WIDE the epilogue passes each wave's 64x32 bf16 piece through a wave-
//       private 4 KiB LDS region above the 128 KiB pipeline buffers (never
//       overlapping them: the next tile's loads are landing), ordered by the
//       in-order LDS queue of the one wave that touches it (lgkmcnt only), and
//       stores whole 64-byte rows as dwordx4: 8 stores per lane for 64.
template <int SWZ, bool WIDE>
__global__ __launch_bounds__(512) void gemm_swiglu_persist_kernel(
    u16* __restrict__ out, const u16* __restrict__ x,
    const u16* __restrict__ w, int M, int N, long K, int xcd_swz,
    int group_m) {
  extern __shared__ __attribute__((aligned(1024))) char smem[];

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wm = wave >> 2;
  const int wn = wave & 3;

  const int I = N >> 1;
  const int MT = (M + 255) >> 8;
  const int NT = I >> 7;
  const int tiles = MT * NT;

  const int nb = gridDim.x;
  const int nx = xcd_swz ? min(8, nb) : 1;
  const int xl = blockIdx.x % nx, slot = blockIdx.x / nx;
  const int slots = (nb - xl + nx - 1) / nx;  // blocks with this label
  const int q = tiles / nx, r = tiles % nx;
  const int span0 = xl < r ? xl * (q + 1) : r * (q + 1) + (xl - r) * q;
  const int span_n = q + (xl < r ? 1 : 0);
  if (slot >= span_n) return;  // no tile: out before the first barrier
  const int cnt = (span_n - slot + slots - 1) / slots;

  const u32 Kb = (u32)K * 2u;
  const int KT = (int)(K >> 6);  // even, >= 2
  const long klb = (long)(KT - 1) * 128;
  u32 bo0, bo1;  // the unclamped lane offsets (both B halves, every tile)
  lane_offsets<SWZ>(bo0, bo1, 128, Kb, wave, lane);

  int mt, nt;
#define TILE_AT(IDX)                                                     \
  if (group_m < 0)                                                       \
    tile_mn_banded(xl, (IDX), nx, MT, NT, group_m, mt, nt);              \
  else                                                                   \
    tile_mn(span0 + (IDX), MT, NT, group_m, mt, nt);
  TILE_AT(slot)
  int m0 = mt * 256, nb0 = nt * 128;
  TileSrc cur = swiglu_tile_src<SWZ>(x, w, M, I, Kb, m0, nb0, wave, lane);

  char* const sw = smem + wave * 2048;  // this wave's 2 KiB of every slot

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

  // prologue, first tile only: K-tile 0 whole, K-tile 1's first three
  // half-tiles; the wait leaves the last 6 loads in flight
#define S_B0(T) (USrc{T.b0, bo0, bo1})
#define S_A0(T) (USrc{T.a0, T.a0o0, T.a0o1})
#define S_B1(T) (USrc{T.b1, bo0, bo1})
#define S_A1(T) (USrc{T.a1, T.a1o0, T.a1o1})
  stage_half(sw + SLOT_B0 * HT, S_B0(cur), 0);
  stage_half(sw + SLOT_A0 * HT, S_A0(cur), 0);
  stage_half(sw + SLOT_B1 * HT, S_B1(cur), 0);
  stage_half(sw + SLOT_A1 * HT, S_A1(cur), 0);
  stage_half(sw + KTILE_B + SLOT_B0 * HT, S_B0(cur), 128);
  stage_half(sw + KTILE_B + SLOT_A0 * HT, S_A0(cur), 128);
  stage_half(sw + KTILE_B + SLOT_B1 * HT, S_B1(cur), 128);
  asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  if (wm == 1) __builtin_amdgcn_s_barrier();  // stagger waves 4..7

  bf16x8 fa[4][2], fb0[2][2], fb1[2][2];

  // epilogue coordinates: D[16,16] lane l holds rows (l/16)*4+r, col l%16
  const int drow = (lane >> 4) * 4;
  const int dcol = lane & 15;
  // WIDE: this wave's 64 rows x 64 B staging piece, 16-byte chunks XORed with
  // (row / 4) % 4 so that the four row groups of one ds_write spread out
  char* const ep = smem + 2 * KTILE_B + wave * 4096;

  for (int it = 0; it < cnt; ++it) {
    for (int t = 0; t < KT - 2; t += 2) {
      const long k1 = (long)(t + 1) * 128;
      KTILE_G(0, S_A1(cur), k1, S_B0(cur), S_A0(cur), S_B1(cur), k1 + 128)
      KTILE_G(1, S_A1(cur), k1 + 128, S_B0(cur), S_A0(cur), S_B1(cur),
              k1 + 256)
    }
    // the seam: sources of the next tile, recomputed here (M-edge clamping
    // included) and not carried through the loop; the block's last tile
    // stages itself again from its last K-tile, as the one-tile kernel does
    const bool more = it + 1 < cnt;
    TILE_AT(slot + (more ? it + 1 : it) * slots)
    const int m0n = mt * 256, nb0n = nt * 128;
    const TileSrc nx_ =
        swiglu_tile_src<SWZ>(x, w, M, I, Kb, m0n, nb0n, wave, lane);
    const long kz0 = more ? 0 : klb, kz1 = more ? 128 : klb;
    KTILE_G(0, S_A1(cur), klb, S_B0(nx_), S_A0(nx_), S_B1(nx_), kz0)
    KTILE_G(1, S_A1(nx_), kz0, S_B0(nx_), S_A0(nx_), S_B1(nx_), kz1)
    if (!more) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");

#pragma unroll
    for (int a = 0; a < 2; ++a) {
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const int gn = nb0 + wn * 32 + j * 16 + dcol;  // < I (I % 128 == 0)
          const int gm = m0 + a * 128 + wm * 64 + i * 16 + drow;
#pragma unroll
          for (int rr = 0; rr < 4; ++rr) {
            // both halves rounded to bf16 first: the unfused pipeline's
            // arithmetic (GEMM output in bf16, then silu_mul_kernel)
            const float gf = bf2f(f2bf(acc[a][0][i][j][rr]));
            const float uf = bf2f(f2bf(acc[a][1][i][j][rr]));
            const float s = gf / (1.f + __expf(-gf));
            const u16 v = f2bf(s * uf);
            if (WIDE) {
              const u32 row = (u32)(i * 16 + drow + rr);
              const u32 col = (u32)(j * 16 + dcol);
              *(u16*)(ep + row * 64u + ((((col >> 3) ^ (row >> 2)) & 3u) << 4) +
                      (col & 7u) * 2u) = v;
            } else if (gm + rr < M) {
              out[(long)(gm + rr) * I + gn] = v;
            }
            acc[a][0][i][j][rr] = 0.f;
            acc[a][1][i][j][rr] = 0.f;
          }
        }
      if (WIDE) {
#pragma unroll
        for (int p = 0; p < 4; ++p) {
          const u32 row = (u32)(p * 16 + (lane >> 2));
          const u32 ch = (u32)(lane & 3);
          const u32x4 v =
              *(const u32x4*)(ep + row * 64u + (((ch ^ (row >> 2)) & 3u) << 4));
          const int gm = m0 + a * 128 + wm * 64 + (int)row;
          if (gm < M)
            *(u32x4*)(out + (long)gm * I + nb0 + wn * 32 + ch * 8) = v;
        }
      }
    }
    cur = nx_;
    m0 = m0n;
    nb0 = nb0n;
  }
  if (wm == 0) __builtin_amdgcn_s_barrier();  // balances the stagger
}

#undef TILE_AT
#undef S_B0
#undef S_A0
#undef S_B1
#undef S_A1
#undef KTILE_G
#undef PHASE_SYNC_MFMA

// epi: 0 plain, 1 residual (res != nullptr), 2 SwiGLU (N = 2I rows of w,
// out [M, I], I % 128 == 0). Any M >= 1, any N >= 1 (epi 0/1), K % 64 == 0.
// group_m: tile order of tile_mn (0 = plain; < 0 = tile_mn_banded in groups
// of -group_m, which needs xcd_swz). variant 1 (epi 2 only,
// K % 128 == 0): the persistent kernel on num_blocks blocks (0: one per CU
// of the current device; < 0: one per tile, which leaves the walk to the
// hardware's dispatcher), wide = dwordx4 epilogue stores. The defaults of
// the trailing arguments are the one-tile-per-block kernel in plain order.
// Returns 0, the hipError_t of an attribute call, or < 0 for arguments no
// instantiation takes. No allocation and no sync: capturable.
extern "C" int sutro_gemm_tn_pipe_launch(void* out, const void* x,
                                         const void* w, const void* res,
                                         int M, int N, long K, int epi,
                                         int swz_mode, int xcd_swz,
                                         hipStream_t stream, int variant,
                                         int group_m, int num_blocks,
                                         int wide) {
  constexpr int LDS_BYTES = 2 * KTILE_B;
  constexpr int MAX_DEV = 64;
  const int mt = (M + 255) / 256;
  const int ntl = (epi == 2) ? (N / 2) / 128 : (N + 255) / 256;
  dim3 grid(mt * ntl), block(512);
  if (group_m < 0 && !xcd_swz) return -4;
  if (variant == 1) {
    if (epi != 2 || K < 128 || K % 128 != 0 || K > (1L << 23)) return -2;
    int dev = 0;
    const int ed = (int)hipGetDevice(&dev);
    if (ed != 0) return ed;
    const bool slot_ok = dev >= 0 && dev < MAX_DEV;
    if (num_blocks < 0) {
      num_blocks = mt * ntl;  // one tile per block, dispatched by the hardware
    } else if (num_blocks == 0) {
      static int cus[MAX_DEV];  // CU count, queried once per device
      int n = slot_ok ? cus[dev] : 0;
      if (n == 0) {
        const int e = (int)hipDeviceGetAttribute(
            &n, hipDeviceAttributeMultiprocessorCount, dev);
        if (e != 0) return e;
        if (n <= 0) return -3;
        if (slot_ok) cus[dev] = n;
      }
      num_blocks = n;
    }
    static bool pattr_set[3][2][MAX_DEV];
#define LAUNCH_P(SWZ, WIDE)                                                  \
  if (swz_mode == SWZ && (wide != 0) == WIDE) {                              \
    constexpr int LDS_P = LDS_BYTES + (WIDE ? 8 * 4096 : 0);                 \
    if (!slot_ok || !pattr_set[SWZ][WIDE][dev]) {                            \
      const int e = (int)hipFuncSetAttribute(                                \
          (const void*)gemm_swiglu_persist_kernel<SWZ, WIDE>,                \
          hipFuncAttributeMaxDynamicSharedMemorySize, LDS_P);                \
      if (e != 0) return e;                                                  \
      if (slot_ok) pattr_set[SWZ][WIDE][dev] = true;                         \
    }                                                                        \
    gemm_swiglu_persist_kernel<SWZ, WIDE>                                    \
        <<<dim3(num_blocks), block, LDS_P, stream>>>(                        \
            (u16*)out, (const u16*)x, (const u16*)w, M, N, K, xcd_swz,       \
            group_m);                                                        \
    return 0;                                                                \
  }
    LAUNCH_P(0, false) LAUNCH_P(1, false) LAUNCH_P(2, false)
    LAUNCH_P(0, true) LAUNCH_P(1, true) LAUNCH_P(2, true)
#undef LAUNCH_P
    return -1;
  }
  if (variant != 0) return -1;
  // dynamic LDS above 64 KiB needs the attribute, which is per device and
  // per instantiation: set once each (setting it twice in a race is harmless)
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
        xcd_swz, group_m);                                                   \
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
