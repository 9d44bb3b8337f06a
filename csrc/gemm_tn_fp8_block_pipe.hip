// Block-scaled FP8 (OCP e4m3) TN GEMM for MI355X, the arithmetic of the
// published block-FP8 checkpoints (`weight` + `weight_scale_inv`):
//
//   out[M, N] bf16 = sum over kb ascending of
//       (A_q[M, kb] . W_q[N, kb]^T in f32) * (a_s[kb, m] * w_s[n / 128, kb])
//
// kb = one group of 128 K elements, a_s [K/128, M] f32 (one scale per row and
// K group, K-block-major, row stride lda_s), w_s [N/128, K/128] f32 (one
// scale per 128x128 weight block). The statement is
// torch_ref.fp8_block_linear; EPI 1 adds a bf16 residual in f32 before the
// one rounding, EPI 2 is silu(g) * u on the merged [2I, K] gate_up weight.
// The file also holds the activation quantiser that writes A_q and a_s.
//
// The tile, the staging and the barriers are csrc/gemm_tn_fp8_pipe.hip's,
// unchanged: 256x256 output tile, 8 waves as 2(M)x4(N), `global_load_lds`
// dwordx4 staging of 128-byte LDS rows, swizzle mode 2, bijective XCD remap,
// 2 K-tile buffers x 4 half-tiles of 16 KiB of dynamic LDS in staging
// order B0, A0, B1, A1 (plain: nb0 = n0, nb1 = n0 + 128; SwiGLU:
// nb0 = n0, nb1 = I + n0), wave (wm, wn) owning four 64x32 quadrants, one
// per phase, waves 4..7 one barrier behind their SIMD partners. One K-tile
// is one scale group in K, and each 128-row half-tile of W lies inside one
// scale block in N, so the weight scale of a (half-tile, K-tile) pair is
// uniform over the block.
//
// What differs is the arithmetic of a phase. The 8 MFMAs
// (mfma_scale_f32_16x16x128_f8f6f4, hardware block scales e8m0 1.0) start
// from a zero C and give the unscaled partial products p of this K-tile;
// they are folded into the running accumulators by
//     acc[r] = fma(p[r], a_s[row r] * w_s, acc[r])
// with one f32 product per (row, half-tile) as the factor. D[16,16] lane l
// holds rows (l/16)*4 + r of column l%16, so a lane needs the 4 scales of
// rows (l/16)*4 .. +3 of each of its 4 m-fragments: one 16-byte read per
// fragment, 4 per A half-tile and K-tile.
//
// Where the scales come from. The register budget decides it: at 8 waves per
// CU a wave has 256 registers, the per-channel kernel uses 220, and the scales
// of both A half-tiles held in registers a K-tile ahead would be 32 more
// beside the products p. An ordinary register load is no way either: the
// compiler waits for one with vmcnt(0) while LDS-DMA loads are pending, which
// drains the prefetch. So the activation scales take the road of the tiles,
// `global_load_lds` (4 bytes a lane), into 8 KiB above the two K-tile
// buffers: 1 KiB PRIVATE to each wave = 2 buffers x [A half][64 rows] f32,
// the scales of the wave's own 2 x 64 rows for one K-tile each.
//   ph0 of tile t: 2 loads bring the scales of tile t+1 into buffer (t+1)&1,
//                  issued BEFORE stage (t+1).A1; lane l supplies row l of
//                  the 64 (clamped to M - 1, so a_s [K/128, M] is never read
//                  past its end; such rows are never stored);
//   ph0 / ph2 of tile t+1: 4 16-byte ds_reads fetch the scales of A0 / A1,
//                  beside the fragments of the same half and with their
//                  lifetime (16 registers).
// The two weight scales have a block-uniform address; they are loaded in ph2
// for tile t+1 by an ordinary load, for which the compiler chooses a scalar
// load (lgkmcnt) and waits itself, and are held beside those of tile t until
// the end of ph3. All of these are pinned in place by sched_barrier(0).
//
// Schedule per K-tile t (buffer P = t & 1); counts are ds_reads per wave (a
// fragment = 2 of them, S = the 4 scale reads):
//   ph0: ds_read B0(4) A0(8) S0(4) | stage scales(t+1), (t+1).A1
//                                                    | lgkmcnt(12) | C00
//   ph1: ds_read B1(4)             | stage (t+2).B0  |             | C01
//   ph2: ds_read A1(8) S1(4)       | load w scales(t+1), stage (t+2).A0
//                                                    |             | C10
//   ph3:                           | stage (t+2).B1  | vmcnt(6)    | C11
// each phase: reads + loads, s_barrier, lgkmcnt(0), 8 MFMA with the fold of
// each behind the next one's issue, s_barrier.
//
// Ordering, re-derived with the scale traffic in the stream.
//  RAW  vmcnt counts in order. The scale loads of ph0 are issued before stage
//       (t+1).A1, so the vector memory operations after that stage and up to
//       ph3's wait are (t+2).B0 [2], (t+2).A0 [2], (t+2).B1 [2] = 6, as in
//       the per-channel kernel (were the weight-scale loads of ph2 vector
//       loads there would be 8, and vmcnt(6) only stricter). vmcnt(6)
//       therefore retires (t+1).A1, the scales of tile t+1 and everything
//       older. Tile t+1 has landed before ph3's first barrier and is first
//       read in the next phase; the scales are read by the wave that loaded
//       and waited for them. The prologue issues its two scale loads before
//       the 14 staging loads, so its vmcnt(6) still leaves only tile 1's
//       three half-tiles.
//  WAR  staging slots and phases are unchanged: a slot is restaged >= 2
//       phases after its last ds_read, except B0 (read ph0, restaged ph1),
//       whose 4 reads are issued first and are retired by ph0's lgkmcnt(12):
//       16 issued, at most the 8 A0 and 4 scale reads outstanding, LDS reads
//       retire in order, and nothing else is outstanding on that counter (a
//       scalar weight-scale load of ph2 was retired by ph2's lgkmcnt(0)).
//       Scale buffer (t+1)&1 was last read in ph2 of tile t-1 by the wave
//       that restages it in ph0 of tile t, two lgkmcnt(0) later.
// The tail keeps the counts uniform: tiles past the end are staged, and their
// scales loaded, from the last K-tile.
//
// Cost of the fold, per MFMA: 4 v_fma_f32 plus 2 of the 16 factor multiplies
// of the phase, issued while the next MFMA runs. It has not been tuned or
// timed yet (profiles/PROFILES.md, capture B1).
#include "common.h"

typedef int i32x8 __attribute__((ext_vector_type(8)));

namespace {

// e8m0 1.0 in every byte: the hardware block scale is a no-op
constexpr int SCALE_ONE = 0x7f7f7f7f;

__device__ __forceinline__ f32x4 mfma128z(i32x8 a, i32x8 b) {
  return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(
      a, b, f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0, SCALE_ONE, 0, SCALE_ONE);
}

// direct HBM->LDS 16-byte copy; lds is the wave-uniform base, lane l lands at
// lds + l*16
__device__ __forceinline__ void glds16(const char* g, char* lds) {
  __builtin_amdgcn_global_load_lds(
      (const __attribute__((address_space(1))) u32*)g,
      (__attribute__((address_space(3))) u32*)lds, 16, 0, 0);
}

// the same for 4 bytes a lane: lane l lands at lds + l*4
__device__ __forceinline__ void glds4(const char* g, char* lds) {
  __builtin_amdgcn_global_load_lds(
      (const __attribute__((address_space(1))) u32*)g,
      (__attribute__((address_space(3))) u32*)lds, 4, 0, 0);
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

// ---- activation quantiser: bf16 [R, K] -> e4m3 [R, K] + f32 [K/128, R] ----
// Every group of 128 consecutive K elements of a row gets its own scale, by
// the rule of quant_rows_fp8 (csrc/grouped_gemm_fp8.hip): scale = amax / 448
// (true f32 division; 1 for an all-zero group), code = e4m3_rne(clamp(x /
// scale, -448, 448)) — torch_ref.quantize_rows_fp8_block128, which this
// matches bit for bit. A group is 16 lanes of one 16-byte load each, so a
// wave takes 4 groups and the amax is a 16-lane reduction. The scale goes to
// out_scale[kb * lds + row] (K-block-major, row stride lds >= R).
__global__ void __launch_bounds__(256) quant_rows_fp8_block128_kernel(
    u8* __restrict__ out_q,         // [R, K] e4m3
    float* __restrict__ out_scale,  // [K/128, lds]
    const u16* __restrict__ x,      // [R, K] bf16
    long R, int KB, long lds) {
  const int lane = threadIdx.x & 63;
  const long g = ((long)blockIdx.x * 4 + (threadIdx.x >> 6)) * 4 + (lane >> 4);
  const bool live = g < R * KB;
  const long off = g * 128 + (lane & 15) * 8;  // group g starts at g * 128
  u16x8 v = u16x8{0, 0, 0, 0, 0, 0, 0, 0};
  if (live) v = *(const u16x8*)(x + off);
  float amax = 0.f;
#pragma unroll
  for (int e = 0; e < 8; ++e) amax = fmaxf(amax, fabsf(bf2f(v[e])));
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) amax = fmaxf(amax, __shfl_xor(amax, o, 64));
  if (!live) return;
  const float scale = amax > 0.f ? amax / 448.0f : 1.0f;
  if ((lane & 15) == 0) out_scale[(g % KB) * lds + g / KB] = scale;
  u32 w[2];
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    float f[4];
#pragma unroll
    for (int e = 0; e < 4; ++e)
      f[e] = fminf(fmaxf(bf2f(v[p * 4 + e]) / scale, -448.0f), 448.0f);
    w[p] = (u32)f2fp8x2(f[0], f[1]) | ((u32)f2fp8x2(f[2], f[3]) << 16);
  }
  *(u32x2*)(out_q + off) = u32x2{w[0], w[1]};
}

// K % 128 == 0, lds >= R. Static grid, no host sync, no hipGetLastError: runs
// inside captured decode steps.
extern "C" void sutro_quant_rows_fp8_block128(void* out_q, float* out_scale,
                                              const void* x, long R, long K,
                                              long lds, hipStream_t stream) {
  if (R == 0) return;
  const long KB = K / 128;
  const long groups = R * KB;
  hipLaunchKernelGGL(quant_rows_fp8_block128_kernel,
                     dim3((unsigned)((groups + 15) / 16)), dim3(256), 0,
                     stream, (u8*)out_q, out_scale, (const u16*)x, R, (int)KB,
                     lds);
}

// ---- the GEMM ----

// EPI: 0 = plain store, 1 = residual add, 2 = SwiGLU (out is [M, N/2])
// no-packed-fp32-ops: beside MFMAs a v_pk_fma_f32 costs more than the two
// v_fma_f32 it replaces, and plain -O3 would pack the fold
#if defined(__HIP_DEVICE_COMPILE__)
#define NO_PACKED_F32 __attribute__((target("no-packed-fp32-ops")))
#else
#define NO_PACKED_F32  // the host pass does not know the feature
#endif
template <int EPI>
NO_PACKED_F32 __global__ __launch_bounds__(512) void
gemm_tn_fp8_block_pipe_kernel(
    u16* __restrict__ out, const u8* __restrict__ a,
    const float* __restrict__ a_scale, long lda_s, const u8* __restrict__ w,
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

  const int KT = (int)(Kp >> 7);
  const int klast = KT - 1;

  // scales. Activation: lane l copies the scale of row l of this wave's 64
  // rows of half x (clamped to the last valid row, so a [K/128, M] tensor is
  // never read past its end) to byte l * 4 of [buffer][A half][64 rows] in
  // the wave's private area; the 4 accumulator rows of m-fragment i are then
  // the 16 bytes at row i*16 + (lane/16)*4.
  // Weight: block row of each B half-tile (a half wholly past the edge takes
  // the last valid block; its columns are never stored), K group kb.
  const char* asg[2];
#pragma unroll
  for (int x = 0; x < 2; ++x)
    asg[x] = (const char*)(a_scale +
                           min(m0 + x * 128 + wm * 64 + lane, M - 1));
  const long lda_b = lda_s * 4;
  char* const scw = smem + 2 * KTILE_B + wave * 1024;
  const u32 scr = (u32)(lane >> 4) * 16u;
  const long wsr0 = (long)(nb0 >> 7) * KT;
  const long wsr1 = (long)(min(nb1, N - 128) >> 7) * KT;
#define STAGE_ASC(BUF_, KB_)                                             \
  glds4(asg[0] + (long)(KB_) * lda_b, scw + (BUF_) * 512);               \
  glds4(asg[1] + (long)(KB_) * lda_b, scw + (BUF_) * 512 + 256);
#define READ_ASC(BUF_, X_)                                               \
  _Pragma("unroll") for (int i = 0; i < 4; ++i)                          \
      asc[i] = *(const f32x4*)(scw + (BUF_) * 512 + (X_) * 256 + i * 64 + \
                               scr);

  f32x4 asc[4];          // [m frag]: scales of this lane's 4 rows, one half
  float wsc[2], wsn[2];  // weight scales of B0 / B1: this tile, next tile

  f32x4 acc[2][2][4][2];  // [A half][B half][m frag][n frag]
#pragma unroll
  for (int x = 0; x < 2; ++x)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[x][b][i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  // prologue: the scales ph0 of tile 0 needs, then tile 0 whole and tile 1's
  // first three half-tiles; of the 14 staging loads the wait leaves the last
  // 6 (tile 1) in flight
  {
    STAGE_ASC(0, 0)
    wsc[0] = w_scale[wsr0];
    wsc[1] = w_scale[wsr1];
    __builtin_amdgcn_sched_barrier(0);
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

  // fold of MFMA (i, j): the row factors of fragment i (made once, with
  // j == 0) and one fma per accumulator element; scalar fmas on purpose
#define FOLD(A_, B_, I_, J_, P_)                                         \
  {                                                                      \
    if ((J_) == 0) {                                                     \
      _Pragma("unroll") for (int r = 0; r < 4; ++r)                      \
          f[r] = asc[I_][r] * wsc[B_];                                   \
    }                                                                    \
    _Pragma("unroll") for (int r = 0; r < 4; ++r)                        \
        acc[A_][B_][I_][J_][r] =                                         \
            __builtin_fmaf(P_[r], f[r], acc[A_][B_][I_][J_][r]);         \
  }

  // 8 MFMAs from a zero C, each folded while the next one runs
#define PHASE_SYNC_MFMA(A_, B_, FB_)                                     \
  __builtin_amdgcn_sched_barrier(0);                                     \
  __builtin_amdgcn_s_barrier();                                          \
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                     \
  __builtin_amdgcn_sched_barrier(0);                                     \
  __builtin_amdgcn_s_setprio(1);                                         \
  {                                                                      \
    float f[4];                                                          \
    f32x4 pe, po;                                                        \
    pe = mfma128z(fa[0], FB_[0]);                                        \
    po = mfma128z(fa[0], FB_[1]);                                        \
    FOLD(A_, B_, 0, 0, pe)                                               \
    pe = mfma128z(fa[1], FB_[0]);                                        \
    FOLD(A_, B_, 0, 1, po)                                               \
    po = mfma128z(fa[1], FB_[1]);                                        \
    FOLD(A_, B_, 1, 0, pe)                                               \
    pe = mfma128z(fa[2], FB_[0]);                                        \
    FOLD(A_, B_, 1, 1, po)                                               \
    po = mfma128z(fa[2], FB_[1]);                                        \
    FOLD(A_, B_, 2, 0, pe)                                               \
    pe = mfma128z(fa[3], FB_[0]);                                        \
    FOLD(A_, B_, 2, 1, po)                                               \
    po = mfma128z(fa[3], FB_[1]);                                        \
    FOLD(A_, B_, 3, 0, pe)                                               \
    FOLD(A_, B_, 3, 1, po)                                               \
  }                                                                      \
  __builtin_amdgcn_s_setprio(0);                                         \
  __builtin_amdgcn_sched_barrier(0);                                     \
  __builtin_amdgcn_s_barrier();                                          \
  __builtin_amdgcn_sched_barrier(0);

  // one K-tile out of buffer P; kn1/kn2 = byte offsets of tiles t+1, t+2,
  // kbn = K group of tile t+1 (clamped)
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
    READ_ASC(P, 0)                                                       \
    __builtin_amdgcn_sched_barrier(0);                                   \
    STAGE_ASC((P) ^ 1, kbn)                                              \
    __builtin_amdgcn_sched_barrier(0);                                   \
    stage_half(nxt + SLOT_A1 * HT, sA1, kn1);                            \
    __builtin_amdgcn_sched_barrier(0);                                   \
    asm volatile("s_waitcnt lgkmcnt(12)" ::: "memory");                  \
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
    READ_ASC(P, 1)                                                       \
    __builtin_amdgcn_sched_barrier(0);                                   \
    wsn[0] = w_scale[wsr0 + kbn];                                        \
    wsn[1] = w_scale[wsr1 + kbn];                                        \
    __builtin_amdgcn_sched_barrier(0);                                   \
    stage_half(own + SLOT_A0 * HT, sA0, kn2);                            \
    PHASE_SYNC_MFMA(1, 0, fb0)                                           \
    /* ph3 */                                                            \
    stage_half(own + SLOT_B1 * HT, sB1, kn2);                            \
    __builtin_amdgcn_sched_barrier(0);                                   \
    asm volatile("s_waitcnt vmcnt(6)" ::: "memory");                     \
    PHASE_SYNC_MFMA(1, 1, fb1)                                           \
    wsc[0] = wsn[0];                                                     \
    wsc[1] = wsn[1];                                                     \
  }

  for (int t = 0; t < KT; t += 2) {
    {
      const int kbn = min(t + 1, klast);
      const long kn1 = (long)kbn * 128;
      const long kn2 = (long)min(t + 2, klast) * 128;
      KTILE(0)
    }
    if (t + 1 < KT) {
      const int kbn = min(t + 2, klast);
      const long kn1 = (long)kbn * 128;
      const long kn2 = (long)min(t + 3, klast) * 128;
      KTILE(1)
    }
  }
#undef KTILE
#undef PHASE_SYNC_MFMA
#undef FOLD
#undef READ_ASC
#undef STAGE_ASC

  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  if (wm == 0) __builtin_amdgcn_s_barrier();  // balances the stagger

  // epilogue: D[16,16] lane l holds rows (l/16)*4+r, col l%16; the
  // accumulators already carry their scales
  const int drow = (lane >> 4) * 4;
  const int dcol = lane & 15;
#pragma unroll
  for (int x = 0; x < 2; ++x)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int gm = m0 + x * 128 + wm * 64 + i * 16 + drow;
      if (EPI == 2) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const int gn = nb0 + wn * 32 + j * 16 + dcol;  // < I (I % 128 == 0)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            if (gm + r >= M) continue;
            // f32 SwiGLU on the unrounded products, one rounding
            const float g = acc[x][0][i][j][r];
            const float u = acc[x][1][i][j][r];
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
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              if (gm + r >= M) continue;
              const long o = (long)(gm + r) * N + gn;
              float v = acc[x][b][i][j][r];
              // a separate f32 add, then the one rounding to bf16
              if (EPI == 1) v = __fadd_rn(v, bf2f(res[o]));
              out[o] = f2bf(v);
            }
          }
      }
    }
}

// epi: 0 plain, 1 residual (res != nullptr), 2 SwiGLU (N = 2I rows of w,
// out [M, I]). 1 <= M <= 2^31 - 256 (the row-tile count is taken in int),
// N % 128 == 0 (epi 2: I % 128 == 0), Kp % 128 == 0. a_scale is [Kp/128, M]
// with row stride lda_s >= M, w_scale is [N/128, Kp/128] contiguous.
// No hipGetLastError and no sync: it runs under hipGraph capture.
// Returns 0, or the hipError_t of the LDS-size attribute call.
extern "C" int sutro_gemm_tn_fp8_block_pipe_launch(
    void* out, const void* a, const float* a_scale, long lda_s, const void* w,
    const float* w_scale, const void* res, int M, int N, long Kp, int epi,
    int xcd_swz, hipStream_t stream) {
  // two K-tile buffers + 8 waves x 1 KiB of activation scales
  constexpr int LDS_BYTES = 2 * KTILE_B + 8 * 1024;
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
          (const void*)gemm_tn_fp8_block_pipe_kernel<EPI>,                   \
          hipFuncAttributeMaxDynamicSharedMemorySize, LDS_BYTES);            \
      if (e != 0) return e;                                                  \
      if (dev >= 0 && dev < MAX_DEV) attr_set[EPI][dev] = true;              \
    }                                                                        \
    gemm_tn_fp8_block_pipe_kernel<EPI><<<grid, block, LDS_BYTES, stream>>>(  \
        (u16*)out, (const u8*)a, a_scale, lda_s, (const u8*)w, w_scale,      \
        (const u16*)res, M, N, Kp, xcd_swz);                                 \
    return 0;                                                                \
  }
  LAUNCH(0)
  LAUNCH(1)
  LAUNCH(2)
#undef LAUNCH
  return -1;
}
