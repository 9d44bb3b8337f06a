// Weight-streaming FP8 (OCP e4m3, W8A8) TN GEMM for small token counts,
// 1 <= M <= 256, on MI355X:
//
//   out[M, N] bf16 = (A_q[M, Kp] . W_q[N, Kp]^T) * a_scale[m] * w_scale[n]
//                    (+ residual[M, N], added in f32 before the one rounding)
//
// the arithmetic contract of csrc/gemm_tn_fp8_pipe.hip (plain and residual
// epilogues): e4m3 codes, f32 a_scale [M] and w_scale [N], Kp a multiple of
// 128 with a zero tail, N % 64 == 0. At these M the problem is a stream of
// weight bytes, each used once, so the weights never touch LDS and the grid
// is sized to keep many loads in flight, not to reuse operands.
//
// Operand roles are swapped relative to the 256-row kernel: a weight
// fragment (16 N-rows x 128 K-bytes) is the 16-row operand of
// mfma_scale_f32_16x16x128_f8f6f4 (cbsz = blgp = 0, both hardware block
// scales e8m0 1.0) and 16 tokens are its 16 columns. One weight fragment is
// loaded once and feeds MG = ceil(M_chunk / 16) MFMAs, one accumulator per
// 16-token group.
//
// Loads. HBM -> VGPR directly, two 16-byte global loads per lane and
// fragment: lane l supplies row l & 15 and bytes 32q .. 32q+31 of the
// 128-byte K-tile, q = l >> 4 (lds_frag_row's lane map of fp8_gemm.h
// without the LDS hop, so no swizzle). Activation fragments are loaded the
// same way; A_q is at most 256 x Kp bytes and stays in L2. Token rows past M
// are clamped to row M - 1 on load and never stored.
//
// Work split. grid = (N / 16, ceil(M / 64)): a block owns a strip of 16
// weight rows and the 64-token chunk blockIdx.y; weights are re-read per
// chunk. The block's W waves split K interleaved: wave w takes K-tiles
// t = w, w + W, w + 2W, ..., so at any moment the waves read adjacent
// 128-byte segments of the same weight rows. Each wave runs its own register
// pipeline over its tiles: a ring of DEPTH + 1 stages, the loads of its
// tile j + DEPTH are issued into the free stage before the MFMAs of tile j,
// and the waits the compiler places are counted (vmcnt(DEPTH * (2 + 2 MG))
// in the steady state: only tile j has to have landed). The tail keeps the
// counts uniform by re-loading the wave's last tile into stages that are
// never read. No LDS and no barrier in the main loop. With DEPTH = 4 a wave
// keeps 8 KB of weights in flight: N = 5120 gives 320 blocks, times 4 waves
// about 10 MB over the device (reasoning, not a measurement).
//
// The loads are inline asm with explicit `s_waitcnt vmcnt(N)`: written as
// plain C++ loads the same loop compiled to a vmcnt(0) at the head of every
// ring rotation (the compiler's wait insertion merges the loop's entry and
// back edge), which drains the pipeline once per RING tiles. A stage's
// registers reach the MFMAs only through `landed`, which orders them behind
// the wait; the dead tail loads are drained before the ring is released.
//
// Reduction. Every wave writes its f32 accumulators to LDS (W x MG x 1 KiB);
// after the one barrier the partials are summed in fixed wave order
// 0 .. W-1, multiplied by a_scale[m] * w_scale[n] in the 256-row kernel's
// expression order, the residual is added, and the value is rounded once.
// The 16x16 accumulator layout gives a lane 4 consecutive n of one token:
// one 8-byte store, guarded by m < M. A wave without a K-tile (fewer tiles
// than waves) contributes zeros. No atomics, no workspace, static grid.
//
// Invariance. Which K-tiles go to which wave, and the order of the final
// sum, depend on Kp and W only; a token's 16-column slot never mixes with
// its neighbours'. So a token's output bits do not depend on M, on its row
// index or on its chunk (tests/test_gpu_dense_fp8_skinny.py).
//
// Measured (profiles/PROFILES.md capture D2): at M <= 16 the kernel streams
// weights at the device-copy rate; from there its time grows almost linearly
// with M, because every block re-reads its whole 64-token activation chunk
// from L2 (4 activation bytes per weight byte at MG = 4). 4 waves per block
// beat 8 at every measured point, so 4 is the default; W stays a launch
// parameter for that A/B. Deviations from the issue's baseline: none.
// Follow-up: a wider weight strip per block (BN = 32 / 64) to cut the
// activation re-reads.
#include "fp8_gemm.h"

namespace {

constexpr int DEPTH = 4;         // K-tiles a wave keeps in flight
constexpr int RING = DEPTH + 1;  // register stages
constexpr int BN = 16;           // weight rows per block
constexpr int MCHUNK = 64;       // tokens per block

// 32 operand bytes of one lane, straight from global memory, as two 16-byte
// loads the compiler does not track: the kernel places its own counted
// s_waitcnt, which the compiler's wait insertion would turn into vmcnt(0) at
// the head of the unrolled ring loop (seen in the ISA of the plain C++ form).
// The two halves stay separate registers until `landed` has ordered them
// behind the wait.
__device__ __forceinline__ void gload32(u32x4& lo, u32x4& hi, const u8* p) {
  asm volatile("global_load_dwordx4 %0, %1, off"
               : "=v"(lo) : "v"(p) : "memory");
  asm volatile("global_load_dwordx4 %0, %1, off offset:16"
               : "=v"(hi) : "v"(p) : "memory");
}

// one pipeline stage: the weight fragment and MG activation fragments
template <int MG>
struct Stage {
  u32x4 w0, w1, a0[MG], a1[MG];
};

// makes every later use of the stage depend on this point of the volatile
// asm sequence (i.e. on the s_waitcnt before it); emits no instruction
template <int MG>
__device__ __forceinline__ void landed(Stage<MG>& s) {
  asm volatile("" : "+v"(s.w0), "+v"(s.w1));
#pragma unroll
  for (int g = 0; g < MG; ++g)
    asm volatile("" : "+v"(s.a0[g]), "+v"(s.a1[g]));
}

__device__ __forceinline__ i32x8 frag(u32x4 lo, u32x4 hi) {
  return i32x8{(int)lo[0], (int)lo[1], (int)lo[2], (int)lo[3],
               (int)hi[0], (int)hi[1], (int)hi[2], (int)hi[3]};
}

}  // namespace

// NO_PACKED_F32: the reduction's adds stay scalar v_add_f32

// W waves, MG 16-token groups (1..4), EPI: 0 = plain store, 1 = residual add
template <int W, int MG, int EPI>
__global__ __launch_bounds__(W * 64) NO_PACKED_F32
void gemm_tn_fp8_skinny_kernel(
    u16* __restrict__ out, const u8* __restrict__ a,
    const float* __restrict__ a_scale, const u8* __restrict__ w,
    const float* __restrict__ w_scale, const u16* __restrict__ res, int M,
    int N, long Kp) {
  __shared__ f32x4 part[W][MG][64];

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int n0 = blockIdx.x * BN;
  const int m0 = blockIdx.y * MCHUNK;

  // this lane's operand rows at K-tile 0: weight row n0 + l % 16 (N % 16 == 0,
  // always valid) and one token row per group, clamped to the last valid one
  const long koff = (long)(lane >> 4) * 32;
  const u8* wp = w + (long)(n0 + (lane & 15)) * Kp + koff;
  const u8* ap[MG];
#pragma unroll
  for (int g = 0; g < MG; ++g)
    ap[g] = a + (long)min(m0 + g * 16 + (lane & 15), M - 1) * Kp + koff;

  f32x4 acc[MG];
#pragma unroll
  for (int g = 0; g < MG; ++g) acc[g] = f32x4{0.f, 0.f, 0.f, 0.f};

  // this wave's K-tiles: t = wave + j * W, j = 0 .. cnt-1 (a function of Kp)
  const int KT = (int)(Kp >> 7);
  const int cnt = wave < KT ? (KT - wave + W - 1) / W : 0;

  if (cnt > 0) {
    Stage<MG> st[RING];
    const int jlast = cnt - 1;
    // loads of one tile in flight: 2 weight + 2 MG activation
    constexpr int L = 2 + 2 * MG;

    // loads of the wave's tile j into stage S; j is clamped, so past the
    // end the wave re-loads its last tile into a stage that is never read
    // and the counted wait below is the same at every step
#define LOAD_TILE(S, J)                                                  \
  {                                                                      \
    const long kb = (long)(wave + min((J), jlast) * W) * 128;            \
    gload32(st[S].w0, st[S].w1, wp + kb);                                \
    _Pragma("unroll") for (int g = 0; g < MG; ++g)                       \
        gload32(st[S].a0[g], st[S].a1[g], ap[g] + kb);                   \
  }

#pragma unroll
    for (int s = 0; s < DEPTH; ++s) LOAD_TILE(s, s)

    for (int j0 = 0; j0 < cnt; j0 += RING) {
#pragma unroll
      for (int s = 0; s < RING; ++s) {
        const int j = j0 + s;
        LOAD_TILE((s + DEPTH) % RING, j + DEPTH)
        // tiles j+1 .. j+DEPTH may still be in flight, tile j has landed
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"(DEPTH * L) : "memory");
        landed(st[s]);
        if (j < cnt) {  // the last ring may be partial
          const i32x8 wf = frag(st[s].w0, st[s].w1);
#pragma unroll
          for (int g = 0; g < MG; ++g)
            acc[g] = mfma128(wf, frag(st[s].a0[g], st[s].a1[g]), acc[g]);
        }
      }
    }
#undef LOAD_TILE
    // the dead tail loads still target the ring: drain them while the ring
    // registers are live, before anything else may be allocated there
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
    for (int s = 0; s < RING; ++s) landed(st[s]);
  }

#pragma unroll
  for (int g = 0; g < MG; ++g) part[wave][g][lane] = acc[g];
  __syncthreads();

  // D[16,16]: lane l holds rows (l / 16) * 4 + r (= n here), col l % 16 (=
  // token). One (group, lane) slot per thread.
  for (int idx = threadIdx.x; idx < MG * 64; idx += W * 64) {
    const int g = idx >> 6, l = idx & 63;
    const int m = m0 + g * 16 + (l & 15);
    if (m >= M) continue;
    f32x4 s = part[0][g][l];
#pragma unroll
    for (int x = 1; x < W; ++x) {  // fixed order 0 .. W-1
      const f32x4 p = part[x][g][l];
#pragma unroll
      for (int r = 0; r < 4; ++r) s[r] = __fadd_rn(s[r], p[r]);
    }
    const int n = n0 + (l >> 4) * 4;
    const float as = a_scale[m];
    const f32x4 ws = *(const f32x4*)(w_scale + n);
    const long o = (long)m * N + n;  // 8-byte aligned: n % 4 == 0, N % 64 == 0
    u16x4 rr = u16x4{0, 0, 0, 0};
    if (EPI == 1) rr = *(const u16x4*)(res + o);
    u16x4 v;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float f = s[r] * as * ws[r];
      // a separate f32 add (no contraction into the scale multiply), then
      // the one rounding to bf16
      if (EPI == 1) f = __fadd_rn(f, bf2f(rr[r]));
      v[r] = f2bf(f);
    }
    *(u16x4*)(out + o) = v;
  }
}

// 1 <= M <= 256, N % 64 == 0, Kp % 128 == 0 (the binding enforces all three),
// res may be nullptr, waves 4 or 8. No hipGetLastError and no sync: it runs
// under hipGraph capture. Returns 0, or -1 for arguments it does not take.
extern "C" int sutro_gemm_tn_fp8_skinny_launch(
    void* out, const void* a, const float* a_scale, const void* w,
    const float* w_scale, const void* res, int M, int N, long Kp, int waves,
    hipStream_t stream) {
  if (M < 1 || M > 256 || N < 16 || N % 16 != 0 || Kp < 128 || Kp % 128 != 0)
    return -1;
  const int mg = M > MCHUNK ? MCHUNK / 16 : (M + 15) / 16;
  const dim3 grid((unsigned)(N / BN), (unsigned)((M + MCHUNK - 1) / MCHUNK));
#define LAUNCH(W_, MG_)                                                      \
  if (waves == W_ && mg == MG_) {                                            \
    if (res)                                                                 \
      gemm_tn_fp8_skinny_kernel<W_, MG_, 1><<<grid, W_ * 64, 0, stream>>>(   \
          (u16*)out, (const u8*)a, a_scale, (const u8*)w, w_scale,           \
          (const u16*)res, M, N, Kp);                                        \
    else                                                                     \
      gemm_tn_fp8_skinny_kernel<W_, MG_, 0><<<grid, W_ * 64, 0, stream>>>(   \
          (u16*)out, (const u8*)a, a_scale, (const u8*)w, w_scale, nullptr,  \
          M, N, Kp);                                                         \
    return 0;                                                                \
  }
  LAUNCH(4, 1) LAUNCH(4, 2) LAUNCH(4, 3) LAUNCH(4, 4)
  LAUNCH(8, 1) LAUNCH(8, 2) LAUNCH(8, 3) LAUNCH(8, 4)
#undef LAUNCH
  return -1;
}
