// Shared pieces of the MFMA decode attention kernels: the per-row kernel
// (attn_decode_mfma.hip) and the shared-prefix partial kernel
// (attn_decode_prefix.hip) run the SAME per-page body, so one MFMA column sees
// the same sequence of floating-point operations whether it runs alone or
// beside columns of other rows — the two routes are bit-identical by
// construction. Layout notes are at the top of attn_decode_mfma.hip.
#pragma once

#include "common.h"

#define BS 32
#define MAXG 8
#define QT_PAD_B 256 // Qt row bytes (128 bf16)
#define PV_PAD 40    // padded row length (elems) for P and Vt tiles

typedef s16x8 bf16frag;

__device__ __forceinline__ f32x4 mfma16(bf16frag a, bf16frag b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}

// 8 consecutive KV elements at byte pointer p -> bf16 fragment.
// bf16 cache: one 16B load. e4m3 cache: 8B load + native pk converts.
template <bool KV8>
__device__ __forceinline__ bf16frag load_kv_frag(const u8* p) {
  if constexpr (!KV8) return *(const s16x8*)p;
  const u32x2 raw = *(const u32x2*)p;
  float f[8];
  fp8x4_to_f32(raw[0], f);
  fp8x4_to_f32(raw[1], f + 4);
  bf16frag r;
#pragma unroll
  for (int j = 0; j < 8; ++j) r[j] = (short)f2bf(f[j]);
  return r;
}

// The lanes of a wave hand data to each other through LDS (Q^T, V^T, P, alpha).
// The hardware runs one wave's LDS operations in order, but the compiler
// reasons per thread: without a fence it may reuse an LDS value it loaded
// before another lane's store (seen in the D=64 partial kernel: the alpha
// read sank into the `hi4 == 0` branch that writes alpha, so the other lanes
// rescaled with the previous column block's alpha). Call this between a
// cross-lane LDS write and the reads that depend on it. At wavefront scope
// it emits no instruction.
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront", "local");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront", "local");
}

// row-local XOR swizzle; mask keeps the offset inside the 2*D-byte row
template <int D>
__device__ __forceinline__ int qt_swz(int head, int byte_in_row) {
  constexpr int mask = (D == 128) ? 15 : 7;
  return head * (2 * D) + (byte_in_row ^ ((head & mask) << 4));
}

// ---- stage one page's V^T (d-major) into vt[D][PV_PAD]: 64 lanes x
// (BS*D/512) iterations of 8 elements = the page. pos-major across lanes so
// the scatter writes spread over the banks.
template <int D, bool KV8>
__device__ __forceinline__ void mfma_stage_vt(u16* vt, const u8* vsrc,
                                              int lane) {
  constexpr int ES = KV8 ? 1 : 2;
#pragma unroll
  for (int it = 0; it < (BS * D) / ((int)WAVE * 8); ++it) {
    const int flat = it * (int)WAVE + lane;   // 8-elem chunk id
    const int pos = flat & 31;
    const int d0 = (flat >> 5) * 8;
    const bf16frag vx = load_kv_frag<KV8>(vsrc + (pos * D + d0) * ES);
#pragma unroll
    for (int j = 0; j < 8; ++j) vt[(d0 + j) * PV_PAD + pos] = (u16)vx[j];
  }
}

// ---- one page's K as MFMA A fragments, straight from the paged cache:
// ka[half][kk] = row pos half*16 + l%16, dims kk*32 + (l/16)*8..+8
template <int D, bool KV8>
__device__ __forceinline__ void mfma_load_k(bf16frag (&ka)[2][D / 32],
                                            const u8* kpage, int lo16,
                                            int hi4) {
  constexpr int ES = KV8 ? 1 : 2;
#pragma unroll
  for (int half = 0; half < 2; ++half)
#pragma unroll
    for (int kk = 0; kk < D / 32; ++kk)
      ka[half][kk] = load_kv_frag<KV8>(
          kpage + ((long)(half * 16 + lo16) * D + kk * 32 + hi4 * 8) * ES);
}

// ---- the per-page body for ONE 16-column block: K.Q MFMAs, the eight-score
// online-softmax update, the P -> bf16 round trip through LDS, the alpha
// rescale and the PV MFMAs. `qt` is the block's swizzled Q^T image, `vt` the
// page's V^T image, `p`/`alpha` wave-private LDS scratch. State (m_run,
// l_run for column lo16; acc = O[column hi4*4+r][d lo16 + 16*b]) is updated
// in place. The caller runs wave_lds_sync() between staging `qt` and the
// first call; `vt` is covered by the sync inside.
// LOWER (local attention): positions below `lo` are masked the way positions
// >= `valid` are. The mask is a select on the score, so a page with lo <= 0
// runs the arithmetic of the LOWER = false body; without the flag the
// comparison is not compiled and the body is the shared-prefix kernel's.
template <int D, bool LOWER = false>
__device__ __forceinline__ void mfma_page_update(
    const u16* qt, const u16* vt, u16* p, float* alpha,
    const bf16frag (&ka)[2][D / 32], int valid, int lo16, int hi4,
    float& m_run, float& l_run, f32x4 (&acc)[D / 16], int lo = 0) {
  constexpr int DB = D / 16;
  // ---- QK^T via MFMA: two 16-position halves
  f32x4 s01[2];
#pragma unroll
  for (int half = 0; half < 2; ++half) {
    f32x4 d = (f32x4)(0.f);
#pragma unroll
    for (int kk = 0; kk < D / 32; ++kk) {
      // B = Qt frag: B[k][head]: lane reads qt[head l%16][kk*32+(l/16)*8]
      bf16frag qb = *(const s16x8*)((const char*)qt +
                                    qt_swz<D>(lo16, (kk * 32 + hi4 * 8) * 2));
      d = mfma16(ka[half][kk], qb, d);
    }
    s01[half] = d;
  }

  // ---- online softmax: lane owns head lo16; 8 scores (2 halves x 4 r)
  float sv[8];
#pragma unroll
  for (int half = 0; half < 2; ++half)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int pos = half * 16 + hi4 * 4 + r;
      float x = s01[half][r];
      if (pos >= valid) x = -1e30f;
      if constexpr (LOWER)
        if (pos < lo) x = -1e30f;
      sv[half * 4 + r] = x;
    }
  float tmax = sv[0];
#pragma unroll
  for (int i = 1; i < 8; ++i) tmax = fmaxf(tmax, sv[i]);
  tmax = fmaxf(tmax, __shfl_xor(tmax, 16, 64));
  tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64));
  const float m_new = fmaxf(m_run, tmax);
  const float al = __expf(m_run - m_new);
  m_run = m_new;
  float psum = 0.f;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    sv[i] = __expf(sv[i] - m_new);
    psum += sv[i];
  }
  psum += __shfl_xor(psum, 16, 64);
  psum += __shfl_xor(psum, 32, 64);
  l_run = l_run * al + psum;
  if (hi4 == 0) alpha[lo16] = al;
  // write P[head][pos] (bf16)
#pragma unroll
  for (int half = 0; half < 2; ++half)
#pragma unroll
    for (int r = 0; r < 4; ++r)
      p[lo16 * PV_PAD + half * 16 + hi4 * 4 + r] = f2bf(sv[half * 4 + r]);
  // alpha, P and the page's V^T are read by other lanes than wrote them
  wave_lds_sync();

  // ---- rescale O by alpha of the row's head ((l/16)*4+r)
  float alr[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) alr[r] = alpha[hi4 * 4 + r];
#pragma unroll
  for (int b = 0; b < DB; ++b)   // NOT 8: at head_dim 64 acc has DB=4
#pragma unroll                   // entries — the out-of-bounds writes here
    for (int r = 0; r < 4; ++r)  // poisoned the whole accumulator chain
      acc[b][r] *= alr[r];       // (ROADMAP.md: D=64 post-mortem)

  // ---- PV via MFMA: A = P[head16, pos32], B = Vt-read V[pos32, d16]
  bf16frag pa = *(const s16x8*)(p + lo16 * PV_PAD + hi4 * 8);
#pragma unroll
  for (int b = 0; b < DB; ++b) {
    // B frag: V[pos=(l/16)*8+j][d = b*16 + l%16] from vt[d][pos]
    bf16frag vb = *(const s16x8*)(vt + (b * 16 + lo16) * PV_PAD + hi4 * 8);
    acc[b] = mfma16(pa, vb, acc[b]);
  }
}
