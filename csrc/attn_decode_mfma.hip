// MFMA decode attention (bf16 KV, head_dim 128): one wave per (seq, kv_head).
//
// Per KV page (32 positions), matrix cores do both halves of the work:
//   scores: S[pos16, head16] = K[pos16, k128] x Qt[k128, head16]
//           two 16-position halves x 4 k-steps of mfma_f32_16x16x32_bf16;
//           K fragments load STRAIGHT from the paged cache (lane l reads 16B
//           at row l%16, dims (l/16)*8 — no staging); Qt sits in LDS
//           XOR-swizzled ((head&15)<<4) so B-fragment reads are conflict-free.
//   softmax: D layout gives lane l all of head l%16's scores for 4+4
//           positions -> per-head state is ONE scalar per lane and the
//           cross-lane reduce is TWO shuffles (vs 12 per head in the VALU
//           kernel) for all 16 heads at once.
//   PV:     O[head16, d16] += P[head16, pos32] x V[pos32, d16]; P and a
//           transposed V image round-trip through LDS (40-element row pad,
//           16B-aligned conflict-free ds_read_b128), 8 d-blocks x 1 k-step.
//
// Fragment layout (gfx950 v_mfma_f32_16x16x32_bf16, verified by the probe):
//   A[16,32]: lane l holds A[l%16][(l/16)*8 + j], j=0..7
//   B[32,16]: lane l holds B[(l/16)*8 + j][l%16]
//   C/D     : lane l holds D[(l/16)*4 + r][l%16], r=0..3 (guide §3)
#include "attn_decode_mfma.h"
#include <cstdlib>

template <int D>
struct MfmaSmem {
  u16 qt[16 * D];           // Q^T as [head16][kD], row-swizzled
  u16 vt[D * PV_PAD];       // V^T [dD][pos32+pad]
  u16 p[16 * PV_PAD];       // P [head16][pos32+pad] (1.25 KB)
  float alpha[16];
  float linv[16];
};

// CONT (shared-prefix decode, attn_decode_prefix.hip): a row with
// row_prefix_pages[row] = P > 0 resumes from the f32 softmax state the
// partial kernel left for its first P pages and starts its page loop at P.
// LOCAL (local attention; never together with CONT): `window` W > 0 keeps the
// last W positions, so the page loop starts at page max(0, L - W) / 32 and
// that page masks the positions below L - W; `sinks` (f32 [Hq], or null)
// seeds head h's softmax state with m = sinks[h], l = 1, O = 0: one more
// logit in the denominator that adds nothing to the output. Without the flag
// neither argument is read and the kernel is the one it was before them.
template <int D, bool KV8, bool CONT = false, bool LOCAL = false>
__global__ __launch_bounds__(256) void attn_decode_mfma_kernel(
    u16* __restrict__ out,            // [n_dec, Hq, D]
    const u16* __restrict__ q,        // [n_dec, Hq, D]
    const u8* __restrict__ k_cache,   // [nb, Hk, BS, D] bf16 or e4m3
    const u8* __restrict__ v_cache,
    const int* __restrict__ block_tables,  // [S, bt_stride]
    const int* __restrict__ seq_lens,      // [S]
    int bt_stride, int n_dec, int Hq, int Hk, int seq_offset, float scale,
    const int* __restrict__ row_prefix_pages = nullptr,  // [n_dec] (CONT)
    const float* __restrict__ part_o = nullptr,          // [n_dec, Hq, D]
    const float* __restrict__ part_m = nullptr,          // [n_dec, Hq]
    const float* __restrict__ part_l = nullptr,
    int window = 0,                                      // (LOCAL)
    const float* __restrict__ sinks = nullptr) {         // [Hq] (LOCAL)
  static_assert(!(CONT && LOCAL), "the shared-prefix resume takes no window");
  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = threadIdx.x / WAVE;
  const long item = (long)blockIdx.x * (blockDim.x / WAVE) + wid;
  const int G = Hq / Hk;
  if (item >= (long)n_dec * Hk) return;
  const int sd = (int)(item / Hk);
  const int kh = (int)(item - (long)sd * Hk);
  const int sg = seq_offset + sd;
  const int L = seq_lens[sg];
  const int npages = (L + BS - 1) / BS;
  const int* bt = block_tables + (long)sg * bt_stride;

  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  MfmaSmem<D>* sm = ((MfmaSmem<D>*)smem_raw) + wid;

  const int lo16 = lane & 15;   // head column / A row
  const int hi4 = lane >> 4;    // 0..3

  // ---- stage Q^T: qt[head][k] = q[head][k] * scale (heads >= G zeroed).
  // lane l writes head l%16, 8 dims at (l/16)*8 + 32*t (4 iterations).
  {
    const int head = lo16;
#pragma unroll
    for (int t = 0; t < D / 32; ++t) {
      const int k0 = hi4 * 8 + t * 32;
      u16x8 val = {};
      if (head < G) {
        const u16* qrow = q + ((long)sd * Hq + kh * G + head) * D;
#pragma unroll
        for (int j = 0; j < 8; ++j) val[j] = f2bf(bf2f(qrow[k0 + j]) * scale);
      }
      *(u16x8*)((char*)sm->qt + qt_swz<D>(head, k0 * 2)) = val;
    }
  }

  wave_lds_sync();

  float m_run = -1e30f, l_run = 0.f;   // for head lo16
  constexpr int DB = D / 16;           // d-blocks
  f32x4 acc[DB];                       // O[head hi4*4+r][d lo16 + 16*dblk]
#pragma unroll
  for (int b = 0; b < DB; ++b) acc[b] = (f32x4)(0.f);

  int pg0 = 0;
  if constexpr (CONT) {
    pg0 = min(row_prefix_pages[sd], npages);
    if (pg0 > 0) {
      const long hrow = (long)sd * Hq + kh * G;
      if (lo16 < G) {
        m_run = part_m[hrow + lo16];
        l_run = part_l[hrow + lo16];
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int head = hi4 * 4 + r;
        if (head >= G) continue;
#pragma unroll
        for (int b = 0; b < DB; ++b)
          acc[b][r] = part_o[(hrow + head) * D + b * 16 + lo16];
      }
    }
  }

  int first_pos = 0;   // first visible position (LOCAL)
  if constexpr (LOCAL) {
    if (window > 0) first_pos = max(0, L - window);
    pg0 = first_pos / BS;   // holds position L - 1 at the latest: pg0 < npages
    if (sinks != nullptr && lo16 < G) {
      m_run = sinks[kh * G + lo16];
      l_run = 1.f;
    }
  }

  constexpr int ES = KV8 ? 1 : 2;  // bytes per cache element
  for (int pg = pg0; pg < npages; ++pg) {
    const long kv_base = (((long)bt[pg] * Hk + kh) * BS) * D * ES;
    const int valid = min(BS, L - pg * BS);
    // stage V^T (d-major) while the K fragment loads are in flight
    mfma_stage_vt<D, KV8>(sm->vt, v_cache + kv_base, lane);
    bf16frag ka[2][D / 32];
    mfma_load_k<D, KV8>(ka, k_cache + kv_base, lo16, hi4);
    mfma_page_update<D, LOCAL>(sm->qt, sm->vt, sm->p, sm->alpha, ka, valid,
                               lo16, hi4, m_run, l_run, acc,
                               first_pos - pg * BS);
  }

  // ---- epilogue: divide rows by their head's l and scatter
  if (hi4 == 0) sm->linv[lo16] = 1.0f / l_run;
  wave_lds_sync();
  float li[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) li[r] = sm->linv[hi4 * 4 + r];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int head = hi4 * 4 + r;
    if (head >= G) continue;
    u16* orow = out + ((long)sd * Hq + kh * G + head) * D;
#pragma unroll
    for (int b = 0; b < DB; ++b) orow[b * 16 + lo16] = f2bf(acc[b][r] * li[r]);
  }
}

// CONT: the shared-prefix route passes the partial-state buffers;
// LOCAL: the local-attention route passes a window and/or sinks
template <bool CONT, bool LOCAL = false>
static void launch_decode_mfma(void* out, const void* q, const void* k_cache,
                               const void* v_cache, const int* block_tables,
                               const int* seq_lens, int bt_stride, int n_dec,
                               int Hq, int Hk, int seq_offset, float scale,
                               int kv_fp8, int head_dim,
                               const int* row_prefix_pages,
                               const float* part_o, const float* part_m,
                               const float* part_l, hipStream_t s,
                               int window = 0, const float* sinks = nullptr) {
  // 2 waves/block (bf16 D=128: 31.4 KB LDS -> 5 blocks/CU)
  static const char* wpb_env = getenv("SUTRO_DECODE_WPB");
  const int wpb = wpb_env ? atoi(wpb_env) : 2;
  const long items = (long)n_dec * Hk;
  const long blocks = (items + wpb - 1) / wpb;
#define LAUNCH_MFMA(D, KV8)                                                  \
  if (head_dim == D && kv_fp8 == (KV8 ? 1 : 0)) {                            \
    hipLaunchKernelGGL((attn_decode_mfma_kernel<D, KV8, CONT, LOCAL>),       \
                       dim3((unsigned)blocks), dim3(wpb * WAVE),             \
                       sizeof(MfmaSmem<D>) * wpb, s, (u16*)out,              \
                       (const u16*)q, (const u8*)k_cache,                    \
                       (const u8*)v_cache, block_tables, seq_lens,           \
                       bt_stride, n_dec, Hq, Hk, seq_offset, scale,          \
                       row_prefix_pages, part_o, part_m, part_l, window,     \
                       sinks);                                               \
    return;                                                                  \
  }
  LAUNCH_MFMA(128, false)
  LAUNCH_MFMA(128, true)
  LAUNCH_MFMA(64, false)
  LAUNCH_MFMA(64, true)
#undef LAUNCH_MFMA
}

extern "C" void sutro_attn_decode_mfma(void* out, const void* q,
                                       const void* k_cache,
                                       const void* v_cache,
                                       const int* block_tables,
                                       const int* seq_lens, int bt_stride,
                                       int n_dec, int Hq, int Hk,
                                       int seq_offset, float scale, int kv_fp8,
                                       int head_dim, hipStream_t s) {
  launch_decode_mfma<false>(out, q, k_cache, v_cache, block_tables, seq_lens,
                            bt_stride, n_dec, Hq, Hk, seq_offset, scale,
                            kv_fp8, head_dim, nullptr, nullptr, nullptr,
                            nullptr, s);
}

// local attention: window > 0 and/or sinks != null (either may be neutral)
extern "C" void sutro_attn_decode_mfma_local(
    void* out, const void* q, const void* k_cache, const void* v_cache,
    const int* block_tables, const int* seq_lens, int bt_stride, int n_dec,
    int Hq, int Hk, int seq_offset, float scale, int kv_fp8, int head_dim,
    int window, const float* sinks, hipStream_t s) {
  launch_decode_mfma<false, true>(out, q, k_cache, v_cache, block_tables,
                                  seq_lens, bt_stride, n_dec, Hq, Hk,
                                  seq_offset, scale, kv_fp8, head_dim, nullptr,
                                  nullptr, nullptr, nullptr, s, window, sinks);
}

// per-row kernel resuming from the partial kernel's state (decode-only batch:
// row i of every buffer is sequence i)
extern "C" void sutro_attn_decode_mfma_cont(
    void* out, const void* q, const void* k_cache, const void* v_cache,
    const int* block_tables, const int* seq_lens, int bt_stride, int n_dec,
    int Hq, int Hk, float scale, int kv_fp8, int head_dim,
    const int* row_prefix_pages, const float* part_o, const float* part_m,
    const float* part_l, hipStream_t s) {
  launch_decode_mfma<true>(out, q, k_cache, v_cache, block_tables, seq_lens,
                           bt_stride, n_dec, Hq, Hk, 0, scale, kv_fp8,
                           head_dim, row_prefix_pages, part_o, part_m, part_l,
                           s);
}

// ---- debug probe: run the D=64 decode stages for one (seq, kv_head) and
// dump the vt and p LDS images plus the output, to localize a stage that
// breaks on hardware but not in the CPU simulation (tools/sim_mfma_decode.py)
__global__ void hd64_stage_probe_kernel(
    float* __restrict__ vt_dump,     // [64 * PV_PAD]
    float* __restrict__ p_dump,      // [16 * PV_PAD]
    u16* __restrict__ out,           // [Hq=1, 64]
    const u16* __restrict__ q,       // [1, 64]
    const u16* __restrict__ k_cache, // one page [32, 64]
    const u16* __restrict__ v_cache,
    int L, float scale) {
  constexpr int D = 64;
  const int lane = threadIdx.x & (WAVE - 1);
  __shared__ MfmaSmem<D> smw;
  MfmaSmem<D>* sm = &smw;
  const int lo16 = lane & 15;
  const int hi4 = lane >> 4;
  const int G = 1;
  {
    const int head = lo16;
#pragma unroll
    for (int t = 0; t < D / 32; ++t) {
      const int k0 = hi4 * 8 + t * 32;
      u16x8 val = {};
      if (head < G) {
        const u16* qrow = q + head * D;
#pragma unroll
        for (int j = 0; j < 8; ++j) val[j] = f2bf(bf2f(qrow[k0 + j]) * scale);
      }
      *(u16x8*)((char*)sm->qt + qt_swz<D>(head, k0 * 2)) = val;
    }
  }
  float m_run = -1e30f, l_run = 0.f;
  constexpr int DB = D / 16;
  f32x4 acc[DB];
#pragma unroll
  for (int b = 0; b < DB; ++b) acc[b] = (f32x4)(0.f);
  const int valid = L;
  {
    const u8* vsrc = (const u8*)v_cache;
#pragma unroll
    for (int it = 0; it < (BS * D) / ((int)WAVE * 8); ++it) {
      const int flat = it * (int)WAVE + lane;
      const int pos = flat & 31;
      const int d0 = (flat >> 5) * 8;
      const bf16frag vx = load_kv_frag<false>(vsrc + (pos * D + d0) * 2);
#pragma unroll
      for (int j = 0; j < 8; ++j)
        sm->vt[(d0 + j) * PV_PAD + pos] = (u16)vx[j];
    }
  }
  // dump vt
  for (int i = lane; i < D * PV_PAD; i += WAVE)
    vt_dump[i] = bf2f(sm->vt[i]);
  f32x4 s01[2];
#pragma unroll
  for (int half = 0; half < 2; ++half) {
    f32x4 d = (f32x4)(0.f);
#pragma unroll
    for (int kk = 0; kk < D / 32; ++kk) {
      const u8* krow = (const u8*)k_cache +
                       ((long)(half * 16 + lo16) * D + kk * 32 + hi4 * 8) * 2;
      bf16frag ka = load_kv_frag<false>(krow);
      bf16frag qb = *(const s16x8*)((char*)sm->qt +
                                    qt_swz<D>(lo16, (kk * 32 + hi4 * 8) * 2));
      d = mfma16(ka, qb, d);
    }
    s01[half] = d;
  }
  float sv[8];
#pragma unroll
  for (int half = 0; half < 2; ++half)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int pos = half * 16 + hi4 * 4 + r;
      float x = s01[half][r];
      if (pos >= valid) x = -1e30f;
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
  if (hi4 == 0) sm->alpha[lo16] = al;
#pragma unroll
  for (int half = 0; half < 2; ++half)
#pragma unroll
    for (int r = 0; r < 4; ++r)
      sm->p[lo16 * PV_PAD + half * 16 + hi4 * 4 + r] = f2bf(sv[half * 4 + r]);
  // dump p
  for (int i = lane; i < 16 * PV_PAD; i += WAVE)
    p_dump[i] = bf2f(sm->p[i]);
  float alr[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) alr[r] = sm->alpha[hi4 * 4 + r];
#pragma unroll
  for (int b = 0; b < DB; ++b)
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[b][r] *= alr[r];
  bf16frag pa = *(const s16x8*)(sm->p + lo16 * PV_PAD + hi4 * 8);
#pragma unroll
  for (int b = 0; b < DB; ++b) {
    bf16frag vb = *(const s16x8*)(sm->vt + (b * 16 + lo16) * PV_PAD + hi4 * 8);
    acc[b] = mfma16(pa, vb, acc[b]);
  }
  if (hi4 == 0) sm->linv[lo16] = 1.0f / l_run;
  float li[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) li[r] = sm->linv[hi4 * 4 + r];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int head = hi4 * 4 + r;
    if (head >= G) continue;
    u16* orow = out + head * D;
#pragma unroll
    for (int b = 0; b < DB; ++b) orow[b * 16 + lo16] = f2bf(acc[b][r] * li[r]);
  }
}

extern "C" void sutro_hd64_stage_probe(float* vt_dump, float* p_dump, void* out,
                                       const void* q, const void* k,
                                       const void* v, int L, float scale,
                                       hipStream_t s) {
  hipLaunchKernelGGL(hd64_stage_probe_kernel, dim3(1), dim3(64), 0, s, vt_dump,
                     p_dump, (u16*)out, (const u16*)q, (const u16*)k,
                     (const u16*)v, L, scale);
}

// ---- probe: C[16,16] = A[16,32] @ B[32,16] with the exact frag loaders ----
__global__ void mfma16_probe_kernel(float* __restrict__ c,
                                    const u16* __restrict__ a,   // [16,32]
                                    const u16* __restrict__ b) { // [32,16]
  const int lane = threadIdx.x & (WAVE - 1);
  const int lo16 = lane & 15, hi4 = lane >> 4;
  bf16frag af, bf;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    af[j] = (short)a[lo16 * 32 + hi4 * 8 + j];
    bf[j] = (short)b[(hi4 * 8 + j) * 16 + lo16];
  }
  f32x4 d = (f32x4)(0.f);
  d = mfma16(af, bf, d);
#pragma unroll
  for (int r = 0; r < 4; ++r) c[(hi4 * 4 + r) * 16 + lo16] = d[r];
}

extern "C" void sutro_mfma16_probe(float* c, const void* a, const void* b,
                                   hipStream_t s) {
  hipLaunchKernelGGL(mfma16_probe_kernel, dim3(1), dim3(64), 0, s, c,
                     (const u16*)a, (const u16*)b);
}
