// Split-KV MFMA decode attention: one row's KV range split across the waves of
// a block and across blocks, for the shapes where one wave per (seq, kv_head)
// (attn_decode_mfma.hip) leaves the chip idle: a few rows, or long rows.
//
// Two levels, both deterministic (no atomics, no counters):
//   inside a block  SPLIT_W = 4 waves serve one (seq, kv_head, block-split).
//                   Wave w walks its own contiguous run of pages through the
//                   per-page body of attn_decode_mfma.h with its own Q^T / V^T
//                   / P images and its own f32 state (m, l, acc). Waves 1..3
//                   then publish (m, l, acc) to LDS — acc goes over the wave's
//                   own V^T image, which is dead by then, so the merge needs
//                   no LDS beyond the four page-walk slices — and wave 0 folds
//                   them into its registers in ascending wave order.
//   across blocks   block-split s of S leaves the block's combined,
//                   un-normalised state in an f32 workspace and
//                   attn_decode_merge_kernel folds the splits in ascending s.
//                   With S == 1 the split kernel normalises and stores bf16
//                   itself: no workspace traffic, no second launch.
//
// Chunking is a function of the row's own length L and S alone:
//   npages   = ceil(L / 32)
//   per_wave = max(ceil(npages / (S * SPLIT_W)), SPLIT_MIN_PAGES)
//   wave (s, w) covers pages [(s*W + w) * per_wave, min(.. + per_wave, npages))
// so non-empty parts are a prefix of the (s, w) order, both merges know how
// many there are from L (split_parts below) and never read a slot that was not
// written: the workspace needs no clearing. A row's bits do not depend on its
// neighbours, and the grid (n_dec * Hk * S blocks) does not depend on the
// lengths: the launch replays from a hipGraph with other seq_lens.
//
// Merge of parts i (LDS and global alike, split_fold below):
//   M = max m_i;  w_i = e(m_i - M);  l = sum l_i w_i;  O = sum O_i w_i
// with e the page body's __expf in the units of its m. A row with one
// non-empty part has w = e(0) = 1 exactly and the epilogue is the per-row
// kernel's acc * (1.0f / l): bit-identical to attn_decode_mfma_kernel.
//
// `sinks` (f32 [Hq] or null) seed the state of the wave that owns page 0, as
// the per-row kernel's LOCAL route does. No window: a windowed layer reads at
// most five pages and stays on the per-row kernel.
//
// Resource usage (gfx950, -Rpass-analysis=kernel-resource-usage) is recorded
// in profiles/PROFILES.md, capture S1.
#include "attn_decode_mfma.h"

#define SPLIT_W 4          // waves per block (ops.DECODE_SPLIT_WAVES)
#define SPLIT_MIN_PAGES 4  // fewest pages worth a wave (ops.DECODE_SPLIT_MIN_PAGES)
#define SPLIT_S_MAX 16     // most block-splits a row takes (ops rule: S_MAX)

// one wave's page-walk images; the layout of the per-row kernel's MfmaSmem
template <int D>
struct SplitSmem {
  u16 qt[16 * D];        // Q^T as [head16][kD], row-swizzled
  u16 vt[D * PV_PAD];    // V^T [dD][pos32+pad]; after the walk: acc, f32
  u16 p[16 * PV_PAD];    // P [head16][pos32+pad]
  float alpha[16];       // after the walk: m per head column
  float linv[16];        // after the walk: l per head column
};
static_assert(sizeof(SplitSmem<128>) * SPLIT_W <= 64 * 1024, "LDS budget");
// acc of a wave is 16 heads x D f32 = 64 D bytes; its V^T image has 80 D
static_assert(16 * 128 * sizeof(float) <= sizeof(SplitSmem<128>::vt) &&
              16 * 64 * sizeof(float) <= sizeof(SplitSmem<64>::vt),
              "acc must fit the V^T image");

__device__ __forceinline__ int split_per_wave(int npages, int S) {
  const int parts = S * SPLIT_W;
  return max((npages + parts - 1) / parts, SPLIT_MIN_PAGES);
}

// non-empty waves of the row in (s, w) order: ceil(npages / per_wave)
__device__ __forceinline__ int split_parts(int npages, int per_wave) {
  return (npages + per_wave - 1) / per_wave;
}

// fold part (m_i, l_i, o_i...) into the running (M, l, o): the one statement
// of the merge arithmetic. The first part enters with weight e(0) = 1.
template <int N>
__device__ __forceinline__ void split_fold(float M, float m_i, float l_i,
                                           const float (&o_i)[N], bool first,
                                           float& l, float (&o)[N]) {
  const float w = __expf(m_i - M);
  if (first) {
    l = l_i * w;
#pragma unroll
    for (int j = 0; j < N; ++j) o[j] = o_i[j] * w;
  } else {
    l = fmaf(l_i, w, l);
#pragma unroll
    for (int j = 0; j < N; ++j) o[j] = fmaf(o_i[j], w, o[j]);
  }
}

template <int D, bool KV8>
__global__ __launch_bounds__(SPLIT_W* WAVE) NO_PACKED_F32
void attn_decode_split_kernel(
    u16* __restrict__ out,            // [n_dec, Hq, D] (written when S == 1)
    float* __restrict__ ws_o,         // [n_dec, Hq, S, D] un-normalised
    float* __restrict__ ws_m,         // [n_dec, Hq, S]
    float* __restrict__ ws_l,         // [n_dec, Hq, S]
    const u16* __restrict__ q,        // [n_dec, Hq, D]
    const u8* __restrict__ k_cache,   // [nb, Hk, BS, D] bf16 or e4m3
    const u8* __restrict__ v_cache,
    const int* __restrict__ block_tables,  // [.., bt_stride]
    const int* __restrict__ seq_lens,
    int bt_stride, int n_dec, int Hq, int Hk, int S, int seq_offset,
    float scale, const float* __restrict__ sinks) {  // [Hq] or null
  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = threadIdx.x / WAVE;
  const int s = (int)(blockIdx.x % (unsigned)S);
  const int item = (int)(blockIdx.x / (unsigned)S);  // < n_dec * Hk
  const int sd = item / Hk;
  const int kh = item - sd * Hk;
  const int G = Hq / Hk;
  const int sg = seq_offset + sd;
  const int L = seq_lens[sg];
  const int npages = (L + BS - 1) / BS;
  const int per_wave = split_per_wave(npages, S);
  // this block's non-empty waves are 0 .. nw-1
  const int nw = min(max(split_parts(npages, per_wave) - s * SPLIT_W, 0),
                     SPLIT_W);
  if (nw == 0) return;  // block-uniform: an empty block-split touches nothing
  const int* bt = block_tables + (long)sg * bt_stride;

  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  SplitSmem<D>* slices = (SplitSmem<D>*)smem_raw;
  SplitSmem<D>* sm = slices + wid;

  const int lo16 = lane & 15;   // head column / A row
  const int hi4 = lane >> 4;    // 0..3
  constexpr int DB = D / 16;    // d-blocks
  constexpr int ES = KV8 ? 1 : 2;

  float m_run = -1e30f, l_run = 0.f;   // for head lo16
  f32x4 acc[DB];                       // O[head hi4*4+r][d lo16 + 16*dblk]
#pragma unroll
  for (int b = 0; b < DB; ++b) acc[b] = (f32x4)(0.f);

  if (wid < nw) {  // wave-uniform
    // ---- stage Q^T: qt[head][k] = q[head][k] * scale (heads >= G zeroed)
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

    const int pg_begin = (s * SPLIT_W + wid) * per_wave;
    const int pg_end = min(pg_begin + per_wave, npages);
    if (pg_begin == 0 && sinks != nullptr && lo16 < G) {
      m_run = sinks[kh * G + lo16];
      l_run = 1.f;
    }
    for (int pg = pg_begin; pg < pg_end; ++pg) {
      const long kv_base = (((long)bt[pg] * Hk + kh) * BS) * D * ES;
      const int valid = min(BS, L - pg * BS);
      mfma_stage_vt<D, KV8>(sm->vt, v_cache + kv_base, lane);
      bf16frag ka[2][D / 32];
      mfma_load_k<D, KV8>(ka, k_cache + kv_base, lo16, hi4);
      mfma_page_update<D>(sm->qt, sm->vt, sm->p, sm->alpha, ka, valid, lo16,
                          hi4, m_run, l_run, acc);
    }

    // ---- publish: m, l per head column; acc (waves > 0) over the V^T image,
    // lane-major so wave 0's lane reads back the element it owns itself.
    // The fence keeps the f32 stores behind the body's last V^T reads.
    wave_lds_sync();
    if (hi4 == 0) {
      sm->alpha[lo16] = m_run;
      sm->linv[lo16] = l_run;
    }
    if (wid > 0) {
      float* pub = (float*)sm->vt;
#pragma unroll
      for (int b = 0; b < DB; ++b)
#pragma unroll
        for (int r = 0; r < 4; ++r) pub[(b * 4 + r) * (int)WAVE + lane] = acc[b][r];
    }
  }
  __syncthreads();
  if (wid != 0) return;

  // ---- wave 0 folds the block's parts, ascending, per accumulator row
  // (head hi4*4+r); every lane of a row computes the row's M and l itself
  const long hrow = (long)sd * Hq + kh * G;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int head = hi4 * 4 + r;
    float M = slices[0].alpha[head];
    for (int w = 1; w < nw; ++w) M = fmaxf(M, slices[w].alpha[head]);
    float o[DB], o_i[DB], l = 0.f;
#pragma unroll
    for (int b = 0; b < DB; ++b) o_i[b] = acc[b][r];
    split_fold<DB>(M, slices[0].alpha[head], slices[0].linv[head], o_i, true,
                   l, o);
    for (int w = 1; w < nw; ++w) {
      const float* pub = (const float*)slices[w].vt;
#pragma unroll
      for (int b = 0; b < DB; ++b) o_i[b] = pub[(b * 4 + r) * (int)WAVE + lane];
      split_fold<DB>(M, slices[w].alpha[head], slices[w].linv[head], o_i,
                     false, l, o);
    }
    if (head >= G) continue;
    if (S == 1) {
      const float li = 1.0f / l;
      u16* orow = out + (hrow + head) * D;
#pragma unroll
      for (int b = 0; b < DB; ++b) orow[b * 16 + lo16] = f2bf(o[b] * li);
    } else {
      const long slot = (hrow + head) * S + s;
      float* wrow = ws_o + slot * D;
#pragma unroll
      for (int b = 0; b < DB; ++b) wrow[b * 16 + lo16] = o[b];
      if (lo16 == 0) {
        ws_m[slot] = M;
        ws_l[slot] = l;
      }
    }
  }
}

// One wave per (row, q head): folds the row's non-empty block-splits in
// ascending s and writes bf16. Lane d owns elements d, d + 64 of the head.
template <int D>
__global__ __launch_bounds__(256) NO_PACKED_F32
void attn_decode_merge_kernel(
    u16* __restrict__ out,             // [n_dec, Hq, D]
    const float* __restrict__ ws_o,    // [n_dec, Hq, S, D]
    const float* __restrict__ ws_m,    // [n_dec, Hq, S]
    const float* __restrict__ ws_l,
    const int* __restrict__ seq_lens, int n_dec, int Hq, int S,
    int seq_offset) {
  const int lane = threadIdx.x & (WAVE - 1);
  const long item = (long)blockIdx.x * (blockDim.x / WAVE) + threadIdx.x / WAVE;
  if (item >= (long)n_dec * Hq) return;
  const int sd = (int)(item / Hq);
  const int L = seq_lens[seq_offset + sd];
  const int npages = (L + BS - 1) / BS;
  const int per_wave = split_per_wave(npages, S);
  // non-empty block-splits: 0 .. nb-1 (block s holds waves s*W .. s*W+W-1)
  const int nb = min((split_parts(npages, per_wave) + SPLIT_W - 1) / SPLIT_W, S);
  constexpr int N = D / (int)WAVE;
  const float* wm = ws_m + item * S;
  const float* wl = ws_l + item * S;
  const float* wo = ws_o + item * S * D;
  float M = wm[0];
  for (int s = 1; s < nb; ++s) M = fmaxf(M, wm[s]);
  float o[N], o_i[N], l = 0.f;
  for (int s = 0; s < nb; ++s) {
#pragma unroll
    for (int j = 0; j < N; ++j) o_i[j] = wo[(long)s * D + j * (int)WAVE + lane];
    split_fold<N>(M, wm[s], wl[s], o_i, s == 0, l, o);
  }
  const float li = 1.0f / l;
#pragma unroll
  for (int j = 0; j < N; ++j)
    out[item * D + j * (int)WAVE + lane] = f2bf(o[j] * li);
}

extern "C" int sutro_attn_decode_split_min_pages() { return SPLIT_MIN_PAGES; }
extern "C" int sutro_attn_decode_split_waves() { return SPLIT_W; }
extern "C" int sutro_attn_decode_split_max() { return SPLIT_S_MAX; }

// Returns 0, or -1 (nothing launched) for a head layout or S the kernels do
// not take: the caller raises.
extern "C" int sutro_attn_decode_split(
    void* out, float* ws_o, float* ws_m, float* ws_l, const void* q,
    const void* k_cache, const void* v_cache, const int* block_tables,
    const int* seq_lens, int bt_stride, int n_dec, int Hq, int Hk,
    int head_dim, int kv_fp8, int seq_offset, float scale, int S,
    const float* sinks, hipStream_t st) {
  if ((head_dim != 128 && head_dim != 64) || Hk <= 0 || Hq % Hk != 0 ||
      Hq / Hk > MAXG || S < 1 || S > SPLIT_S_MAX)
    return -1;
  if (n_dec == 0) return 0;
  const long blocks = (long)n_dec * Hk * S;
  if (blocks >= (1L << 31)) return -1;
#define LAUNCH_SPLIT(D, KV8)                                                 \
  if (head_dim == D && kv_fp8 == (KV8 ? 1 : 0))                              \
    hipLaunchKernelGGL((attn_decode_split_kernel<D, KV8>),                   \
                       dim3((unsigned)blocks), dim3(SPLIT_W * WAVE),         \
                       sizeof(SplitSmem<D>) * SPLIT_W, st, (u16*)out, ws_o,  \
                       ws_m, ws_l, (const u16*)q, (const u8*)k_cache,        \
                       (const u8*)v_cache, block_tables, seq_lens,           \
                       bt_stride, n_dec, Hq, Hk, S, seq_offset, scale, sinks);
  LAUNCH_SPLIT(128, false)
  LAUNCH_SPLIT(128, true)
  LAUNCH_SPLIT(64, false)
  LAUNCH_SPLIT(64, true)
#undef LAUNCH_SPLIT
  if (S > 1) {
    const long items = (long)n_dec * Hq;
    const unsigned mblocks = (unsigned)((items + 3) / 4);
    if (head_dim == 128)
      hipLaunchKernelGGL((attn_decode_merge_kernel<128>), dim3(mblocks),
                         dim3(4 * WAVE), 0, st, (u16*)out, ws_o, ws_m, ws_l,
                         seq_lens, n_dec, Hq, S, seq_offset);
    else
      hipLaunchKernelGGL((attn_decode_merge_kernel<64>), dim3(mblocks),
                         dim3(4 * WAVE), 0, st, (u16*)out, ws_o, ws_m, ws_l,
                         seq_lens, n_dec, Hq, S, seq_offset);
  }
  return 0;
}
